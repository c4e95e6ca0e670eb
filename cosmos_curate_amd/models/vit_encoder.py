"""The ViT encoder the three vision towers share, MI355X-native.

Everything CLIP (clip_vit.ClipVisionTowerAMD), SigLIP
(siglip_vit.SiglipVisionTowerAMD) and InternVideo2
(internvideo2_vit.InternVideo2VisionTowerAMD) have in common: the
patch-embed-as-GEMM front, the fused-QKV weight layout and the pre-norm
encoder layer [norm1, QKV GEMM, (QK-norm,) attention, out-proj + residual,
norm2, fc1 + activation, fc2 + residual].  What differs between the towers
is data: the config (clip_weights.VitConfig or a config with its fields:
geometry, activation, norm kind and eps, QK-norm) and where the checkpoint
keeps a layer's tensors (_layer_weights: which keys, and whether QKV has a
bias).  The layer branches on those values, never on the tower it serves;
embeddings and pooling stay in the tower files.

- every contraction runs on the hand-written MFMA bf16 kernel
  (cc_gemm_bf16*, csrc/cc_gemm.hip) through the C ABI, bias / activation /
  residual fused into its epilogue;
- attention is one cc_attn call straight off the QKV GEMM output
  (csrc/cc_attn.hip; the kernel for a sequence length is the library's
  choice, cc::attn_plan) for every head dim the library takes — the
  multiples of 8 from 64 to 128, asked of cc_attn_plan itself; any other
  head dim takes torch sdpa (``force_sdpa = True`` sends every tower
  there, for A/B runs);
- norm1 and norm2 never materialise on the GPU: their affine part is folded
  into the QKV / fc1 weights once at construction (fold_layernorm, or
  fold_rmsnorm for an RMSNorm tower) and the GEMM epilogue finishes the
  normalisation from per-row statistics that the GEMM producing the
  residual stream wrote (``fold_ln = False`` restores
  the norm kernel + plain GEMM chain);
- the remaining norms run the fused HIP kernels (f32 statistics);
- an MLP width that is no multiple of 64 (SigLIP-so400m's 4304) is
  zero-padded once at construction to the next one, which the GEMM's
  K % 64 == 0 needs — exact, see VitEncoderAMD;
- activations are bf16 end-to-end.

No CPU fallback: _linear() requires the HIP extension + a GPU (the tests
may monkeypatch _linear to torch on CPU to pin arithmetic structure; the
product never does).
"""

from __future__ import annotations

import ctypes
import math

import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models import clip_weights as cw

# VitConfig.act -> cc_gemm_bf16_ex epilogue activation code
ACT_CODES = {"quick_gelu": 1, "gelu_tanh": 2, "gelu_erf": 3}


def cc_linear(
    x: torch.Tensor,
    w_bf16: torch.Tensor,
    bias_f32: torch.Tensor | None,
    act: int = 0,
    residual: torch.Tensor | None = None,
) -> torch.Tensor:
    """C[M,N] = act(x[M,K] @ w[N,K]^T + bias) [+ residual], bf16 out.

    act 1 = quick-gelu, 2 = tanh-gelu; residual fused into the epilogue
    (cc_gemm_bf16_ex).

    x and residual may be row-strided 2-D views (unit column stride, e.g.
    the CLS rows ``t[:, 0]`` of a [n, seq, H] tensor): the kernel reads
    them in place through cc_gemm_bf16_strided — no gather copy."""
    lib = hotpath.require_gpu()
    assert x.dtype == torch.bfloat16 and w_bf16.dtype == torch.bfloat16
    assert w_bf16.is_contiguous()
    M, K = x.shape
    N = w_bf16.shape[0]
    lda = _row_stride(x)
    if lda is None or lda % 8 != 0:
        x = x.contiguous()
        lda = K
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    ldr = N
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == torch.bfloat16
        ldr = _row_stride(residual)
        if ldr is None:
            residual = residual.contiguous()
            ldr = N
    bias_p = bias_f32.data_ptr() if bias_f32 is not None else None
    res_p = residual.data_ptr() if residual is not None else None
    if lda == K and ldr == N:
        hotpath.check(
            lib.cc_gemm_bf16_ex(
                x.data_ptr(), w_bf16.data_ptr(), out.data_ptr(), M, N, K,
                bias_p, 1, act, res_p, stream,
            )
        )
    else:
        hotpath.check(
            lib.cc_gemm_bf16_strided(
                x.data_ptr(), lda, w_bf16.data_ptr(), out.data_ptr(), M, N, K,
                bias_p, 1, act, res_p, ldr, stream,
            )
        )
    return out


def fold_layernorm(
    w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fold a LayerNorm's affine part into the linear layer it feeds.

    linear(layer_norm(x), w, b) = rstd * (W' x - mean * s) + c with
    W' = bf16(w * gamma) per input column, s[n] = sum_k W'[n, k] and
    c = w_bf16 @ beta + b.  ``s`` is the f32 value of the sum of the
    ROUNDED W', the numbers the MFMA really multiplies: with any other sum
    the row mean does not cancel.  Pure CPU arithmetic on the checkpoint;
    returns (W' bf16, s f32, c f32).
    """
    w_fold = (w.float() * gamma.float()[None, :]).to(torch.bfloat16)
    colsum = w_fold.double().sum(dim=1).float()
    cbias = (w.to(torch.bfloat16).double() @ beta.double() + b.double()).float()
    return w_fold.contiguous(), colsum.contiguous(), cbias.contiguous()


def fold_rmsnorm(
    w: torch.Tensor, b: torch.Tensor | None, weight: torch.Tensor
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fold_layernorm for an RMSNorm (weight only, no mean subtraction):
    linear(rmsnorm(x), w, b) = rstd * (W' x) + c with W' = bf16(w * weight)
    per input column and c = b, or zeros for a layer without bias.  The
    column sum multiplies a zero mean in the epilogue and is not needed:
    zeros.  Returns (W' bf16, zeros f32, c f32) for cc_linear_ln(rms=True)."""
    w_fold = (w.float() * weight.float()[None, :]).to(torch.bfloat16)
    zeros = torch.zeros(w.shape[0], dtype=torch.float32)
    cbias = zeros.clone() if b is None else b.float()
    return w_fold.contiguous(), zeros, cbias.contiguous()


def cc_ln_stats(x: torch.Tensor) -> torch.Tensor:
    """Row statistics of x [M, H] bf16 as the folded GEMMs read them: f32
    partial (sum, sum of squares) per 64-column block, [M, H/64, 2]."""
    lib = hotpath.require_gpu()
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    M, H = x.shape
    stats = torch.empty((M, H // 64, 2), dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    hotpath.check(
        lib.cc_ln_stats_bf16(x.data_ptr(), M, H, stats.data_ptr(), stream))
    return stats


def cc_linear_ln(
    x: torch.Tensor,
    stats: torch.Tensor,
    w_fold: torch.Tensor,
    colsum: torch.Tensor,
    cbias: torch.Tensor,
    act: int,
    eps: float,
    row_step: int = 1,
    rms: bool = False,
) -> torch.Tensor:
    """act(linear(layer_norm(x))) with the LayerNorm folded away
    (cc_gemm_bf16_ln): x is the raw LN input, ``stats`` its row statistics,
    (w_fold, colsum, cbias) from fold_layernorm.  ``row_step`` > 1 takes
    every row_step-th row of x and of stats, in place.  ``rms``: the norm is
    an RMSNorm (cc_gemm_bf16_rms) and (w_fold, colsum, cbias) come from
    fold_rmsnorm; the statistics are the same partials."""
    lib = hotpath.require_gpu()
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    assert w_fold.dtype == torch.bfloat16 and w_fold.is_contiguous()
    rows, K = x.shape
    assert stats.shape == (rows, K // 64, 2) and stats.is_contiguous()
    M = (rows + row_step - 1) // row_step
    N = w_fold.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    murstd = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    entry = lib.cc_gemm_bf16_rms if rms else lib.cc_gemm_bf16_ln
    hotpath.check(
        entry(
            x.data_ptr(), row_step, stats.data_ptr(), murstd.data_ptr(),
            w_fold.data_ptr(), colsum.data_ptr(), cbias.data_ptr(),
            out.data_ptr(), M, N, K, act, eps, stream,
        )
    )
    return out


def cc_rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """RMSNorm over the last dim of a bf16 tensor, f32 weight
    (cc_rmsnorm_bf16): bf16(bf16(x * rstd) * w)."""
    assert x.dtype == torch.bfloat16
    if not x.is_cuda:
        # CPU tensors only (the monkeypatched structure tests): the
        # kernel's rounding order in torch f32
        xf = x.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
        return (y.to(torch.bfloat16).float() * w).to(torch.bfloat16)
    lib = hotpath.require_gpu()
    xc = x.contiguous()
    out = torch.empty_like(xc)
    h = xc.shape[-1]
    stream = torch.cuda.current_stream(x.device).cuda_stream
    hotpath.check(
        lib.cc_rmsnorm_bf16(
            xc.data_ptr(), w.data_ptr(), out.data_ptr(), xc.numel() // h, h,
            eps, stream))
    return out


def cc_qk_rmsnorm(
    qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, eps: float
) -> torch.Tensor:
    """QK-normalisation in place on a fused-QKV GEMM output [M, 3H] bf16
    (cc_qk_rmsnorm_bf16): the q and the k section of every row each go
    through an RMSNorm of width H; v is not touched.  Returns qkv."""
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    M, ld = qkv.shape
    H = ld // 3
    if not qkv.is_cuda:  # CPU tensors only, as in cc_rmsnorm
        qkv[:, :H] = cc_rmsnorm(qkv[:, :H], wq, eps)
        qkv[:, H:2 * H] = cc_rmsnorm(qkv[:, H:2 * H], wk, eps)
        return qkv
    lib = hotpath.require_gpu()
    stream = torch.cuda.current_stream(qkv.device).cuda_stream
    hotpath.check(
        lib.cc_qk_rmsnorm_bf16(
            qkv.data_ptr(), M, H, ld, wq.data_ptr(), wk.data_ptr(), eps,
            stream))
    return qkv


def cc_linear_res_stats(
    x: torch.Tensor, w_bf16: torch.Tensor, bias_f32: torch.Tensor,
    residual: torch.Tensor,
) -> tuple[torch.Tensor, torch.Tensor]:
    """(x @ w^T + bias + residual, its row statistics): cc_linear with a
    residual whose epilogue also writes what cc_ln_stats would compute from
    the output (cc_gemm_bf16_res_stats)."""
    lib = hotpath.require_gpu()
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    assert residual.dtype == torch.bfloat16 and residual.is_contiguous()
    M, K = x.shape
    N = w_bf16.shape[0]
    assert residual.shape == (M, N)
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    stats = torch.empty((M, N // 64, 2), dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    hotpath.check(
        lib.cc_gemm_bf16_res_stats(
            x.data_ptr(), w_bf16.data_ptr(), out.data_ptr(), M, N, K,
            bias_f32.data_ptr(), residual.data_ptr(), stats.data_ptr(), stream,
        )
    )
    return out, stats


def _row_stride(t: torch.Tensor) -> int | None:
    """Row stride (elements) of a 2-D tensor the GEMM can read in place:
    unit column stride and rows that do not overlap; None otherwise."""
    rows, cols = t.shape
    if t.stride(1) != 1 and cols != 1:
        return None
    if rows == 1:
        return cols
    return t.stride(0) if t.stride(0) >= cols else None


def cc_layernorm(
    x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float
) -> torch.Tensor:
    """LayerNorm over the last dim, f32 weights, output in x's dtype."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        # fused HIP LN (f32 stats, torch layer_norm opmath semantics)
        lib = hotpath.require_gpu()
        xc = x.contiguous()
        out = torch.empty_like(xc)
        h = xc.shape[-1]
        m = xc.numel() // h
        stream = torch.cuda.current_stream(x.device).cuda_stream
        hotpath.check(
            lib.cc_layernorm_bf16(
                xc.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                m, h, eps, stream,
            )
        )
        return out
    # CPU tensors only (the monkeypatched structure tests)
    return torch.nn.functional.layer_norm(
        x.float(), (x.shape[-1],), w, b, eps=eps
    ).to(x.dtype)


def patchify(
    pixel_values: torch.Tensor, cfg: cw.VitConfig, patch_k: int
) -> torch.Tensor:
    """(N,3,image,image) -> the patch GEMM's A operand [N*g*g, patch_k]
    bf16: column order c*P*P + ky*P + kx (conv-weight flatten), zero-padded
    to patch_k."""
    g = cfg.image // cfg.patch
    k0 = 3 * cfg.patch * cfg.patch
    x = pixel_values.to(torch.bfloat16)
    n = x.shape[0]
    # patch extraction: (n,c,ph,ky,pw,kx) -> (n,ph,pw,c,ky,kx)
    patches = (
        x.reshape(n, 3, g, cfg.patch, g, cfg.patch)
        .permute(0, 2, 4, 1, 3, 5)
        .reshape(n * g * g, k0)
    )
    if patch_k != k0:
        patches = torch.nn.functional.pad(patches, (0, patch_k - k0))
    return patches


class VitEncoderAMD(torch.nn.Module):
    """Patch-embed weight + ``cfg.layers`` pre-norm encoder layers.

    ``prefix`` is what the state dict puts before ``embeddings.`` /
    ``encoder.layers.`` in the HF key layout; a tower whose checkpoint is
    laid out otherwise overrides _patch_weight / _layer_weights.  The
    patch-embed GEMM's K = 3*patch^2 is zero-padded to the kernel's
    64-multiple requirement (588 -> 640 for L/14) — exact, the padded
    columns multiply zeros.

    ``cfg.norm`` makes norm1 / norm2 LayerNorms or RMSNorms (eps
    ``cfg.ln_eps`` either way); with ``cfg.qk_norm`` q and k each go through
    an RMSNorm of the hidden width, at the same eps, before attention.

    ``fold_ln`` (default True): on the GPU, norm1 and norm2 are folded into
    the QKV and fc1 GEMMs (_layer_folded).  False runs the norm kernel and
    the plain GEMMs — for A/B runs and parity tests; it is also what CPU
    tensors and head dims cc_attn does not take get.

    ``force_sdpa`` (default False): True sends attention through torch
    sdpa and its permute copies even where cc_attn takes the head dim (and
    with it turns the fold off) — for A/B runs and parity tests.

    MLP width: when ``cfg.intermediate`` is no multiple of 64 the fc1 / fc2
    buffers are padded to the next one (``self.intermediate``): zero rows
    on w_fc1, b_fc1 and on the folded wf_fc1, s_fc1, c_fc1, zero columns on
    w_fc2.  Exact: a padded fc1 output is act(0 + 0) = 0 for both
    activations — on the folded route rstd*(0 - mean*0) + 0 = 0 — and the
    padded fc2 columns multiply those zeros.  Checkpoints stay unpadded.
    """

    fold_ln = True
    force_sdpa = False

    def __init__(
        self, sd: dict[str, torch.Tensor], cfg: cw.VitConfig, prefix: str
    ) -> None:
        super().__init__()
        self.cfg = cfg
        self.heads = cfg.heads
        self.layers = cfg.layers
        self.scale = 1.0 / math.sqrt(cfg.hidden // cfg.heads)
        self.act = ACT_CODES[cfg.act]
        self.rms = {"layernorm": False, "rmsnorm": True}[cfg.norm]
        self.prefix = prefix
        reg = self.register_buffer

        k0 = 3 * cfg.patch * cfg.patch
        self.patch_k = (k0 + 63) // 64 * 64  # cc_gemm needs K % 64 == 0
        # fc2's K: the MLP width, zero-padded to a multiple of 64
        self.intermediate = (cfg.intermediate + 63) // 64 * 64
        mlp_pad = self.intermediate - cfg.intermediate
        pad_rows = lambda t: torch.nn.functional.pad(  # noqa: E731
            t, (0, 0, 0, mlp_pad) if t.dim() == 2 else (0, mlp_pad))
        w_patch = self._patch_weight(sd).reshape(cfg.hidden, k0)
        if self.patch_k != k0:
            w_patch = torch.nn.functional.pad(w_patch, (0, self.patch_k - k0))
        reg("w_patch", w_patch.to(torch.bfloat16).contiguous())
        for i in range(cfg.layers):
            t = self._layer_weights(sd, i)
            assert (t["ln1_b"] is None) == (t["ln2_b"] is None) == self.rms
            t["w_fc1"], t["b_fc1"] = pad_rows(t["w_fc1"]), pad_rows(t["b_fc1"])
            t["w_fc2"] = torch.nn.functional.pad(t["w_fc2"], (0, mlp_pad))
            # GEMM weights (w_*) bf16, everything else f32; an absent bias
            # is a None buffer
            for name, v in t.items():
                if v is not None:
                    dt = torch.bfloat16 if name.startswith("w_") else torch.float32
                    v = v.to(dt).contiguous()
                reg(f"{name}_{i}", v)
            # norm1 / norm2 folded into the GEMM they feed (derived, so kept
            # out of the state dict); row order (q, k, v) as in w_qkv
            p = self._layer_params(i)
            for name, ln in (("qkv", "ln1"), ("fc1", "ln2")):
                w, b = t["w_" + name], p("b_" + name)
                folded = (
                    fold_rmsnorm(w, b, p(ln + "_w")) if self.rms
                    else fold_layernorm(w, b, p(ln + "_w"), p(ln + "_b")))
                for pre, f in zip(("wf", "s", "c"), folded):
                    reg(f"{pre}_{name}_{i}", f, persistent=False)

    def _patch_weight(self, sd: dict[str, torch.Tensor]) -> torch.Tensor:
        """The patch-embedding weight; flattens to [hidden, 3*patch^2]."""
        return sd[self.prefix + "embeddings.patch_embedding.weight"]

    def _layer_weights(
        self, sd: dict[str, torch.Tensor], i: int
    ) -> dict[str, torch.Tensor | None]:
        """Layer ``i``'s checkpoint tensors, unconverted and unpadded, under
        the buffer base names, in registration order: ``w_qkv`` [3*hidden,
        hidden] with rows ordered (q, k, v) and ``b_qkv`` (None: QKV has no
        bias), ``w_out`` / ``b_out``, ``ln1_w`` / ``ln1_b`` and ``ln2_w`` /
        ``ln2_b`` (the biases None for an RMSNorm), ``w_fc1`` / ``b_fc1``,
        ``w_fc2`` / ``b_fc2``, and with ``cfg.qk_norm`` ``qn_w`` / ``kn_w``.
        Here: the HF key layout under ``prefix``."""
        q = f"{self.prefix}encoder.layers.{i}."
        qkv = [q + f"self_attn.{x}_proj." for x in "qkv"]
        return {
            "w_qkv": torch.cat([sd[x + "weight"] for x in qkv], dim=0),
            "b_qkv": torch.cat([sd[x + "bias"] for x in qkv]),
            "w_out": sd[q + "self_attn.out_proj.weight"],
            "b_out": sd[q + "self_attn.out_proj.bias"],
            "ln1_w": sd[q + "layer_norm1.weight"],
            "ln1_b": sd[q + "layer_norm1.bias"],
            "ln2_w": sd[q + "layer_norm2.weight"],
            "ln2_b": sd[q + "layer_norm2.bias"],
            "w_fc1": sd[q + "mlp.fc1.weight"],
            "b_fc1": sd[q + "mlp.fc1.bias"],
            "w_fc2": sd[q + "mlp.fc2.weight"],
            "b_fc2": sd[q + "mlp.fc2.bias"],
        }

    # the one contraction primitive; tests may monkeypatch this
    def _linear(
        self,
        x: torch.Tensor,
        w: torch.Tensor,
        b: torch.Tensor | None,
        act: int = 0,
        residual: torch.Tensor | None = None,
    ) -> torch.Tensor:
        return cc_linear(x, w, b, act, residual)

    # the one stand-alone norm primitive; no bias makes it an RMSNorm
    def _ln(
        self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None,
        eps: float | None = None,
    ) -> torch.Tensor:
        eps = self.cfg.ln_eps if eps is None else eps
        if b is None:
            return cc_rmsnorm(x, w, eps)
        return cc_layernorm(x, w, b, eps)

    def _layer_params(self, i: int):
        """Accessor of layer ``i``'s buffers by base name (``"w_qkv"``...)."""
        return lambda name: getattr(self, f"{name}_{i}")

    def _patches(
        self,
        pixel_values: torch.Tensor | None,
        patches: torch.Tensor | None,
        n: int | None,
    ) -> tuple[torch.Tensor, int]:
        """The forward() input contract of both towers: pixels, or prebuilt
        GEMM-ready ``patches`` [n*g*g, patch_k] bf16
        (cc_clip_preprocess_patches output) with ``n`` frames."""
        if patches is None:
            return patchify(pixel_values, self.cfg, self.patch_k), pixel_values.shape[0]
        g = self.cfg.image // self.cfg.patch
        assert n is not None and patches.shape == (n * g * g, self.patch_k)
        return patches, n

    def _native_attn(self, t: torch.Tensor) -> bool:
        """Whether attention on ``t`` runs cc_attn: a GPU tensor, a head dim
        the library takes, and no ``force_sdpa``."""
        return (
            not self.force_sdpa and t.is_cuda
            and hotpath.attn_supported(self.heads, self.cfg.hidden)
        )

    def _attention(self, qkv_flat: torch.Tensor, n: int, seq: int) -> torch.Tensor:
        """(n*seq, 3*hidden) fused QKV rows -> (n*seq, hidden)."""
        hidden = self.cfg.hidden
        hd = hidden // self.heads
        if self._native_attn(qkv_flat):
            # fused attention straight off the QKV GEMM output
            # (csrc/cc_attn.hip) — no permute copies
            lib = hotpath.require_gpu()
            attn = torch.empty(
                (n * seq, hidden), dtype=torch.bfloat16, device=qkv_flat.device
            )
            stream = torch.cuda.current_stream(qkv_flat.device).cuda_stream
            hotpath.check(
                lib.cc_attn(
                    qkv_flat.data_ptr(), attn.data_ptr(), n, seq, self.heads,
                    hidden, ctypes.c_float(self.scale), stream,
                )
            )
            return attn
        qkv = qkv_flat.reshape(n, seq, 3, self.heads, hd)
        q = qkv[:, :, 0].permute(0, 2, 1, 3)  # (n, heads, seq, hd)
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        attn = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, scale=self.scale
        )
        return attn.permute(0, 2, 1, 3).reshape(n * seq, hidden)

    def _layer(self, h: torch.Tensor, i: int, n: int, seq: int) -> torch.Tensor:
        """Encoder layer ``i``: (n, seq, H) -> (n, seq, H)."""
        H = self.cfg.hidden
        p = self._layer_params(i)
        y = self._ln(h, p("ln1_w"), p("ln1_b"))
        qkv_flat = self._linear(y.reshape(n * seq, H), p("w_qkv"), p("b_qkv"))
        if self.cfg.qk_norm:
            cc_qk_rmsnorm(qkv_flat, p("qn_w"), p("kn_w"), self.cfg.ln_eps)
        attn = self._attention(qkv_flat, n, seq)
        # residual add fused into the out-proj epilogue
        h = self._linear(
            attn, p("w_out"), p("b_out"), residual=h.reshape(n * seq, H)
        ).reshape(n, seq, H)
        y = self._ln(h, p("ln2_w"), p("ln2_b"))
        # activation fused into the fc1 epilogue
        y = self._linear(
            y.reshape(n * seq, H), p("w_fc1"), p("b_fc1"), act=self.act)
        return self._linear(
            y, p("w_fc2"), p("b_fc2"), residual=h.reshape(n * seq, H)
        ).reshape(n, seq, H)

    def _folds(self, h: torch.Tensor) -> bool:
        """Whether ``h`` takes the folded-norm route."""
        return self.fold_ln and self._native_attn(h)

    def _layer_folded(
        self, h: torch.Tensor, stats: torch.Tensor, i: int, n: int, seq: int
    ) -> tuple[torch.Tensor, torch.Tensor]:
        """Encoder layer ``i`` without norm kernels: (h (n*seq, H), its row
        statistics) -> the same pair for the layer's output.  QKV and fc1
        read the raw residual stream and normalise in their epilogue;
        out-proj and fc2 write the statistics of what they store."""
        p = self._layer_params(i)
        eps = self.cfg.ln_eps
        qkv_flat = cc_linear_ln(
            h, stats, p("wf_qkv"), p("s_qkv"), p("c_qkv"), 0, eps, rms=self.rms)
        if self.cfg.qk_norm:
            cc_qk_rmsnorm(qkv_flat, p("qn_w"), p("kn_w"), eps)
        attn = self._attention(qkv_flat, n, seq)
        h, stats = cc_linear_res_stats(attn, p("w_out"), p("b_out"), h)
        y = cc_linear_ln(
            h, stats, p("wf_fc1"), p("s_fc1"), p("c_fc1"), self.act, eps,
            rms=self.rms)
        return cc_linear_res_stats(y, p("w_fc2"), p("b_fc2"), h)

    def _encode_folded(
        self, h: torch.Tensor, n: int, seq: int, layers: int
    ) -> tuple[torch.Tensor, torch.Tensor]:
        """The first ``layers`` layers on the folded route: (n, seq, H) ->
        ((n, seq, H), row statistics of the result).  One read-only pass
        takes the statistics of the embedding; after that each layer's
        GEMMs hand them on."""
        H = self.cfg.hidden
        h = h.reshape(n * seq, H)
        stats = cc_ln_stats(h)
        for i in range(layers):
            h, stats = self._layer_folded(h, stats, i, n, seq)
        return h.reshape(n, seq, H), stats

    def _encode(
        self, h: torch.Tensor, n: int, seq: int, layers: int | None = None
    ) -> torch.Tensor:
        """The first ``layers`` encoder layers (default: all of them)."""
        layers = self.layers if layers is None else layers
        if self._folds(h):
            return self._encode_folded(h, n, seq, layers)[0]
        for i in range(layers):
            h = self._layer(h, i, n, seq)
        return h
