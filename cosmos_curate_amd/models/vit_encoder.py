"""The ViT encoder both vision towers share, MI355X-native.

Everything CLIP (clip_vit.ClipVisionTowerAMD) and SigLIP
(siglip_vit.SiglipVisionTowerAMD) have in common: the patch-embed-as-GEMM
front, the fused-QKV weight layout and the pre-norm encoder layer
[LN1, QKV GEMM, attention, out-proj + residual, LN2, fc1 + activation,
fc2 + residual].  What differs between the towers is data, read from
clip_weights.VitConfig (activation, LN eps, geometry) and the state-dict
key prefix; embeddings and pooling stay in the tower files.

- every contraction runs on the hand-written MFMA bf16 kernel
  (cc_gemm_bf16*, csrc/cc_gemm.hip) through the C ABI, bias / activation /
  residual fused into its epilogue;
- attention is one cc_attn call straight off the QKV GEMM output
  (csrc/cc_attn.hip; the kernel for a sequence length is the library's
  choice, cc::attn_plan); head dims other than 64 take torch sdpa;
- layernorms run the fused HIP kernel (f32 statistics);
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
ACT_CODES = {"quick_gelu": 1, "gelu_tanh": 2}


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
    ``encoder.layers.``.  The patch-embed GEMM's K = 3*patch^2 is
    zero-padded to the kernel's 64-multiple requirement (588 -> 640 for
    L/14) — exact, the padded columns multiply zeros.
    """

    def __init__(
        self, sd: dict[str, torch.Tensor], cfg: cw.VitConfig, prefix: str
    ) -> None:
        super().__init__()
        self.cfg = cfg
        self.heads = cfg.heads
        self.layers = cfg.layers
        self.scale = 1.0 / math.sqrt(cfg.hidden // cfg.heads)
        self.act = ACT_CODES[cfg.act]
        reg = self.register_buffer
        to_bf = lambda t: t.to(torch.bfloat16).contiguous()  # noqa: E731
        to_f32 = lambda t: t.float().contiguous()  # noqa: E731

        k0 = 3 * cfg.patch * cfg.patch
        self.patch_k = (k0 + 63) // 64 * 64  # cc_gemm needs K % 64 == 0
        w_patch = sd[prefix + "embeddings.patch_embedding.weight"].reshape(
            cfg.hidden, k0)
        if self.patch_k != k0:
            w_patch = torch.nn.functional.pad(w_patch, (0, self.patch_k - k0))
        reg("w_patch", to_bf(w_patch))
        for i in range(cfg.layers):
            q = f"{prefix}encoder.layers.{i}."
            # fused QKV: [3*hidden, hidden] rows ordered (q, k, v)
            qkv = [q + f"self_attn.{x}_proj." for x in "qkv"]
            reg(f"w_qkv_{i}", to_bf(torch.cat([sd[x + "weight"] for x in qkv], dim=0)))
            reg(f"b_qkv_{i}", to_f32(torch.cat([sd[x + "bias"] for x in qkv])))
            reg(f"w_out_{i}", to_bf(sd[q + "self_attn.out_proj.weight"]))
            reg(f"b_out_{i}", to_f32(sd[q + "self_attn.out_proj.bias"]))
            reg(f"ln1_w_{i}", to_f32(sd[q + "layer_norm1.weight"]))
            reg(f"ln1_b_{i}", to_f32(sd[q + "layer_norm1.bias"]))
            reg(f"ln2_w_{i}", to_f32(sd[q + "layer_norm2.weight"]))
            reg(f"ln2_b_{i}", to_f32(sd[q + "layer_norm2.bias"]))
            reg(f"w_fc1_{i}", to_bf(sd[q + "mlp.fc1.weight"]))
            reg(f"b_fc1_{i}", to_f32(sd[q + "mlp.fc1.bias"]))
            reg(f"w_fc2_{i}", to_bf(sd[q + "mlp.fc2.weight"]))
            reg(f"b_fc2_{i}", to_f32(sd[q + "mlp.fc2.bias"]))

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

    def _ln(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return cc_layernorm(x, w, b, self.cfg.ln_eps)

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

    def _attention(self, qkv_flat: torch.Tensor, n: int, seq: int) -> torch.Tensor:
        """(n*seq, 3*hidden) fused QKV rows -> (n*seq, hidden)."""
        hidden = self.cfg.hidden
        hd = hidden // self.heads
        if qkv_flat.is_cuda and hd == 64:
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

    def _encode(
        self, h: torch.Tensor, n: int, seq: int, layers: int | None = None
    ) -> torch.Tensor:
        """The first ``layers`` encoder layers (default: all of them)."""
        for i in range(self.layers if layers is None else layers):
            h = self._layer(h, i, n, seq)
        return h
