"""InternVideo2 vision tower (the video embedder of the reference's split
pipeline) on the MFMA GEMM path.

Architecture (InternVideo2 stage 2, ``pretrain_internvideo2_1b_patch14_224``
+ ``vision_proj``): a per-frame patch-14 conv (tubelet 1) over T frames,
one sequence [CLS; T*256 tokens] + a learned position table, 40 pre-norm
blocks

    x += ls1 * proj(attn(rmsnorm1(x)))      qkv without bias; q and k, each
                                            [tokens, hidden], go through an
                                            RMSNorm of the whole hidden
                                            width before the head split
    x += ls2 * fc2(gelu_erf(fc1(rmsnorm2(x))))

no final norm, an attention-pooling head (``clip_projector``: one query per
clip, the LayerNorm of the token mean, over LayerNorm_k / LayerNorm_v of the
tokens; 16 heads, output projection to 768), ``vision_proj`` to 512 and an
L2 norm.  The CLIP-teacher decoders of the model's forward do not feed the
embedding and are not evaluated.

Everything that is O(tokens) runs on the hand-written kernels, through the
primitives of vit_encoder:

- the patch GEMM, conv bias in its epilogue;
- one cc_ln_stats pass over the assembled sequence; after that the GEMMs
  that write the residual stream hand the row statistics on;
- per block: QKV GEMM with rmsnorm1 folded in (cc_linear_rms), QK-norm in
  place on its output (cc_qk_rmsnorm), cc_attn at head dim 88, out-proj +
  residual + statistics, fc1 with rmsnorm2 folded in and the erf-GELU
  epilogue, fc2 + residual + statistics;
- LayerScale is folded into the out-proj and fc2 weights and biases once at
  construction (row n scaled by gamma[n] in f32, then cast to bf16): exact
  in real arithmetic, free at run time, and the reason the residual
  epilogue stays usable;
- the pooling head's K and V are one [2*hidden, hidden] GEMM with
  LayerNorm_k folded into the K rows and LayerNorm_v into the V rows
  (fold_layernorm), reading the statistics the last fc2 wrote.

What is O(clips) runs in torch f32, following the SigLIP MAP head's
precedent: the token mean, LayerNorm_q, the q projection, the one-query
softmax over K/V, the projection to 768, vision_proj and the L2 norm.

``fold_norms = False`` runs cc_rmsnorm / cc_layernorm plus the plain GEMMs
instead, for A/B runs and parity tests.

Out of scope, and refused loudly: T = 1 (the single-image position table),
a position table of another T than the config's (no temporal
interpolation), and widths the kernels are not instantiated for (the 6B
geometry) — the kernels reject those before any launch.
"""

from __future__ import annotations

import torch

from cosmos_curate_amd.models import internvideo2_weights as iw
from cosmos_curate_amd.models.vit_encoder import (
    ACT_CODES,
    VitEncoderAMD,
    cc_linear,
    cc_linear_ln,
    cc_linear_res_stats,
    cc_linear_rms,
    cc_ln_stats,
    cc_layernorm,
    cc_qk_rmsnorm,
    cc_rmsnorm,
    fold_layernorm,
    fold_rmsnorm,
    patchify,
)


def fold_layerscale(
    w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor
) -> tuple[torch.Tensor, torch.Tensor]:
    """gamma * linear(x, w, b) = linear(x, gamma[:, None] * w, gamma * b):
    (the scaled weight in bf16, the scaled bias in f32), scaled in f32."""
    g = gamma.float()
    return ((g[:, None] * w.float()).to(torch.bfloat16).contiguous(),
            (g * b.float()).contiguous())


class InternVideo2VisionTowerAMD(VitEncoderAMD):
    """(B, T, 3, image, image) pixels or prebuilt patch rows -> (B, proj)
    f32 unit-norm video embeddings.

    Shares VitEncoderAMD's attention call and input contract; the weights
    (checkpoint key names, internvideo2_weights) and the block are its own.
    """

    fold_norms = True

    def __init__(
        self,
        sd: dict[str, torch.Tensor],
        cfg: iw.InternVideo2Config = iw.INTERNVIDEO2_1B,
        layers: int | None = None,
    ) -> None:
        """``layers``: build only the first so many blocks (tests)."""
        torch.nn.Module.__init__(self)
        if cfg.num_frames < 2:
            msg = ("InternVideo2 tower: num_frames 1 needs the single-image "
                   "position table, which is not implemented")
            raise NotImplementedError(msg)
        self.cfg = cfg
        self.heads = cfg.heads
        self.layers = cfg.layers if layers is None else layers
        self.scale = float(cfg.hidden // cfg.heads) ** -0.5
        self.act = ACT_CODES["gelu_erf"]
        ve = "vision_encoder."
        H = cfg.hidden
        pos = sd[ve + "pos_embed"]
        if tuple(pos.shape) != (1, cfg.num_pos, H):
            per = cfg.tokens_per_frame
            msg = (f"InternVideo2 tower: position table {tuple(pos.shape)} "
                   f"does not match num_frames {cfg.num_frames} (needs "
                   f"(1, {cfg.num_pos}, {H}); the table holds "
                   f"{(pos.shape[1] - 1) / per:g} frames).  Temporal "
                   "interpolation of a position table is not implemented: "
                   "set num_frames to the checkpoint's")
            raise ValueError(msg)
        reg = self.register_buffer
        to_bf = lambda t: t.to(torch.bfloat16).contiguous()  # noqa: E731
        to_f32 = lambda t: t.float().contiguous()  # noqa: E731

        k0 = 3 * cfg.patch * cfg.patch
        self.patch_k = (k0 + 63) // 64 * 64  # cc_gemm needs K % 64 == 0
        # [H, 3, 1, P, P]: tubelet 1, so the 3-D conv is a per-frame GEMM
        w_patch = sd[ve + "patch_embed.proj.weight"].reshape(H, k0)
        reg("w_patch", to_bf(torch.nn.functional.pad(w_patch, (0, self.patch_k - k0))))
        reg("b_patch", to_f32(sd[ve + "patch_embed.proj.bias"]))
        reg("cls_token", to_f32(sd[ve + "cls_token"].reshape(1, 1, H)))
        reg("pos_embed", to_f32(pos))
        for i in range(self.layers):
            b = f"{ve}blocks.{i}."
            if b + "attn.qkv.bias" in sd or b + "attn.q_bias" in sd:
                msg = "InternVideo2 tower: a qkv bias is not implemented"
                raise NotImplementedError(msg)
            reg(f"norm1_w_{i}", to_f32(sd[b + "norm1.weight"]))
            reg(f"norm2_w_{i}", to_f32(sd[b + "norm2.weight"]))
            reg(f"qn_w_{i}", to_f32(sd[b + "attn.q_norm.weight"]))
            reg(f"kn_w_{i}", to_f32(sd[b + "attn.k_norm.weight"]))
            reg(f"w_qkv_{i}", to_bf(sd[b + "attn.qkv.weight"]))
            reg(f"w_fc1_{i}", to_bf(sd[b + "mlp.fc1.weight"]))
            reg(f"b_fc1_{i}", to_f32(sd[b + "mlp.fc1.bias"]))
            # LayerScale folded into the GEMM that feeds the residual add
            for name, lin, ls in (("out", "attn.proj", "ls1"), ("fc2", "mlp.fc2", "ls2")):
                w, bias = fold_layerscale(
                    sd[b + lin + ".weight"], sd[b + lin + ".bias"], sd[b + ls + ".gamma"])
                reg(f"w_{name}_{i}", w)
                reg(f"b_{name}_{i}", bias)
            # rmsnorm1 / rmsnorm2 folded into QKV / fc1 (derived buffers)
            for name, w, bias, nw in (
                ("qkv", sd[b + "attn.qkv.weight"], None, f"norm1_w_{i}"),
                ("fc1", sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"], f"norm2_w_{i}"),
            ):
                for pre, t in zip(("wf", "s", "c"),
                                  fold_rmsnorm(w, bias, getattr(self, nw))):
                    reg(f"{pre}_{name}_{i}", t, persistent=False)
        # pooling head: K and V as one GEMM, their LayerNorms folded in
        cp = ve + "clip_projector."
        for n in "kv":
            reg(f"pool_ln{n}_w", to_f32(sd[cp + f"norm1_{n}.weight"]))
            reg(f"pool_ln{n}_b", to_f32(sd[cp + f"norm1_{n}.bias"]))
            reg(f"pool_w{n}", to_bf(sd[cp + f"cross_attn.{n}.weight"]))
            reg(f"pool_b{n}", to_f32(sd[cp + f"cross_attn.{n}_bias"]))
        folded = [
            fold_layernorm(sd[cp + f"cross_attn.{n}.weight"],
                           sd[cp + f"cross_attn.{n}_bias"].float(),
                           sd[cp + f"norm1_{n}.weight"], sd[cp + f"norm1_{n}.bias"])
            for n in "kv"
        ]
        for pre, k_part, v_part in zip(("wf", "s", "c"), *folded):
            reg(f"{pre}_pool_kv", torch.cat([k_part, v_part]).contiguous(),
                persistent=False)
        # O(clips) part of the head, torch f32
        reg("pool_lnq_w", to_f32(sd[cp + "norm1_q.weight"]))
        reg("pool_lnq_b", to_f32(sd[cp + "norm1_q.bias"]))
        reg("pool_wq", to_f32(sd[cp + "cross_attn.q.weight"]))
        reg("pool_bq", to_f32(sd[cp + "cross_attn.q_bias"]))
        reg("pool_wo", to_f32(sd[cp + "cross_attn.proj.weight"]))
        reg("pool_bo", to_f32(sd[cp + "cross_attn.proj.bias"]))
        reg("vproj_w", to_f32(sd["vision_proj.weight"]))
        reg("vproj_b", to_f32(sd["vision_proj.bias"]))

    def _block_folded(
        self, h: torch.Tensor, stats: torch.Tensor, i: int, n: int, seq: int
    ) -> tuple[torch.Tensor, torch.Tensor]:
        """Block ``i`` without norm kernels: (h (n*seq, H), its row
        statistics) -> the same pair for the block's output."""
        p = self._layer_params(i)
        eps = self.cfg.rms_eps
        qkv = cc_linear_rms(h, stats, p("wf_qkv"), p("s_qkv"), p("c_qkv"), 0, eps)
        cc_qk_rmsnorm(qkv, p("qn_w"), p("kn_w"), eps)
        attn = self._attention(qkv, n, seq)
        h, stats = cc_linear_res_stats(attn, p("w_out"), p("b_out"), h)
        y = cc_linear_rms(h, stats, p("wf_fc1"), p("s_fc1"), p("c_fc1"), self.act, eps)
        return cc_linear_res_stats(y, p("w_fc2"), p("b_fc2"), h)

    def _block(self, h: torch.Tensor, i: int, n: int, seq: int) -> torch.Tensor:
        """Block ``i`` with the stand-alone norm kernel and plain GEMMs."""
        p = self._layer_params(i)
        eps = self.cfg.rms_eps
        qkv = cc_linear(cc_rmsnorm(h, p("norm1_w"), eps), p("w_qkv"), None)
        cc_qk_rmsnorm(qkv, p("qn_w"), p("kn_w"), eps)
        attn = self._attention(qkv, n, seq)
        h = cc_linear(attn, p("w_out"), p("b_out"), residual=h)
        y = cc_linear(cc_rmsnorm(h, p("norm2_w"), eps), p("w_fc1"), p("b_fc1"),
                      act=self.act)
        return cc_linear(y, p("w_fc2"), p("b_fc2"), residual=h)

    def _pool(self, h: torch.Tensor, stats: torch.Tensor | None, n: int,
              seq: int) -> torch.Tensor:
        """clip_projector + vision_proj: (n*seq, H) -> (n, proj) f32."""
        cfg = self.cfg
        H = cfg.hidden
        hd = H // cfg.pool_heads
        if stats is not None:
            kv = cc_linear_ln(h, stats, self.wf_pool_kv, self.s_pool_kv,
                              self.c_pool_kv, 0, cfg.pool_ln_eps)
        else:
            kv = torch.cat([
                cc_linear(cc_layernorm(h, getattr(self, f"pool_ln{x}_w"),
                                       getattr(self, f"pool_ln{x}_b"), cfg.pool_ln_eps),
                          getattr(self, f"pool_w{x}"), getattr(self, f"pool_b{x}"))
                for x in "kv"], dim=1)
        kv = kv.reshape(n, seq, 2, cfg.pool_heads, hd).float()
        k = kv[:, :, 0].transpose(1, 2)  # (n, heads, seq, hd)
        v = kv[:, :, 1].transpose(1, 2)
        q = torch.nn.functional.layer_norm(
            h.reshape(n, seq, H).float().mean(dim=1), (H,), self.pool_lnq_w,
            self.pool_lnq_b, eps=cfg.pool_ln_eps)
        q = (q @ self.pool_wq.T + self.pool_bq) * hd ** -0.5
        q = q.reshape(n, cfg.pool_heads, 1, hd)
        att = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
        o = (att @ v).reshape(n, H)
        o = o @ self.pool_wo.T + self.pool_bo
        return o @ self.vproj_w.T + self.vproj_b

    @torch.no_grad()
    def forward(
        self,
        pixel_values: torch.Tensor | None = None,
        *,
        patches: torch.Tensor | None = None,
        n: int | None = None,
    ) -> torch.Tensor:
        """``pixel_values`` (B, T, 3, image, image), or ``patches``
        [B*T*g*g, patch_k] bf16 (cc_clip_preprocess_patches output, frames
        in (clip, time) order) with ``n`` = B clips."""
        cfg = self.cfg
        H, T = cfg.hidden, cfg.num_frames
        if patches is None:
            if pixel_values.dim() != 5 or pixel_values.shape[1] != T:
                msg = (f"InternVideo2 tower: expected (B, {T}, 3, {cfg.image}, "
                       f"{cfg.image}) pixels, got {tuple(pixel_values.shape)}")
                raise ValueError(msg)
            n = pixel_values.shape[0]
            patches = patchify(pixel_values.flatten(0, 1), cfg, self.patch_k)
        else:
            assert n is not None
            assert patches.shape == (n * T * cfg.tokens_per_frame, self.patch_k)
        seq = cfg.num_pos
        tok = cc_linear(patches, self.w_patch, self.b_patch)
        h = torch.cat([self.cls_token.to(torch.bfloat16).expand(n, 1, H),
                       tok.reshape(n, seq - 1, H)], dim=1)
        h = (h.float() + self.pos_embed).to(torch.bfloat16).reshape(n * seq, H)
        if self.fold_norms:
            stats = cc_ln_stats(h)
            for i in range(self.layers):
                h, stats = self._block_folded(h, stats, i, n, seq)
        else:
            stats = None
            for i in range(self.layers):
                h = self._block(h, i, n, seq)
        e = self._pool(h, stats, n, seq)
        return e / torch.linalg.vector_norm(e, dim=-1, keepdim=True)
