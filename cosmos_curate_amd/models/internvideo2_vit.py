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

Everything that is O(tokens) runs on the hand-written kernels (DESIGN.md
§17).  The patch weight, the blocks and the _linear / _ln primitives are
the shared encoder (vit_encoder.VitEncoderAMD): its layer run with the
config's RMSNorm, QK-norm and erf-GELU and a QKV without bias, over the
checkpoint's ``vision_encoder.blocks.{i}.*`` keys (_layer_weights).  On the
folded route that is one cc_ln_stats pass over the assembled sequence and,
per block, QKV GEMM with rmsnorm1 folded in, QK-norm in place on its
output, cc_attn at head dim 88, out-proj + residual + statistics, fc1 with
rmsnorm2 folded in and the erf-GELU epilogue, fc2 + residual + statistics.
This file keeps what is InternVideo2's own:

- the patch bias, the CLS token and the position table;
- LayerScale, folded into the out-proj and fc2 weights and biases as they
  are gathered (row n scaled by gamma[n] in f32, then cast to bf16): exact
  in real arithmetic, free at run time, and the reason the residual
  epilogue stays usable;
- the pooling head's K and V are one [2*hidden, hidden] GEMM with
  LayerNorm_k folded into the K rows and LayerNorm_v into the V rows
  (fold_layernorm), reading the statistics the last fc2 wrote.

What is O(clips) runs in torch f32, following the SigLIP MAP head's
precedent: the token mean, LayerNorm_q, the q projection, the one-query
softmax over K/V, the projection to 768, vision_proj and the L2 norm.

``fold_ln = False`` runs cc_rmsnorm / cc_layernorm plus the plain GEMMs
instead, for A/B runs and parity tests; it is also the route of CPU tensors
(the structure tests, with _linear monkeypatched to torch).

Out of scope, and refused loudly: T = 1 (the single-image position table),
a position table of another T than the config's (no temporal
interpolation), and widths the kernels are not instantiated for (the 6B
geometry) — the kernels reject those before any launch.
"""

from __future__ import annotations

import torch

from cosmos_curate_amd.models import internvideo2_weights as iw
from cosmos_curate_amd.models.vit_encoder import (
    VitEncoderAMD,
    cc_linear_ln,
    fold_layernorm,
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
    f32 unit-norm video embeddings."""

    def __init__(
        self,
        sd: dict[str, torch.Tensor],
        cfg: iw.InternVideo2Config = iw.INTERNVIDEO2_1B,
    ) -> None:
        if cfg.num_frames < 2:
            msg = ("InternVideo2 tower: num_frames 1 needs the single-image "
                   "position table, which is not implemented")
            raise NotImplementedError(msg)
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
        super().__init__(sd, cfg, ve)
        reg = self.register_buffer
        to_f32 = lambda t: t.float().contiguous()  # noqa: E731
        reg("b_patch", to_f32(sd[ve + "patch_embed.proj.bias"]))
        reg("cls_token", to_f32(sd[ve + "cls_token"].reshape(1, 1, H)))
        reg("pos_embed", to_f32(pos))
        # pooling head: K and V as one GEMM, their LayerNorms folded in
        cp = ve + "clip_projector."
        for n in "kv":
            reg(f"pool_ln{n}_w", to_f32(sd[cp + f"norm1_{n}.weight"]))
            reg(f"pool_ln{n}_b", to_f32(sd[cp + f"norm1_{n}.bias"]))
            reg(f"pool_w{n}",
                sd[cp + f"cross_attn.{n}.weight"].to(torch.bfloat16).contiguous())
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

    def _patch_weight(self, sd: dict[str, torch.Tensor]) -> torch.Tensor:
        # [H, 3, 1, P, P]: tubelet 1, so the 3-D conv is a per-frame GEMM
        return sd[self.prefix + "patch_embed.proj.weight"]

    def _layer_weights(
        self, sd: dict[str, torch.Tensor], i: int
    ) -> dict[str, torch.Tensor | None]:
        b = f"{self.prefix}blocks.{i}."
        if b + "attn.qkv.bias" in sd or b + "attn.q_bias" in sd:
            msg = "InternVideo2 tower: a qkv bias is not implemented"
            raise NotImplementedError(msg)
        # LayerScale folded into the GEMM that feeds the residual add
        w_out, b_out = fold_layerscale(
            sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"], sd[b + "ls1.gamma"])
        w_fc2, b_fc2 = fold_layerscale(
            sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"], sd[b + "ls2.gamma"])
        return {
            "w_qkv": sd[b + "attn.qkv.weight"], "b_qkv": None,
            "w_out": w_out, "b_out": b_out,
            "ln1_w": sd[b + "norm1.weight"], "ln1_b": None,
            "ln2_w": sd[b + "norm2.weight"], "ln2_b": None,
            "w_fc1": sd[b + "mlp.fc1.weight"], "b_fc1": sd[b + "mlp.fc1.bias"],
            "w_fc2": w_fc2, "b_fc2": b_fc2,
            "qn_w": sd[b + "attn.q_norm.weight"],
            "kn_w": sd[b + "attn.k_norm.weight"],
        }

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
                self._linear(self._ln(h, getattr(self, f"pool_ln{x}_w"),
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
        tok = self._linear(patches, self.w_patch, self.b_patch)
        h = torch.cat([self.cls_token.to(torch.bfloat16).expand(n, 1, H),
                       tok.reshape(n, seq - 1, H)], dim=1)
        h = (h.float() + self.pos_embed).to(torch.bfloat16)
        stats = None
        if self._folds(h):
            # the last fc2's statistics feed the pooling head's K/V GEMM
            h, stats = self._encode_folded(h, n, seq, self.layers)
        else:
            h = self._encode(h, n, seq)
        e = self._pool(h.reshape(n * seq, H), stats, n, seq)
        return e / torch.linalg.vector_norm(e, dim=-1, keepdim=True)
