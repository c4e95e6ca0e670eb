"""SigLIP vision tower on the MFMA GEMM path (BASELINE config #3's
"SigLIP-L/14" embedder).  Two geometries, both data in clip_weights:
google/siglip-so400m-patch14-224 (hidden 1152, 16 heads of 72, MLP 4304,
27 layers — the only patch-14 SigLIP tower released, so what "L/14" can
mean) and the SigLIP-L stand-in google/siglip-large-patch16-256.  so400m
runs the same kernels: cc_attn at head dim 72, the LayerNorm family at
H = 1152, and an MLP width the shared encoder pads to 4352.

Architecture per transformers SiglipVisionModel (the numerics oracle used
by tests/test_gpu_vit.py::test_siglip_gpu_vs_oracle_cosine): conv patch
embed WITH bias, no class token, learned position embeddings, pre-norm
encoder layers with gelu_pytorch_tanh MLPs, post_layernorm, then a
MultiheadAttentionPooling "MAP" head (1 learned probe query
cross-attending over the tokens) whose pooled vector is the embedding.
LayerNorm eps = 1e-6 (SiglipVisionConfig default; CLIP uses 1e-5).

The patch GEMM, the encoder layers and the _linear / _ln primitives are
the shared encoder (vit_encoder.VitEncoderAMD) — the same HIP kernels as
the CLIP tower, with the activation and LN eps read from the VitConfig.
This file keeps what is SigLIP's own: the patch bias and position add,
post-LN, and the tiny MAP head (1 query per frame), which runs in torch
f32.
"""

from __future__ import annotations

import torch

from cosmos_curate_amd.models import clip_weights as cw
from cosmos_curate_amd.models.vit_encoder import VitEncoderAMD


class SiglipVisionTowerAMD(VitEncoderAMD):
    """SigLIP vision tower + MAP pooling head, bf16 MFMA path."""

    def __init__(self, sd: dict[str, torch.Tensor],
                 cfg: cw.VitConfig = cw.SIGLIP_L16_256) -> None:
        super().__init__(sd, cfg, "")
        reg = self.register_buffer
        reg("b_patch", sd["embeddings.patch_embedding.bias"].float().contiguous())
        reg("pos_emb", sd["embeddings.position_embedding.weight"].clone())
        reg("post_ln_w", sd["post_layernorm.weight"].float().contiguous())
        reg("post_ln_b", sd["post_layernorm.bias"].float().contiguous())
        # MAP head (torch f32)
        reg("probe", sd["head.probe"].float().contiguous())
        reg("h_inproj_w", sd["head.attention.in_proj_weight"].float().contiguous())
        reg("h_inproj_b", sd["head.attention.in_proj_bias"].float().contiguous())
        reg("h_outproj_w", sd["head.attention.out_proj.weight"].float().contiguous())
        reg("h_outproj_b", sd["head.attention.out_proj.bias"].float().contiguous())
        reg("h_ln_w", sd["head.layernorm.weight"].float().contiguous())
        reg("h_ln_b", sd["head.layernorm.bias"].float().contiguous())
        reg("h_fc1_w", sd["head.mlp.fc1.weight"].float().contiguous())
        reg("h_fc1_b", sd["head.mlp.fc1.bias"].float().contiguous())
        reg("h_fc2_w", sd["head.mlp.fc2.weight"].float().contiguous())
        reg("h_fc2_b", sd["head.mlp.fc2.bias"].float().contiguous())

    def _map_head(self, x: torch.Tensor) -> torch.Tensor:
        """MAP pooling head (SiglipMultiheadAttentionPoolingHead), torch
        f32: probe cross-attention over the (B, seq, H) tokens."""
        cfg = self.cfg
        B = x.shape[0]
        hd = cfg.hidden // self.heads
        xf = x.float()
        probe = self.probe.expand(B, 1, cfg.hidden)
        wq, wk, wv = self.h_inproj_w.chunk(3, dim=0)
        bq, bk, bv = self.h_inproj_b.chunk(3, dim=0)
        q = (probe @ wq.T + bq).reshape(B, 1, self.heads, hd).transpose(1, 2)
        k = (xf @ wk.T + bk).reshape(B, -1, self.heads, hd).transpose(1, 2)
        v = (xf @ wv.T + bv).reshape(B, -1, self.heads, hd).transpose(1, 2)
        att = torch.softmax((q @ k.transpose(-1, -2)) * (hd ** -0.5), dim=-1)
        o = (att @ v).transpose(1, 2).reshape(B, 1, cfg.hidden)
        o = o @ self.h_outproj_w.T + self.h_outproj_b
        res = o
        o = torch.nn.functional.layer_norm(
            o, (cfg.hidden,), self.h_ln_w, self.h_ln_b, eps=cfg.ln_eps)
        o = o @ self.h_fc1_w.T + self.h_fc1_b
        o = torch.nn.functional.gelu(o, approximate="tanh")
        o = o @ self.h_fc2_w.T + self.h_fc2_b
        return (res + o)[:, 0]

    @torch.no_grad()
    def forward(
        self,
        pixel_values: torch.Tensor | None = None,
        *,
        patches: torch.Tensor | None = None,
        n: int | None = None,
    ) -> torch.Tensor:
        """(N,3,image,image) bf16 or prebuilt patches -> (N, hidden) f32
        L2-normalized MAP-pooled embeddings."""
        cfg = self.cfg
        patches, n = self._patches(pixel_values, patches, n)
        seq = (cfg.image // cfg.patch) ** 2  # no class token
        tok = self._linear(patches, self.w_patch, self.b_patch)
        h = (tok.reshape(n, seq, cfg.hidden).float()
             + self.pos_emb.unsqueeze(0)).to(torch.bfloat16)
        h = self._encode(h, n, seq)
        h = self._ln(h, self.post_ln_w, self.post_ln_b)
        pooled = self._map_head(h)
        return pooled / torch.linalg.vector_norm(pooled, dim=-1, keepdim=True)
