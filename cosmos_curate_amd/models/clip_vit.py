"""CLIP ViT-B/32 vision tower, MI355X-native forward.

Product counterpart of ``CLIPModel.get_image_features``
(/root/reference/cosmos_curate/models/clip.py:64-74): same arithmetic as
transformers' CLIPVisionModelWithProjection (conv patch embed -> cls+pos ->
pre-LN -> 12 x [LN1, MHA, LN2, quick-gelu MLP] -> post-LN on cls ->
visual projection).

The patch GEMM, the encoder layers and the _linear / _ln primitives are
the shared encoder (vit_encoder.VitEncoderAMD, see there for how they map
onto the HIP kernels).  This file keeps what is CLIP's own:

- the [CLS; tokens] + position embedding + pre-LN assembly, one fused
  kernel on the GPU (cc_embed_assemble_ln), the torch chain on CPU;
- the last encoder layer computing only what the CLS pooling reads: K/V
  for every token, everything else for the CLS rows;
- post-LN on the CLS rows, the visual projection (cc_gemm_bf16) and the
  f32 L2 normalization (clip.py:74).
"""

from __future__ import annotations

import ctypes

import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models import clip_weights as cw
from cosmos_curate_amd.models.vit_encoder import VitEncoderAMD, cc_linear_ln


class ClipVisionTowerAMD(VitEncoderAMD):
    """CLIP vision tower + projection on the MFMA GEMM path.

    Parameterized over the tower geometry (clip_weights.VitConfig):
    ViT-B/32 (flagship, configs #1/#2) and ViT-L/14 (the reference's own
    CLIP model, models/clip.py:33; BASELINE config #3 class).

    ``prune_last_layer`` (default True): the embedding reads only the CLS
    row of the last encoder layer, so that layer computes Q, attention,
    out-proj, LN2 and the MLP for the CLS rows only (_last_layer_cls).
    False runs the full layer on every token — for A/B runs and parity
    tests; it is also what head dims other than 64 get on the GPU.
    """

    prune_last_layer = True

    def __init__(
        self,
        state_dict: dict[str, torch.Tensor] | None = None,
        cfg: cw.VitConfig = cw.VIT_B32,
    ) -> None:
        if state_dict is None:
            state_dict = (
                cw.make_clip_vit_b32_weights() if cfg is cw.VIT_B32
                else cw.make_clip_vit_weights(cfg)
            )
        sd = state_dict
        p = "vision_model."
        super().__init__(sd, cfg, p)
        reg = self.register_buffer
        to_f32 = lambda t: t.float().contiguous()  # noqa: E731
        reg("cls_emb", sd[p + "embeddings.class_embedding"].clone())
        reg("pos_emb", sd[p + "embeddings.position_embedding.weight"].clone())
        reg("pre_ln_w", to_f32(sd[p + "pre_layrnorm.weight"]))
        reg("pre_ln_b", to_f32(sd[p + "pre_layrnorm.bias"]))
        reg("post_ln_w", to_f32(sd[p + "post_layernorm.weight"]))
        reg("post_ln_b", to_f32(sd[p + "post_layernorm.bias"]))
        reg("w_proj", sd["visual_projection.weight"].to(torch.bfloat16).contiguous())

    @torch.no_grad()
    def forward(
        self,
        pixel_values: torch.Tensor | None = None,
        *,
        patches: torch.Tensor | None = None,
        n: int | None = None,
    ) -> torch.Tensor:
        """(N,3,224,224) bf16 -> (N,proj) f32 L2-normalized embeddings.

        Alternatively accepts prebuilt GEMM-ready ``patches``
        [N*g*g, patch_k] bf16 (cc_clip_preprocess_patches output) with
        ``n`` = N, skipping the torch reshape/permute/pad chain.
        """
        cfg = self.cfg
        patches, n = self._patches(pixel_values, patches, n)
        tok_flat = self._linear(patches, self.w_patch, None)  # (n*g*g, hidden)
        seq = (cfg.image // cfg.patch) ** 2 + 1  # patches + CLS
        if tok_flat.is_cuda:
            # fused [CLS; tok] + pos-embed + pre-LN (csrc/cc_ln.hip) — one
            # bandwidth pass instead of the cat/f32-add/cast/LN chain
            lib = hotpath.require_gpu()
            h = torch.empty((n * seq, cfg.hidden), dtype=torch.bfloat16,
                            device=tok_flat.device)
            stream = torch.cuda.current_stream(tok_flat.device).cuda_stream
            hotpath.check(lib.cc_embed_assemble_ln(
                tok_flat.data_ptr(), self.cls_emb.data_ptr(),
                self.pos_emb.data_ptr(), self.pre_ln_w.data_ptr(),
                self.pre_ln_b.data_ptr(), h.data_ptr(), n, seq, cfg.hidden,
                ctypes.c_float(cfg.ln_eps), stream))
            h = h.reshape(n, seq, cfg.hidden)
        else:
            tok = tok_flat.reshape(n, seq - 1, cfg.hidden)
            cls = self.cls_emb.to(tok.dtype).expand(n, 1, cfg.hidden)
            h = torch.cat([cls, tok], dim=1)  # (n, tokens, hidden)
            h = (h.float() + self.pos_emb.unsqueeze(0)).to(torch.bfloat16)
            h = self._ln(h, self.pre_ln_w, self.pre_ln_b)
        # pooling reads only the CLS row of the last layer's output, so
        # that layer runs everything past K/V on the CLS rows alone
        cls_only = (
            self.prune_last_layer and cfg.has_cls
            and (cfg.hidden // self.heads == 64 or not h.is_cuda)
        )
        if cls_only:
            stats = None
            if self._folds(h):
                h, stats = self._encode_folded(h, n, seq, self.layers - 1)
            else:
                h = self._encode(h, n, seq, self.layers - 1)
            cls_rows = self._last_layer_cls(h, self.layers - 1, n, seq, stats)
        else:
            cls_rows = self._encode(h, n, seq)[:, 0]
        pooled = self._ln(cls_rows, self.post_ln_w, self.post_ln_b)
        emb = self._linear(pooled.to(torch.bfloat16), self.w_proj, None).float()
        return emb / torch.linalg.vector_norm(emb, dim=-1, keepdim=True)

    def _last_layer_cls(
        self, h: torch.Tensor, i: int, n: int, seq: int,
        stats: torch.Tensor | None = None,
    ) -> torch.Tensor:
        """Encoder layer ``i`` for the CLS rows only: (n, seq, H) -> (n, H).

        Every token still feeds attention as a key and a value, so LN1 and
        the K/V two thirds of the QKV projection run on all rows.  The Q
        projection, the attention output, out-proj, LN2 and the MLP are
        row-wise, so computing them for row 0 of each frame gives exactly
        the rows the full layer would have produced there.  The CLS rows
        of the LN1 output (A of the Q GEMM) and of ``h`` (residual of
        out-proj) are read in place through row strides.

        With ``stats`` (the row statistics of ``h``, folded route) LN1 is
        not run at all: the K/V GEMM and the Q GEMM read ``h`` itself, the
        Q GEMM its CLS rows and their statistics at a row step of ``seq``.
        LN2 at M = frames stays the LN kernel.
        """
        H = self.cfg.hidden
        hd = H // self.heads
        p = self._layer_params(i)
        w_qkv, b_qkv = p("w_qkv"), p("b_qkv")
        # rows ordered (q, k, v): contiguous slices, no weight copies
        if stats is not None:
            wf, s, c = p("wf_qkv"), p("s_qkv"), p("c_qkv")
            eps = self.cfg.ln_eps
            hf = h.reshape(n * seq, H)
            kv = cc_linear_ln(hf, stats, wf[H:], s[H:], c[H:], 0, eps)
            q = cc_linear_ln(hf, stats, wf[:H], s[:H], c[:H], 0, eps,
                             row_step=seq)
        else:
            y = self._ln(h, p("ln1_w"), p("ln1_b"))
            kv = self._linear(y.reshape(n * seq, H), w_qkv[H:], b_qkv[H:])
            q = self._linear(y[:, 0], w_qkv[:H], b_qkv[:H])
        if kv.is_cuda:
            lib = hotpath.require_gpu()
            attn = torch.empty((n, H), dtype=torch.bfloat16, device=kv.device)
            stream = torch.cuda.current_stream(kv.device).cuda_stream
            hotpath.check(
                lib.cc_attn_cls(
                    q.data_ptr(), kv.data_ptr(),
                    kv.data_ptr() + H * kv.element_size(), 2 * H,
                    attn.data_ptr(), n, seq, self.heads, H,
                    ctypes.c_float(self.scale), stream,
                )
            )
        else:
            kvh = kv.reshape(n, seq, 2, self.heads, hd)
            attn = torch.nn.functional.scaled_dot_product_attention(
                q.reshape(n, 1, self.heads, hd).permute(0, 2, 1, 3),
                kvh[:, :, 0].permute(0, 2, 1, 3),
                kvh[:, :, 1].permute(0, 2, 1, 3),
                scale=self.scale,
            )
            attn = attn.permute(0, 2, 1, 3).reshape(n, H)
        h1 = self._linear(attn, p("w_out"), p("b_out"), residual=h[:, 0])
        y = self._ln(h1, p("ln2_w"), p("ln2_b"))
        y = self._linear(y, p("w_fc1"), p("b_fc1"), act=self.act)
        return self._linear(y, p("w_fc2"), p("b_fc2"), residual=h1)
