"""Cosmos-Embed1 video tower (``cosmos-embed1-224p|336p|448p``) on the MFMA
path: an EVA ViT-g/14 per frame, a learned temporal encoding, a BLIP-2
Q-Former whose 32 queries cross-attend to every token of every frame, a
projection, the mean over the queries and an L2 norm.

The published modelling code and checkpoint are not available offline, so the
tower is specified by its two halves as ``transformers`` defines them, and
the state dict is keyed by their names:

    vision_model.*   Blip2VisionModel  (1408 wide, 39 layers, 16 heads of 88,
                     MLP 6144, patch 14, pre-LN at eps 1e-6, erf-GELU, fused
                     QKV with bias, post_layernorm)
    qformer.*        Blip2QFormerModel (768 wide, 12 post-LN BERT layers, 12
                     heads of 64, MLP 3072, cross-attention to the 1408-wide
                     encoder tokens in every second layer, eps 1e-12)
    query_tokens [32, 768], temporal_encoding [T, 1408], vision_proj.*

Vision half: the shared encoder (vit_encoder.VitEncoderAMD) with the
checkpoint's ``encoder.layers.{i}.self_attn.qkv`` / ``projection`` keys;
patch-embed as GEMM, class token + position table, folded LayerNorms,
cc_attn at head dim 88, and post_layernorm over ALL tokens (cc_layernorm):
the Q-Former reads every one of them.  temporal_encoding[t] is then added
to every token of frame t and a clip's frames are concatenated to
[T*(P+1), 1408].

Q-Former: LayerNorm(query_tokens) does not depend on the input and is
computed once at construction.  Per layer: self-attention over the 32
queries (fused QKV GEMM, cc_attn's small rung), on even layers
cross-attention (Q GEMM from the queries; K and V of ALL cross-attention
layers come from ONE GEMM over the encoder tokens, N = layers/2 * 1536, and
each layer hands cc_attn_cross its column window), and the query FFN with
the erf-GELU epilogue.  Every post-LN is the GEMM's residual epilogue
followed by cc_layernorm at 768.  Every contraction is cc_linear.

Head (O(clips), torch f32): vision_proj on the 32 query rows, their mean,
L2 norm.

Three facts cannot be checked offline: that the temporal
encoding is a learned table added after the vision half, that the head is
the mean over the queries, and the processor's mean / std.  The text tower
is not implemented.
"""

from __future__ import annotations

import ctypes
import dataclasses

import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models.clip_weights import _randn
from cosmos_curate_amd.models.vit_encoder import (
    ACT_CODES,
    VitEncoderAMD,
    cc_layernorm,
    cc_linear,
    patchify,
)


@dataclasses.dataclass(frozen=True)
class CosmosEmbed1Config:
    """Geometry of a variant: Blip2VisionConfig's and Blip2QFormerConfig's
    defaults, the input resolution and the embedding width."""

    name: str
    image: int
    proj: int                  # vision_proj output, the embedding width
    num_frames: int = 8
    # vision half; the names are the ones the shared encoder reads
    hidden: int = 1408
    layers: int = 39
    heads: int = 16
    intermediate: int = 6144
    patch: int = 14
    ln_eps: float = 1e-6
    act: str = "gelu_erf"
    norm: str = "layernorm"
    qk_norm: bool = False
    # Q-Former
    q_hidden: int = 768
    q_layers: int = 12
    q_heads: int = 12
    q_intermediate: int = 3072
    q_cross_every: int = 2     # cross_attention_frequency
    q_ln_eps: float = 1e-12
    num_queries: int = 32
    # the processor's normalisation; not verifiable offline, so a field: the
    # ImageNet constants internvideo2_prep documents for both models
    mean: tuple[float, float, float] = (0.485, 0.456, 0.406)
    std: tuple[float, float, float] = (0.229, 0.224, 0.225)

    @property
    def tokens_per_frame(self) -> int:
        """P + 1: the patches and the class token."""
        return (self.image // self.patch) ** 2 + 1

    @property
    def num_keys(self) -> int:
        return self.num_frames * self.tokens_per_frame

    @property
    def cross_layers(self) -> tuple[int, ...]:
        return tuple(range(0, self.q_layers, self.q_cross_every))


VARIANTS = {
    "224p": CosmosEmbed1Config("cosmos_embed1_224p", image=224, proj=256),
    "336p": CosmosEmbed1Config("cosmos_embed1_336p", image=336, proj=768),
    "448p": CosmosEmbed1Config("cosmos_embed1_448p", image=448, proj=768),
}

_QF_ATTN = ("attention", "crossattention")


def make_cosmos_embed1_weights(cfg: CosmosEmbed1Config) -> dict[str, torch.Tensor]:
    """Deterministic stand-in state dict, keyed as the module docstring says.
    Norm weights are 1 + 0.2 randn so that a dropped one shows; the
    Q-Former's query / key weights are drawn at std 0.05, which puts the
    attention logits at a standard deviation of a few units: at 0.02 every
    softmax is close to uniform and attention without scores would pass."""
    sd: dict[str, torch.Tensor] = {}
    tag = cfg.name + ":"
    H, Q = cfg.hidden, cfg.q_hidden

    def linear(key: str, n_out: int, n_in: int, std: float = 0.02) -> None:
        sd[key + ".weight"] = _randn(tag + key + ".w", n_out, n_in, std=std)
        sd[key + ".bias"] = _randn(tag + key + ".b", n_out)

    def norm(key: str, width: int) -> None:
        sd[key + ".weight"] = 1.0 + _randn(tag + key + ".w", width, std=0.2)
        sd[key + ".bias"] = _randn(tag + key + ".b", width)

    v = "vision_model."
    sd[v + "embeddings.class_embedding"] = _randn(tag + "cls", 1, 1, H)
    sd[v + "embeddings.position_embedding"] = _randn(
        tag + "pos", 1, cfg.tokens_per_frame, H)
    sd[v + "embeddings.patch_embedding.weight"] = _randn(
        tag + "patch", H, 3, cfg.patch, cfg.patch)
    sd[v + "embeddings.patch_embedding.bias"] = _randn(tag + "patch.b", H)
    for i in range(cfg.layers):
        b = f"{v}encoder.layers.{i}."
        norm(b + "layer_norm1", H)
        linear(b + "self_attn.qkv", 3 * H, H)
        sd[b + "self_attn.qkv.bias"][H:2 * H] = 0.0  # Blip2Attention: no k bias
        linear(b + "self_attn.projection", H, H)
        norm(b + "layer_norm2", H)
        linear(b + "mlp.fc1", cfg.intermediate, H)
        linear(b + "mlp.fc2", H, cfg.intermediate)
    norm(v + "post_layernorm", H)
    sd["temporal_encoding"] = _randn(tag + "temporal", cfg.num_frames, H, std=0.5)
    sd["query_tokens"] = _randn(tag + "queries", cfg.num_queries, Q, std=1.0)
    norm("qformer.layernorm", Q)
    for i in range(cfg.q_layers):
        b = f"qformer.encoder.layer.{i}."
        for a in _QF_ATTN[: 2 if i in cfg.cross_layers else 1]:
            n_in = H if a == "crossattention" else Q
            linear(b + a + ".attention.query", Q, Q, std=0.05)
            linear(b + a + ".attention.key", Q, n_in, std=0.05)
            linear(b + a + ".attention.value", Q, n_in)
            linear(b + a + ".output.dense", Q, Q)
            norm(b + a + ".output.LayerNorm", Q)
        linear(b + "intermediate_query.dense", cfg.q_intermediate, Q)
        linear(b + "output_query.dense", Q, cfg.q_intermediate)
        norm(b + "output_query.LayerNorm", Q)
    linear("vision_proj", cfg.proj, Q)
    return sd


class CosmosEmbed1TowerAMD(VitEncoderAMD):
    """(B, T, 3, image, image) pixels or prebuilt patch rows -> (B, proj) f32
    unit-norm video embeddings.  ``cross_splits`` is handed to cc_attn_cross
    (0: its plan's choice)."""

    cross_splits = 0

    def __init__(self, sd: dict[str, torch.Tensor], cfg: CosmosEmbed1Config) -> None:
        if not hotpath.attn_cross_supported(cfg.q_heads, cfg.q_hidden):
            msg = (f"Cosmos-Embed1 tower: cc_attn_cross does not take "
                   f"{cfg.q_heads} heads at width {cfg.q_hidden}")
            raise ValueError(msg)
        v = "vision_model."
        pos = sd[v + "embeddings.position_embedding"]
        if tuple(pos.shape) != (1, cfg.tokens_per_frame, cfg.hidden):
            msg = (f"Cosmos-Embed1 tower: position table {tuple(pos.shape)} does "
                   f"not match image {cfg.image} (needs (1, "
                   f"{cfg.tokens_per_frame}, {cfg.hidden})); interpolating a "
                   "position table is not implemented")
            raise ValueError(msg)
        if tuple(sd["temporal_encoding"].shape) != (cfg.num_frames, cfg.hidden):
            msg = (f"Cosmos-Embed1 tower: temporal_encoding "
                   f"{tuple(sd['temporal_encoding'].shape)} is not "
                   f"({cfg.num_frames}, {cfg.hidden})")
            raise ValueError(msg)
        super().__init__(sd, cfg, v)
        reg = self.register_buffer
        f32 = lambda t: t.float().contiguous()  # noqa: E731
        bf16 = lambda t: t.to(torch.bfloat16).contiguous()  # noqa: E731
        reg("b_patch", f32(sd[v + "embeddings.patch_embedding.bias"]))
        reg("cls_token", f32(sd[v + "embeddings.class_embedding"].reshape(1, 1, -1)))
        reg("pos_embed", f32(pos))
        reg("post_ln_w", f32(sd[v + "post_layernorm.weight"]))
        reg("post_ln_b", f32(sd[v + "post_layernorm.bias"]))
        reg("temporal", f32(sd["temporal_encoding"]))

        Q = cfg.q_hidden
        self.q_scale = (Q // cfg.q_heads) ** -0.5
        self.q_act = ACT_CODES["gelu_erf"]
        # LayerNorm(query_tokens): input-independent, so once, in f32
        reg("q0", bf16(torch.nn.functional.layer_norm(
            sd["query_tokens"].float().reshape(-1, Q), (Q,),
            sd["qformer.layernorm.weight"].float(),
            sd["qformer.layernorm.bias"].float(), eps=cfg.q_ln_eps)))
        kv_w, kv_b = [], []
        for i in range(cfg.q_layers):
            b = f"qformer.encoder.layer.{i}."
            qkv = [b + f"attention.attention.{x}." for x in ("query", "key", "value")]
            reg(f"qw_qkv_{i}", bf16(torch.cat([sd[x + "weight"] for x in qkv])))
            reg(f"qb_qkv_{i}", f32(torch.cat([sd[x + "bias"] for x in qkv])))
            outs = [("out", "attention.output"), ("fc2", "output_query")]
            if i in cfg.cross_layers:
                x = b + "crossattention.attention."
                reg(f"qw_xq_{i}", bf16(sd[x + "query.weight"]))
                reg(f"qb_xq_{i}", f32(sd[x + "query.bias"]))
                kv_w += [sd[x + "key.weight"], sd[x + "value.weight"]]
                kv_b += [sd[x + "key.bias"], sd[x + "value.bias"]]
                outs.append(("xout", "crossattention.output"))
            for name, key in outs:
                reg(f"qw_{name}_{i}", bf16(sd[b + key + ".dense.weight"]))
                reg(f"qb_{name}_{i}", f32(sd[b + key + ".dense.bias"]))
                reg(f"qln_{name}_w_{i}", f32(sd[b + key + ".LayerNorm.weight"]))
                reg(f"qln_{name}_b_{i}", f32(sd[b + key + ".LayerNorm.bias"]))
            reg(f"qw_fc1_{i}", bf16(sd[b + "intermediate_query.dense.weight"]))
            reg(f"qb_fc1_{i}", f32(sd[b + "intermediate_query.dense.bias"]))
        # [Wk; Wv] of every cross-attention layer, one below the other
        reg("qw_kv_all", bf16(torch.cat(kv_w)))
        reg("qb_kv_all", f32(torch.cat(kv_b)))
        reg("vproj_w", f32(sd["vision_proj.weight"]))
        reg("vproj_b", f32(sd["vision_proj.bias"]))

    def _layer_weights(
        self, sd: dict[str, torch.Tensor], i: int
    ) -> dict[str, torch.Tensor | None]:
        b = f"{self.prefix}encoder.layers.{i}."
        return {
            "w_qkv": sd[b + "self_attn.qkv.weight"],
            "b_qkv": sd[b + "self_attn.qkv.bias"],
            "w_out": sd[b + "self_attn.projection.weight"],
            "b_out": sd[b + "self_attn.projection.bias"],
            "ln1_w": sd[b + "layer_norm1.weight"], "ln1_b": sd[b + "layer_norm1.bias"],
            "ln2_w": sd[b + "layer_norm2.weight"], "ln2_b": sd[b + "layer_norm2.bias"],
            "w_fc1": sd[b + "mlp.fc1.weight"], "b_fc1": sd[b + "mlp.fc1.bias"],
            "w_fc2": sd[b + "mlp.fc2.weight"], "b_fc2": sd[b + "mlp.fc2.bias"],
        }

    def _post_ln(self, x: torch.Tensor, residual: torch.Tensor, name: str,
                 i: int) -> torch.Tensor:
        """LayerNorm(dense(x) + residual) of Q-Former layer ``i``: the
        GEMM's residual epilogue, then cc_layernorm."""
        g = lambda n: getattr(self, f"{n}_{i}")  # noqa: E731
        y = cc_linear(x, g(f"qw_{name}"), g(f"qb_{name}"), residual=residual)
        return cc_layernorm(y, g(f"qln_{name}_w"), g(f"qln_{name}_b"),
                            self.cfg.q_ln_eps)

    def _query_attention(self, qkv: torch.Tensor, n: int) -> torch.Tensor:
        """Self-attention of the queries, (n*32, 3*768) fused QKV rows ->
        (n*32, 768): cc_attn, whose plan puts 32 tokens on the small rung."""
        cfg = self.cfg
        lib = hotpath.require_gpu()
        attn = torch.empty((qkv.shape[0], cfg.q_hidden), dtype=torch.bfloat16,
                           device=qkv.device)
        stream = torch.cuda.current_stream(qkv.device).cuda_stream
        hotpath.check(lib.cc_attn(
            qkv.data_ptr(), attn.data_ptr(), n, cfg.num_queries, cfg.q_heads,
            cfg.q_hidden, ctypes.c_float(self.q_scale), stream))
        return attn

    def _qformer(self, enc: torch.Tensor, n: int) -> torch.Tensor:
        """Encoder tokens (n*nk, 1408) -> the queries' last hidden state
        (n*32, 768)."""
        cfg = self.cfg
        Q, nq, nk = cfg.q_hidden, cfg.num_queries, cfg.num_keys
        kv_all = cc_linear(enc, self.qw_kv_all, self.qb_kv_all)
        h = self.q0.repeat(n, 1)
        for i in range(cfg.q_layers):
            g = lambda name: getattr(self, f"{name}_{i}")  # noqa: E731
            qkv = cc_linear(h, g("qw_qkv"), g("qb_qkv"))
            h = self._post_ln(self._query_attention(qkv, n), h, "out", i)
            if i in cfg.cross_layers:
                j = cfg.cross_layers.index(i)
                qx = cc_linear(h, g("qw_xq"), g("qb_xq"))
                ax = hotpath.attn_cross(
                    qx, kv_all[:, 2 * Q * j: 2 * Q * (j + 1)], n, nq, nk,
                    cfg.q_heads, scale=self.q_scale, splits=self.cross_splits)
                h = self._post_ln(ax, h, "xout", i)
            y = cc_linear(h, g("qw_fc1"), g("qb_fc1"), act=self.q_act)
            h = self._post_ln(y, h, "fc2", i)
        return h

    @torch.no_grad()
    def forward(
        self,
        pixel_values: torch.Tensor | None = None,
        *,
        patches: torch.Tensor | None = None,
        n: int | None = None,
    ) -> torch.Tensor:
        """``pixel_values`` (B, T, 3, image, image), or ``patches``
        [B*T*P, patch_k] bf16 (cc_clip_preprocess_patches output, frames in
        (clip, time) order) with ``n`` = B clips."""
        cfg = self.cfg
        H, T, seq = cfg.hidden, cfg.num_frames, cfg.tokens_per_frame
        if patches is None:
            want = (T, 3, cfg.image, cfg.image)
            if pixel_values.dim() != 5 or tuple(pixel_values.shape[1:]) != want:
                msg = (f"Cosmos-Embed1 tower: expected (B, {T}, 3, {cfg.image}, "
                       f"{cfg.image}) pixels, got {tuple(pixel_values.shape)}")
                raise ValueError(msg)
            n = pixel_values.shape[0]
            patches = patchify(pixel_values.flatten(0, 1), cfg, self.patch_k)
        else:
            assert n is not None
            assert patches.shape == (n * T * (seq - 1), self.patch_k)
        frames = n * T
        tok = cc_linear(patches, self.w_patch, self.b_patch)
        h = torch.cat([self.cls_token.to(torch.bfloat16).expand(frames, 1, H),
                       tok.reshape(frames, seq - 1, H)], dim=1)
        h = (h.float() + self.pos_embed).to(torch.bfloat16)
        h = self._encode(h, frames, seq)
        h = cc_layernorm(h, self.post_ln_w, self.post_ln_b, cfg.ln_eps)
        enc = (h.reshape(n, T, seq, H).float()
               + self.temporal[None, :, None, :]).to(torch.bfloat16)
        q = self._qformer(enc.reshape(n * T * seq, H), n)
        e = q.float() @ self.vproj_w.T + self.vproj_b
        e = e.reshape(n, cfg.num_queries, cfg.proj).mean(dim=1)
        return e / torch.linalg.vector_norm(e, dim=-1, keepdim=True)
