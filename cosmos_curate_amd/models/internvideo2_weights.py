"""InternVideo2 vision-tower geometry and deterministic stand-in weights.

The tower is the vision encoder ``pretrain_internvideo2_1b_patch14_224``
plus the ``vision_proj`` head of the InternVideo2 stage-2 model: 40 blocks
of hidden 1408 (16 heads of 88, MLP 6144), RMSNorm, QK-normalisation,
LayerScale, erf-GELU, an attention-pooling ``clip_projector`` to 768 and a
linear ``vision_proj`` to 512.

Checkpoints are not available offline, so — like clip_weights — every
tensor comes from its own name-seeded generator and the fp32 reference
(tests/iv2_ref.py) loads the same dict.  Keys are spelled as the
checkpoint spells them (``vision_encoder.blocks.{i}.attn.qkv.weight`` ...),
so a local ``.pth`` loads through the same constructor.

Two departures from the model's initial values, both so that parity tests
can see a broken block:
- LayerScale gammas are uniform in [0.5, 1.5].  The model initialises them
  to 1e-5, which scales both branches of every block to nothing.
- norm weights are 1 + 0.2 * randn rather than ones, so a dropped or
  swapped weight shows.
"""

from __future__ import annotations

import dataclasses

import torch

from cosmos_curate_amd.models.clip_weights import _randn, _seed_for


@dataclasses.dataclass(frozen=True)
class InternVideo2Config:
    """Vision-tower geometry (PretrainInternVideo2 constructor fields)."""

    name: str
    hidden: int
    layers: int
    heads: int
    intermediate: int
    patch: int
    pool_dim: int              # clip_projector output (clip_embed_dim)
    proj: int                  # vision_proj output, the embedding width
    image: int = 224
    num_frames: int = 4        # T; tubelet_size is 1
    pool_heads: int = 16       # attn_pool_num_heads
    rms_eps: float = 1e-6
    pool_ln_eps: float = 1e-5
    # what the shared encoder layer (vit_encoder) reads besides the geometry
    act: str = "gelu_erf"
    norm: str = "rmsnorm"
    qk_norm: bool = True

    @property
    def ln_eps(self) -> float:
        """The block-norm eps under the name the shared encoder reads."""
        return self.rms_eps

    @property
    def tokens_per_frame(self) -> int:
        return (self.image // self.patch) ** 2

    @property
    def num_pos(self) -> int:
        """CLS + T * (image/patch)^2."""
        return 1 + self.num_frames * self.tokens_per_frame


# InternVideo2-1B, stage 2.  num_frames 4 is the embedding pipeline's
# setting; 8 is the checkpoint's native one
# (dataclasses.replace(INTERNVIDEO2_1B, num_frames=8)).
INTERNVIDEO2_1B = InternVideo2Config(
    "internvideo2_1b", hidden=1408, layers=40, heads=16, intermediate=6144,
    patch=14, pool_dim=768, proj=512)


def _uniform(name: str, n: int, lo: float, hi: float) -> torch.Tensor:
    g = torch.Generator().manual_seed(_seed_for(name))
    return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float32)


def _norm_weight(name: str, n: int) -> torch.Tensor:
    return 1.0 + _randn(name, n, std=0.2)


def make_internvideo2_weights(
    cfg: InternVideo2Config = INTERNVIDEO2_1B,
) -> dict[str, torch.Tensor]:
    """Deterministic state dict of this geometry, checkpoint key names."""
    sd: dict[str, torch.Tensor] = {}
    tag = f"{cfg.name}:"
    ve = "vision_encoder."
    H = cfg.hidden
    sd[ve + "patch_embed.proj.weight"] = _randn(
        tag + "patch", H, 3, 1, cfg.patch, cfg.patch)
    sd[ve + "patch_embed.proj.bias"] = _randn(tag + "patch.b", H)
    sd[ve + "cls_token"] = _randn(tag + "cls", 1, 1, H)
    sd[ve + "pos_embed"] = _randn(tag + "pos", 1, cfg.num_pos, H)
    for i in range(cfg.layers):
        b = f"{ve}blocks.{i}."
        t = f"{tag}b{i}."
        sd[b + "norm1.weight"] = _norm_weight(t + "norm1", H)
        sd[b + "attn.qkv.weight"] = _randn(t + "qkv.w", 3 * H, H)  # no bias
        sd[b + "attn.q_norm.weight"] = _norm_weight(t + "q_norm", H)
        sd[b + "attn.k_norm.weight"] = _norm_weight(t + "k_norm", H)
        sd[b + "attn.proj.weight"] = _randn(t + "proj.w", H, H)
        sd[b + "attn.proj.bias"] = _randn(t + "proj.b", H)
        sd[b + "ls1.gamma"] = _uniform(t + "ls1", H, 0.5, 1.5)
        sd[b + "norm2.weight"] = _norm_weight(t + "norm2", H)
        sd[b + "mlp.fc1.weight"] = _randn(t + "fc1.w", cfg.intermediate, H)
        sd[b + "mlp.fc1.bias"] = _randn(t + "fc1.b", cfg.intermediate)
        sd[b + "mlp.fc2.weight"] = _randn(t + "fc2.w", H, cfg.intermediate)
        sd[b + "mlp.fc2.bias"] = _randn(t + "fc2.b", H)
        sd[b + "ls2.gamma"] = _uniform(t + "ls2", H, 0.5, 1.5)
    cp = ve + "clip_projector."
    for n in "qkv":
        sd[cp + f"norm1_{n}.weight"] = _norm_weight(f"{tag}pool.norm_{n}.w", H)
        sd[cp + f"norm1_{n}.bias"] = _randn(f"{tag}pool.norm_{n}.b", H)
        sd[cp + f"cross_attn.{n}.weight"] = _randn(f"{tag}pool.{n}.w", H, H)
        sd[cp + f"cross_attn.{n}_bias"] = _randn(f"{tag}pool.{n}.b", H)
    sd[cp + "cross_attn.proj.weight"] = _randn(tag + "pool.proj.w", cfg.pool_dim, H)
    sd[cp + "cross_attn.proj.bias"] = _randn(tag + "pool.proj.b", cfg.pool_dim)
    sd["vision_proj.weight"] = _randn(tag + "vproj.w", cfg.proj, cfg.pool_dim)
    sd["vision_proj.bias"] = _randn(tag + "vproj.b", cfg.proj)
    return sd


def make_internvideo2_weights_stress(
    cfg: InternVideo2Config = INTERNVIDEO2_1B,
) -> dict[str, torch.Tensor]:
    """The stand-in dict with outlier channels: in every block two LayerScale
    channels (one of ls1, one of ls2) and two norm weights (one of norm1, one
    of norm2) at 8.0 — the outlier-gain pattern of
    clip_weights.make_clip_vit_weights_stress."""
    sd = make_internvideo2_weights(cfg)
    for i in range(cfg.layers):
        b = f"vision_encoder.blocks.{i}."
        for j, key in enumerate(("ls1.gamma", "ls2.gamma", "norm1.weight",
                                 "norm2.weight")):
            g = torch.Generator().manual_seed(
                _seed_for(f"{cfg.name}:stress:{i}:{key}"))
            ch = int(torch.randint(cfg.hidden, (1,), generator=g))
            t = sd[b + key].clone()
            t[ch] = 8.0
            sd[b + key] = t
    return sd


def load_internvideo2_state_dict(path: str) -> dict[str, torch.Tensor]:
    """A local InternVideo2 stage-2 checkpoint (``.pth``/``.pt``) reduced to
    the keys the tower reads: ``vision_encoder.*`` (without the CLIP-teacher
    decoders) and ``vision_proj.*``.  No network: the operator provides the
    file."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    for wrap in ("module", "model"):
        if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    out = {
        k: v.float() for k, v in sd.items()
        if k.startswith(("vision_encoder.", "vision_proj."))
        and ".clip_decoder" not in k and ".final_clip_decoder" not in k
    }
    if "vision_encoder.pos_embed" not in out:
        msg = f"{path} holds no vision_encoder.pos_embed: not an InternVideo2 checkpoint"
        raise ValueError(msg)
    return out
