"""Plain-torch fp32 reference of the InternVideo2 vision tower.

Written from the model description, not from the product
module: it loads the same state dict as
models/internvideo2_vit.InternVideo2VisionTowerAMD and is what the GPU
parity tests compare against.  Moved to a GPU in bf16
(``InternVideo2Ref(sd, cfg).to("cuda", torch.bfloat16)``) it is also the
torch yardstick of tools/iv2_bench.py.

forward: (B, T, 3, image, image) float pixels -> (B, proj) unit-norm.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """Normalise in f32, cast back to x's type, multiply by the weight."""
    xf = x.float()
    xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return w * xf.to(x.dtype)


class InternVideo2Ref(torch.nn.Module):
    def __init__(self, sd: dict[str, torch.Tensor], cfg) -> None:
        super().__init__()
        self.cfg = cfg
        for k, v in sd.items():
            self.register_buffer(k.replace(".", "__"), v.clone().float())

    def p(self, key: str) -> torch.Tensor:
        return getattr(self, key.replace(".", "__"))

    def block(self, x: torch.Tensor, i: int) -> torch.Tensor:
        cfg = self.cfg
        b = f"vision_encoder.blocks.{i}."
        B, N, H = x.shape
        hd = H // cfg.heads
        y = rmsnorm(x, self.p(b + "norm1.weight"), cfg.rms_eps)
        q, k, v = F.linear(y, self.p(b + "attn.qkv.weight")).chunk(3, dim=-1)
        # QK-norm over the whole hidden width, before the head split
        q = rmsnorm(q, self.p(b + "attn.q_norm.weight"), cfg.rms_eps)
        k = rmsnorm(k, self.p(b + "attn.k_norm.weight"), cfg.rms_eps)
        q, k, v = (t.reshape(B, N, cfg.heads, hd).transpose(1, 2) for t in (q, k, v))
        a = F.scaled_dot_product_attention(q, k, v, scale=hd ** -0.5)
        a = a.transpose(1, 2).reshape(B, N, H)
        a = F.linear(a, self.p(b + "attn.proj.weight"), self.p(b + "attn.proj.bias"))
        x = x + self.p(b + "ls1.gamma") * a
        y = rmsnorm(x, self.p(b + "norm2.weight"), cfg.rms_eps)
        y = F.linear(y, self.p(b + "mlp.fc1.weight"), self.p(b + "mlp.fc1.bias"))
        y = F.gelu(y, approximate="none")
        y = F.linear(y, self.p(b + "mlp.fc2.weight"), self.p(b + "mlp.fc2.bias"))
        return x + self.p(b + "ls2.gamma") * y

    def pool(self, x: torch.Tensor) -> torch.Tensor:
        """clip_projector: one query per clip (the LayerNorm of the token
        mean) cross-attending over LayerNorm_k / LayerNorm_v of the tokens."""
        cfg = self.cfg
        cp = "vision_encoder.clip_projector."
        B, N, H = x.shape
        hd = H // cfg.pool_heads

        def ln(t: torch.Tensor, n: str) -> torch.Tensor:
            return F.layer_norm(t, (H,), self.p(cp + f"norm1_{n}.weight"),
                                self.p(cp + f"norm1_{n}.bias"), cfg.pool_ln_eps)

        def lin(t: torch.Tensor, n: str) -> torch.Tensor:
            return F.linear(t, self.p(cp + f"cross_attn.{n}.weight"),
                            self.p(cp + f"cross_attn.{n}_bias"))

        q = lin(ln(x.mean(1, keepdim=True), "q"), "q")
        k = lin(ln(x, "k"), "k")
        v = lin(ln(x, "v"), "v")
        q = q.reshape(B, 1, cfg.pool_heads, hd).transpose(1, 2) * hd ** -0.5
        k = k.reshape(B, N, cfg.pool_heads, hd).transpose(1, 2)
        v = v.reshape(B, N, cfg.pool_heads, hd).transpose(1, 2)
        att = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        o = (att @ v).transpose(1, 2).reshape(B, H)
        return F.linear(o, self.p(cp + "cross_attn.proj.weight"),
                        self.p(cp + "cross_attn.proj.bias"))

    @torch.no_grad()
    def forward(self, pixels: torch.Tensor, layers: int | None = None) -> torch.Tensor:
        cfg = self.cfg
        ve = "vision_encoder."
        B, T = pixels.shape[:2]
        assert T == cfg.num_frames
        w = self.p(ve + "patch_embed.proj.weight")
        dt = w.dtype
        # tubelet 1: the 3-D conv is a per-frame 2-D conv
        tok = F.conv2d(pixels.to(dt).flatten(0, 1), w[:, :, 0],
                       self.p(ve + "patch_embed.proj.bias"), stride=cfg.patch)
        tok = tok.flatten(2).transpose(1, 2).reshape(B, -1, cfg.hidden)
        x = torch.cat([self.p(ve + "cls_token").expand(B, -1, -1), tok], dim=1)
        x = x + self.p(ve + "pos_embed")
        for i in range(cfg.layers if layers is None else layers):
            x = self.block(x, i)
        e = self.pool(x)  # no final norm
        e = F.linear(e, self.p("vision_proj.weight"), self.p("vision_proj.bias"))
        e = e.float()
        return e / torch.linalg.vector_norm(e, dim=-1, keepdim=True)
