"""CPU restatement of the TransNetV2 head kernels (csrc/cc_tnheads.hip) and
the tolerances their tests use.  All torch / numpy; nothing here looks at the
code under test.

Each function restates one kernel's arithmetic, in the dtype of its inputs
(f32 as the kernels compute, f64 as the yardstick).  The order of the sums
inside is torch's, not the kernels': that difference is what the bounds below
allow, and only the histogram is held to bit-equality.

Bounds.  An f32 result in which every term passes through at most ``K``
roundings (a ``K``-term chain, or sums nested to that depth), with magnitude
sum ``S`` (the same expression over absolute values), is within ``K * 2^-24 *
S`` of the exact value to first order; ``sum_bound`` allows twice that.  A
normalised output adds ``4 * 2^-24 * |want|`` for the root and the division.
"""

from __future__ import annotations

import numpy as np
import torch
from torch.nn import functional as F

U = 2.0 ** -24  # unit roundoff of f32
LOOKUP, HALF = 101, 50


def rb(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def sum_bound(k: int, abs_sum: torch.Tensor) -> torch.Tensor:
    """Allowed |got - want| of an f32 sum of depth ``k`` with magnitude sum
    ``abs_sum``: 2 K 2^-24 S."""
    return 2.0 * k * U * abs_sum


def normalized_bound(want_e: torch.Tensor, e_bound: torch.Tensor) -> torch.Tensor:
    """Allowed |got - want| of ``e / max(|e|_2, 1e-12)`` over the last axis,
    given the elementwise bound on ``e``: with n = |e|_2, d(e/n) <= de/n +
    |e|/n * dn/n, dn <= |de|_2 plus the f32 sum of squares (depth = width + 1,
    halved by the root), plus 4 * 2^-24 |want| for the root and the division."""
    n = want_e.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    width = want_e.shape[-1]
    rel_n = e_bound.norm(dim=-1, keepdim=True) / n + (width + 1) * U
    return e_bound / n + (want_e.abs() / n) * (rel_n + 4.0 * U)


# ---- 1. colour histogram -----------------------------------------------------

def hist512(frames_u8) -> np.ndarray:
    """u8 [n, pixels, 3] -> f32 [n, 512], every operation in f32 as the
    kernel does it: integer counts, sqrt of the f32 sum of squares, one
    division."""
    f = np.asarray(frames_u8).astype(np.int64)
    bins = ((f[..., 0] >> 5) << 6) | ((f[..., 1] >> 5) << 3) | (f[..., 2] >> 5)
    c = np.stack([np.bincount(b, minlength=512) for b in bins])
    sq = (c * c).sum(axis=1)
    assert sq.max() <= 2 ** 24, "the sum of squared counts must stay exact in f32"
    norm = np.maximum(np.sqrt(sq.astype(np.float32)), np.float32(1e-12))
    out = c.astype(np.float32) / norm[:, None]
    assert out.dtype == np.float32
    return out


# ---- 2. frame-similarity embedding -------------------------------------------

def framesim_means(maps: list[torch.Tensor]) -> torch.Tensor:
    """maps [n, hw_i, C_i] -> [n, sum C_i]: spatial means in map order."""
    return torch.cat([m.sum(dim=1) / m.shape[1] for m in maps], dim=1)


def framesim_project(maps: list[torch.Tensor], proj_wt: torch.Tensor,
                     proj_b: torch.Tensor) -> torch.Tensor:
    """The embedding before its normalisation, [n, 128]."""
    return framesim_means(maps) @ proj_wt + proj_b


def framesim_embed(maps: list[torch.Tensor], proj_wt: torch.Tensor,
                   proj_b: torch.Tensor) -> torch.Tensor:
    e = framesim_project(maps, proj_wt, proj_b)
    return e / e.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def framesim_project_bound(maps: list[torch.Tensor], proj_wt: torch.Tensor,
                           proj_b: torch.Tensor) -> torch.Tensor:
    """Bound on the projection: a pixel's value is rounded by at most hw adds
    and the division of its mean, then the product and K adds of the chain,
    then the bias."""
    depth = max(m.shape[1] for m in maps) + proj_wt.shape[0] + 3
    s = framesim_project([m.abs() for m in maps], proj_wt.abs(), proj_b.abs())
    return sum_bound(depth, s)


# ---- 3. similarity band + Linear(101, 128) + relu -------------------------------

def band(x: torch.Tensor) -> torch.Tensor:
    """x [B, T, D] -> s [B, T, 101]: s[b,t,j] = <x[b,t], x[b,t+j-50]>, 0 where
    the partner lies outside the window.  Only the band, never T x T."""
    t = x.shape[1]
    xp = F.pad(x, [0, 0, HALF, HALF])
    return torch.stack([(x * xp[:, j:j + t]).sum(dim=-1) for j in range(LOOKUP)], dim=-1)


def simband_fc(x: torch.Tensor, fc_wt: torch.Tensor, fc_b: torch.Tensor) -> torch.Tensor:
    """relu(band(x) @ fc_wt + fc_b), fc_wt [101, 128] -> [B, T, 128]."""
    return F.relu(band(x) @ fc_wt + fc_b)


def simband_fc_bound(x: torch.Tensor, fc_wt: torch.Tensor, fc_b: torch.Tensor) -> torch.Tensor:
    """D roundings in a band entry, then the product, 101 adds and the bias;
    relu only shrinks a difference."""
    s = band(x.abs()) @ fc_wt.abs() + fc_b.abs()
    return sum_bound(x.shape[-1] + LOOKUP + 2, s)


# ---- 4. fc1, split bf16 ----------------------------------------------------------

def split(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """hi = bf16(x), lo = bf16(x - hi), both returned in x's dtype (x is f32
    or holds f32 values)."""
    hi = rb(x.float())
    lo = rb(x.float() - hi)
    return hi.to(x.dtype), lo.to(x.dtype)


def fc1_split(hd: torch.Tensor, feat: torch.Tensor, w_hi: torch.Tensor,
              w_lo: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The kernel's five products, before the relu: feat.w_hi + feat.w_lo +
    hd_hi.w_hi + hd_hi.w_lo + hd_lo.w_hi + bias.  hd [M, KH], feat [M, KF]
    (bf16 values), w_* [N, KH+KF] (bf16 values); all in one dtype."""
    kh = hd.shape[1]
    hd_hi, hd_lo = split(hd)
    acc = feat @ w_hi[:, kh:].T
    acc = acc + feat @ w_lo[:, kh:].T
    acc = acc + hd_hi @ w_hi[:, :kh].T
    acc = acc + hd_hi @ w_lo[:, :kh].T
    acc = acc + hd_lo @ w_hi[:, :kh].T
    return acc + bias


def fc1_relu(hd, feat, w_hi, w_lo, bias) -> torch.Tensor:
    return F.relu(fc1_split(hd, feat, w_hi, w_lo, bias))


def fc1_abs_sum(hd, feat, w_hi, w_lo, bias) -> torch.Tensor:
    """S of the split sum: the same five products over magnitudes."""
    kh = hd.shape[1]
    hd_hi, hd_lo = (t.abs() for t in split(hd))
    w_hi, w_lo, feat = w_hi.abs(), w_lo.abs(), feat.abs()
    return (feat @ (w_hi + w_lo)[:, kh:].T + hd_hi @ (w_hi + w_lo)[:, :kh].T
            + hd_lo @ w_hi[:, :kh].T + bias.abs())


# ---- 5. classifier -------------------------------------------------------------------

def cls_sigmoid(y: torch.Tensor, w: torch.Tensor, b: float) -> torch.Tensor:
    return torch.sigmoid(y @ w + b)


def cls_sigmoid_bound(y: torch.Tensor, w: torch.Tensor, b: float,
                      want: torch.Tensor) -> torch.Tensor:
    """The logit is a sum of depth N + 1 (a lane's chain, the tree, the bias);
    the sigmoid's slope is at most 1/4; then expf (2 ulp), one add, one
    division: 8 * 2^-24 |want| covers them."""
    s = y.abs() @ w.abs() + abs(b)
    return sum_bound(y.shape[-1] + 1, s) / 4 + 8.0 * U * want.abs()


# ---- the heads end to end --------------------------------------------------------------

def heads(packed, frames_u8: torch.Tensor, feats_cl: list[torch.Tensor]) -> torch.Tensor:
    """``NativeHeads`` restated in f32: frames u8 (B,T,H,W,3), features
    channels-last (B,T,h,w,C) holding bf16 values -> (B,T,1).  ``packed`` is
    a ``PackedHeads``."""
    b, t = frames_u8.shape[:2]
    n = b * t
    hist = torch.from_numpy(hist512(frames_u8.reshape(n, -1, 3).numpy()))
    maps = [f.float().reshape(n, -1, f.shape[-1]) for f in feats_cl]
    emb = framesim_embed(maps, packed.proj_wt, packed.proj_b)
    hd = torch.cat([
        simband_fc(hist.view(b, t, 512), packed.hist_fc_wt, packed.hist_fc_b),
        simband_fc(emb.view(b, t, -1), packed.sim_fc_wt, packed.sim_fc_b)], dim=-1)
    y = fc1_relu(hd.view(n, -1), feats_cl[-1].float().reshape(n, -1),
                 packed.fc1_hi.float(), packed.fc1_lo.float(), packed.fc1_b)
    return cls_sigmoid(y, packed.cls_w, packed.cls_b).view(b, t, 1)
