"""Attention inputs that make the softmax scores matter, plain references,
and deliberately wrong variants.  CPU only, torch only; shared by
test_attn_ref_cpu.py (which proves the checker's power without a GPU) and
test_gpu_attn_scores.py (which holds the kernels to it).

With QKV ~ 0.5 randn the logits have a standard deviation of about 0.25,
the softmax is close to uniform and the output is close to the mean of V:
an assertion of 2e-2 then passes attention without a softmax.  The families
below put the mass of every row on a few keys (`peaked`), and each of the
others aims at one intricate part of the kernels: the mask at seq
(`neg_offset`), the max subtraction (`pos_offset`), the running max and the
rescale of O (`rising`, `falling`), the last key and its tile (`last_key`),
the denominator (`zero_q`).

Everything is [n, heads, seq, hd]; inputs are bf16, deterministic from a
seed; scale = hd**-0.5.
"""

import torch

N, HEADS = 2, 3
HDS = [64, 72, 80, 88, 96, 104, 112, 120, 128]
TILE = 64  # key tile of the online-softmax kernels

FAMILIES = ("peaked", "neg_offset", "pos_offset", "rising", "falling",
            "last_key", "zero_q")

# Standard deviation of q and k in `peaked`; the logits' is SIGMA**2 = 1.8, so
# a handful of keys carry each row.  Chosen where a scale off by 5 % shows
# best against BOUND: at 1.0 the rows are too flat for the scale to matter
# (smallest error of wrong_scale over PROBLEMS 0.015), from 1.75 the short
# rows turn one-hot, which no scale changes (0.023 at 1.75 and 2.0, 0.019 at
# 2.5), and from 1.4 the emulation's own error in `rising` grows past the
# floor that `last_key` sets (0.0043 at 1.4, 0.0052 at 1.5), and BOUND with it.
SIGMA = 1.35


def scale_of(hd):
    return hd ** -0.5


def make_inputs(family, seq, hd, seed, n=N, heads=HEADS):
    """bf16 q, k, v of shape [n, heads, seq, hd]."""
    g = torch.Generator().manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32)

    q = SIGMA * randn(n, heads, seq, hd)
    k = SIGMA * randn(n, heads, seq, hd)
    v = randn(n, heads, seq, hd)
    # a per-head direction with a.a * scale = 8
    a = randn(1, heads, 1, hd)
    a = a * (8.0 / scale_of(hd)) ** 0.5 / a.norm(dim=-1, keepdim=True)
    tile = (torch.arange(seq) // TILE).float().reshape(1, 1, seq, 1)
    if family == "peaked":
        pass
    elif family == "neg_offset":  # every real logit about -8
        q, k = q + a, k - a
    elif family == "pos_offset":  # every logit about +32
        q, k = q + 2 * a, k + 2 * a
    elif family == "rising":  # the row max moves up by 4 at every key tile
        q, k = q + a, k + 0.5 * tile * a
    elif family == "falling":  # the row max is settled in tile 0
        q, k = q + a, k - 0.5 * tile * a
    elif family == "last_key":  # every row's mass on key seq-1
        q = 0.3 * randn(n, heads, seq, hd) + a
        k = 0.3 * randn(n, heads, seq, hd)
        k[:, :, seq - 1] = a[:, :, 0]
        v[:, :, seq - 1] = 4.0
    elif family == "zero_q":  # uniform softmax: the output is the mean of V
        q = torch.zeros_like(q)
    else:
        raise ValueError(family)
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)


def old_inputs(n, heads, seq, hd, seed):
    """What the sdpa-parity tests feed: torch.manual_seed(seed), then fused
    QKV rows of 0.5 randn.  Returned as q, k, v [n, heads, seq, hd]."""
    g = torch.Generator().manual_seed(seed)  # the same stream as the global one
    qkv = (torch.randn(n * seq, 3 * heads * hd, generator=g) * 0.5).to(torch.bfloat16)
    return tuple(qkv.reshape(n, seq, 3, heads, hd)[:, :, i].permute(0, 2, 1, 3)
                 for i in range(3))


def fuse_qkv(q, k, v):
    """[n, heads, seq, hd] x 3 -> the fused [n*seq, 3*hidden] rows the
    kernels read (row = token; Q, K, V sections, heads inside each)."""
    n, heads, seq, hd = q.shape
    qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4)  # n seq 3 heads hd
    return qkv.reshape(n * seq, 3 * heads * hd).contiguous()


def unfuse_out(out, n, heads, seq, hd):
    """[n*seq, hidden] -> [n, heads, seq, hd]."""
    return out.reshape(n, seq, heads, hd).permute(0, 2, 1, 3)


# ---- references ----

def ref64(q, k, v, scale=None):
    """softmax(Q K^T scale) V, entirely in float64."""
    scale = scale_of(q.shape[-1]) if scale is None else scale
    q, k, v = q.double(), k.double(), v.double()
    return torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v


def emulate(q, k, v, normalized):
    """The numerics contract stated at the top of cc_attn.hip, written
    plainly: f32 scores, max and exp; P rounded to bf16 before PV — the
    normalised P (the resident rungs) or the unnormalised one with the sum
    taken before rounding (the online-softmax kernels); f32 PV; bf16 out."""
    s = q.float() @ k.float().transpose(-1, -2) * scale_of(q.shape[-1])
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    total = e.sum(dim=-1, keepdim=True)
    if normalized:
        o = (e / total).to(torch.bfloat16).float() @ v.float()
    else:
        o = e.to(torch.bfloat16).float() @ v.float() / total
    return o.to(torch.bfloat16)


def error(got, want, v):
    """max |got - want| / max |v|: the output is a convex combination of V
    rows, so max |v| is its natural scale."""
    return ((got.double() - want).abs().max() / v.double().abs().max()).item()


# ---- wrong variants: float64, each one defect a kernel could have ----

def _append_zero_keys(k, v, count):
    n, heads, _, hd = k.shape
    pad = torch.zeros(n, heads, count, hd, dtype=k.dtype)
    return torch.cat([k, pad], dim=2), torch.cat([v, pad], dim=2)


def wrong_mean_v(q, k, v):
    return v.double().mean(dim=2, keepdim=True).expand(*q.shape).clone()


def wrong_drop_last(q, k, v):
    return ref64(q, k[:, :, :-1], v[:, :, :-1])


def wrong_drop_last16(q, k, v):
    d = min(16, k.shape[2] - 1)
    return ref64(q, k[:, :, :-d], v[:, :, :-d])


def wrong_one_zero_key(q, k, v):
    return ref64(q, *_append_zero_keys(k, v, 1))


def wrong_zero_pad64(q, k, v):
    return ref64(q, *_append_zero_keys(k, v, -k.shape[2] % TILE))


def wrong_scale(q, k, v):
    """Scale x 1.05 (a padded head dim of 80 for hd 72 would be x 0.95)."""
    return ref64(q, k, v, scale=1.05 * scale_of(q.shape[-1]))


def wrong_neighbour_k(q, k, v):
    return ref64(q, k.roll(1, dims=1), v)


def wrong_no_rescale(q, k, v):
    """Online softmax over 64-key tiles; the sum follows the running max, O
    is not rescaled when the max moves."""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) * scale_of(q.shape[-1])
    m = torch.full(s.shape[:-1] + (1,), -1e30, dtype=torch.float64)
    total = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for k0 in range(0, k.shape[2], TILE):
        st = s[..., k0:k0 + TILE]
        m_new = torch.maximum(m, st.amax(dim=-1, keepdim=True))
        p = torch.exp(st - m_new)
        total = total * torch.exp(m - m_new) + p.sum(dim=-1, keepdim=True)
        o = o + p @ v[:, :, k0:k0 + TILE]  # the defect: no exp(m - m_new) on o
        m = m_new
    return o / total


ALL_BUT_ZERO_Q = tuple(f for f in FAMILIES if f != "zero_q")

# variant -> (function, the families that must expose it, where it applies).
# A variant applies where it differs from the right answer at all: with one
# key every softmax is 1 (mean, neighbour's K) and nothing can be dropped;
# at a multiple of 64 there is no pad; within one tile the max never moves
# between tiles.  The scale is held from seq 33: with fewer keys a row's
# mass often sits on one key, which no scale changes.
WRONG = {
    "mean_v": (wrong_mean_v, ALL_BUT_ZERO_Q, lambda seq: seq > 1),
    "drop_last": (wrong_drop_last, ("last_key",), lambda seq: seq > 1),
    "drop_last16": (wrong_drop_last16, ("last_key",), lambda seq: seq > 1),
    "one_zero_key": (wrong_one_zero_key, ("neg_offset",), lambda seq: True),
    "zero_pad64": (wrong_zero_pad64, ("neg_offset",), lambda seq: seq % TILE != 0),
    "scale_x1.05": (wrong_scale, ("peaked",), lambda seq: seq >= 33),
    "neighbour_k": (wrong_neighbour_k, ("peaked",), lambda seq: seq > 1),
    "no_rescale": (wrong_no_rescale, ("rising",), lambda seq: seq > TILE),
}


# ---- the case grid of test_gpu_attn_scores.py ----
# The smallest shapes at which each rung's structure is still exercised.
# small: one key, a ragged tile, the full tile.  mid: one key past a q-tile,
# three q-tiles, the rung's last seq.  flash: less than one KV tile; two Q
# and two KV tiles; three; one past mid's range; six KV tiles, the last
# with one row.  planned (cc_attn's own choice) runs every head dim, because
# the pad columns of a head are the next head's live data.
RUNG_CASES = [
    (rung, seq, hd, family)
    for rung, seqs in (("small", (1, 33, 64)), ("mid", (65, 129, 288)),
                       ("flash", (33, 65, 129, 289, 321)))
    for seq in seqs for hd in (64, 72, 128) for family in FAMILIES
]
PLANNED_CASES = [("planned", seq, hd, family) for seq in (50, 289) for hd in HDS
                 for family in ("neg_offset", "last_key")]
CLS_CASES = [("cls", seq, 64, family) for seq in (1, 64, 65, 129, 257)
             for family in FAMILIES]
GRID = RUNG_CASES + PLANNED_CASES + CLS_CASES
PROBLEMS = sorted({(family, seq, hd) for _, seq, hd, family in GRID},
                  key=lambda p: (FAMILIES.index(p[0]), p[1], p[2]))


def seed_of(family, seq, hd):
    return 100000 * FAMILIES.index(family) + 1000 * (hd // 8) + seq


# The bound on error(kernel output, ref64): 3 x the worst error of `emulate`
# (both modes) over PROBLEMS.  The kernels differ from the emulation only
# in the order of their f32 MFMA accumulation, in __expf and (the online
# kernels) in which running max P is rounded under; all of that is far below
# the 2^-9 rounding of P and O that the emulation carries.
#   measured worst emulation error: 0.003890 (last_key, seq 129, hd 72,
#   normalised P: one key at |v| = 4 carries the row, so P and O each round
#   at half a bf16 ulp of it, 2 x 2^-9 = 0.0039), over all 205 PROBLEMS
BOUND = 0.01168
