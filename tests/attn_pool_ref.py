"""Plain float64 reference of cc_attn_pool (include/cc_hotpath.h): scores
u_h . xhat_t over the normalised tokens, zhat_h = sum_t softmax_t(score) *
xhat_t; and the inputs its tests share: tokens N(0,1) * (0.5 + 1.5 * rand_t) +
2 * N(0,1)_t in bf16, U scaled to scores of standard deviation 6, so that a
few tokens carry each head.
"""

import torch

# max |got - ref| <= BOUND_REL * max |rstd_t * x_t|: the one rounded operand
# is w = e * rstd in bf16, l is summed unrounded.  bf16's unit roundoff is
# 2^-8, relative error at most 2^-8 / (1 + 2^-8), so one token alone (seq 1)
# can come to just under the bound; with more, each token's error is weighted
# by its probability and the f32 summation order and exp add about 1e-6.
BOUND_REL = 2.0 ** -8
SCORE_STD = 6.0
LN_EPS = 1e-6


def make_inputs(n, seq, H, heads, shared, stats, seed):
    """(x bf16 [n, seq, H], u f32 [1 or n, heads, H], mu, rstd f64 [n, seq] or
    None, None)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    spread = 0.5 + 1.5 * torch.rand(n, seq, 1, generator=gen, dtype=torch.float64)
    x = (r(n, seq, H) * spread + 2.0 * r(n, seq, 1)).to(torch.bfloat16)
    mu = rstd = None
    if stats:
        xd = x.double()
        mu = xd.mean(dim=-1)
        rstd = torch.rsqrt(xd.var(dim=-1, unbiased=False) + LN_EPS)
    u = r(1 if shared else n, heads, H)
    scores = torch.einsum("nth,nkh->nkt", normalised(x, mu, rstd), u.expand(n, -1, -1))
    return x, (u * (SCORE_STD / scores.std())).float(), mu, rstd


def normalised(x, mu, rstd):
    xd = x.double()
    return xd if mu is None else (xd - mu[..., None]) * rstd[..., None]


def zhat_ref(x, u, mu, rstd):
    """f64 [n, heads, H]."""
    xh = normalised(x, mu, rstd)
    scores = torch.einsum("nth,nkh->nkt", xh, u.double().expand(x.shape[0], -1, -1))
    return torch.softmax(scores, dim=-1) @ xh


def scale_of(x, rstd):
    """max |rstd_t * x_t|, what the bound is relative to."""
    xd = x.double()
    return float((xd if rstd is None else xd * rstd[..., None]).abs().max())
