"""cc_attn_pool against float64 (attn_pool_ref.py) at the smallest shapes where
it can go wrong: one token, a ragged chunk, one chunk, one token into the
second, three chunks, nine (the plan splits them in two); the widths whose
column slices deal 4+4, 4+4+1 and 4+4+2+1 fragments; 12 heads; explicit
splits, empty ones included.  Guards as test_gpu_attn_scores.py.
"""

import functools

import pytest
import torch

import attn_pool_ref as R
from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
CC_ERR_UNSUPPORTED = -6  # include/cc_hotpath.h

# (seq, H, murstd, shared U, heads, splits, n)
CASES = [
    (1, 1152, True, True, 16, 0, 2), (31, 1152, False, True, 16, 0, 3),
    (32, 1152, True, False, 16, 1, 2), (33, 1152, True, True, 16, 0, 3),
    (65, 1152, False, False, 12, 0, 2), (257, 1152, True, True, 16, 0, 3),
    (33, 1024, True, False, 16, 1, 2), (33, 1408, False, True, 12, 0, 3),
    (257, 1024, False, True, 16, 0, 2), (257, 1408, True, False, 16, 0, 3),
    (33, 1152, True, True, 16, 3, 2), (33, 1408, True, False, 12, 3, 3),
    (257, 1408, True, False, 16, 3, 2), (257, 1024, False, True, 12, 3, 3),
    (257, 1152, True, False, 12, 1, 2), (1, 1408, False, False, 16, 3, 3),
    (65, 1024, True, True, 16, 3, 2), (31, 1408, True, False, 12, 1, 3),
    (32, 1024, False, True, 16, 0, 2), (65, 1408, True, True, 16, 1, 3),
]


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


@functools.lru_cache(maxsize=None)
def _problem(case):
    """Inputs and their float64 reference, computed once and not modified."""
    seq, H, stats, shared, heads, _, n = case
    x, u, mu, rstd = R.make_inputs(n, seq, H, heads, shared, stats, hash(case) & 0xFFFF)
    return x, u, mu, rstd, R.zhat_ref(x, u, mu, rstd)


def _guarded(rows_cpu, fill=float("nan")):
    buf = torch.full((rows_cpu.shape[0] + 2, rows_cpu.shape[1]), fill,
                     dtype=rows_cpu.dtype, device="cuda")
    buf[1:-1].copy_(rows_cpu)
    return buf, buf[1:-1]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_attn_pool(lib, case):
    seq, H, stats, shared, heads, splits, n = case
    x, u, mu, rstd, ref = _problem(case)
    scale = R.scale_of(x, rstd)
    bound = R.BOUND_REL * scale
    if seq > 1:
        # the case is sensitive to the scores: uniform pooling is far off
        uniform = R.normalised(x, mu, rstd).mean(dim=1, keepdim=True)
        assert (uniform - ref).abs().max() >= 20 * bound

    x_buf, xd = _guarded(x.reshape(n * seq, H))
    msd = _guarded(torch.stack([mu, rstd], dim=-1).reshape(n * seq, 2).float())[1] if stats else None
    u_hi, u_lo, usum = (t.cuda() for t in hotpath.attn_pool_probe(u[0] if shared else u))
    plan = hotpath.attn_pool_plan(n, seq, heads, H, splits)
    ws = torch.empty(max(plan.workspace_floats, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    outs = []
    hotpath.timing_enable(True)
    try:
        for _ in range(2):
            out_buf = torch.full((n * heads + 2, H), SENTINEL, dtype=torch.float32,
                                 device="cuda")
            out = out_buf[1:-1]
            hotpath.check(lib.cc_attn_pool(
                xd.data_ptr(), H, msd.data_ptr() if stats else None,
                u_hi.data_ptr(), u_lo.data_ptr(), 0 if shared else 16 * H,
                usum.data_ptr(), out.data_ptr(), n, seq, heads, H, splits,
                ws.data_ptr(), ws.numel(), stream))
            torch.cuda.synchronize()
            assert torch.all(out_buf[[0, -1]] == SENTINEL), "wrote outside the output rows"
            outs.append(out)
        launches = hotpath.timing_report("attn_pool")[1]
        combines = hotpath.timing_report("attn_pool_combine")[1]
    finally:
        hotpath.timing_enable(False)
    assert launches == 2 and combines == (2 if plan.splits > 1 else 0)
    assert torch.isnan(x_buf[0]).all() and torch.isnan(x_buf[-1]).all()
    assert torch.isfinite(outs[0]).all(), "a guard row or a masked token reached the output"
    assert torch.equal(outs[0], outs[1]), "attn_pool differs from run to run"
    err = float((outs[0].cpu().double().reshape(n, heads, H) - ref).abs().max())
    print(f"attn_pool {case} splits {plan.splits}: err {err:.3e} = "
          f"{err / bound:.2f} x bound ({err / scale:.2e} of the scale)")
    assert err <= bound


@pytest.mark.parametrize("heads,H", [(17, 1152), (16, 1536), (16, 1100), (0, 1024)])
def test_unsupported_geometry_is_refused_before_any_launch(lib, heads, H):
    assert not hotpath.attn_pool_supported(heads, H)
    buf = torch.zeros(16 * 1536, dtype=torch.float32, device="cuda")
    hotpath.timing_enable(True)
    try:
        rc = lib.cc_attn_pool(buf.data_ptr(), H, None, buf.data_ptr(),
                              buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr(),
                              1, 1, heads, H, 0, None, 0, 0)
        launches = hotpath.timing_report("attn_pool")[1]
    finally:
        hotpath.timing_enable(False)
    assert rc == CC_ERR_UNSUPPORTED and launches == 0
