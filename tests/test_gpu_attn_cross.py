"""cc_attn_cross against float64 attention (attn_ref.ref64) on the inputs
whose softmax scores matter, under attn_ref.BOUND.  Q is the first nq rows of
a problem, K and V all of its nk rows: every row tested is one the bound was
derived over.  The shapes are the smallest that reach a single key (1), a
ragged chunk (33), a full chunk (64), one key past a chunk (65), waves with
unequal chunk counts (129: five chunks on four waves), a ragged last split
(289 at 3 splits) and the combine kernel (every splits > 1).

Inputs sit between NaN rows, and in the strided cases between NaN columns,
so a read outside the rows and columns named shows in the output.
"""

import functools

import pytest
import torch

import attn_ref as R
from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

HD, CHUNK = 64, 32
HIDDEN = R.HEADS * HD
NKS = (1, 33, 64, 65, 129, 289, 321)
NQS = (1, 17, 32)


def _clamped(nk, splits):
    """What the plan makes of a forced split count (no split empty)."""
    chunks = -(-nk // CHUNK)
    per = -(-chunks // min(splits, chunks))
    return -(-chunks // per)


# splits 0 is the plan's choice, 1 at these sizes; a forced count runs only
# where the clamp leaves it as it is
CASES = [(nk, nq, splits) for nk in NKS for nq in NQS if nq <= nk
         for splits in (0, 1, 2, 3) if splits == 0 or _clamped(nk, splits) == splits]


@functools.lru_cache(maxsize=None)
def _problem(family, nk):
    """q, k, v and their float64 reference, computed once and not modified."""
    q, k, v = R.make_inputs(family, nk, HD, R.seed_of(family, nk, HD))
    return q, k, v, R.ref64(q, k, v)


def _placed(rows_cpu, ld, col):
    """`rows_cpu` on the device as a window at column `col` of a NaN buffer
    with two more rows and `ld` columns."""
    buf = torch.full((rows_cpu.shape[0] + 2, ld), float("nan"),
                     dtype=torch.bfloat16, device="cuda")
    view = buf[1:-1, col:col + rows_cpu.shape[1]]
    view.copy_(rows_cpu)
    return view


def _check(family, nk, nq, splits, ldq=HIDDEN, ldkv=2 * HIDDEN, kv_col=0):
    hotpath.require_gpu()
    q, k, v, ref = _problem(family, nk)
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(-1, HIDDEN)  # noqa: E731
    qd = _placed(rows(q[:, :, :nq]), ldq, 0)
    kvd = _placed(torch.cat([rows(k), rows(v)], dim=1), ldkv, kv_col)
    want = 1 if splits == 0 else splits
    assert hotpath.attn_cross_plan(R.N, nq, nk, R.HEADS, HIDDEN, splits).splits == want
    outs = []
    hotpath.timing_enable(True)
    try:
        for _ in range(2):
            outs.append(hotpath.attn_cross(qd, kvd, R.N, nq, nk, R.HEADS, splits=splits))
        torch.cuda.synchronize()
        launches = [hotpath.timing_report(k)[1] for k in ("attn_cross", "attn_cross_combine")]
    finally:
        hotpath.timing_enable(False)
    assert launches == [2, 2 if want > 1 else 0]
    assert torch.equal(outs[0], outs[1]), "attn_cross differs from run to run"
    got = R.unfuse_out(outs[0].cpu(), R.N, R.HEADS, nq, HD)
    assert torch.isfinite(got.float()).all(), "a masked key or a pad reached the output"
    err = R.error(got, ref[:, :, :nq], v)
    print(f"attn_cross nk {nk} nq {nq} splits {want} {family}: "
          f"err {err:.5f} = {err / R.BOUND:.2f} x BOUND")
    assert err <= R.BOUND


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("nk,nq,splits", CASES)
def test_attn_cross(nk, nq, splits, family):
    _check(family, nk, nq, splits)


def test_hoisted_kv_layout():
    """K/V as a column window of a wider GEMM output: ldkv > 2H, offset > 0."""
    _check("last_key", 129, 32, 2, ldkv=3 * 2 * HIDDEN + 8, kv_col=2 * HIDDEN + 8)


def test_strided_q():
    _check("neg_offset", 65, 17, 1, ldq=HIDDEN + 8)
