"""The attention plan above head dim 64, through cc_attn_plan (no GPU).

cc_attn takes every head dim that is a multiple of 8 from 64 to 128
(csrc/cc_attn_plan.hpp).  The rung rule as built above head dim 64: seq <= 64
small; 193..288 at head dim >= 96 mid; everything else flash (the header has
the measurements behind it).  The tables below state it at B/32's 50, L/14's
257 and so400m-384's 729, and on both sides of each boundary;
tests/test_attn_plan_cpu.py pins the rule at head dim 64.
"""

import pytest

from cosmos_curate_amd import build as cc_build
from cosmos_curate_amd import hotpath

CC_ERR_UNSUPPORTED = -6

N, HEADS = 3, 5

HDS = [72, 80, 88, 96, 104, 112, 120, 128]


def _rule(hd, seq):
    """The rule as built, restated: (rung, workgroups per (frame, head)).
    flash launches one workgroup per 64-row q-tile."""
    if seq <= 64:
        return "small", 1
    if hd >= 96 and 193 <= seq <= 288:
        return "mid", 1
    return "flash", -(-seq // 64)


# the issue's three lengths, written out: (hd, seq) -> (rung, per head)
TABLE = {(hd, 50): ("small", 1) for hd in HDS}
TABLE.update({(hd, 257): ("flash", 5) for hd in (72, 80, 88)})
TABLE.update({(hd, 257): ("mid", 1) for hd in (96, 104, 112, 120, 128)})
TABLE.update({(hd, 729): ("flash", 12) for hd in HDS})


@pytest.fixture(scope="module")
def lib():
    cc_build.build(verbose=False)
    return hotpath.load()


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("seq", [50, 257, 729])
def test_attn_plan_accepts_head_dims(lib, hd, seq):
    rung, per_head = TABLE[hd, seq]
    assert _rule(hd, seq) == (rung, per_head)
    p = hotpath.attn_plan(N, seq, HEADS, HEADS * hd)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid, p.block) == (
        rung, N * HEADS * per_head, 256)
    assert hotpath.attn_supported(HEADS, HEADS * hd)


@pytest.mark.parametrize(
    ("heads", "hidden"),
    [
        (HEADS, HEADS * 56),   # below the range
        (HEADS, HEADS * 136),  # above it
        (HEADS, HEADS * 68),   # inside, not a multiple of 8
        (HEADS, HEADS * 72 + 1),  # hidden % heads != 0
        (16, 1152 + 8),        # 72.5
    ],
)
def test_attn_plan_rejects_head_dims(lib, heads, hidden):
    out = hotpath.AttnPlan()
    assert lib.cc_attn_plan(N, 50, heads, hidden, out) == CC_ERR_UNSUPPORTED
    assert lib.cc_last_error().decode()
    assert not hotpath.attn_supported(heads, hidden)
    with pytest.raises(RuntimeError):
        hotpath.attn_plan(N, 50, heads, hidden)


@pytest.mark.parametrize("hd", [72, 88, 96, 128])
@pytest.mark.parametrize("seq", [1, 64, 65, 192, 193, 256, 288, 289, 1024])
def test_attn_plan_boundaries(lib, hd, seq):
    rung, per_head = _rule(hd, seq)
    p = hotpath.attn_plan(N, seq, HEADS, HEADS * hd)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid, p.block) == (
        rung, N * HEADS * per_head, 256)


def test_attn_plan_so400m_layer(lib):
    """The so400m-224 layer: 16 heads of 72 over 256 tokens, 4 q-tiles."""
    p = hotpath.attn_plan(1, 256, 16, 1152)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid, p.block) == ("flash", 64, 256)
