"""The attention rung rule, pinned through cc_attn_plan (no GPU).

cc::attn_plan (csrc/cc_attn_plan.hpp) decides which kernel a cc_attn call
runs (k_attn_small / k_attn_mid / k_attn_flash) and its grid, and it is the
only validation of the shape arguments.  The table states the rule on both
sides of each threshold and at the tower shapes (B/32's 50, L/14's 257,
SigLIP-384's 576); the GPU side (tests/test_gpu_vit.py) checks that cc_attn
executes the plan.
"""

import pytest

from cosmos_curate_amd import build as cc_build
from cosmos_curate_amd import hotpath

CC_ERR_INVALID = -1
CC_ERR_UNSUPPORTED = -6

N, HEADS = 3, 12


@pytest.fixture(scope="module")
def lib():
    cc_build.build(verbose=False)
    return hotpath.load()


@pytest.mark.parametrize(
    ("seq", "rung"),
    [(1, "small"), (50, "small"), (64, "small"),
     (65, "mid"), (257, "mid"), (288, "mid"),
     (289, "flash"), (576, "flash"), (1024, "flash")],
)
def test_attn_plan_table(lib, seq, rung):
    p = hotpath.attn_plan(N, seq, HEADS, HEADS * 64)
    n_qtiles = -(-seq // 64)
    grid = N * HEADS * (n_qtiles if rung == "flash" else 1)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid, p.block) == (rung, grid, 256)


@pytest.mark.parametrize(
    ("n_frames", "seq", "heads", "hidden", "code"),
    [
        (N, 50, 0, 0, CC_ERR_INVALID),             # heads == 0 == hidden/64
        (N, 0, HEADS, HEADS * 64, CC_ERR_INVALID),
        (0, 50, HEADS, HEADS * 64, CC_ERR_INVALID),
        (-1, 50, HEADS, HEADS * 64, CC_ERR_INVALID),
        (N, 50, HEADS, HEADS * 32, CC_ERR_UNSUPPORTED),  # hd 32
        (N, 50, HEADS, HEADS * 64 + 8, CC_ERR_UNSUPPORTED),
        (2**31, 50, HEADS, HEADS * 64, CC_ERR_INVALID),  # grid > 0x7fffffff
        # flash counts the q-tiles: 2^27 frames x 2 heads fit alone, not x 9
        (2**27, 576, 2, 128, CC_ERR_INVALID),
        (2**62, 50, HEADS, HEADS * 64, CC_ERR_INVALID),  # no int64 wrap
    ],
)
def test_attn_plan_rejects(lib, n_frames, seq, heads, hidden, code):
    out = hotpath.AttnPlan()
    rc = lib.cc_attn_plan(n_frames, seq, heads, hidden, out)
    assert rc == code
    assert lib.cc_last_error().decode()
    with pytest.raises(RuntimeError):
        hotpath.attn_plan(n_frames, seq, heads, hidden)


def test_attn_plan_largest_grid(lib):
    """The bound itself is accepted: exactly 0x7fffffff workgroups."""
    p = hotpath.attn_plan(0x7FFFFFFF, 64, 1, 64)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid) == ("small", 0x7FFFFFFF)
    # 2^27 frames x 2 heads x 5 q-tiles
    p = hotpath.attn_plan(2**27, 289, 2, 128)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid) == ("flash", 2**27 * 10)


def test_attn_plan_null_out(lib):
    assert lib.cc_attn_plan(N, 50, HEADS, HEADS * 64, None) == CC_ERR_INVALID
