"""cc_attn_cross's launch plan (csrc/cc_attncross_plan.hpp), which needs no
GPU: the splits cover the keys, none is empty, the grid and the workspace
follow from them, and what the kernel does not take is refused with a message.
"""

import pytest

from cosmos_curate_amd import build as cc_build
from cosmos_curate_amd import hotpath

N, NQ, HEADS, H = 8, 32, 12, 768  # the Q-Former's cross-attention at batch 8
NKS = (2056, 4616, 8200, 1, 33)   # 224p, 336p, 448p; one key; one past a chunk


@pytest.fixture(scope="module", autouse=True)
def lib():
    cc_build.build(verbose=False)
    return hotpath.load()


@pytest.mark.parametrize("splits", [0, 1, 2, 3, 4, 8, 1000])
@pytest.mark.parametrize("nk", NKS)
def test_plan_covers_the_keys(nk, splits):
    p = hotpath.attn_cross_plan(N, NQ, nk, HEADS, H, splits)
    keys = p.chunk * p.chunks_per_split
    chunks = -(-nk // p.chunk)
    assert p.splits * keys >= nk
    assert (p.splits - 1) * keys < nk, "the last split is empty"
    assert 1 <= p.splits <= chunks and (splits == 0 or p.splits <= splits)
    assert p.grid == N * HEADS * p.splits and p.block == 256
    assert (p.workspace_floats == 0) == (p.splits == 1)
    assert p.workspace_floats in (0, p.grid * (64 + 32 * 64))


def test_plans_own_choice_is_the_measured_one():
    """4 splits at the three real shapes (the table in cc_attncross_plan.hpp);
    a short key range is not split below eight chunks a split."""
    assert [hotpath.attn_cross_plan(N, NQ, nk, HEADS, H).splits for nk in NKS] == [
        4, 4, 4, 1, 1]
    # one clip: 32 wanted, 257 chunks at 9 a split leave 29 non-empty
    assert hotpath.attn_cross_plan(1, NQ, 8200, HEADS, H).splits == 29
    assert hotpath.attn_cross_plan(1, NQ, 514, HEADS, H).splits == 2


def test_forced_splits_are_clamped_to_the_chunks():
    assert hotpath.attn_cross_plan(N, NQ, 1, HEADS, H, 4).splits == 1
    assert hotpath.attn_cross_plan(N, NQ, 33, HEADS, H, 4).splits == 2
    assert hotpath.attn_cross_plan(N, NQ, 2056, HEADS, H, 4).splits == 4


@pytest.mark.parametrize("nq,heads,hidden,what", [
    (32, 8, 704, "head dim 64"),  # head dim 88
    (33, 12, 768, "at most 32 queries"),
])
def test_plan_refuses_with_a_message(nq, heads, hidden, what):
    assert hotpath.attn_cross_supported(12, 768)
    assert hotpath.attn_cross_supported(heads, hidden) == (hidden == 64 * heads)
    with pytest.raises(RuntimeError, match=f"cc error -6.*{what}"):
        hotpath.attn_cross_plan(N, nq, 2056, heads, hidden)
