"""The k-means step's launch rule, pinned through cc_kmeans_plan (no GPU).

cc::kmeans_plan (csrc/cc_kmeans_plan.hpp) is the only validation of the
shapes cc_kmeans_assign and cc_kmeans_accumulate take, and it sizes their
grids and the accumulate workspace; the GPU side (tests/test_gpu_kmeans.py)
checks that the kernels compute what they should at these shapes.
"""

import pytest

from cosmos_curate_amd import build as cc_build
from cosmos_curate_amd import hotpath

CC_ERR_INVALID = -1
CC_ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def lib():
    cc_build.build(verbose=False)
    return hotpath.load()


@pytest.mark.parametrize(
    ("m", "d", "k"),
    [(1, 64, 1), (63, 64, 5), (129, 512, 33), (257, 512, 128), (1000, 512, 129),
     (4097, 768, 130), (3000, 1152, 257), (5000, 512, 3),
     (1_000_000, 512, 1000), (100_000, 1152, 1000)],
)
def test_kmeans_plan_table(lib, m, d, k):
    p = hotpath.kmeans_plan(m, d, k)
    assert (p.tile_rows, p.tile_cents, p.assign_block) == (128, 128, 256)
    assert (p.assign_grid, p.cent_tiles, p.d_chunks) == (-(-m // 128), -(-k // 128), d // 32)
    pieces = -(-m // p.piece_rows)
    assert (p.piece_rows, p.pieces) == (512, pieces)
    assert p.acc_block % 64 == 0 and 0 <= p.acc_block - d // 4 < 64
    assert p.combine_grid_y == -(-d // 256)
    # head[pieces][d] and tail[pieces][d], f64
    assert p.workspace_bytes == 2 * pieces * d * 8
    assert lib.cc_kmeans_workspace_bytes(m, d, k) == p.workspace_bytes


@pytest.mark.parametrize(
    ("m", "d", "k", "code"),
    [
        (100, 96, 4, CC_ERR_UNSUPPORTED),    # not a multiple of 64
        (100, 32, 4, CC_ERR_UNSUPPORTED),    # below the smallest width
        (100, 1216, 4, CC_ERR_UNSUPPORTED),  # the first multiple past 1152
        (100, 512, 0, CC_ERR_INVALID),
        (0, 512, 4, CC_ERR_INVALID),
        (-1, 512, 4, CC_ERR_INVALID),
        (100, 0, 4, CC_ERR_INVALID),
        (100, 512, 2**30 + 1, CC_ERR_INVALID),
        (128 * (2**31 - 1) + 1, 512, 4, CC_ERR_INVALID),  # grid > 0x7fffffff
        (2**62, 512, 4, CC_ERR_INVALID),                  # no int64 wrap
    ],
)
def test_kmeans_plan_rejects(lib, m, d, k, code):
    assert lib.cc_kmeans_plan(m, d, k, hotpath.KmeansPlan()) == code
    assert lib.cc_last_error().decode()
    assert lib.cc_kmeans_workspace_bytes(m, d, k) == code
    with pytest.raises(RuntimeError):
        hotpath.kmeans_plan(m, d, k)


def test_kmeans_plan_bounds_accepted(lib):
    """Both ends of d, and exactly 0x7fffffff assign workgroups."""
    assert hotpath.kmeans_plan(1, 64, 1).d_chunks == 2
    assert hotpath.kmeans_plan(1, 1152, 2**30).cent_tiles == 2**23
    assert hotpath.kmeans_plan(128 * (2**31 - 1), 64, 1).assign_grid == 2**31 - 1
    assert lib.cc_kmeans_plan(1, 64, 1, None) == CC_ERR_INVALID
