"""The GEMM dispatch rule, pinned through cc_gemm_plan (no GPU).

cc::gemm_plan (csrc/cc_gemm_plan.hpp) decides which kernel body a
cc_gemm_bf16* call runs, its grid, the persistent fleet size, the XCD remap
and the epilogue.  A slip there breaks no parity test — it only loses
speed — so the table below states the rule at the shapes that matter: the
flagship B/32 step at 64 clips (M = 235200), the CLS-only last layer at
M = frames = 4704, the L/14 shapes, and each threshold of
the rule (M 128/129, K < 256, K % 128, the 48 Mi-element remap, the
16-tile-wide remap limit, the half-fleet `underfill` exception).
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


# (M, N, K, kwargs) -> (body, tiles_x, tiles_y, grid, block, remap, staged)
BIAS = {"has_bias": True}
BIAS_RES = {"has_bias": True, "has_residual": True}
BIAS_ACT = {"has_bias": True, "act": 1}
PLAN_TABLE = [
    ((235200, 2304, 768, BIAS), (256, 9, 919, 256, 512, 1, 1)),
    ((235200, 768, 768, BIAS_RES), (256, 3, 919, 256, 512, 1, 1)),
    ((235200, 3072, 768, BIAS_ACT), (256, 12, 919, 256, 512, 1, 1)),
    ((235200, 768, 3072, BIAS_RES), (256, 3, 919, 256, 512, 1, 1)),
    ((4704, 512, 768, {}), (128, 4, 37, 148, 256, 0, 0)),
    ((4704, 768, 3072, BIAS_RES), (128, 6, 37, 222, 256, 0, 0)),  # underfill
    ((4704, 3072, 768, BIAS_ACT), (256, 12, 19, 228, 512, 1, 1)),
    ((4704, 1024, 4096, BIAS_RES), (128, 8, 37, 296, 256, 0, 0)),
    ((4704, 4096, 1024, BIAS_ACT), (256, 16, 19, 256, 512, 1, 1)),
    ((4704, 3072, 768, {"lda": 38400}), (128, 24, 37, 888, 256, 0, 0)),
    ((128, 3072, 768, BIAS), (128, 24, 1, 24, 256, 0, 0)),
    ((129, 3072, 768, BIAS), (256, 12, 1, 12, 512, 1, 1)),
    ((300, 1536, 128, BIAS), (128, 12, 3, 36, 256, 0, 0)),    # K < 256
    ((1024, 2048, 192, BIAS), (128, 16, 8, 128, 256, 0, 0)),  # K % 128 != 0
    ((8192, 8192, 192, {}), (128, 64, 64, 4096, 256, 1, 0)),
    ((8192, 8192, 8192, {}), (256, 32, 32, 256, 512, 0, 0)),
    ((2000, 768, 1536, BIAS), (256, 3, 8, 24, 512, 1, 1)),
]


@pytest.mark.parametrize(("args", "want"), PLAN_TABLE)
def test_gemm_plan_table(lib, args, want):
    M, N, K, kw = args
    p = hotpath.gemm_plan(M, N, K, **kw)
    got = (p.body, p.tiles_x, p.tiles_y, p.grid, p.block, p.xcd_remap,
           p.epi_staged)
    assert got == want


def test_gemm_plan_ignores_environment(lib, monkeypatch):
    """cc_gemm_plan answers for the build, not for the A/B knobs."""
    monkeypatch.setenv("CC_GEMM_TILE", "0")
    monkeypatch.setenv("CC_GEMM_PERSIST", "0")
    p = hotpath.gemm_plan(235200, 2304, 768, has_bias=True)
    assert (p.body, p.grid) == (256, 256)


def _plan_rc(lib, M, N, K, lda, ldr, has_residual):
    out = hotpath.GemmPlan()
    rc = lib.cc_gemm_plan(M, N, K, lda, ldr, 0, 0, int(has_residual), out)
    return rc, lib.cc_last_error().decode()


@pytest.mark.parametrize(
    ("M", "N", "K", "lda", "ldr", "has_residual", "code"),
    [
        (16, 16, 60, 60, 16, False, CC_ERR_UNSUPPORTED),    # K % 64 != 0
        (256, 256, 128, 132, 256, False, CC_ERR_INVALID),   # lda = K + 4
        (256, 256, 128, 64, 256, False, CC_ERR_INVALID),    # lda < K
        (256, 256, 128, 128, 128, True, CC_ERR_INVALID),    # ldr < N
    ],
)
def test_gemm_plan_rejects(lib, M, N, K, lda, ldr, has_residual, code):
    rc, msg = _plan_rc(lib, M, N, K, lda, ldr, has_residual)
    assert rc == code
    assert msg


def test_gemm_plan_ldr_ignored_without_residual(lib):
    rc, _ = _plan_rc(lib, 256, 256, 128, 128, 1, False)
    assert rc == 0
    dense = hotpath.gemm_plan(4704, 3072, 768, has_bias=True)
    odd = hotpath.gemm_plan(4704, 3072, 768, has_bias=True, ldr=5)
    assert (odd.body, odd.grid) == (dense.body, dense.grid) == (256, 228)
