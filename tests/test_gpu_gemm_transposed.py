"""The 256² GEMM epilogue on inputs whose f32 sums really round (DESIGN.md
§27): the body computes transposed accumulator fragments, and C and the
statistics must be what they were before, bit for bit.

Problems, forms and checks are those of tools/gemm_transposed_golden.py,
which wrote tests/golden/gemm_transposed_hashes.json from the library of the
parent commit of the operand swap.  Inputs are seeded standard-normal bf16
from the CPU generator; building a problem asserts on the CPU that the f32
sum of one output element's products depends on the order of k, so a
changed order of accumulation cannot hide behind exact sums.  Every case is
checked against torch f32 (rtol = atol = 2e-2), for an untouched
sentinel-filled spare row, for two bit-equal runs and against the recorded
SHA-256 of C and of the statistics.

The N edge of the scalar f32 path is reached through cc_gemm_bf16_ex under
CC_GEMM_TILE=1, in a child process as in tests/test_gpu_gemm_epilogue.py.
No N has both N % 256 == 128 and N % 4 != 0; the case takes N = 386, whose
last column tile holds 130 columns and whose rows are not 16-byte aligned.
"""

import importlib.util
import pathlib
import sys

import pytest

from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "gemm_transposed_hashes.json"

_spec = importlib.util.spec_from_file_location(
    "gemm_transposed_golden", ROOT / "tools" / "gemm_transposed_golden.py")
gtg = importlib.util.module_from_spec(_spec)
sys.modules[_spec.name] = gtg
_spec.loader.exec_module(gtg)
geg = gtg.geg

_problems = {}


def _problem(M, N, K):
    """One problem per shape, shared by its forms and left unchanged."""
    if (M, N, K) not in _problems:
        _problems.clear()
        _problems[(M, N, K)] = gtg.build_problem(M, N, K)
    return _problems[(M, N, K)]


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


@pytest.fixture(scope="module")
def golden():
    return geg.load_golden(GOLDEN)


def test_fixture_lists_every_case(golden):
    want = {geg.case_id(*c) for c in gtg.CASES}
    want |= {geg.case_id(M, N, K, f) for M, N, K, _, forms in gtg.FORCED
             for f in forms}
    assert set(golden) == want


@pytest.mark.parametrize(("M", "N", "K", "form"), gtg.CASES)
def test_transposed_case(lib, golden, M, N, K, form):
    assert hotpath.gemm_plan(
        M, N, K, has_bias=form != "bare",
        act=int(form[3:]) if form.startswith("act") else 0,
        has_residual=form.startswith("res")).body == 256
    gtg.check_case(lib, _problem(M, N, K), form,
                   golden[geg.case_id(M, N, K, form)])


@pytest.mark.parametrize(("M", "N", "K", "tile", "forms"), gtg.FORCED)
def test_transposed_forced_tile(M, N, K, tile, forms):
    """The default plan gives this shape to the 128² body (asserted), so a
    child process runs it with CC_GEMM_TILE set and makes the same checks
    against the recorded file."""
    assert hotpath.gemm_plan(M, N, K, has_bias=True).body == 128
    got, log = gtg.run_shape_in_child(M, N, K, tile, GOLDEN)
    print(log)
    assert set(got) == {geg.case_id(M, N, K, f) for f in forms}
