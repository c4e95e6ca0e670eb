"""The 256² GEMM epilogue across its edges and the persistent walk
(DESIGN.md §19): staged bias / column-sum tables, batched residual loads,
range-checked stores and the counted rep-top wait.

Problems, checks and the recorded hashes are those of
tools/gemm_epilogue_golden.py, which wrote tests/golden/
gemm_epilogue_hashes.json at the parent of the epilogue change; every case
is checked against torch f32, for untouched spare rows, for run-to-run
equality and against the recorded SHA-256 of C and of the statistics.
"""

import importlib.util
import pathlib
import sys

import pytest

from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "gemm_epilogue_hashes.json"

_spec = importlib.util.spec_from_file_location(
    "gemm_epilogue_golden", ROOT / "tools" / "gemm_epilogue_golden.py")
geg = importlib.util.module_from_spec(_spec)
sys.modules[_spec.name] = geg
_spec.loader.exec_module(geg)

IN_PROCESS = [(M, N, K, f) for M, N, K, tile, forms in geg.SHAPES
              if tile is None for f in forms]
FORCED = [s for s in geg.SHAPES if s[3] is not None]

_problems = {}


def _problem(M, N, K):
    """One problem per shape, shared by its forms and left unchanged; only
    the current shape is kept (the largest is 100 MB)."""
    if (M, N, K) not in _problems:
        _problems.clear()
        _problems[(M, N, K)] = geg.build_problem(M, N, K)
    return _problems[(M, N, K)]


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


@pytest.fixture(scope="module")
def golden():
    return geg.load_golden(GOLDEN)


def test_fixture_lists_every_case(golden):
    want = {geg.case_id(M, N, K, f) for M, N, K, _, forms in geg.SHAPES
            for f in forms}
    assert set(golden) == want


@pytest.mark.parametrize(("M", "N", "K", "form"), IN_PROCESS)
def test_epilogue_case(lib, golden, M, N, K, form):
    assert hotpath.gemm_plan(
        M, N, K, has_bias=True, act=int(form[3:]) if form.startswith("act") else 0,
        has_residual=form.startswith("res")).body == 256
    geg.check_case(lib, _problem(M, N, K), form,
                   golden[geg.case_id(M, N, K, form)])


@pytest.mark.parametrize(("M", "N", "K", "tile", "forms"), FORCED)
def test_epilogue_forced_tile(M, N, K, tile, forms):
    """The column-edge shape: the default plan gives it to the 128² body,
    so a child process runs it with CC_GEMM_TILE set (the knob is read once
    per process) and makes the same checks against the recorded file."""
    assert hotpath.gemm_plan(M, N, K, has_bias=True).body == 128
    got, log = geg.run_shape_in_child(M, N, K, tile, GOLDEN)
    print(log)
    assert set(got) == {geg.case_id(M, N, K, f) for f in forms}
