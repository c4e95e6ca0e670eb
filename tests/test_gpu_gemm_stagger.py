"""The 256² GEMM K-loop at the shapes where its schedule can go wrong
(DESIGN.md §26): an odd number of K-tile pairs, the long fc2 K, and
workgroups that enter and leave the K-loop three times.

Problems and checks are those of tools/gemm_epilogue_golden.py; the shapes
and the recorded hashes are those of tools/gemm_stagger_golden.py, which
wrote tests/golden/gemm_stagger_hashes.json from the library of the parent
commit of the schedule change.  Every case is checked against torch f32
(rtol = atol = 2e-2), for untouched spare rows, for three bit-equal runs and
against the recorded SHA-256 of C and of the statistics.
"""

import importlib.util
import pathlib
import sys

import pytest

from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "gemm_stagger_hashes.json"

_spec = importlib.util.spec_from_file_location(
    "gemm_stagger_golden", ROOT / "tools" / "gemm_stagger_golden.py")
gsg = importlib.util.module_from_spec(_spec)
sys.modules[_spec.name] = gsg
_spec.loader.exec_module(gsg)
geg = gsg.geg

_problems = {}


def _problem(M, N, K):
    """One problem per shape, shared by its forms and left unchanged; only
    the current shape is kept (the largest is 70 MB)."""
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
    assert set(golden) == {geg.case_id(*c) for c in gsg.CASES}


@pytest.mark.parametrize(("M", "N", "K", "form"), gsg.CASES)
def test_stagger_case(lib, golden, M, N, K, form):
    assert hotpath.gemm_plan(
        M, N, K, has_bias=True, has_residual=form.startswith("res")).body == 256
    p = _problem(M, N, K)
    # torch f32, spare rows, two equal runs, the recorded hashes
    got = geg.check_case(lib, p, form, golden[geg.case_id(M, N, K, form)])
    # a third run
    assert geg.hashes_of(p, *geg.run_form(lib, p, form)) == got
