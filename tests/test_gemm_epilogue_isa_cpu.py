"""What hipcc emits between a 256² tile's last MFMA and the next tile's
first, for the three instantiations a flagship step runs.

The properties below are what keeps the next tile's prefetch in flight
across the epilogue; none of them shows in a result, and each has been
lost before to a change that looked harmless in the source (an ordinary
load beside the LDS-DMA, a spill reload, an LDS read whose type hipcc's
alias analysis cannot tell from the DMA's).  Parsing is
tools/gemm_epilogue_isa.py's; only mnemonics of waits, loads and stores
are read.
"""

import importlib.util
import pathlib
import shutil
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

_spec = importlib.util.spec_from_file_location(
    "gemm_epilogue_isa", ROOT / "tools" / "gemm_epilogue_isa.py")
isa = importlib.util.module_from_spec(_spec)
sys.modules[_spec.name] = isa  # dataclasses look the module up
_spec.loader.exec_module(isa)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None,
                                reason="needs hipcc")


@pytest.fixture(scope="module")
def tails(tmp_path_factory):
    listing = isa.compile_listing(tmp_path_factory.mktemp("isa") / "cc_gemm.s")
    records = isa.analyse(listing.read_text())
    print(isa.table(records))
    return records


@pytest.mark.parametrize("name", list(isa.FLAGSHIP))
def test_flagship_tail(tails, name):
    t = tails[isa.FLAGSHIP[name]]
    stats = isa.FLAGSHIP[name][5]
    residual = isa.FLAGSHIP[name][2]
    assert t.vmcnt0_waits == 0, "a full drain between two tiles' MFMAs"
    assert t.vgpr_loads_compiler == 0, \
        "a VGPR-destination load hipcc counts: it waits vmcnt(0) for it"
    assert t.vgpr_loads_asm == (16 if residual else 0)
    # the same stores on every path: 4 passes x 4 chunks, C (+ stats)
    assert t.stores == (32 if stats else 16)
    assert t.stores_under_execz == 0, "a store behind a divergent branch"
    # the next prologue: 12 operand loads + the tables
    assert t.lds_dma == isa_prologue_loads(isa.FLAGSHIP[name])


def isa_prologue_loads(params):
    _, bias, _, _, ln, _ = params
    return 12 + (1 if bias else 0) + (1 if ln else 0)
