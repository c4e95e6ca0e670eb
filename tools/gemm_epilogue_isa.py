"""What the compiled 256² GEMM does between a tile's last MFMA and the next
tile's first: waits, loads and stores of every
k_gemm_bf16_t256 instantiation, read from the assembly hipcc emits.

    python tools/gemm_epilogue_isa.py            # compile, print the table
    python tools/gemm_epilogue_isa.py FILE.s     # a listing made elsewhere

The "tail" of an instantiation is every basic block that is inside the
persistent (rep) loop and outside the K-loop, told by the loop depth hipcc
writes beside each block label (depth 1; the K-loop is depth 2, the first
prologue and its drain depth 0).  hipcc lays the blocks out in any order,
so the tail is a set of lines, not a range: it holds the epilogue, the next
tile's prologue and the rep-top wait, on every path.

tests/test_gemm_epilogue_isa_cpu.py asserts on the same records.  Only the
mnemonics of waits, loads and stores are read.
"""

from __future__ import annotations

import pathlib
import re
import shutil
import subprocess
import sys
import tempfile
from dataclasses import dataclass

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "cosmos_curate_amd" / "csrc" / "cc_gemm.hip"

# <ACT, HAS_BIAS, HAS_RES, EPI_STAGED, LN_IN, STATS> of the launches of a
# flagship step: qkv, fc1, and out-proj / fc2 with the statistics
FLAGSHIP = {
    "qkv": (0, 1, 0, 1, 1, 0),
    "fc1": (1, 1, 0, 1, 1, 0),
    "out-proj, fc2": (0, 1, 1, 1, 0, 1),
}

_FUNC = re.compile(r"^(_ZN\S*k_gemm_bf16_t256I(\S+?)EEv\S*):")
_ARGS = re.compile(r"L[ib](\d+)E")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_STORE = re.compile(r"^\s*(global_store|buffer_store|flat_store)_")
# a load that writes VGPRs: LDS-DMA (global_load_lds_*, "... lds") does not
_VLOAD = re.compile(r"^\s*(global_load|buffer_load|flat_load|scratch_load)_(?!lds)")


def hipcc_flags():
    sys.path.insert(0, str(ROOT))
    from cosmos_curate_amd import build

    extra = next(e for name, e in build.SOURCES if name == SRC.name)
    return [*build.COMMON, *extra]


def compile_listing(out: pathlib.Path) -> pathlib.Path:
    """cc_gemm.hip -> device assembly, with the flags of build.py."""
    cmd = ["hipcc", *hipcc_flags(), "--cuda-device-only", "-S", str(SRC),
           "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


@dataclass
class Tail:
    params: tuple
    lines: int = 0
    vmcnt0_waits: int = 0       # s_waitcnt whose vmcnt field is 0
    counted_waits: int = 0      # s_waitcnt vmcnt(N > 0)
    vgpr_loads_compiler: int = 0  # VGPR-destination loads outside asm blocks
    vgpr_loads_asm: int = 0
    lds_dma: int = 0
    stores: int = 0
    stores_under_execz: int = 0


def _functions(text):
    cur, body = None, []
    for line in text.splitlines():
        m = _FUNC.match(line)
        if m:
            cur, body = m.group(2), []
        elif cur is not None:
            body.append(line)
            if "s_endpgm" in line:
                yield tuple(int(v) for v in _ARGS.findall(cur + "E")), body
                cur = None


_BLOCK = re.compile(r"^(\.LBB\S+:|; %bb\.\d+:)")
_DEPTH = re.compile(r"Depth=(\d+)")


def _tail_lines(body):
    """Indices of the lines in blocks of loop depth 1."""
    tail, depth = [], 0
    for i, line in enumerate(body):
        s = line.strip()
        if _BLOCK.match(s):
            # the label's own comment and the comment lines under it
            notes = [s]
            for nxt in body[i + 1:]:
                if not nxt.strip().startswith(";") or "Loop" not in nxt:
                    break
                notes.append(nxt)
            depth = max((int(d) for n in notes for d in _DEPTH.findall(n)),
                        default=0)
        if depth == 1:
            tail.append(i)
    return tail


def analyse(text):
    """-> {template parameters: Tail} for every 256² instantiation."""
    out = {}
    for params, body in _functions(text):
        t = Tail(params)
        tail = set(_tail_lines(body))
        in_asm = False
        open_execz = {}  # label -> stores seen since the branch
        for i, line in enumerate(body):
            s = line.strip()
            if s.startswith(";;#ASMSTART"):
                in_asm = True
            elif s.startswith(";;#ASMEND"):
                in_asm = False
            if i not in tail:
                continue
            t.lines += 1
            if s.startswith("s_waitcnt"):
                m = _VMCNT.search(s)
                if m:
                    if int(m.group(1)) == 0:
                        t.vmcnt0_waits += 1
                    else:
                        t.counted_waits += 1
            elif "global_load_lds" in s or (s.startswith("buffer_load") and s.endswith(" lds")):
                t.lds_dma += 1
            elif _VLOAD.match(s):
                if in_asm:
                    t.vgpr_loads_asm += 1
                else:
                    t.vgpr_loads_compiler += 1
            elif _STORE.match(s):
                t.stores += 1
                if open_execz:
                    t.stores_under_execz += 1
            elif s.startswith("s_cbranch_execz"):
                open_execz[s.split()[-1]] = True
            elif s.endswith(":") or re.match(r"^\.L\S+:", s):
                open_execz.pop(s.split(":")[0], None)
        out[params] = t
    return out


def table(records):
    head = (f"{'<ACT,BIAS,RES,STAGED,LN,STATS>':32s} {'lines':>6s} {'vmcnt(0)':>8s} "
            f"{'vmcnt(N)':>8s} {'vload cc':>8s} {'vload asm':>9s} {'lds-dma':>7s} "
            f"{'stores':>6s} {'st@execz':>8s}")
    rows = [head]
    names = {v: k for k, v in FLAGSHIP.items()}
    for params, t in sorted(records.items()):
        rows.append(
            f"{str(params):32s} {t.lines:6d} {t.vmcnt0_waits:8d} {t.counted_waits:8d} "
            f"{t.vgpr_loads_compiler:8d} {t.vgpr_loads_asm:9d} {t.lds_dma:7d} "
            f"{t.stores:6d} {t.stores_under_execz:8d}  {names.get(params, '')}")
    return "\n".join(rows)


def main():
    if len(sys.argv) > 1:
        text = pathlib.Path(sys.argv[1]).read_text()
    else:
        if not shutil.which("hipcc"):
            sys.exit("hipcc not found")
        with tempfile.TemporaryDirectory() as d:
            text = compile_listing(pathlib.Path(d) / "cc_gemm.s").read_text()
    print(table(analyse(text)))


if __name__ == "__main__":
    main()
