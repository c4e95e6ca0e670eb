"""Recorded hashes for the shapes that exercise the 256² GEMM K-loop schedule
(tests/test_gpu_gemm_stagger.py runs the same cases).

A change of the K-loop's schedule moves loads, waits and barriers and no
arithmetic: every accumulator receives the same MFMAs in the same order, so
C and the (sum, sum²) partials must stay bit-identical.  This script records
their SHA-256 per (shape, form), with the problems and checks of
tools/gemm_epilogue_golden.py:

    python tools/gemm_stagger_golden.py --write tests/golden/gemm_stagger_hashes.json

Run it at the commit whose results are the reference (the parent of the
change under test), never at the code under test.

The shapes are the smallest at which a schedule of the K-loop can go wrong
and which tests/test_gpu_gemm_epilogue.py does not have:

- 6 and 18 K-tiles: an odd number of K-tile pairs, so the loop ends on the
  other buffer parity than at 4, 12 or 24.  The LN forms need row statistics
  at K, which the library has at 128, 1152, 1408 and multiples of 256 and
  rejects elsewhere, so they run at K = 1152 (18 K-tiles, the smallest such
  K with an odd number of pairs) and the other forms at K = 384.
- 48 K-tiles, the fc2 K: a long steady state, with the statistics.
- 520 tiles on 256 workgroups at the minimum K: some workgroups walk three
  tiles, so the loop is entered and left three times around live epilogues
  and both copies of each table; once more with a ragged last row tile.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location(
    "gemm_epilogue_golden", ROOT / "tools" / "gemm_epilogue_golden.py")
geg = sys.modules.get(_spec.name)
if geg is None:
    geg = importlib.util.module_from_spec(_spec)
    sys.modules[_spec.name] = geg
    _spec.loader.exec_module(geg)

# (M, N, K, forms)
SHAPES = (
    (300, 1536, 384, ("bias", "res")),
    (300, 1536, 1152, ("ln0", "ln1")),
    (600, 768, 3072, ("res_stats",)),
    (16640, 2048, 256, ("bias", "res")),
    (16500, 2048, 256, ("res",)),
)

CASES = [(M, N, K, f) for M, N, K, forms in SHAPES for f in forms]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--write", metavar="JSON", required=True,
                    help="record the hashes of every case to this file")
    ap.add_argument("--recorded-at", default="unknown",
                    help="the commit the hashes come from")
    args = ap.parse_args()
    lib = geg.hotpath.require_gpu()
    hashes = {}
    for M, N, K, forms in SHAPES:
        hashes.update(geg.run_shape(lib, M, N, K, forms, None))
    doc = {
        "about": "SHA-256 of the first M rows of C (and of stats) per shape "
                 "and form; tools/gemm_stagger_golden.py --write",
        "recorded_at": args.recorded_at,
        "hashes": hashes,
    }
    pathlib.Path(args.write).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"{len(hashes)} cases recorded")


if __name__ == "__main__":
    main()
