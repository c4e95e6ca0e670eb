"""Derive a small committed fixture from a real H.264 MP4.

    python -m oracle.make_sparse_mp4 IN.mp4 tests/golden/NAME.sparse.mp4.xz

The container tests never decode pixels: they read the sample tables,
the parameter sets and the first bytes of each slice (slice header ->
picture order count), and compare a few whole samples byte for byte.
So the fixture keeps the file's size and layout, every box outside mdat,
every NAL length prefix and the first KEEP bytes of every NAL, and whole
samples at the indices in WHOLE; the rest of each NAL payload becomes
0xFF (never a start code, never an emulation-prevention pattern), which
xz then shrinks to a few tens of KB.  tests/golden_videos.py loads it.
"""

from __future__ import annotations

import lzma
import pathlib
import sys

from oracle import mp4_demux

KEEP = 64  # bytes of each NAL kept after its 4-byte length prefix


def whole_samples(n: int) -> set[int]:
    return {i for i in (0, 1, 100, 239, n // 2, n - 1) if 0 <= i < n}


def sparsify(data: bytes) -> bytes:
    trk = mp4_demux.parse_mp4(data)[0]
    buf = bytearray(data)
    whole = whole_samples(len(trk.sizes))
    for i, (off, size) in enumerate(zip(trk.offsets, trk.sizes)):
        if i in whole:
            continue
        p, end = off, off + size
        while p + 4 <= end:
            n = int.from_bytes(data[p:p + 4], "big")
            assert p + 4 + n <= end, f"sample {i}: NAL overruns the sample"
            if n > KEEP:
                buf[p + 4 + KEEP:p + 4 + n] = b"\xff" * (n - KEEP)
            p += 4 + n
        assert p == end, f"sample {i}: trailing bytes after the last NAL"
    return bytes(buf)


def main() -> None:
    src, dst = map(pathlib.Path, sys.argv[1:3])
    out = lzma.compress(sparsify(src.read_bytes()), preset=9 | lzma.PRESET_EXTREME)
    dst.write_bytes(out)
    print(f"{dst}: {len(out)} bytes")


if __name__ == "__main__":
    main()
