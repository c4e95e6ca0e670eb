"""Real H.264 MP4 fixtures, committed as tests/golden/*.sparse.mp4.xz.

Each is the original file with its box layout, sample tables, parameter
sets, NAL length prefixes, slice headers and a few whole samples intact
and the remaining slice payload blanked (oracle/make_sparse_mp4.py), so
demux / remux / bitstream-pin tests read exactly what they read from the
originals while the repository stays small.

  test_clip_10s, test_video_30s   854x480 24 fps Sintel excerpts, one IDR
  cockatoo, realshort             ffmpeg sample streams; cockatoo carries
                                  B-frames (275/280 nonzero ctts entries)
"""

from __future__ import annotations

import functools
import lzma
import pathlib

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
NAMES = ("test_clip_10s", "test_video_30s", "cockatoo", "realshort")


@functools.lru_cache(maxsize=None)
def video_bytes(name: str) -> bytes:
    assert name in NAMES, name
    return lzma.decompress((GOLDEN / f"{name}.sparse.mp4.xz").read_bytes())
