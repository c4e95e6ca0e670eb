"""The motion filter's score in plain numpy, float64 throughout: the contract
cc_motion_score_rows is tested against (include/cc_hotpath.h).

Rows paint sequentially, pass-major (the position of a row's block size in
BLOCK_OPTIONS) and in row order inside a pass, so the later write is the row
with the highest (pass, row index).  Pixels are clamp(dst + o, 0, N-1) with
the add in float32, then truncated.  Magnitudes, sums and the bilinear blend
are float64 computed from the float32 row values.
"""

import numpy as np

BLOCK_OPTIONS = ((8, 8), (16, 16), (16, 8), (8, 16))


def _paint(mv, h, w):
    mag = np.zeros((h, w))
    mv = np.asarray(mv, dtype=np.float32).reshape(-1, 10)
    for bw, bh in BLOCK_OPTIONS:
        for r in mv[(mv[:, 0] == bw) & (mv[:, 1] == bh)]:
            xs = np.clip(r[4] + np.arange(-(bw // 2), bw // 2, dtype=np.float32), 0, w - 1)
            ys = np.clip(r[5] + np.arange(-(bh // 2), bh // 2, dtype=np.float32), 0, h - 1)
            s = float(r[9]) or 1.0
            mag[ys.astype(np.int64)[:, None], xs.astype(np.int64)] = (
                np.hypot(float(r[7]) / s, float(r[8]) / s) / (h + w))
    return mag


def _axis(n, o):
    s = (np.arange(o) + 0.5) * (n / o) - 0.5
    c0 = np.clip(np.floor(s), 0, n - 1).astype(np.int64)
    return c0, np.minimum(c0 + 1, n - 1), np.clip(s - c0, 0, 1)


def score(frames, h, w, oh, ow):
    """(per_patch_min, global_mean) of one clip of (n, 10) float32 MV arrays."""
    if not len(frames):
        return 0.0, 0.0
    total = np.zeros((h, w))
    for mv in frames:
        total += _paint(mv, h, w)
    avg = total / len(frames)
    y0, y1, wy = _axis(h, oh)
    x0, x1, wx = _axis(w, ow)
    top = avg[y0][:, x0] * (1 - wx) + avg[y0][:, x1] * wx
    bot = avg[y1][:, x0] * (1 - wx) + avg[y1][:, x1] * wx
    patches = top * (1 - wy)[:, None] + bot * wy[:, None]
    return float(patches.min()), float(total.sum() / (len(frames) * h * w))
