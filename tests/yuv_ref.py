"""Numpy restatement of the 8/10/12-bit 4:2:0 semi-planar -> RGB arithmetic
(cc_yuv420sp_to_rgb / cc_yuv420sp_to_rgb_resize, include/cc_hotpath.h).

Test helper, not a test.  The kernels promise bit-exact agreement with this
file: every step is f32 and in this order.

    s  = sample >> (16 - depth)                (depth 8: s = sample)
    x  = float(s) * 2^-(depth-8)               (exact in f32)
    yf = x_Y - yoff;  u = x_U - 128;  v = x_V - 128
    fy = CY*yf
    R = fy + CVR*v;  G = fy + CVG*v + CUG*u;  B = fy + CUB*u
    round with floor(x + 0.5), clamp to [0, 255]

Chroma is the nearest 2x2 co-sited sample.  The coefficient table below is
written out on its own (not derived from the kernel source); every row but
BT.601 limited is the double-precision formula rounded to f32, and BT.601
limited is the five literals the 8-bit path has always used.
"""

from __future__ import annotations

import numpy as np

MATRICES = (0, 1, 2)  # BT.601, BT.709, BT.2020-NCL
DEPTHS = (8, 10, 12)

# (Kr, Kb) per matrix code
KR_KB = {0: (0.299, 0.114), 1: (0.2126, 0.0722), 2: (0.2627, 0.0593)}

# (matrix, full_range, depth-or-None) -> (yoff, CY, CVR, CVG, CUG, CUB).
# Limited-range rows do not depend on the depth (key depth None).
COEF: dict[tuple[int, int, int | None], tuple[float, ...]] = {
    (0, 0, None): (16.0, 1.1643835, 1.5960267, -0.8129676, -0.3917623, 2.0172321),
    (1, 0, None): (16.0, 1.16438353, 1.79274106, -0.532909334, -0.21324861, 2.11240172),
    (2, 0, None): (16.0, 1.16438353, 1.6786741, -0.650424302, -0.187326103, 2.14177227),
    (0, 1, 8): (0.0, 1.0, 1.40199995, -0.714136302, -0.344136298, 1.77199996),
    (0, 1, 10): (0.0, 0.997067451, 1.39788854, -0.712042034, -0.343127102, 1.7668035),
    (0, 1, 12): (0.0, 0.996336997, 1.39686441, -0.711520374, -0.342875719, 1.76550913),
    (1, 1, 8): (0.0, 1.0, 1.57480001, -0.46812427, -0.187324271, 1.8556),
    (1, 1, 10): (0.0, 0.997067451, 1.57018185, -0.466751486, -0.186774939, 1.85015833),
    (1, 1, 12): (0.0, 0.996336997, 1.56903148, -0.466409534, -0.186638102, 1.84880292),
    (2, 1, 8): (0.0, 1.0, 1.47459996, -0.571353137, -0.164553121, 1.88139999),
    (2, 1, 10): (0.0, 0.997067451, 1.47027564, -0.569677591, -0.164070562, 1.87588274),
    (2, 1, 12): (0.0, 0.996336997, 1.46919858, -0.56926024, -0.163950369, 1.87450838),
}


def coefficients(depth: int, matrix: int, full_range: int) -> tuple[np.float32, ...]:
    """The f32 row (yoff, CY, CVR, CVG, CUG, CUB) for one configuration."""
    row = COEF[(matrix, 1, depth) if full_range else (matrix, 0, None)]
    return tuple(np.float32(c) for c in row)


def formula(depth: int, matrix: int, full_range: int) -> tuple[float, ...]:
    """The same row from the defining formula, in double precision."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        yoff = 0.0
        cy = sc = 255.0 * 2.0 ** (depth - 8) / (2.0**depth - 1.0)
    else:
        yoff, cy, sc = 16.0, 255.0 / 219.0, 255.0 / 224.0
    return (yoff, cy, 2 * (1 - kr) * sc, -2 * kr * (1 - kr) / kg * sc,
            -2 * kb * (1 - kb) / kg * sc, 2 * (1 - kb) * sc)


def _round_u8(x: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(x + np.float32(0.5)), 0, 255).astype(np.uint8)


def _samples(a: np.ndarray, depth: int) -> np.ndarray:
    """Raw plane samples (u8 at depth 8, MSB-aligned u16 otherwise) -> x."""
    if depth == 8:
        assert a.dtype == np.uint8, a.dtype
        return a.astype(np.float32)
    assert a.dtype == np.uint16, a.dtype
    s = (a >> np.uint16(16 - depth)).astype(np.float32)
    return s * np.float32(2.0 ** -(depth - 8))


def yuv420sp_to_rgb(y: np.ndarray, uv: np.ndarray, depth: int, matrix: int,
                    full_range: int) -> np.ndarray:
    """One frame: Y (H,W), interleaved UV (H/2,W) -> RGB888 (H,W,3)."""
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and uv.shape == (h // 2, w), (y.shape, uv.shape)
    yoff, cy, cvr, cvg, cug, cub = coefficients(depth, matrix, full_range)
    yf = _samples(y, depth) - yoff
    c = _samples(uv, depth).reshape(h // 2, w // 2, 2) - np.float32(128.0)
    u = np.repeat(np.repeat(c[:, :, 0], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(c[:, :, 1], 2, axis=0), 2, axis=1)
    fy = cy * yf
    r = fy + cvr * v
    g = fy + cvg * v + cug * u
    b = fy + cub * u
    assert r.dtype == g.dtype == b.dtype == np.float32
    return np.stack([_round_u8(r), _round_u8(g), _round_u8(b)], axis=-1)


def yuv420sp_to_rgb_batch(ys: np.ndarray, uvs: np.ndarray, depth: int, matrix: int,
                          full_range: int) -> np.ndarray:
    return np.stack([yuv420sp_to_rgb(ys[i], uvs[i], depth, matrix, full_range)
                     for i in range(len(ys))])
