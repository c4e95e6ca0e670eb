"""Numpy restatement of the PQ (HDR10) -> SDR chain of cc_yuv420sp_hdr_to_rgb
/ cc_yuv420sp_hdr_to_rgb_resize (include/cc_hotpath.h).

Test helper, not a test.  The kernels promise bit-exact agreement with
``chain_f32``: every step is f32 and in this order, and the only
transcendental steps are two tables the caller passes in (the library's own,
in the GPU tests, so that no libm detail can enter).

    r8, g8, b8   the three f32 values tests/yuv_ref.py rounds to u8
    i  = clip(floor(c8*16 + 0.5), 0, 4080);  L = tin[i]       inverse PQ
    BT.2020 -> BT.709 linear, row = (m0*R + m1*G) + m2*B, then max(., 0)
    m  = max(max(r, g), b);  s = (1 + m*inv_w2) / (1 + m)
    c  = min(c*s, 1)                                extended Reinhard
    y  = sqrt(sqrt(c));  j = floor(y*4095 + 0.5);  out = tout[j]

``tables`` restates the two tables in double; ``chain_f64`` is the closed
form in float64 (pow instead of tables) that shares the quantisation of the
PQ index, which is part of the definition.
"""

from __future__ import annotations

import numpy as np

import yuv_ref

F32 = np.float32
N_IN = 4081  # used entries of tin: the 12-bit grid of the 8-bit scale
N_TAB = 4096  # entries of each table in the image
TABLE_BYTES = 5 * N_TAB

# SMPTE ST 2084
M1 = 2610.0 / 16384.0
M2 = 2523.0 / 4096.0 * 128.0
C1 = 3424.0 / 4096.0
C2 = 2413.0 / 4096.0 * 32.0
C3 = 2392.0 / 4096.0 * 32.0

# BT.2087 BT.2020 -> BT.709, linear light
GAMUT = ((1.6605, -0.5876, -0.0728),
         (-0.1246, 1.1329, -0.0083),
         (-0.0182, -0.1006, 1.1187))


def pq_eotf_nits(e: np.ndarray) -> np.ndarray:
    """PQ code value in [0, 1] -> luminance in nits (float64)."""
    p = np.power(np.asarray(e, dtype=np.float64), 1.0 / M2)
    return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def tables(white: float = 203.0) -> tuple[np.ndarray, np.ndarray]:
    """(tin f32[4096], tout u8[4096]) as cc_hdr_tables_build defines them."""
    tin = np.zeros(N_TAB, dtype=F32)
    tin[:N_IN] = (pq_eotf_nits(np.arange(N_IN) / (N_IN - 1.0)) / white).astype(F32)
    j = np.arange(N_TAB) / (N_TAB - 1.0)
    tout = np.floor(255.0 * np.power(j, 4.0 / 2.4) + 0.5).astype(np.uint8)
    return tin, tout


def split_image(img: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The library's table image (uint8[20480]) -> (tin, tout)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.shape == (TABLE_BYTES,), img.shape
    return img[: 4 * N_TAB].view(F32).copy(), img[4 * N_TAB:].copy()


def inv_w2(peak: float, white: float = 203.0) -> np.float32:
    return F32(1.0 / (peak / white) ** 2)


def _pq_index(c8: np.ndarray) -> np.ndarray:
    x = np.asarray(c8, dtype=F32)
    return np.clip(np.floor(x * F32(16.0) + F32(0.5)), F32(0.0),
                   F32(N_IN - 1)).astype(np.int32)


def chain_f32(rgb8: np.ndarray, tin: np.ndarray, tout: np.ndarray,
              iw2: np.float32) -> np.ndarray:
    """(..., 3) f32 R'G'B' on the 8-bit scale -> (..., 3) u8, the kernel's
    arithmetic."""
    assert tin.dtype == F32 and tout.dtype == np.uint8
    iw2 = F32(iw2)
    lin = tin[_pq_index(rgb8)]
    lr, lg, lb = lin[..., 0], lin[..., 1], lin[..., 2]
    ch = []
    for m0, m1, m2 in GAMUT:
        v = (F32(m0) * lr + F32(m1) * lg) + F32(m2) * lb
        ch.append(np.maximum(v, F32(0.0)))
    m = np.maximum(np.maximum(ch[0], ch[1]), ch[2])
    s = (F32(1.0) + m * iw2) / (F32(1.0) + m)
    out = []
    for c in ch:
        v = np.minimum(c * s, F32(1.0))
        y = np.sqrt(np.sqrt(v))
        assert y.dtype == F32
        j = np.floor(y * F32(N_TAB - 1) + F32(0.5)).astype(np.int32)
        out.append(tout[j])
    return np.stack(out, axis=-1)


def chain_f64(rgb8: np.ndarray, peak: float, white: float = 203.0) -> np.ndarray:
    """The same chain in float64 closed form, unrounded (..., 3) on the
    0..255 scale.  Shares the PQ index quantisation with chain_f32; nothing
    else is quantised."""
    e = _pq_index(rgb8).astype(np.float64) / (N_IN - 1.0)
    lin = pq_eotf_nits(e) / white
    c = np.maximum(lin @ np.array(GAMUT, dtype=np.float64).T, 0.0)
    m = c.max(axis=-1, keepdims=True)
    w = peak / white
    s = (1.0 + m / (w * w)) / (1.0 + m)
    return 255.0 * np.power(np.minimum(c * s, 1.0), 1.0 / 2.4)


def rgb_prime(y: np.ndarray, uv: np.ndarray, depth: int, matrix: int,
              full_range: int) -> np.ndarray:
    """One frame: Y (H,W), interleaved UV (H/2,W) -> unrounded f32 R'G'B'
    (H,W,3) on the 8-bit scale: yuv_ref.yuv420sp_to_rgb's expressions up to,
    not including, its rounding."""
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and uv.shape == (h // 2, w), (y.shape, uv.shape)
    yoff, cy, cvr, cvg, cug, cub = yuv_ref.coefficients(depth, matrix, full_range)
    yf = yuv_ref._samples(y, depth) - yoff
    c = yuv_ref._samples(uv, depth).reshape(h // 2, w // 2, 2) - F32(128.0)
    u = np.repeat(np.repeat(c[:, :, 0], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(c[:, :, 1], 2, axis=0), 2, axis=1)
    fy = cy * yf
    rgb = np.stack([fy + cvr * v, fy + cvg * v + cug * u, fy + cub * u], axis=-1)
    assert rgb.dtype == F32
    return rgb


def yuv420sp_hdr_to_rgb(y: np.ndarray, uv: np.ndarray, depth: int, matrix: int,
                        full_range: int, tin: np.ndarray, tout: np.ndarray,
                        iw2: np.float32) -> np.ndarray:
    """One frame -> tone-mapped RGB888 (H,W,3)."""
    return chain_f32(rgb_prime(y, uv, depth, matrix, full_range), tin, tout, iw2)


def yuv420sp_hdr_to_rgb_batch(ys: np.ndarray, uvs: np.ndarray, depth: int,
                              matrix: int, full_range: int, tin: np.ndarray,
                              tout: np.ndarray, iw2: np.float32) -> np.ndarray:
    return np.stack([yuv420sp_hdr_to_rgb(ys[i], uvs[i], depth, matrix, full_range,
                                         tin, tout, iw2)
                     for i in range(len(ys))])
