"""Numpy restatement of the antialiased separable resize + center crop of
cc_resize_aa_table_build / cc_resize_aa_u8 (include/cc_hotpath.h).

Test helper, not a test.  It is the written definition of the chain
torchvision runs for source-resolution frames,
``Resize(size, BICUBIC | BILINEAR, antialias=True)`` + ``CenterCrop(size)``:

Sizes (torchvision): the short side becomes ``size``, the long side
``int(size * long / short)`` (truncating); the crop sits at
``int(round((resized - size) / 2.0))`` with Python's round (half to even).

Weight table per axis (torch's _compute_indices_min_size_weights_aa,
align_corners=False), everything in double:

    scale    = in_size / out_size
    support  = (interp/2)*scale if scale >= 1 else interp/2   (interp 4 | 2)
    invscale = 1/scale if scale >= 1 else 1
    taps     = 2*ceil(support) + 1
    center   = scale*(i + 0.5)
    first    = max(int(center - support + 0.5), 0)
    count    = min(int(center + support + 0.5), in_size) - first
    w[j]     = filter((j + first - center + 0.5)*invscale),  j < count

the weights divided by their double sum, rounded to f32 once, zero up to
``taps``.  Per output pixel and channel, in f32, multiply then add, no FMA:

    hrow[y] = sum_k wx[ox][k] * float(src[y][firstx[ox] + k])   k ascending from 0.0f
    v       = sum_k wy[oy][k] * hrow[firsty[oy] + k]            k ascending from 0.0f
    out     = u8(rint(min(max(v, 0), 255)))                     half to even

The kernel promises bit-exact agreement with ``resize`` fed the same tables.
"""

from __future__ import annotations

import math

import numpy as np

F32 = np.float32
BILINEAR, BICUBIC = 0, 1  # CC_RESIZE_AA_BILINEAR, CC_RESIZE_AA_BICUBIC
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC}
_INTERP = {BILINEAR: 2, BICUBIC: 4}


def output_size(h: int, w: int, size: int) -> tuple[int, int]:
    """torchvision Resize(size) of an (h, w) image -> (rh, rw)."""
    if h <= w:
        return size, int(size * w / h)
    return int(size * h / w), size


def crop_offset(resized: int, size: int) -> int:
    """torchvision CenterCrop's top / left (Python round: half to even)."""
    return int(round((resized - size) / 2.0))


def geometry(h: int, w: int, size: int) -> tuple[int, int, int, int]:
    """(rh, rw, top, left) of Resize(size) + CenterCrop(size)."""
    rh, rw = output_size(h, w, size)
    return rh, rw, crop_offset(rh, size), crop_offset(rw, size)


def _filter(filt: int, x: float) -> float:
    x = abs(x)
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5  # torch's antialias bicubic, not cv2's -0.75
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return a * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


def table(filt: int, in_size: int, out_size: int, off: int = 0,
          length: int | None = None):
    """One axis, outputs [off, off + length) -> (first i32[length],
    count i32[length], w f32[length][taps], taps)."""
    if length is None:
        length = out_size - off
    interp = _INTERP[filt]
    scale = in_size / out_size
    support = (interp / 2.0) * scale if scale >= 1.0 else interp / 2.0
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    taps = 2 * math.ceil(support) + 1
    first = np.zeros(length, dtype=np.int32)
    count = np.zeros(length, dtype=np.int32)
    w = np.zeros((length, taps), dtype=F32)
    for n, i in enumerate(range(off, off + length)):
        center = scale * (i + 0.5)
        lo = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - lo
        ws = [_filter(filt, (j + lo - center + 0.5) * invscale) for j in range(cnt)]
        total = 0.0
        for v in ws:
            total += v
        first[n], count[n] = lo, cnt
        w[n, :cnt] = np.array([v / total for v in ws], dtype=np.float64).astype(F32)
    return first, count, w, taps


def split_table(img: np.ndarray, length: int, taps: int):
    """The library's table image (bytes) -> (first, count, w)."""
    words = np.ascontiguousarray(img, dtype=np.uint8).view(np.int32)
    assert words.size == length * (2 + taps), (words.size, length, taps)
    first = words[:length].copy()
    count = words[length:2 * length].copy()
    w = words[2 * length:].view(F32).reshape(length, taps).copy()
    return first, count, w


def resize(src: np.ndarray, ty, tx) -> np.ndarray:
    """(H, W, C) u8 and the two axes' (first, count, w) -> (len_y, len_x, C)
    u8, the kernel's arithmetic."""
    assert src.dtype == np.uint8 and src.ndim == 3
    fy, cy, wy = ty[:3]
    fx, cx, wx = tx[:3]
    assert wy.dtype == F32 and wx.dtype == F32
    h, w, _ = src.shape
    assert int((fy + cy).max()) <= h and int((fx + cx).max()) <= w
    srcf = src.astype(F32)
    hrow = np.zeros((h, len(fx), src.shape[2]), dtype=F32)
    for k in range(int(cx.max())):
        live = (k < cx)[None, :, None]
        cols = np.minimum(fx + k, w - 1)
        hrow = np.where(live, hrow + wx[:, k][None, :, None] * srcf[:, cols, :], hrow)
    v = np.zeros((len(fy), len(fx), src.shape[2]), dtype=F32)
    for k in range(int(cy.max())):
        live = (k < cy)[:, None, None]
        rows = np.minimum(fy + k, h - 1)
        v = np.where(live, v + wy[:, k][:, None, None] * hrow[rows], v)
    assert v.dtype == F32
    return np.rint(np.minimum(np.maximum(v, F32(0.0)), F32(255.0))).astype(np.uint8)


def resize_full(src: np.ndarray, oh: int, ow: int, filt: int = BICUBIC) -> np.ndarray:
    """(H, W, C) u8 -> (oh, ow, C) u8, no crop."""
    h, w, _ = src.shape
    return resize(src, table(filt, h, oh), table(filt, w, ow))


def resize_center_crop(src: np.ndarray, size: int, filt: int = BICUBIC) -> np.ndarray:
    """(H, W, C) u8 -> (size, size, C) u8: Resize(size, antialias=True) +
    CenterCrop(size), computing only the cropped region."""
    h, w, _ = src.shape
    rh, rw, top, left = geometry(h, w, size)
    return resize(src, table(filt, h, rh, top, size), table(filt, w, rw, left, size))


def textured_frame(h: int, w: int, seed: int) -> np.ndarray:
    """Sinusoids, checker edges and sigma-25 noise, (h, w, 3) u8."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3), dtype=np.float64)
    for c in range(3):
        img[..., c] = (128.0 + 60.0 * np.sin(xx * (0.9 + 0.3 * c) + yy * 0.21)
                       + 40.0 * np.sin(yy * (1.3 - 0.2 * c)))
    img += 50.0 * ((((yy // 7) + (xx // 5)) % 2) - 0.5)[..., None]
    img += rng.normal(0.0, 25.0, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
