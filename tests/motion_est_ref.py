"""Numpy restatement of the block-matching arithmetic of cc_motion_estimate
(include/cc_hotpath.h) and of the 10-column row expansion.

Test helper, not a test.  The kernel promises bit-exact agreement with this
file.  All integer:

    Y8(s)  = s for 8-bit samples, s >> 8 for 16-bit (MSB-aligned) ones
    grid   nby = ceil(h/16), nbx = ceil(w/16)
    C(y,x) = Y8(cur[min(y,h-1)][min(x,w-1)])
    R(y,x) = Y8(ref[clamp(y,0,h-1)][clamp(x,0,w-1)])
    SAD(by,bx,dx,dy) = sum_{j,i in 0..15} |C(16by+j,16bx+i) - R(16by+j+dy,16bx+i+dx)|
    cost   = SAD + lambda*(|dx|+|dy|),  dx,dy in [-R, R]
    winner = lexicographic minimum of (cost, dx^2+dy^2, dy, dx)

Written from the contract, not from the kernel: one pass per candidate over
an edge-padded plane, vectorised over blocks, with an explicit four-level
comparison instead of a packed key.
"""

from __future__ import annotations

import numpy as np

BLOCK = 16


def y8(plane: np.ndarray) -> np.ndarray:
    """(h, w) uint8 or uint16 samples -> the 8 bits the search compares."""
    if plane.dtype == np.uint8:
        return plane.astype(np.int32)
    assert plane.dtype == np.uint16, plane.dtype
    return (plane >> np.uint16(8)).astype(np.int32)


def estimate_pair(cur: np.ndarray, ref: np.ndarray, search_range: int,
                  lam: int) -> tuple[np.ndarray, np.ndarray]:
    """One (cur, ref) pair of (h, w) planes -> mv int16 (nby, nbx, 2) =
    (dx, dy) and cost uint32 (nby, nbx)."""
    assert cur.shape == ref.shape and cur.ndim == 2
    h, w = cur.shape
    r = search_range
    nby, nbx = -(-h // BLOCK), -(-w // BLOCK)
    ph, pw = nby * BLOCK, nbx * BLOCK
    c = np.pad(y8(cur), ((0, ph - h), (0, pw - w)), mode="edge")
    # R over every coordinate a candidate can touch: [-r, ph + r) x [-r, pw + r)
    rp = np.pad(y8(ref), ((r, ph - h + r), (r, pw - w + r)), mode="edge")
    cb = c.reshape(nby, BLOCK, nbx, BLOCK)

    best_cost = np.full((nby, nbx), np.iinfo(np.int64).max, dtype=np.int64)
    best_len = np.zeros((nby, nbx), dtype=np.int64)
    best_dy = np.zeros((nby, nbx), dtype=np.int64)
    best_dx = np.zeros((nby, nbx), dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            shifted = rp[r + dy : r + dy + ph, r + dx : r + dx + pw]
            sad = np.abs(cb - shifted.reshape(nby, BLOCK, nbx, BLOCK)).sum(axis=(1, 3))
            cost = sad.astype(np.int64) + lam * (abs(dx) + abs(dy))
            ln = dx * dx + dy * dy
            better = (cost < best_cost) | ((cost == best_cost) & (
                (ln < best_len) | ((ln == best_len) & (
                    (dy < best_dy) | ((dy == best_dy) & (dx < best_dx))))))
            best_cost = np.where(better, cost, best_cost)
            best_len = np.where(better, ln, best_len)
            best_dy = np.where(better, dy, best_dy)
            best_dx = np.where(better, dx, best_dx)
    mv = np.stack([best_dx, best_dy], axis=-1).astype(np.int16)
    return mv, best_cost.astype(np.uint32)


def estimate(cur: np.ndarray, ref: np.ndarray, search_range: int,
             lam: int) -> tuple[np.ndarray, np.ndarray]:
    """(n, h, w) pairs -> mv int16 (n, nby, nbx, 2), cost uint32 (n, nby, nbx)."""
    out = [estimate_pair(c, r, search_range, lam) for c, r in zip(cur, ref)]
    return np.stack([m for m, _ in out]), np.stack([c for _, c in out])


def rows(mv: np.ndarray) -> np.ndarray:
    """(nby, nbx, 2) block vectors -> (nby*nbx, 10) float32 rows, raster
    order, columns [w, h, src_x, src_y, dst_x, dst_y, flags, motion_x,
    motion_y, motion_scale] in quarter-pel units."""
    nby, nbx, _ = mv.shape
    out = []
    for by in range(nby):
        for bx in range(nbx):
            dx, dy = int(mv[by, bx, 0]), int(mv[by, bx, 1])
            dst_x, dst_y = BLOCK * bx + 8, BLOCK * by + 8
            out.append([BLOCK, BLOCK, dst_x + dx, dst_y + dy, dst_x, dst_y, 0,
                        4 * dx, 4 * dy, 4])
    return np.array(out, dtype=np.float32).reshape(-1, 10)


def textured(h: int, w: int, seed: int) -> np.ndarray:
    """Seeded random 8-bit texture."""
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def translating(n: int, h: int, w: int, seed: int, step: tuple[int, int] = (3, -2)
                ) -> np.ndarray:
    """(n, h, w) uint8 frames of one random texture whose content moves by
    ``step`` = (x, y) pixels per frame: frame k+1 at (y, x) shows what frame
    k shows at (y - step_y, x - step_x).  True translation (fresh texture
    enters at the edges), not a roll."""
    sx, sy = step
    span_x, span_y = abs(sx) * (n - 1), abs(sy) * (n - 1)
    tex = textured(h + span_y, w + span_x, seed)
    frames = np.empty((n, h, w), dtype=np.uint8)
    for k in range(n):
        oy = -sy * k if sy < 0 else span_y - sy * k
        ox = -sx * k if sx < 0 else span_x - sx * k
        frames[k] = tex[oy : oy + h, ox : ox + w]
    return frames


def static_with_noise(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """(n, h, w) uint8 frames: one texture plus fresh uniform noise in
    [-2, 2] on every frame after the first."""
    rng = np.random.default_rng(seed + 1)
    base = textured(h, w, seed).astype(np.int16)
    frames = np.empty((n, h, w), dtype=np.uint8)
    frames[0] = base
    for k in range(1, n):
        noise = rng.integers(-2, 3, size=(h, w), dtype=np.int16)
        frames[k] = np.clip(base + noise, 0, 255)
    return frames


def stripes(h: int, w: int, period: int = 8) -> np.ndarray:
    """Period-``period`` pattern along x, constant along y."""
    x = np.arange(w)
    return np.broadcast_to(((x % period) * (256 // period)).astype(np.uint8),
                           (h, w)).copy()
