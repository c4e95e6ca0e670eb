"""Time cc_motion_estimate on one MI355X at 1080p and 2160p.

    python tools/motion_est_bench.py [--pairs 10 --range 16 --launches 20
                                      --warmup 3] [--out LOG]

8-bit luma, 10 (cur, ref) pairs per launch of consecutive frames in one
allocation, as the stage launches them.  Kernel time is the library's own
event timing (hotpath.timing_enable / timing_report("motion_estimate")),
summed over the timed launches after a warm-up.  Prints (and with --out
also writes) microseconds per pair, the SAD pixel-operations per second
that follow from the shape (blocks x 256 pixels x (2R+1)^2 candidates per
pair), and, for scale, the host-to-device time of the same planes.  There
is no earlier version of this kernel and no reference implementation to
compare with, so the tool reports and gates nothing.  Needs a GPU; there is
no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from cosmos_curate_amd import hotpath  # noqa: E402

GEOMETRIES = (("1080p", 1080, 1920), ("2160p", 2160, 3840))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--range", type=int, default=16, dest="search_range")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, r = args.pairs, args.search_range

    hotpath.require_gpu()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = [f"{n} pairs per launch, 8-bit, R={r}, lambda=4; {args.launches} timed "
             f"launches after {args.warmup} warm-up; device "
             f"{torch.cuda.get_device_name(0)}"]
    for name, h, w in GEOMETRIES:
        rng = np.random.default_rng(0)
        # a drifting random texture: real work for the search, not a flat tie
        tex = rng.integers(0, 256, size=(h + 2 * n, w + 3 * n), dtype=np.uint8)
        host = torch.from_numpy(np.stack(
            [tex[2 * k : 2 * k + h, 3 * k : 3 * k + w] for k in range(n + 1)])).pin_memory()
        frames = torch.empty_like(host, device=dev)
        nby, nbx = -(-h // 16), -(-w // 16)
        mv = torch.empty((n, nby, nbx, 2), dtype=torch.int16, device=dev)

        def run() -> None:
            hotpath.estimate_motion(
                frames.data_ptr() + h * w, frames.data_ptr(), n, h, w, w,
                mv.data_ptr(), stream, search_range=r, mv_lambda=4)

        h2d: list[float] = []
        for it in range(args.warmup + args.launches):
            if it == args.warmup:
                torch.cuda.synchronize()
                hotpath.timing_enable(True)  # resets the totals
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            frames.copy_(host, non_blocking=True)
            e1.record()
            run()
            e1.synchronize()
            if it >= args.warmup:
                h2d.append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        total_ms, count = hotpath.timing_report("motion_estimate")
        hotpath.timing_enable(False)
        if count != args.launches:
            raise RuntimeError(f"expected {args.launches} timed launches, saw {count}")
        us_pair = total_ms * 1e3 / (count * n)
        sad_ops = nby * nbx * 256 * (2 * r + 1) ** 2  # per pair
        moved = int(np.count_nonzero(mv.cpu().numpy()))
        lines.append(
            f"{name} ({h}x{w}, {nby * nbx} blocks): {us_pair:.1f} us/pair kernel "
            f"({total_ms / count:.3f} ms/launch) = {sad_ops / us_pair / 1e6:.2f} "
            f"T SAD pixel-ops/s; h2d of the {n + 1} planes "
            f"({(n + 1) * h * w / 1e6:.1f} MB, pinned) median "
            f"{float(np.median(h2d)):.3f} ms; {moved} non-zero vector components")
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
