"""Time the motion filter's score on one MI355X: the torch flow-field path
against cc_motion_score_rows / cc_motion_score_blocks.

    python tools/motion_score_bench.py [--calls 30 --warmup 3] [--out LOG]

Wall time of whole calls (host work, upload, kernels, read-back), legs
alternating in one process, median of --calls after --warmup:

  (a) check_if_small_motion(use_gpu=True)   the torch path
  (b) check_if_small_motion(backend="native")
  (c) estimate_clip_motion + (a)  against  score_clip_motion

at 1080p (10 frames of 8160 rows) and 2160p (10 frames of 32 400 rows), the
rows being blocks_to_mv_rows of a random block field (16 x 16 blocks that tile
the frame, so both paths are defined and must agree), and a batch of 32 such
1080p clips through one score_clips_native call against 32 torch calls.
Reports and gates nothing: the default backend stays torch.  Needs a GPU;
there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from cosmos_curate_amd import hotpath  # noqa: E402
from cosmos_curate_amd.pipelines.video.filtering.motion import (  # noqa: E402
    motion_estimation as me,
)
from cosmos_curate_amd.pipelines.video.filtering.motion.motion_filter_stages import (  # noqa: E402
    DecodedMotionData,
    check_if_small_motion,
    score_clips_native,
)
from cosmos_curate_amd.pipelines.video.utils import raw_backend  # noqa: E402

GEOMETRIES = (("1080p", 1080, 1920), ("2160p", 2160, 3840))
FRAMES = 10
BATCH = 32


def _alternate(legs: dict, calls: int, warmup: int) -> dict[str, float]:
    """Median wall milliseconds of each leg, the legs taking turns."""
    times: dict[str, list[float]] = {k: [] for k in legs}
    for it in range(warmup + calls):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    hotpath.require_gpu()
    lines = [f"median wall ms of {args.calls} calls after {args.warmup} warm-up, legs "
             f"alternating; device {torch.cuda.get_device_name(0)}"]
    for name, h, w in GEOMETRIES:
        rng = np.random.default_rng(0)
        nby, nbx = -(-h // 16), -(-w // 16)
        field = rng.integers(-16, 17, size=(FRAMES, nby, nbx, 2)).astype(np.int16)
        frames = [me.blocks_to_mv_rows(m, h, w) for m in field]
        # a 2 fps payload of FRAMES + 1 frames: every consecutive pair is sampled
        raw = raw_backend.make_synthetic_clip(FRAMES + 1, h, w, 2, seed=3)

        a = check_if_small_motion(frames, (h, w), use_gpu=True)
        b = check_if_small_motion(frames, (h, w), backend="native")
        legs = {
            "a torch": lambda: check_if_small_motion(frames, (h, w), use_gpu=True),
            "b native": lambda: check_if_small_motion(frames, (h, w), backend="native"),
            "c estimate+torch": lambda: (lambda d: check_if_small_motion(
                d.frames, d.frame_size, use_gpu=True))(me.estimate_clip_motion(raw)),
            "c score_clip_motion": lambda: me.score_clip_motion(raw),
        }
        med = _alternate(legs, args.calls, args.warmup)
        lines.append(
            f"{name} ({h}x{w}, {FRAMES} frames of {nby * nbx} rows): "
            + "; ".join(f"{k} {v:.3f}" for k, v in med.items())
            + f"; scores torch {a[1]:.9g}/{a[2]:.9g} native {b[1]:.9g}/{b[2]:.9g}")
        if h == 1080:
            clips = [DecodedMotionData(frames, (h, w))] * BATCH
            legs = {
                f"{BATCH} torch calls": lambda: [
                    check_if_small_motion(c.frames, c.frame_size, use_gpu=True)
                    for c in clips],
                "one score_clips_native": lambda: score_clips_native(clips),
            }
            med = _alternate(legs, max(3, args.calls // 5), 1)
            lines.append(f"{name} batch of {BATCH} clips: "
                         + "; ".join(f"{k} {v:.3f}" for k, v in med.items()))
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
