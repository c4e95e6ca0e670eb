"""Time the full InternVideo2-1B vision tower (40 blocks, stand-in weights)
on one MI355X: the native tower against the same tower written with torch
ops in bf16, the legs alternating in one process.

    python tools/iv2_bench.py [--clips 8 --frames 4,8 --forwards 30
                               --warmup 5 --layers 40] [--out LOG]

Per number of frames T (4 = 1025 tokens per clip, 8 = 2049) the legs are,
eager, on the same pixels:
  - native, norms folded (InternVideo2VisionTowerAMD),
  - native with fold_ln = False (cc_rmsnorm / cc_layernorm + plain GEMMs),
  - torch bf16: tests/iv2_ref.py's module moved to the device in bf16 — the
    yardstick.
Per-forward device time from HIP events around each forward; median, min,
max, p10, p90.  Each native leg's embeddings are first compared with the
yardstick's (cosine).  Then the kernel-time split of a folded forward from
the library's own timers (cc_timing_*): GEMM, attention, qk-norm,
statistics + finalize; the rest of the forward is torch glue (embedding
assembly, pooling head).

The stand-in position table is made for the largest T and cut to each
smaller one.  Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import dataclasses
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import iv2_ref  # noqa: E402
from cosmos_curate_amd import hotpath  # noqa: E402
from cosmos_curate_amd.models import internvideo2_weights as iw  # noqa: E402
from cosmos_curate_amd.models.internvideo2_vit import (  # noqa: E402
    InternVideo2VisionTowerAMD,
)

TIMERS = {
    "GEMM": ("gemm_bf16",),
    "attention": ("attn_small", "attn_mid", "attn_flash"),
    "qk-norm": ("qk_rmsnorm",),
    "stats + finalize": ("ln_stats", "ln_finalize"),
}


def _timed(legs: dict, warmup: int, forwards: int) -> dict[str, np.ndarray]:
    """Alternate the legs; per-forward HIP-event times (ms) after warm-up."""
    times: dict[str, list[float]] = {k: [] for k in legs}
    for it in range(warmup + forwards):
        for name, fn in legs.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: np.array(v) for k, v in times.items()}


def _stat_line(name: str, t: np.ndarray, extra: str = "") -> str:
    return (f"  {name}: median {np.median(t):.3f} ms  min {t.min():.3f}  "
            f"max {t.max():.3f}  p10 {np.percentile(t, 10):.3f}  "
            f"p90 {np.percentile(t, 90):.3f}{extra}")


def bench(sd_max: dict, cfg_max, T: int, clips: int, warmup: int,
          forwards: int) -> list[str]:
    cfg = dataclasses.replace(cfg_max, num_frames=T)
    sd = dict(sd_max)
    sd["vision_encoder.pos_embed"] = sd["vision_encoder.pos_embed"][:, :cfg.num_pos]
    tower = InternVideo2VisionTowerAMD(sd, cfg).cuda()
    ref = iv2_ref.InternVideo2Ref(sd, cfg).to("cuda", torch.bfloat16)
    g = torch.Generator().manual_seed(T)
    px = torch.randn(clips, T, 3, cfg.image, cfg.image, generator=g).to(
        torch.bfloat16).cuda()

    def native(fold: bool):
        def fn() -> torch.Tensor:
            tower.fold_ln = fold
            return tower(px)
        return fn

    legs = {"native, norms folded": native(True),
            "native, fold_ln=False": native(False),
            "torch bf16 (yardstick)": lambda: ref(px)}
    outs = {k: fn().float() for k, fn in legs.items()}
    torch.cuda.synchronize()
    yard = outs["torch bf16 (yardstick)"]
    cos = {k: torch.sum(v * yard, dim=1).min().item() for k, v in outs.items()}

    times = _timed(legs, warmup, forwards)
    lines = [f"tower: {cfg.name}, {cfg.layers} blocks, eager, {clips} clips x T = {T} "
             f"({cfg.num_pos} tokens per clip); per-clip cosine with the yardstick, "
             f"min: folded {cos['native, norms folded']:.6f}, unfolded "
             f"{cos['native, fold_ln=False']:.6f}"]
    ty = times["torch bf16 (yardstick)"]
    ymed = float(np.median(ty))
    spread = float((np.percentile(ty, 90) - np.percentile(ty, 10)) / ymed)
    for name, t in times.items():
        med = float(np.median(t))
        lines.append(_stat_line(
            name, t, f"  | {clips / (med * 1e-3):.1f} clips/s, {ymed / med:.2f}x yardstick"))
    fmed = float(np.median(times["native, norms folded"]))
    verdict = "holds" if fmed <= ymed * (1.0 + spread) else "DOES NOT HOLD"
    lines.append(f"  yardstick spread (p90 - p10) / median = {spread:.4f}; native folded "
                 f"is {fmed / ymed:.3f} of the yardstick: 'not slower by more than the "
                 f"yardstick's own spread' {verdict}")

    # kernel-time split of a folded forward, from the library's timers
    reps = 3
    tower.fold_ln = True
    hotpath.timing_enable(True)
    try:
        for _ in range(reps):
            tower(px)
        torch.cuda.synchronize()
        split = {k: sum(hotpath.timing_report(n)[0] for n in names) / reps
                 for k, names in TIMERS.items()}
        counts = {k: sum(hotpath.timing_report(n)[1] for n in names) // reps
                  for k, names in TIMERS.items()}
    finally:
        hotpath.timing_enable(False)
    total = sum(split.values())
    lines.append(f"  kernel time per folded forward (library timers, {reps} forwards): "
                 f"{total:.3f} ms in native kernels of the {fmed:.3f} ms forward")
    for k, ms in split.items():
        lines.append(f"    {k}: {ms:.3f} ms in {counts[k]} launches, "
                     f"{100 * ms / fmed:.1f}% of the forward")
    del tower, ref
    torch.cuda.empty_cache()
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", default="4,8", help="comma-separated T values")
    ap.add_argument("--forwards", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=iw.INTERNVIDEO2_1B.layers)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    hotpath.require_gpu()
    Ts = [int(t) for t in args.frames.split(",")]
    cfg_max = dataclasses.replace(iw.INTERNVIDEO2_1B, layers=args.layers,
                                  num_frames=max(Ts))
    sd_max = iw.make_internvideo2_weights(cfg_max)
    lines = [f"{args.forwards} forwards per leg after {args.warmup} warm-up, legs "
             f"alternating in one process; device {torch.cuda.get_device_name(0)}"]
    for T in Ts:
        lines += bench(sd_max, cfg_max, T, args.clips, args.warmup, args.forwards)
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
