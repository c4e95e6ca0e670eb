"""Time the TransNetV2 shot detector (stand-in weights) on one MI355X: the
route the stage runs by default against a torch bf16 trunk, the native bf16
trunk with torch heads and the native trunk with native heads, the legs
alternating in one process.

    python tools/transnet_bench.py [--windows 1,8,16 --forwards 30
                                    --warmup 5 --video-frames 1600] [--out LOG]

Per number of 100-frame windows W the legs are, eager, on the same u8
windows, each leg twice ("a" and "b") so the run-to-run spread is on the
page:
  - torch f32 per window: ``_TransNetV2`` as f32 nn.Conv3d, one window per
    call, W calls (what the stage does by default),
  - torch bf16 channels_last: the same trunk modules in bf16 and
    channels_last_3d, W windows in one forward, f32 heads on its features,
  - native: ``TransNetV2(backend="native")``, W windows in one forward, the
    torch heads one window at a time,
  - native, native heads: ``TransNetV2(backend="native", heads="native")``,
    trunk and heads for W windows in one pass.
Device time from HIP events around each launch of a leg; median, min, max.
Then the kernel-time split of a native forward (and of one with native heads)
from the library's own timers (cc_timing_*) and the trunk's achieved FLOP/s: 2*M*N*K over the six DDCNN
blocks (about 82 GFLOP per window) over that kernel time.

Last, the stage's three routes end to end on one synthetic (N, 27, 48, 3)
video, host clock around ``_get_predictions`` / ``_get_predictions_native``
(all end in a device-to-host copy), alternating, each twice.

Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import copy
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from cosmos_curate_amd import hotpath  # noqa: E402
from cosmos_curate_amd.models.transnetv2 import TransNetV2  # noqa: E402
from cosmos_curate_amd.pipelines.video.clipping import (  # noqa: E402
    transnetv2_extraction_stages as tstages,
)

TIMERS = ("conv3x3", "tconv3", "avgpool")
HEAD_TIMERS = ("tn_hist512", "tn_framesim_embed", "tn_simband_fc", "tn_fc1_relu",
               "tn_cls_sigmoid")


def trunk_flop_per_frame() -> float:
    """2*M*N*K of the six DDCNN blocks on one 27x48 frame."""
    total = 0.0
    cin, h, w = 3, 27, 48
    for f in (16, 32, 64):
        for block_in in (cin, 4 * f):
            total += 2.0 * h * w * (9 * block_in * 8 * f + 4 * f * 3 * 2 * f)
        cin, h, w = 4 * f, h // 2, w // 2
    return total


def _timed(legs: dict, warmup: int, forwards: int) -> dict[str, np.ndarray]:
    """Alternate the legs; per-launch HIP-event times (ms) after warm-up."""
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


def _twice(legs: dict) -> dict:
    return {f"{k} ({r})": fn for r in "ab" for k, fn in legs.items()}


def _summary(times: dict[str, np.ndarray], base: str, unit_count: float, unit: str) -> list[str]:
    """One line per leg and repeat, then per leg the spread between its
    repeats and its ratio to ``base`` (medians of the two repeats averaged)."""
    lines = []
    names = sorted({k[:-4] for k in times}, key=[k[:-4] for k in times].index)
    med = {n: [float(np.median(times[f"{n} ({r})"])) for r in "ab"] for n in names}
    for n in names:
        for r, m in zip("ab", med[n]):
            t = times[f"{n} ({r})"]
            lines.append(f"  {n} ({r}): median {m:.3f} ms  min {t.min():.3f}  max {t.max():.3f}"
                         f"  | {unit_count / (m * 1e-3):.1f} {unit}")
    bm = float(np.mean(med[base]))
    for n in names:
        a, b = med[n]
        lines.append(f"  {n}: repeats differ by {abs(a - b) / min(a, b) * 100:.1f}%; "
                     f"{bm / np.mean(med[n]):.2f}x {base}")
    return lines


def _kernel_split(fn, timers: tuple[str, ...], reps: int = 3) -> dict[str, tuple[float, int]]:
    """Per-forward (ms, launches) of each timer over ``reps`` forwards."""
    hotpath.timing_enable(True)  # also clears the totals
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        total = {n: hotpath.timing_report(n) for n in timers}
    finally:
        hotpath.timing_enable(False)
    return {n: (ms / reps, count // reps) for n, (ms, count) in total.items()}


def bench_windows(torch_model, native_model, heads_model, trunk16, nwin: int, warmup: int,
                  forwards: int) -> list[str]:
    gen = torch.Generator().manual_seed(nwin)
    x = torch.randint(0, 256, (nwin, 100, 27, 48, 3), generator=gen, dtype=torch.uint8).cuda()
    net = torch_model._model

    def f32_per_window():
        return torch.cat([torch_model(x[i:i + 1]) for i in range(nwin)])

    @torch.no_grad()
    def bf16_cl():
        y = (x.permute(0, 4, 1, 2, 3).float() / 255.0).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last_3d)
        feats = []
        for stack in trunk16:
            y = stack(y)
            feats.append(y.float())
        return net.heads(x, feats)

    def native():
        return native_model(x)

    def native_heads():
        return heads_model(x)

    legs = {"torch f32 per window": f32_per_window, "torch bf16 channels_last": bf16_cl,
            "native": native, "native, native heads": native_heads}
    outs = {k: fn()[..., 0].float() for k, fn in legs.items()}
    torch.cuda.synchronize()
    dev = {k: float((v - outs["torch f32 per window"]).abs().max()) for k, v in outs.items()}

    times = _timed(_twice(legs), warmup, forwards)
    lines = [f"{nwin} window(s) of 100 frames; max |prediction - torch f32|: "
             f"bf16 channels_last {dev['torch bf16 channels_last']:.2e}, native {dev['native']:.2e}, "
             f"native heads {dev['native, native heads']:.2e}; max |native heads - native| "
             f"{float((outs['native, native heads'] - outs['native']).abs().max()):.2e}"]
    lines += _summary(times, "torch f32 per window", nwin, "windows/s")
    nmed = float(np.mean([np.median(times[f"native ({r})"]) for r in "ab"]))
    lines.append(f"  native: {nwin * 50 / (nmed * 1e-3):.0f} source frames/s "
                 f"(50 kept of each window's 100)")
    hmeds = [float(np.median(times[f"native, native heads ({r})"])) for r in "ab"]
    nmeds = [float(np.median(times[f"native ({r})"])) for r in "ab"]
    hmed = float(np.mean(hmeds))
    spread = abs(nmeds[0] - nmeds[1])
    lines.append(f"  native, native heads: {nwin * 50 / (hmed * 1e-3):.0f} source frames/s; "
                 f"{nmed - hmed:+.3f} ms against native ({nmed / hmed:.2f}x), native's own "
                 f"repeat spread {spread:.3f} ms -> "
                 f"{'faster' if nmed - hmed > spread else 'KNOWN LOSS: not faster by more than the spread'}")

    split = _kernel_split(native, TIMERS)
    ktotal = sum(ms for ms, _ in split.values())
    flop = trunk_flop_per_frame() * 100 * nwin
    lines.append(f"  native kernel time per forward (library timers, 3 forwards): "
                 f"{ktotal:.3f} ms of the {nmed:.3f} ms forward; trunk {flop / 1e9:.1f} GFLOP "
                 f"-> {flop / (ktotal * 1e-3) / 1e12:.1f} TFLOP/s achieved")
    for n, (ms, count) in split.items():
        lines.append(f"    {n}: {ms:.3f} ms in {count} launches, "
                     f"{100 * ms / ktotal:.1f}% of the kernel time")
    split = _kernel_split(native_heads, TIMERS + HEAD_TIMERS)
    ktotal = sum(ms for ms, _ in split.values())
    htotal = sum(split[n][0] for n in HEAD_TIMERS)
    lines.append(f"  native, native heads kernel time per forward: {ktotal:.3f} ms "
                 f"({100 * ktotal / hmed:.1f}%) of the {hmed:.3f} ms forward; head kernels "
                 f"{htotal:.3f} ms")
    for n, (ms, count) in split.items():
        lines.append(f"    {n}: {ms:.3f} ms in {count} launches, "
                     f"{100 * ms / ktotal:.1f}% of the kernel time")
    return lines


def bench_stage(torch_model, native_model, heads_model, n_frames: int, runs: int) -> list[str]:
    gen = np.random.default_rng(1)
    # slowly varying content with a few cuts, so windows differ
    base = gen.integers(0, 256, (8, 27, 48, 3), dtype=np.uint8)
    frames = base[(np.arange(n_frames) * 8) // n_frames].copy()
    frames[:, :, :, 0] += (np.arange(n_frames) % 7).astype(np.uint8)[:, None, None]
    routes = {"stage route torch (f32, one window per call)":
              lambda: tstages._get_predictions(torch_model, frames, 0.4),
              "stage route native":
              lambda: tstages._get_predictions_native(native_model, frames, 0.4),
              "stage route native, native heads":
              lambda: tstages._get_predictions_native(heads_model, frames, 0.4)}
    flags = list({k: fn() for k, fn in routes.items()}.values())
    same = all(np.array_equal(flags[0], f) for f in flags[1:])
    times: dict[str, list[float]] = {f"{k} ({r})": [] for r in "ab" for k in routes}
    for r in "ab":
        for _ in range(runs):
            for k, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[f"{k} ({r})"].append((time.perf_counter() - t0) * 1e3)
    arr = {k: np.array(v) for k, v in times.items()}
    lines = [f"stage routes on one {n_frames}-frame video "
             f"({len(list(tstages._get_batches(frames)))} windows), host clock, median of {runs}; "
             f"flags identical: {same}"]
    lines += _summary(arr, "stage route torch (f32, one window per call)", n_frames,
                      "source frames/s")
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="1,8,16", help="comma-separated window counts")
    ap.add_argument("--forwards", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--video-frames", type=int, default=1600)
    ap.add_argument("--stage-runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    hotpath.require_gpu()
    torch_model = TransNetV2()
    torch_model.setup()
    native_model = TransNetV2(backend="native")
    native_model.setup()
    heads_model = TransNetV2(backend="native", heads="native")
    heads_model.setup()
    trunk16 = copy.deepcopy(torch_model._model.SDDCNN).to(torch.bfloat16).to(
        memory_format=torch.channels_last_3d)

    lines = [f"{args.forwards} launches per leg after {args.warmup} warm-up, legs alternating "
             f"in one process, each leg twice; device {torch.cuda.get_device_name(0)}; "
             f"trunk {trunk_flop_per_frame() / 1e9:.3f} GFLOP per frame"]
    for nwin in (int(w) for w in args.windows.split(",")):
        lines += bench_windows(torch_model, native_model, heads_model, trunk16, nwin, args.warmup,
                               args.forwards)
    lines += bench_stage(torch_model, native_model, heads_model, args.video_frames, args.stage_runs)
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
