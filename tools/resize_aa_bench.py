"""Time the two resize + center-crop chains of the image towers on one MI355X
at the source-resolution geometry, alternating in one process:

  antialias   cc_resize_aa_u8 through hotpath.resize_aa_center_crop: one
              kernel, reads the whole crop window (the 1080x1080x3 source
              bytes under the 224x224 crop at 1080p), writes the crop
  antialias, horizontal taps cut to 4
              the same call with every column's tap count cut to 4 in a copy
              of the x table: the copy to LDS, the barriers and the vertical
              pass stay, the horizontal loop runs one step instead of
              ceil(taps/4); the difference says what the horizontal loop costs
  cubic       today's default, cc_resize_bicubic_u8 to the full resized frame
              (224x398 at 1080p) + the crop's strided copy: touches ~16
              source pixels per output, aliases

    python tools/resize_aa_bench.py [--frames 168 --height 1080 --width 1920
                                     --size 224 --launches 30 --warmup 5]
                                    [--out LOG]

Per-launch device time from HIP events around each call on the current
stream; prints (and with --out also writes) medians, p10/p90, and for the
antialiased leg the GB/s from the bytes it must move (crop window in, crop
out) and that rate as a fraction of the 6.29 TB/s measured copy rate
(DESIGN.md §3).  The yardstick of the antialiased leg is that floor, not the
cubic leg, which reads a small fraction of the source.  Reports only, gates
nothing.  Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from cosmos_curate_amd import hotpath  # noqa: E402

COPY_RATE_GBS = 6290.0  # measured float4 copy rate, MI355X


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=168)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, h, w, size = args.frames, args.height, args.width, args.size

    lib = hotpath.require_gpu()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tabs = hotpath.resize_aa_tables("bicubic", h, w, size)

    # today's chain, with its own size arithmetic (models/clip.py)
    scale = size / min(h, w)
    rh, rw = max(size, round(h * scale)), max(size, round(w * scale))
    top, left = (rh - size) // 2, (rw - size) // 2
    full = torch.empty((n, rh, rw, 3), dtype=torch.uint8, device=dev)

    def run_aa() -> None:
        hotpath.resize_aa_center_crop(src, size, "bicubic")

    def run_cubic() -> None:
        hotpath.check(lib.cc_resize_bicubic_u8(
            src.data_ptr(), n, h, w, full.data_ptr(), rh, rw, stream))
        full[:, top:top + size, left:left + size, :].contiguous()

    # source bytes under the crop: the rows and columns the tables reach
    ty = np.frombuffer(tabs.table_y.cpu().numpy().tobytes(), dtype=np.int32)
    tx = np.frombuffer(tabs.table_x.cpu().numpy().tobytes(), dtype=np.int32)
    rows = int((ty[:size] + ty[size:2 * size]).max() - ty[:size].min())
    cols = int((tx[:size] + tx[size:2 * size]).max() - tx[:size].min())
    aa_bytes = n * (rows * cols * 3 + size * size * 3)

    # the same kernel, window and vertical pass with every column's tap count
    # cut to 4 (one step of the horizontal loop instead of ceil(taps/4)):
    # what is left is the copy to LDS, the barriers and the vertical sums
    words = np.frombuffer(tabs.table_x.cpu().numpy().tobytes(), dtype=np.int32).copy()
    words[size:2 * size] = np.minimum(words[size:2 * size], 4)
    cut_x = torch.from_numpy(words.view(np.uint8)).to(dev)
    out_cut = torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev)
    steps = -(-tabs.taps_x // 4)

    def run_aa_cut() -> None:
        hotpath.check(lib.cc_resize_aa_u8(
            src.data_ptr(), n, h, w, out_cut.data_ptr(), size, size,
            tabs.table_y.data_ptr(), tabs.taps_y, cut_x.data_ptr(), tabs.taps_x, stream))

    cut_name = f"antialias, horizontal taps cut to 4 (1 of {steps} loop steps)"
    legs = {"antialias (cc_resize_aa_u8)": run_aa,
            cut_name: run_aa_cut,
            "cubic (cc_resize_bicubic_u8 + crop)": run_cubic}
    times: dict[str, list[float]] = {k: [] for k in legs}
    for it in range(args.warmup + args.launches):
        for name, fn in legs.items():  # alternate the legs
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1))

    lines = [f"{n} frames of {h}x{w} -> {size}x{size} (resized {tabs.resized_h}x"
             f"{tabs.resized_w}, crop at {tabs.top},{tabs.left}, taps {tabs.taps_y}/"
             f"{tabs.taps_x}, window {rows}x{cols}); {args.launches} launches each after "
             f"{args.warmup} warm-up, alternating; device {torch.cuda.get_device_name(0)}"]
    for name in legs:
        t = np.array(times[name])
        med = float(np.median(t))
        line = (f"{name}: median {med:.4f} ms  min {t.min():.4f}  max {t.max():.4f}  "
                f"p10 {np.percentile(t, 10):.4f}  p90 {np.percentile(t, 90):.4f}")
        if name == "antialias (cc_resize_aa_u8)":
            gbs = aa_bytes / (med * 1e-3) / 1e9
            line += (f"  | {aa_bytes / 1e6:.1f} MB -> {gbs:.0f} GB/s = "
                     f"{gbs / COPY_RATE_GBS:.3f} of the {COPY_RATE_GBS / 1000:.2f} TB/s "
                     f"copy rate (floor {aa_bytes / COPY_RATE_GBS / 1e6:.4f} ms)")
        lines.append(line)
    t_all = float(np.median(times["antialias (cc_resize_aa_u8)"]))
    t_cut = float(np.median(times[cut_name]))
    if steps > 1:
        horiz = (t_all - t_cut) * steps / (steps - 1)
        lines.append(f"horizontal loop (all {steps} steps, from the difference): "
                     f"{horiz:.4f} ms = {horiz / t_all:.2f} of the antialiased median; "
                     f"copy to LDS, barriers, vertical sums, store: {t_all - horiz:.4f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
