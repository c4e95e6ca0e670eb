"""Time the YUV->RGB kernel family on one MI355X, the legs alternating in one
process: cc_nv12_to_rgb (8-bit) and cc_yuv420sp_to_rgb (10-bit P016) at the
same full-resolution geometry — one launcher, the u8 and u16 instantiations
of the same kernels — and cc_nv12_to_rgb_resize at bench.py's own geometry
(its SRC_H x SRC_W source at pitch SRC_W, 224x224 output, 21 frames x 8
clips): the first kernel of bench.py's timed region.  cc_yuv420sp_hdr_to_rgb
(10-bit PQ, BT.2020, tone-mapped) runs on the 10-bit leg's own planes, so
that leg is its yardstick: same bytes moved, plus the chain's arithmetic and
six table reads per pixel.

    python tools/yuv16_bench.py [--frames 8 --height 2160 --width 3840
                                 --launches 30 --warmup 5] [--out LOG]
                                [--legs all|full|resize|hdr]

Per-launch device time from HIP events around each launch on the current
stream; prints (and with --out also writes) medians, spread, the achieved
GB/s from the bytes the algorithm must move (Y + UV in, RGB out), and that
rate as a fraction of the 6.29 TB/s measured copy rate.  The
frame geometry options apply to the two full-resolution legs only.
--legs resize times the fused kernel alone: what ran just before a launch
moves its time (the unchanged 10-bit kernel differs by ~5 % between a
process whose 8-bit leg is slow and one whose 8-bit leg is fast), so a
before/after comparison of one leg runs that leg by itself on both sides.
--legs hdr alternates the 10-bit SDR leg, the HDR leg and the HDR leg on
constant planes (every lane reads the same table entries: the chain's
arithmetic with the table reads taken out of the picture), and prints the
HDR/SDR ratios beside the SDR leg's own (p90 - p10)/median spread.
Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from bench import FRAMES_PER_CLIP, RES, SRC_H, SRC_W  # noqa: E402
from cosmos_curate_amd import hotpath  # noqa: E402

COPY_RATE_GBS = 6290.0  # measured float4 copy rate, MI355X


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", choices=("all", "full", "resize", "hdr"), default="all")
    args = ap.parse_args()
    n, h, w = args.frames, args.height, args.width

    lib = hotpath.require_gpu()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    y8 = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=g)
    uv8 = torch.randint(0, 256, (n, h // 2, w), dtype=torch.uint8, device=dev, generator=g)
    # 16-bit planes as bytes (2 per sample): any bit pattern is a valid sample
    y16 = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device=dev, generator=g)
    uv16 = torch.randint(0, 256, (n, h // 2, 2 * w), dtype=torch.uint8, device=dev,
                         generator=g)
    out8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    out16 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    outhdr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    # mid-grey at 10 bit, MSB-aligned (0x8000 little-endian): one table entry
    yflat = torch.tensor([0x00, 0x80], dtype=torch.uint8, device=dev).repeat(n, h, w)
    uvflat = yflat[:, : h // 2].contiguous()
    tables = hotpath.hdr_tables(hotpath.HDR_TRANSFER_PQ, 203.0)
    inv_w2 = hotpath.hdr_inv_w2(1000.0, 203.0)
    rn = FRAMES_PER_CLIP * 8
    ry = torch.randint(0, 256, (rn, SRC_H, SRC_W), dtype=torch.uint8, device=dev,
                       generator=g)
    ruv = torch.randint(0, 256, (rn, SRC_H // 2, SRC_W), dtype=torch.uint8, device=dev,
                        generator=g)
    rout = torch.empty((rn, RES, RES, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run_nv12() -> None:
        hotpath.check(lib.cc_nv12_to_rgb(
            y8.data_ptr(), uv8.data_ptr(), n, h, w, w, out8.data_ptr(), stream))

    def run_p010() -> None:
        hotpath.check(lib.cc_yuv420sp_to_rgb(
            y16.data_ptr(), uv16.data_ptr(), n, h, w, 2 * w, 10, 1, 0,
            out16.data_ptr(), stream))

    def run_hdr() -> None:
        hotpath.yuv_hdr_to_rgb(
            y16.data_ptr(), uv16.data_ptr(), n, h, w, 2 * w, outhdr.data_ptr(), stream,
            tables=tables.data_ptr(), inv_w2=inv_w2, bit_depth=10, matrix=2)

    def run_hdr_flat() -> None:
        hotpath.yuv_hdr_to_rgb(
            yflat.data_ptr(), uvflat.data_ptr(), n, h, w, 2 * w, outhdr.data_ptr(),
            stream, tables=tables.data_ptr(), inv_w2=inv_w2, bit_depth=10, matrix=2)

    def run_resize() -> None:
        hotpath.check(lib.cc_nv12_to_rgb_resize(
            ry.data_ptr(), ruv.data_ptr(), rn, SRC_H, SRC_W, SRC_W, rout.data_ptr(),
            RES, RES, stream))

    # name -> (launch, bytes the algorithm must move per launch)
    sdr10, hdr10 = "yuv420sp_to_rgb (10-bit, bt709)", "yuv420sp_hdr_to_rgb (10-bit PQ, bt2020)"
    hdr10_flat = "yuv420sp_hdr_to_rgb (the same, constant planes)"
    legs = {"nv12_to_rgb (8-bit, bt601)": (run_nv12, n * h * w * 4.5),
            sdr10: (run_p010, n * h * w * 6.0),
            hdr10: (run_hdr, n * h * w * 6.0),
            hdr10_flat: (run_hdr_flat, n * h * w * 6.0),
            f"nv12_to_rgb_resize ({rn} x {SRC_H}x{SRC_W} -> {RES}x{RES})":
                (run_resize, rn * (SRC_H * SRC_W * 1.5 + RES * RES * 3))}
    if args.legs == "hdr":
        legs = {k: legs[k] for k in (sdr10, hdr10, hdr10_flat)}
    else:
        del legs[hdr10_flat]  # a diagnostic of the hdr comparison only
        if args.legs != "all":
            legs = {k: v for k, v in legs.items()
                    if ("resize" in k) == (args.legs == "resize")}
    times: dict[str, list[float]] = {k: [] for k in legs}
    for it in range(args.warmup + args.launches):
        for name, (fn, _) in legs.items():  # alternate the legs
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1))

    lines = [f"full-resolution legs: {n} frames of {h}x{w}; {args.launches} launches each "
             f"after {args.warmup} warm-up, alternating; device "
             f"{torch.cuda.get_device_name(0)}"]
    for name, (_, nbytes) in legs.items():
        t = np.array(times[name])
        med = float(np.median(t))
        gbs = nbytes / (med * 1e-3) / 1e9
        lines.append(
            f"{name}: median {med:.4f} ms  min {t.min():.4f}  max {t.max():.4f}  "
            f"p10 {np.percentile(t, 10):.4f}  p90 {np.percentile(t, 90):.4f}  | "
            f"{nbytes / 1e6:.1f} MB -> {gbs:.0f} GB/s = {gbs / COPY_RATE_GBS:.3f} of "
            f"the {COPY_RATE_GBS / 1000:.2f} TB/s copy rate")
    if sdr10 in legs and hdr10 in legs:
        s = np.array(times[sdr10])
        sm = float(np.median(s))
        spread = float(np.percentile(s, 90) - np.percentile(s, 10)) / sm
        for name in (hdr10, hdr10_flat):
            if name in legs:
                lines.append(f"{name} / {sdr10}: "
                             f"{float(np.median(times[name])) / sm:.3f} of the SDR "
                             f"median; the SDR leg's own (p90 - p10)/median is {spread:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
