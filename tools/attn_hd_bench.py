"""Time cc_attn above head dim 64 against torch sdpa on one MI355X, the legs
alternating in one process, and the whole SigLIP-so400m-224 tower with
native attention against the forced-sdpa route.

    python tools/attn_hd_bench.py [--frames 64 --heads 16 --hd 72
                                   --seqs 256,729 --launches 30 --warmup 5]
                                  [--tower-frames 64 | --no-tower] [--out LOG]

Per sequence length the legs are, on the same fused-QKV tensor:
  - cc_attn (the rung cc::attn_plan picks),
  - every other rung that can cover the length, through cc_attn_rung — the
    evidence for the rung rule in csrc/cc_attn_plan.hpp,
  - torch sdpa with the permutes the encoder's torch route pays
    (VitEncoderAMD._attention: three strided views in, one permute copy out).
The defaults are the so400m layers: 16 heads of 72 at 256 tokens (224 px)
and at 729 (384 px).  Per-launch device time from HIP events around each
launch on the current stream; median, min, max, p10, p90 and the achieved
TFLOP/s from the 4*seq^2*hd flops per (frame, head) the algorithm needs.
Each leg's output is first compared with sdpa (rtol = atol = 2e-2).

The tower legs run siglip_so400m_14_224 (27 layers, deterministic stand-in
weights) eagerly on one batch of frames, the same tower object with
force_sdpa off and on, alternating; forced sdpa also turns the LayerNorm
fold off, as the encoder does for head dims cc_attn does not take, so the
difference is the whole native route against the whole torch-attention
route.  Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import ctypes
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from cosmos_curate_amd import hotpath  # noqa: E402


def _timed(legs: dict, warmup: int, launches: int) -> dict[str, np.ndarray]:
    """Alternate the legs; per-launch HIP-event times (ms) after warm-up."""
    times: dict[str, list[float]] = {k: [] for k in legs}
    for it in range(warmup + launches):
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
    return (f"  {name}: median {np.median(t):.4f} ms  min {t.min():.4f}  "
            f"max {t.max():.4f}  p10 {np.percentile(t, 10):.4f}  "
            f"p90 {np.percentile(t, 90):.4f}{extra}")


def bench_attention(lib, n: int, heads: int, hd: int, seq: int, warmup: int,
                    launches: int) -> list[str]:
    hidden = heads * hd
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seq)
    qkv = (torch.randn(n * seq, 3 * hidden, device=dev, generator=g) * 0.5).to(
        torch.bfloat16)
    scale = hd ** -0.5
    stream = torch.cuda.current_stream(dev).cuda_stream
    planned = hotpath.attn_plan(n, seq, heads, hidden).rung

    def sdpa() -> torch.Tensor:
        t = qkv.reshape(n, seq, 3, heads, hd)
        q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale)
        return o.permute(0, 2, 1, 3).reshape(n * seq, hidden)

    outs: dict[str, torch.Tensor] = {}

    def native(rung: int):
        out = torch.empty((n * seq, hidden), dtype=torch.bfloat16, device=dev)
        outs[hotpath.ATTN_RUNGS[rung]] = out

        def run() -> None:
            hotpath.check(lib.cc_attn_rung(
                rung, qkv.data_ptr(), out.data_ptr(), n, seq, heads, hidden,
                ctypes.c_float(scale), stream))
        return run

    legs = {}
    # the rungs that can cover seq: small <= 64, mid <= 288, flash any
    for rung, cap in enumerate((64, 288, None)):
        if cap is None or seq <= cap:
            tag = " (plan)" if rung == planned else ""
            legs[f"cc_attn {hotpath.ATTN_RUNGS[rung]}{tag}"] = native(rung)
    legs["torch sdpa + permutes"] = sdpa

    want = sdpa().float()
    for name, fn in legs.items():
        if name.startswith("cc_attn"):
            fn()
    torch.cuda.synchronize()
    for rung_name, out in outs.items():
        torch.testing.assert_close(out.float(), want, rtol=2e-2, atol=2e-2,
                                   msg=lambda m, r=rung_name: f"{r}: {m}")

    times = _timed(legs, warmup, launches)
    flops = 4.0 * seq * seq * hd * heads * n
    lines = [f"attention: {n} frames x {heads} heads x hd {hd}, seq {seq} "
             f"({flops / 1e9:.2f} GFLOP per launch)"]
    ref = float(np.median(times["torch sdpa + permutes"]))
    for name, t in times.items():
        med = float(np.median(t))
        lines.append(_stat_line(
            name, t, f"  | {flops / (med * 1e-3) / 1e12:.1f} TFLOP/s, "
                     f"{ref / med:.2f}x sdpa"))
    return lines


def bench_tower(frames: int, warmup: int, launches: int) -> list[str]:
    from cosmos_curate_amd.models import clip_weights as cw
    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD

    cfg = cw.CONFIGS["siglip_so400m_14_224"]
    tower = SiglipVisionTowerAMD(cw.make_siglip_weights(cfg), cfg).cuda()
    g = torch.Generator().manual_seed(0)
    px = (torch.rand(frames, 3, cfg.image, cfg.image, generator=g) * 2 - 1).to(
        torch.bfloat16).cuda()

    def run(force: bool):
        def fn() -> torch.Tensor:
            tower.force_sdpa = force
            return tower(px)
        return fn

    legs = {"native (cc_attn, LN folded)": run(False),
            "force_sdpa (torch sdpa, LN kernel)": run(True)}
    a, b = (fn() for fn in legs.values())
    torch.cuda.synchronize()
    cos = torch.sum(a * b, dim=1)
    times = _timed(legs, warmup, launches)
    lines = [f"tower: {cfg.name}, {cfg.layers} layers, eager, one batch of "
             f"{frames} frames; native vs force_sdpa per-frame cosine min "
             f"{cos.min().item():.6f}"]
    ref = float(np.median(times["force_sdpa (torch sdpa, LN kernel)"]))
    for name, t in times.items():
        med = float(np.median(t))
        lines.append(_stat_line(
            name, t, f"  | {frames / (med * 1e-3):.0f} frames/s, "
                     f"{ref / med:.2f}x force_sdpa"))
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--hd", type=int, default=72)
    ap.add_argument("--seqs", default="256,729",
                    help="comma-separated sequence lengths")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tower-frames", type=int, default=64)
    ap.add_argument("--no-tower", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    lib = hotpath.require_gpu()
    lines = [f"{args.launches} launches per leg after {args.warmup} warm-up, legs "
             f"alternating in one process; device {torch.cuda.get_device_name(0)}"]
    for seq in (int(s) for s in args.seqs.split(",")):
        lines += bench_attention(lib, args.frames, args.heads, args.hd, seq,
                                 args.warmup, args.launches)
    if not args.no_tower:
        lines += bench_tower(args.tower_frames, args.warmup, args.launches)
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
