"""Time cc_attn_cross against torch sdpa on one MI355X, the legs alternating in
one process, and the share of a full-depth Cosmos-Embed1 forward it takes.

    python tools/attn_cross_bench.py [--clips 8 --nks 2056,4616,8200
                                      --launches 30 --warmup 5]
                                     [--tower 224p | --no-tower] [--out LOG]

Per key count (the Q-Former's cross-attention: 32 queries, 12 heads of 64)
the legs are, on the same q [n*32, 768] and kv [n*nk, 1536]:
  - cc_attn_cross at splits 1, 2, 4, 8 and at the plan's own choice — the
    evidence for the split rule in csrc/cc_attncross_plan.hpp (its combine
    kernel and the workspace allocation are inside the timed call),
  - torch sdpa with the permutes a torch route pays (three strided views in,
    one permute copy out).
Per-launch device time from HIP events around each call on the current
stream; median, min, max, p10, p90, and the achieved GB/s from the K and V
bytes the algorithm has to read once.  Each leg's output is first compared
with sdpa (rtol = atol = 2e-2).

The tower leg runs the variant at full depth (39 + 12 layers, deterministic
stand-in weights) eagerly on one batch of clips, three timed forwards, then
one more under cc_timing for the device time in attn_cross + combine.
Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from attn_hd_bench import _stat_line, _timed  # noqa: E402
from cosmos_curate_amd import hotpath  # noqa: E402

NQ, HEADS, HD = 32, 12, 64
HIDDEN = HEADS * HD


def bench_cross(n: int, nk: int, warmup: int, launches: int) -> list[str]:
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(nk)
    q = torch.randn(n * NQ, HIDDEN, device=dev, generator=g).to(torch.bfloat16)
    kv = torch.randn(n * nk, 2 * HIDDEN, device=dev, generator=g).to(torch.bfloat16)
    scale = HD ** -0.5

    def sdpa() -> torch.Tensor:
        qq = q.reshape(n, NQ, HEADS, HD).permute(0, 2, 1, 3)
        k, v = (kv[:, i * HIDDEN:(i + 1) * HIDDEN].reshape(n, nk, HEADS, HD)
                .permute(0, 2, 1, 3) for i in range(2))
        o = torch.nn.functional.scaled_dot_product_attention(qq, k, v, scale=scale)
        return o.permute(0, 2, 1, 3).reshape(n * NQ, HIDDEN)

    planned = hotpath.attn_cross_plan(n, NQ, nk, HEADS, HIDDEN).splits
    legs = {}
    for splits in (1, 2, 4, 8, 0):
        got = hotpath.attn_cross_plan(n, NQ, nk, HEADS, HIDDEN, splits).splits
        name = (f"cc_attn_cross plan ({got} splits)" if splits == 0
                else f"cc_attn_cross {got} splits")
        legs[name] = (lambda s=splits: hotpath.attn_cross(
            q, kv, n, NQ, nk, HEADS, scale=scale, splits=s))
    legs["torch sdpa + permutes"] = sdpa

    want = sdpa().float()
    for name, fn in legs.items():
        torch.testing.assert_close(fn().float(), want, rtol=2e-2, atol=2e-2,
                                   msg=lambda m, r=name: f"{r}: {m}")
    times = _timed(legs, warmup, launches)
    nbytes = 2.0 * n * nk * 2 * HIDDEN
    lines = [f"cross-attention: {n} clips x {HEADS} heads x hd {HD}, {NQ} queries, "
             f"nk {nk} ({nbytes / 1e6:.1f} MB of K and V; plan: {planned} splits)"]
    ref = float(np.median(times["torch sdpa + permutes"]))
    for name, t in times.items():
        med = float(np.median(t))
        lines.append(_stat_line(
            name, t, f"  | {nbytes / (med * 1e-3) / 1e9:.0f} GB/s, {ref / med:.2f}x sdpa"))
    return lines


def bench_tower(variant: str, clips: int) -> list[str]:
    from cosmos_curate_amd.models import cosmos_embed1_vit as cv

    cfg = cv.VARIANTS[variant]
    tower = cv.CosmosEmbed1TowerAMD(cv.make_cosmos_embed1_weights(cfg), cfg).cuda()
    g = torch.Generator().manual_seed(0)
    px = torch.randn(clips, cfg.num_frames, 3, cfg.image, cfg.image,
                     generator=g).to(torch.bfloat16).cuda()
    tower(px)
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        tower(px)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    hotpath.timing_enable(True)
    try:
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        tower(px)
        e1.record()
        e1.synchronize()
        cross = [hotpath.timing_report(k) for k in ("attn_cross", "attn_cross_combine")]
    finally:
        hotpath.timing_enable(False)
    ms = sum(c[0] for c in cross)
    return [
        f"tower: {cfg.name}, {cfg.layers} + {cfg.q_layers} layers, eager, one batch "
        f"of {clips} clips x {cfg.num_frames} frames, nk {cfg.num_keys}",
        "  forward, host clock to synchronise: " + ", ".join(f"{r:.1f} ms" for r in runs)
        + f"  | {clips / (np.median(runs) * 1e-3):.1f} clips/s",
        f"  under cc_timing: forward {e0.elapsed_time(e1):.1f} ms; attn_cross "
        f"{cross[0][0]:.3f} ms in {cross[0][1]} launches + combine {cross[1][0]:.3f} ms "
        f"in {cross[1][1]} = {100 * ms / np.median(runs):.2f} % of the untimed forward",
    ]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--nks", default="2056,4616,8200",
                    help="comma-separated key counts (224p, 336p, 448p)")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tower", default="224p")
    ap.add_argument("--no-tower", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    hotpath.require_gpu()
    lines = [f"{args.launches} launches per leg after {args.warmup} warm-up, legs "
             f"alternating in one process; device {torch.cuda.get_device_name(0)}"]
    for nk in (int(s) for s in args.nks.split(",")):
        lines += bench_cross(args.clips, nk, args.warmup, args.launches)
    if not args.no_tower:
        lines += bench_tower(args.tower, args.clips)
    text = "\n".join(lines)
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
