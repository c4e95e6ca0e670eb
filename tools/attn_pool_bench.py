"""Time the towers' pooling heads on cc_attn_pool against their torch f32
heads on one MI355X, the legs alternating in one process.

    python tools/attn_pool_bench.py [--siglip-frames 64 --iv2-clips 8
                                     --iv2-frames 8 --launches 20 --warmup 3]
                                    [--no-towers] [--out LOG]

Per tower (siglip_so400m_14_224, 27 layers; InternVideo2-1B, 40 layers;
deterministic stand-in weights), on the same tower object with
``native_pool`` off and on:
  - the head alone, on one tensor of random tokens of the tower's shape
    (SigLIP: _map_head on post-LN tokens; InternVideo2: _pool on the residual
    stream with its row statistics, the folded route's call);
  - the whole forward (skipped with --no-towers).
Device time from HIP events around each leg on the current stream; median,
min, max, p10, p90.  After the legs, the kernel's own time from the library's
timing registry and the bytes/s it reaches against one read of the tokens.
Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import dataclasses
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from cosmos_curate_amd import hotpath  # noqa: E402
from cosmos_curate_amd.models import clip_weights as cw  # noqa: E402
from cosmos_curate_amd.models import internvideo2_weights as iw  # noqa: E402
from cosmos_curate_amd.models.vit_encoder import cc_ln_stats  # noqa: E402


def _timed(legs: dict, warmup: int, launches: int) -> dict[str, np.ndarray]:
    """Alternate the legs; per-call HIP-event times (ms) after warm-up."""
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


def _stat_line(name: str, t: np.ndarray) -> str:
    return (f"  {name}: median {np.median(t):.4f} ms  min {t.min():.4f}  "
            f"max {t.max():.4f}  p10 {np.percentile(t, 10):.4f}  "
            f"p90 {np.percentile(t, 90):.4f}")


def _legs(tower, fn) -> dict:
    def leg(flag):
        def run():
            tower.native_pool = flag
            return fn()
        return run
    return {"torch head ": leg(False), "native head": leg(True)}


def _kernel_line(fn, tower, token_bytes: int, launches: int) -> str:
    """The kernel's own time over ``launches`` native calls of ``fn``."""
    tower.native_pool = True
    hotpath.timing_enable(True)
    try:
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        ms, cnt = hotpath.timing_report("attn_pool")
        cms, ccnt = hotpath.timing_report("attn_pool_combine")
    finally:
        hotpath.timing_enable(False)
    per = ms / cnt
    line = (f"  attn_pool kernel: {per:.4f} ms mean of {cnt} launches, "
            f"{token_bytes / per / 1e9:.3f} TB/s against one read of the tokens "
            f"({token_bytes / 1e6:.1f} MB)")
    if ccnt:
        line += f"; attn_pool_combine {cms / ccnt:.4f} ms"
    return line


class _Log(list):
    """Lines kept for --out and printed as they come."""

    def append(self, line: str) -> None:
        print(line, flush=True)
        super().append(line)


def bench(label, tower, head_fn, tower_fn, token_bytes, args) -> list[str]:
    lines = _Log()
    lines.append(label)
    with torch.no_grad():
        a, b = (leg() for leg in _legs(tower, head_fn).values())
        cos = torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)
        lines.append(f"  head, native vs torch: min cosine {float(cos.min()):.6f}")
        lines.append(" head alone")
        for name, t in _timed(_legs(tower, head_fn), args.warmup, args.launches).items():
            lines.append(_stat_line(name, t))
        lines.append(_kernel_line(head_fn, tower, token_bytes, args.launches))
        if not args.no_towers:
            lines.append(" whole tower")
            for name, t in _timed(_legs(tower, tower_fn), args.warmup,
                                  args.launches).items():
                lines.append(_stat_line(name, t))
    return lines


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--siglip-frames", type=int, default=64)
    ap.add_argument("--iv2-clips", type=int, default=8)
    ap.add_argument("--iv2-frames", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-towers", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hotpath.require_gpu()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    lines: list[str] = []

    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD

    cfg = cw.CONFIGS["siglip_so400m_14_224"]
    if args.no_towers:  # the head does not depend on the depth
        cfg = dataclasses.replace(cfg, layers=1)
    tower = SiglipVisionTowerAMD(cw.make_siglip_weights(cfg), cfg).to(dev)
    n, seq = args.siglip_frames, (cfg.image // cfg.patch) ** 2
    tok = torch.randn(n, seq, cfg.hidden, device=dev, generator=g).to(torch.bfloat16)
    px = torch.randn(n, 3, cfg.image, cfg.image, device=dev, generator=g).to(torch.bfloat16)
    lines += bench(f"siglip_so400m_14_224: {n} frames x {seq} tokens x {cfg.hidden}",
                   tower, lambda: tower._map_head(tok), lambda: tower(px),
                   tok.numel() * 2, args)
    del tower

    from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD

    cfg = dataclasses.replace(iw.INTERNVIDEO2_1B, num_frames=args.iv2_frames)
    if args.no_towers:
        cfg = dataclasses.replace(cfg, layers=1)
    tower = InternVideo2VisionTowerAMD(iw.make_internvideo2_weights(cfg), cfg).to(dev)
    n, seq = args.iv2_clips, cfg.num_pos
    tok = torch.randn(n * seq, cfg.hidden, device=dev, generator=g).to(torch.bfloat16)
    stats = cc_ln_stats(tok)
    px = torch.randn(n, cfg.num_frames, 3, cfg.image, cfg.image, device=dev,
                     generator=g).to(torch.bfloat16)
    lines += bench(f"internvideo2_1b: {n} clips x {seq} tokens x {cfg.hidden}",
                   tower, lambda: tower._pool(tok, stats, n, seq), lambda: tower(px),
                   tok.numel() * 2, args)

    if args.out:
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
