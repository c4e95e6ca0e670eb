"""Time one k-means step of semantic dedup, torch against the native kernels
(csrc/cc_kmeans.hip), on one MI355X, the legs alternating in one process
(DESIGN.md §24).

    python tools/kmeans_bench.py [--launches 30 --warmup 3] [--no-semdedup]
                                 [--out LOG]

Per shape (m, d, k), on unit rows drawn around k/2 planted centres and k of
them as centroids:
  - assign alone: torch ``(e @ cent.T).argmax(1)`` against kmeans_assign;
  - accumulate alone, on the labels assign gave: torch f64 ``index_add_`` of
    sums and counts against kmeans_accumulate (its torch sort included);
  - the step, both in a row.
Device time from HIP events around each leg on the current stream; median,
min, max, p10, p90.  After the legs, the kernels' own times from the
library's timing registry, assign's f32 FLOP/s (2 m d k) against the 155 TF
f32-MFMA ceiling and accumulate's bytes/s against one read of e.  Then, at
the first shape, the whole 20-iteration fit and the whole semdedup with each
backend on the corpus of tools/dedup_scale_bench.py (host clock around a
device synchronise).  Needs a GPU; there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from cosmos_curate_amd import hotpath  # noqa: E402
from cosmos_curate_amd.pipelines.video.dedup import semdedup as sd  # noqa: E402

SHAPES = [(1_000_000, 512, 1000), (1_000_000, 512, 100), (100_000, 768, 100),
          (100_000, 1152, 1000)]
F32_MFMA_PEAK = 155e12


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


class _Log(list):
    """Lines kept for --out and printed as they come."""

    def append(self, line: str) -> None:
        print(line, flush=True)
        super().append(line)


def _corpus(m: int, d: int, k: int, g: torch.Generator):
    dev = torch.device("cuda")
    centres = torch.randn(max(k // 2, 1), d, device=dev, generator=g)
    idx = torch.randint(0, len(centres), (m,), device=dev, generator=g)
    e = centres[idx] + 1.5 * torch.randn(m, d, device=dev, generator=g)
    e = torch.nn.functional.normalize(e, dim=1)
    return e, e[torch.randperm(m, device=dev, generator=g)[:k]].clone()


def torch_assign(e, cent):
    return (e @ cent.T).argmax(dim=1)


def torch_accumulate(e, labels, k):
    sums = torch.zeros((k, e.shape[1]), dtype=torch.float64, device=e.device)
    counts = torch.zeros(k, dtype=torch.float64, device=e.device)
    sums.index_add_(0, labels, e.to(torch.float64))
    counts.index_add_(0, labels, torch.ones_like(labels, dtype=torch.float64))
    return sums, counts


def bench_shape(m: int, d: int, k: int, args, lines: _Log) -> None:
    g = torch.Generator(device="cuda").manual_seed(m + d + k)
    e, cent = _corpus(m, d, k, g)
    lines.append(f"m {m}  d {d}  k {k}")
    lt = torch_assign(e, cent)
    ln, _ = sd.kmeans_assign(e, cent)
    st, ct = torch_accumulate(e, ln, k)
    sn, cn = sd.kmeans_accumulate(e, ln, k)
    rel = ((sn - st).abs().max() / st.abs().max()).item()
    lines.append(f"  native vs torch: labels differ on {(lt != ln).sum().item()} of {m} "
                 f"rows; sums max |diff| / max |sum| {rel:.3g}; counts equal "
                 f"{torch.equal(ct, cn)}; clusters {int(cn.min().item())}..{int(cn.max().item())} rows")
    del lt, st, ct, sn, cn
    for title, legs in (
        (" assign", {"torch ": lambda: torch_assign(e, cent),
                     "native": lambda: sd.kmeans_assign(e, cent)}),
        (" accumulate", {"torch ": lambda: torch_accumulate(e, ln, k),
                         "native": lambda: sd.kmeans_accumulate(e, ln, k)}),
        (" step", {"torch ": lambda: torch_accumulate(e, torch_assign(e, cent), k),
                   "native": lambda: sd.kmeans_accumulate(e, sd.kmeans_assign(e, cent)[0], k)}),
    ):
        lines.append(title)
        for name, t in _timed(legs, args.warmup, args.launches).items():
            lines.append(_stat_line(name, t))
    hotpath.timing_enable(True)
    try:
        for _ in range(args.launches):
            sd.kmeans_accumulate(e, sd.kmeans_assign(e, cent)[0], k)
        torch.cuda.synchronize()
        (a_ms, a_n), (s_ms, s_n), (c_ms, c_n) = (
            hotpath.timing_report(n)
            for n in ("kmeans_assign", "kmeans_accumulate", "kmeans_combine"))
    finally:
        hotpath.timing_enable(False)
    flops, ebytes = 2.0 * m * d * k, 4.0 * m * d
    lines.append(f"  kernels, mean of {a_n} launches: kmeans_assign {a_ms / a_n:.4f} ms = "
                 f"{flops / (a_ms / a_n) / 1e9:.1f} TFLOP/s f32 "
                 f"({100 * flops / (a_ms / a_n) / 1e-3 / F32_MFMA_PEAK:.1f} % of 155 TF); "
                 f"kmeans_accumulate {s_ms / s_n:.4f} ms = "
                 f"{ebytes / (s_ms / s_n) / 1e9:.3f} TB/s against one read of e; "
                 f"kmeans_combine {c_ms / c_n:.4f} ms")


def bench_semdedup(args, lines: _Log) -> None:
    m, d, k = SHAPES[0]
    torch.manual_seed(11)
    base = torch.randn(m, d, device="cuda")
    dup_src = torch.randint(0, m, (m // 10,), device="cuda")
    base[: m // 10] = base[dup_src] + 0.01 * torch.randn(m // 10, d, device="cuda")
    lines.append(f"whole fit and whole semdedup, {m} x {d}, {k} clusters, 20 iterations "
                 f"(seconds, host clock around a synchronise; runs alternate)")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for rep in range(2):
        for backend in sd.KMEANS_BACKENDS:
            cfg = sd.SemDedupConfig(n_clusters=k, n_iters=20, eps=0.05,
                                    kmeans_backend=backend)
            t_fit, _ = clock(lambda: sd.kmeans_fit(base, k, 20, cfg.random_seed,
                                                   backend=backend))
            t_all, out = clock(lambda: sd.semdedup(base, cfg))
            lines.append(f"  run {rep} {backend:6s}: kmeans_fit {t_fit:.3f} s  semdedup "
                         f"{t_all:.3f} s  kept {out['kept']} of {out['total']}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-semdedup", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hotpath.require_gpu()
    lines = _Log()
    with torch.no_grad():
        for m, d, k in SHAPES:
            bench_shape(m, d, k, args, lines)
        if not args.no_semdedup:
            bench_semdedup(args, lines)
    if args.out:
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
