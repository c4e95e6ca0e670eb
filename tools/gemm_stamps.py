"""Where a 256² GEMM tile spends its time, from clock stamps taken inside
the kernel: K-loop µs per K-tile, the first two phases of
the K-loop, and epilogue µs per tile, at the four flagship shapes with their
real epilogue forms.

    python tools/gemm_stamps.py --build     # no GPU needed: compiles the library
    python tools/gemm_stamps.py             # on the GPU: runs and prints the table

The stamped library is a build of its own (cc_gemm.hip with
-DCC_GEMM_STAMPS, linked with the objects of the production build, which
must exist) at tools/libcchot_stamps.so; --lib names another one, so that
the stamped build of another commit can be run by the same script.  The
production library never carries the stamps.

Stamps per tile (100 MHz wall clock, read by every wave, stored by one
lane): 0 rep top, 1-3 the barriers in front of the first three MFMA clusters
of the tile's first K-tile, 4 the end of the K-loop, 5 the end of the
epilogue, 6 + p the end of the write phase of the staged epilogue's pass p
(accumulators -> bf16 -> the wave's LDS slice), 10 + p the end of its
read-back (LDS -> residual add, statistics -> store issue).  "write p0" is
(6 - 4): it also holds the issue of the first residual loads and of the next
tile's prologue; "write p1-3" is the sum of (6 + p) - (10 + p - 1) over the
other three passes, the write phase alone; "read-back" is the sum of
(10 + p) - (6 + p) over the four, which includes the wait for the pass's
residual loads.  A workgroup's next rep top follows its epilogue end directly, so
(5 - 4) is everything between two K-loops except the rep-top wait, which
is (next 0 - 5).  "kernel us" is the last stamp 5 minus the first stamp 0 of
a launch: set it against the production library's kernel time to see what
the stamps themselves cost.  The phases are those of a tile's FIRST K-tile,
where the glds issues queue behind the previous epilogue's stores: they are
not the steady state, which is us/K-tile.
"""

from __future__ import annotations

import argparse
import ctypes
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from cosmos_curate_amd import build as cc_build  # noqa: E402

LIB = ROOT / "tools" / "libcchot_stamps.so"
STAMP_N = 14
M_FLAGSHIP = 224 * 21 * 50  # clips x frames x tokens

# (name, N, K, form of tools/gemm_epilogue_golden.py)
SHAPES = (
    ("qkv", 2304, 768, "ln0"),
    ("fc1", 3072, 768, "ln1"),
    ("out-proj", 768, 768, "res_stats"),
    ("fc2", 768, 3072, "res_stats"),
)


def build(out: pathlib.Path) -> None:
    name, extra = next(s for s in cc_build.SOURCES if s[0] == "cc_gemm.hip")
    obj = out.with_suffix(".gemm.o")
    subprocess.run(
        [cc_build.HIPCC, *cc_build.COMMON, *extra, "-DCC_GEMM_STAMPS", "-c",
         str(cc_build.CSRC / name), "-o", str(obj)], check=True)
    others = [cc_build.LIBDIR / (pathlib.Path(n).stem + ".o")
              for n, _ in cc_build.SOURCES if n != name]
    missing = [o for o in others if not o.exists()]
    if missing:
        sys.exit(f"run the production build first: {missing[0]} is missing")
    subprocess.run(
        [cc_build.HIPCC, cc_build.ARCH, "-shared", "-fPIC", str(obj),
         *map(str, others), "-o", str(out)], check=True)
    obj.unlink()
    print("built", out)


def collect(lib_path: pathlib.Path, M: int, launches: int, stamp_n: int = STAMP_N):
    """Yields (name, N, K, grid, [stamps of one launch in us, tiles x stamp_n]
    per launch) for every shape, after 2 launches of warm-up."""
    import importlib.util

    import torch

    from cosmos_curate_amd import hotpath

    spec = importlib.util.spec_from_file_location(
        "gemm_epilogue_golden", ROOT / "tools" / "gemm_epilogue_golden.py")
    geg = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = geg
    spec.loader.exec_module(geg)

    assert torch.cuda.is_available(), "gemm_stamps needs a GPU"
    lib = ctypes.CDLL(str(lib_path))
    hotpath._declare(lib)
    lib.cc_gemm_stamps_set.argtypes = [ctypes.c_void_p]
    for name, N, K, form in SHAPES:
        torch.manual_seed(1)
        w = (torch.randn(N, K, device="cuda") * 0.05).to(torch.bfloat16)
        p = {
            "M": M, "N": N, "K": K,
            "a": torch.randn(M, K, device="cuda").to(torch.bfloat16),
            "w": w,
            "res": torch.randn(M, N, device="cuda").to(torch.bfloat16),
            "bias": torch.randn(N, device="cuda") * 0.1,
            "colsum": w.float().sum(dim=1).contiguous(),
        }
        plan = hotpath.gemm_plan(M, N, K, has_bias=True,
                                 has_residual=form.startswith("res"))
        assert plan.body == 256
        tiles = plan.tiles_x * plan.tiles_y
        stamps = torch.zeros((tiles, stamp_n), dtype=torch.int64, device="cuda")
        khz = lib.cc_gemm_stamps_set(stamps.data_ptr())
        assert khz > 0, "cc_gemm_stamps_set failed"
        runs = []
        for it in range(launches + 2):
            geg.run_form(lib, p, form)
            if it >= 2:
                runs.append(stamps.cpu().double() * (1e3 / khz))
        lib.cc_gemm_stamps_set(None)
        yield name, N, K, plan.grid, runs
        del p, stamps
        torch.cuda.empty_cache()


def run(lib_path: pathlib.Path, M: int, launches: int) -> None:
    import torch

    print(f"{lib_path.name}: M = {M}, mean over the tiles of {launches} "
          f"launches after 2 of warm-up")
    print(f"{'gemm':9s} {'N':>5s} {'K':>5s} {'tiles':>6s} {'KT':>3s} | "
          f"{'kernel us':>9s} {'K-loop us':>9s} {'us/K-tile':>9s} {'phase 0':>8s} "
          f"{'phase 1':>8s} {'epilogue us':>11s} {'write p0':>8s} "
          f"{'write p1-3':>10s} {'read-back':>9s} {'rep-top us':>10s} "
          f"{'tile round us':>13s}")
    for name, N, K, grid, runs in collect(lib_path, M, launches):
        acc = torch.zeros(10, dtype=torch.float64)
        for s in runs:
            assert (s[:, 5] >= s[:, 4]).all() and (s[:, 4] > s[:, 0]).all()
            assert (s[:, 6] >= s[:, 4]).all() and (s[:, 5] >= s[:, 13]).all()
            wr = sum(s[:, 6 + p] - s[:, 9 + p] for p in (1, 2, 3))
            rb = sum(s[:, 10 + p] - s[:, 6 + p] for p in range(4))
            nxt = s[grid:, 0] - s[:-grid, 5]
            rnd = s[grid:, 0] - s[:-grid, 0]
            nan = torch.tensor(float("nan"), dtype=torch.float64)
            acc += torch.stack([
                s[:, 5].max() - s[:, 0].min(),
                (s[:, 4] - s[:, 0]).mean(), (s[:, 2] - s[:, 1]).mean(),
                (s[:, 3] - s[:, 2]).mean(), (s[:, 5] - s[:, 4]).mean(),
                (s[:, 6] - s[:, 4]).mean(), wr.mean(), rb.mean(),
                nxt.mean() if len(nxt) else nan,
                rnd.mean() if len(rnd) else nan])
        ker, kl, p0, p1, epi, w0, wr, rb, top, rnd = (acc / len(runs)).tolist()
        kt = K // 64
        print(f"{name:9s} {N:5d} {K:5d} {len(runs[0]):6d} {kt:3d} | {ker:9.1f} "
              f"{kl:9.2f} {kl / kt:9.3f} {p0:8.3f} {p1:8.3f} {epi:11.2f} "
              f"{w0:8.2f} {wr:10.2f} {rb:9.2f} {top:10.2f} {rnd:13.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--build", action="store_true",
                    help="compile the stamped library and stop")
    ap.add_argument("--lib", type=pathlib.Path, default=LIB)
    ap.add_argument("--m", type=int, default=M_FLAGSHIP)
    ap.add_argument("--launches", type=int, default=5)
    args = ap.parse_args()
    if args.build:
        build(args.lib)
        return
    if not args.lib.exists():
        sys.exit(f"{args.lib} not built: run with --build first")
    run(args.lib, args.m, args.launches)


if __name__ == "__main__":
    main()
