"""Recorded hashes for the 256² GEMM epilogue on inputs whose f32 sums really
round (tests/test_gpu_gemm_transposed.py runs the same cases).

§27 feeds the MFMA its operands the other way round, so that the instruction
computes the transposed fragment, and rewrites every use of the
accumulator-to-(row, column) map.  Every accumulator still receives the same
products over the same k in the same order, so C and the (sum, sum²) partials
must stay bit-identical.  The inputs of tools/gemm_epilogue_golden.py are
small integers times powers of two: their sums are exact in any order and
cannot tell.  The inputs here are seeded standard-normal bf16 (the weights
scaled by K^-1/2, so nothing overflows), made on the CPU so that they depend
on no device generator, and ``assert_sums_round`` shows on the CPU that the
f32 sum of one output element's products depends on the order of k.

    python tools/gemm_transposed_golden.py --write tests/golden/gemm_transposed_hashes.json

Run it at the commit whose results are the reference (the parent of the
change under test), never at the code under test.

Forms: those of tools/gemm_epilogue_golden.py, and the two outputs of the
scalar epilogue: "bare" (bf16, no bias, no activation, no residual) and
"f32bias" (f32 output with a bias).

``--child M,N,K`` runs the forms of one forced-tile shape in this process and
prints the hashes as one JSON line (CC_GEMM_TILE is read once per process).
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location(
    "gemm_epilogue_golden", ROOT / "tools" / "gemm_epilogue_golden.py")
geg = sys.modules.get(_spec.name)
if geg is None:
    geg = importlib.util.module_from_spec(_spec)
    sys.modules[_spec.name] = geg
    _spec.loader.exec_module(geg)

torch = geg.torch
hotpath = geg.hotpath

SEED = 27

# (M, N, K, forced tile knob or None, forms)
SHAPES = (
    # ragged second row tile, 4 K-tiles (the minimum): every staged form
    # without the statistics, and both outputs of the scalar epilogue
    (300, 1536, 256, None,
     ("bias", "act1", "act2", "act3", "ln0", "ln1", "res", "bare", "f32bias")),
    # the statistics, at an N the LayerNorm kernels have
    (300, 768, 1536, None, ("res_stats",)),
    # the N edge of the scalar f32 path: the last column tile holds 130
    # columns and N % 4 != 0, so no row of C after the first is 16-byte
    # aligned.  Plans to the 128² body; runs under CC_GEMM_TILE=1 in a child
    (300, 386, 256, 1, ("f32bias",)),
)

CASES = [(M, N, K, f) for M, N, K, tile, forms in SHAPES if tile is None
         for f in forms]
FORCED = [s for s in SHAPES if s[3] is not None]


def build_problem(M, N, K):
    """Operands of every form at one shape, from the CPU generator."""
    g = torch.Generator().manual_seed(SEED)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g) * 0.5).contiguous()
    # the column sums in f64, rounded once: no order of summation enters
    colsum = w.double().sum(dim=1).float().contiguous()
    assert_sums_round(a, w)
    return {"M": M, "N": N, "K": K, "a": a.cuda(), "w": w.cuda(),
            "res": res.cuda(), "bias": bias.cuda(), "colsum": colsum.cuda()}


def assert_sums_round(a, w):
    """The products of C[0, 0], summed in f32 front to back and back to
    front, give different bits: these inputs are not exact."""
    prods = (a[0].float() * w[0].float()).numpy()  # bf16 x bf16 is exact in f32
    fwd = bwd = np.float32(0.0)
    for x, y in zip(prods, prods[::-1]):
        fwd = np.float32(fwd + x)
        bwd = np.float32(bwd + y)
    assert fwd.tobytes() != bwd.tobytes(), \
        "the f32 sum of C[0, 0] does not depend on the order of k"


def reference(p, form):
    a, w = p["a"].float(), p["w"].float()
    if form == "bare":
        return a @ w.T
    if form == "f32bias":
        return torch.nn.functional.linear(a, w, p["bias"])
    return geg.reference(p, form)


def run_form(lib, p, form):
    """One launch into sentinel-filled buffers -> (C, stats or None), both
    with their spare rows."""
    if form not in ("bare", "f32bias"):
        return geg.run_form(lib, p, form)
    M, N, K = p["M"], p["N"], p["K"]
    f32 = form == "f32bias"
    out = torch.full((M + 1, N), geg.SENTINEL, device="cuda",
                     dtype=torch.float32 if f32 else torch.bfloat16)
    hotpath.check(lib.cc_gemm_bf16_ex(
        p["a"].data_ptr(), p["w"].data_ptr(), out.data_ptr(), M, N, K,
        p["bias"].data_ptr() if f32 else None, 0 if f32 else 1, 0, None,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out, None


def check_case(lib, p, form, want_hashes, log=print):
    """Every check of one (shape, form); returns the hashes it computed.
    ``want_hashes`` None skips the comparison with the recorded values
    (recording them)."""
    M = p["M"]
    name = geg.case_id(M, p["N"], p["K"], form)
    out, stats = run_form(lib, p, form)
    assert torch.all(out[M:] == geg.SENTINEL), f"{name}: wrote past the M rows of C"
    if stats is not None:
        assert torch.all(stats[M:] == geg.SENTINEL), \
            f"{name}: wrote past the M rows of stats"
    want = reference(p, form)
    err = (out[:M].float() - want).abs()
    log(f"{name}: max abs err {err.max().item():.3e}, worst share of the "
        f"budget {(err / (2e-2 + 2e-2 * want.abs())).max().item():.3f}")
    torch.testing.assert_close(out[:M].float(), want, rtol=2e-2, atol=2e-2)
    out2, stats2 = run_form(lib, p, form)
    assert torch.equal(out, out2), f"{name}: C differs from run to run"
    if stats is not None:
        assert torch.equal(stats, stats2), f"{name}: stats differ from run to run"
    got = geg.hashes_of(p, out, stats)
    if want_hashes is not None:
        assert got == want_hashes, f"{name}: {got} != recorded {want_hashes}"
    return got


def run_shape(lib, M, N, K, forms, golden, log=print):
    p = build_problem(M, N, K)
    return {
        geg.case_id(M, N, K, f): check_case(
            lib, p, f,
            None if golden is None else golden[geg.case_id(M, N, K, f)], log)
        for f in forms
    }


def run_shape_in_child(M, N, K, tile, golden_path=None):
    """The hashes of one shape from a fresh process with CC_GEMM_TILE set;
    with ``golden_path`` the child also compares with the recorded file."""
    env = dict(os.environ, CC_GEMM_TILE=str(tile))
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()),
           "--child", f"{M},{N},{K}"]
    if golden_path:
        cmd += ["--golden", str(golden_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--write", metavar="JSON",
                    help="record the hashes of every case to this file")
    ap.add_argument("--recorded-at", default="unknown",
                    help="with --write: the commit the hashes come from")
    ap.add_argument("--child", metavar="M,N,K",
                    help="run one shape here, print its hashes as JSON")
    ap.add_argument("--golden", metavar="JSON",
                    help="compare with this recorded file")
    args = ap.parse_args()
    lib = hotpath.require_gpu()
    golden = geg.load_golden(args.golden) if args.golden else None
    if args.child:
        M, N, K = map(int, args.child.split(","))
        forms = next(s[4] for s in SHAPES if s[:3] == (M, N, K))
        print(json.dumps(run_shape(lib, M, N, K, forms, golden)))
        return
    hashes = {}
    for M, N, K, tile, forms in SHAPES:
        if tile is None:
            hashes.update(run_shape(lib, M, N, K, forms, golden))
        else:
            got, _ = run_shape_in_child(M, N, K, tile, args.golden)
            hashes.update(got)
    if args.write:
        doc = {
            "about": "SHA-256 of the first M rows of C (and of stats) per "
                     "shape and form; tools/gemm_transposed_golden.py --write",
            "recorded_at": args.recorded_at,
            "hashes": hashes,
        }
        pathlib.Path(args.write).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"{len(hashes)} cases ok")


if __name__ == "__main__":
    main()
