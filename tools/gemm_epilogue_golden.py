"""Problems, checks and recorded hashes for the 256² GEMM epilogue
(tests/test_gpu_gemm_epilogue.py runs the same code).

The epilogue work of §19 moves loads, stores and waits and no arithmetic,
so C and the (sum, sum²) partials must stay bit-identical.  This script
records their SHA-256 per (shape, form):

    python tools/gemm_epilogue_golden.py --write tests/golden/gemm_epilogue_hashes.json

Run it at the commit whose results are the reference (the parent of the
change under test), never at the code under test.  The test then runs
``check_case`` on every case against the recorded file.

Inputs are integer hashes of the index grid scaled by powers of two, so
they are exact in bf16 and depend on no library's random generator.

``--child M,N,K`` runs every form of one shape in this process and prints
the hashes as one JSON line; the test uses it for the shape that needs
CC_GEMM_TILE=1, a knob the library reads once per process.
"""

from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from cosmos_curate_amd import hotpath  # noqa: E402

EPS = 1e-5
SENTINEL = -7.0  # exactly representable in bf16 and f32
STATS_PAD = 3

ALL_FORMS = ("bias", "act1", "act2", "act3", "ln0", "ln1", "res", "res_stats")
_NO_STATS = tuple(f for f in ALL_FORMS if f != "res_stats")
_NO_LN = tuple(f for f in ALL_FORMS if not f.startswith("ln"))

# (M, N, K, forced tile knob or None, forms).  The LN forms need row
# statistics at K and res_stats at N; the LayerNorm kernels exist at 256,
# 768 and 1152 but not at 1536, so those forms run where the width allows.
SHAPES = (
    # ragged M edge in the second row tile; 4 K-tiles (the minimum)
    (300, 1536, 256, None, _NO_STATS),
    # N = 4.5 tiles: the column edge.  N < 1536 and K < 1536 plan to the
    # 128² body, so this one runs under CC_GEMM_TILE=1 in a child process
    (300, 1152, 256, 1, ALL_FORMS),
    # 258 tiles > 256 workgroups: two of them walk a second tile, so the
    # counted rep-top wait and both copies of each table are exercised
    (11008, 1536, 256, None, _NO_STATS),
    # the same walk for the residual + stats form
    (22016, 768, 1536, None, _NO_LN),
    # three row tiles, the last ragged, 12 K-tiles: the flagship K
    (700, 1536, 768, None, _NO_STATS),
)


def case_id(M, N, K, form):
    return f"{M}x{N}x{K}:{form}"


def _grid(rows, cols, mul_i, mul_j, shift=7):
    i = torch.arange(rows, dtype=torch.int64, device="cuda")[:, None]
    j = torch.arange(cols, dtype=torch.int64, device="cuda")[None, :]
    return ((i * mul_i + j * mul_j) >> shift) % 255 - 127


def build_problem(M, N, K):
    """Operands of every form at one shape, all exact in their dtype."""
    a = _grid(M, K, 2654435761, 40503)
    # rows offset by 0..64 so the LN forms see row means away from zero
    a = a + (torch.arange(M, device="cuda")[:, None] % 5) * 16
    w = _grid(N, K, 2246822519, 36313)
    res = _grid(M, N, 374761393, 50021) + 64 + \
        (torch.arange(M, device="cuda")[:, None] % 3) * 32
    bias = _grid(1, N, 1, 2654435761, shift=11)[0]
    w_bf = (w.float() * 2.0**-11).to(torch.bfloat16)
    return {
        "M": M, "N": N, "K": K,
        "a": (a.float() * 2.0**-7).to(torch.bfloat16),
        "w": w_bf,
        "res": (res.float() * 2.0**-6).to(torch.bfloat16),
        "bias": (bias.float() * 2.0**-9).contiguous(),
        # column sums of integers times a power of two: exact in f32 in any
        # order of summation
        "colsum": w_bf.float().sum(dim=1).contiguous(),
    }


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _act(v, act):
    if act == 1:
        return v * torch.sigmoid(1.702 * v)
    if act == 2:
        return torch.nn.functional.gelu(v, approximate="tanh")
    if act == 3:
        return torch.nn.functional.gelu(v)
    return v


def reference(p, form):
    """torch f32 on the same bf16 inputs; computed once per shape and form."""
    a, w = p["a"].float(), p["w"].float()
    if form.startswith("ln"):
        x = torch.nn.functional.layer_norm(a, (p["K"],), eps=EPS)
        return _act(torch.nn.functional.linear(x, w, p["bias"]), int(form[2:]))
    pre = torch.nn.functional.linear(a, w, p["bias"])
    if form.startswith("res"):
        return pre + p["res"].float()
    return _act(pre, {"bias": 0, "act1": 1, "act2": 2, "act3": 3}[form])


def run_form(lib, p, form):
    """One launch into sentinel-filled buffers -> (C, stats or None), both
    with their spare rows."""
    M, N, K = p["M"], p["N"], p["K"]
    out = torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    stats = None
    if form.startswith("ln"):
        rows = torch.empty((M, K // 64, 2), dtype=torch.float32, device="cuda")
        ws = torch.empty((M, 2), dtype=torch.float32, device="cuda")
        hotpath.check(lib.cc_ln_stats_bf16(p["a"].data_ptr(), M, K,
                                           rows.data_ptr(), _stream()))
        hotpath.check(lib.cc_gemm_bf16_ln(
            p["a"].data_ptr(), 1, rows.data_ptr(), ws.data_ptr(),
            p["w"].data_ptr(), p["colsum"].data_ptr(), p["bias"].data_ptr(),
            out.data_ptr(), M, N, K, int(form[2:]), ctypes.c_float(EPS),
            _stream()))
    elif form == "res_stats":
        stats = torch.full((M + STATS_PAD, N // 64, 2), SENTINEL,
                           dtype=torch.float32, device="cuda")
        hotpath.check(lib.cc_gemm_bf16_res_stats(
            p["a"].data_ptr(), p["w"].data_ptr(), out.data_ptr(), M, N, K,
            p["bias"].data_ptr(), p["res"].data_ptr(), stats.data_ptr(),
            _stream()))
    else:
        act = {"bias": 0, "act1": 1, "act2": 2, "act3": 3, "res": 0}[form]
        hotpath.check(lib.cc_gemm_bf16_ex(
            p["a"].data_ptr(), p["w"].data_ptr(), out.data_ptr(), M, N, K,
            p["bias"].data_ptr(), 1, act,
            p["res"].data_ptr() if form == "res" else None, _stream()))
    torch.cuda.synchronize()
    return out, stats


def sha256(t):
    return hashlib.sha256(
        t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def hashes_of(p, out, stats):
    h = {"C": sha256(out[:p["M"]])}
    if stats is not None:
        h["stats"] = sha256(stats[:p["M"]])
    return h


def check_case(lib, p, form, want_hashes, log=print):
    """Every check of one (shape, form); returns the hashes it computed.
    ``want_hashes`` None skips the comparison with the recorded values
    (recording them)."""
    M, N = p["M"], p["N"]
    out, stats = run_form(lib, p, form)
    name = case_id(M, N, p["K"], form)
    # 2. nothing outside the M rows is written
    assert torch.all(out[M:] == SENTINEL), f"{name}: wrote past the M rows of C"
    if stats is not None:
        assert torch.all(stats[M:] == SENTINEL), \
            f"{name}: wrote past the M rows of stats"
    # 1. torch f32 on the same inputs
    want = reference(p, form)
    err = (out[:M].float() - want).abs()
    log(f"{name}: max abs err {err.max().item():.3e}, worst share of the "
        f"budget {(err / (2e-2 + 2e-2 * want.abs())).max().item():.3f}")
    torch.testing.assert_close(out[:M].float(), want, rtol=2e-2, atol=2e-2)
    if form == "res_stats":
        ex, _ = run_form(lib, p, "res")
        assert torch.equal(out, ex), f"{name}: C differs from cc_gemm_bf16_ex"
        got = torch.empty((M, 2), dtype=torch.float32, device="cuda")
        hotpath.check(lib.cc_ln_finalize(
            stats.data_ptr(), M, N, 1, ctypes.c_float(EPS), got.data_ptr(),
            _stream()))
        torch.cuda.synchronize()
        cf = out[:M].float()
        torch.testing.assert_close(got[:, 0], cf.mean(dim=1), rtol=1e-4, atol=0)
        torch.testing.assert_close(
            got[:, 1], torch.rsqrt(cf.var(dim=1, unbiased=False) + EPS),
            rtol=1e-4, atol=0)
    # 3. run to run
    out2, stats2 = run_form(lib, p, form)
    assert torch.equal(out, out2), f"{name}: C differs from run to run"
    if stats is not None:
        assert torch.equal(stats, stats2), f"{name}: stats differ from run to run"
    # 4. the recorded results
    got_h = hashes_of(p, out, stats)
    if want_hashes is not None:
        assert got_h == want_hashes, f"{name}: {got_h} != recorded {want_hashes}"
    return got_h


def run_shape(lib, M, N, K, forms, golden, log=print):
    p = build_problem(M, N, K)
    return {
        case_id(M, N, K, f): check_case(
            lib, p, f, None if golden is None else golden[case_id(M, N, K, f)],
            log)
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


def load_golden(path):
    return json.loads(pathlib.Path(path).read_text())["hashes"]


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
    golden = load_golden(args.golden) if args.golden else None
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
                     "shape and form; tools/gemm_epilogue_golden.py --write",
            "recorded_at": args.recorded_at,
            "hashes": hashes,
        }
        pathlib.Path(args.write).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"{len(hashes)} cases ok")


if __name__ == "__main__":
    main()
