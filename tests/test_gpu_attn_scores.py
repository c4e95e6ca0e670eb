"""The attention kernels against float64 attention on inputs whose softmax
scores matter (attn_ref.py): a few keys carry every row, so the mask at
seq, the running max and the rescale of O, the scale, the pairing of keys
with values and the last key tile all show in the output.  The bound is
attn_ref.BOUND on max |got - ref64| / max |v|, 3 x the worst error of a
plain emulation of the kernels' numerics; test_attn_ref_cpu.py proves that
each of eight wrong attentions lands beyond twice that bound.

Layout and guards as test_gpu_attn_hd.py: fused [n*seq, 3*hidden] QKV
between two NaN rows, the output between two rows of 7.0 in a buffer filled
with 7.0, two runs that must agree bit for bit.  Every case prints its
error, so the log records how far inside the bound each rung sits.
"""

import ctypes
import functools

import pytest
import torch

import attn_ref as R
from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

SENTINEL = 7.0  # exactly representable in bf16


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


@functools.lru_cache(maxsize=None)
def _problem(family, seq, hd):
    """q, k, v and their float64 reference, computed once and not modified."""
    q, k, v = R.make_inputs(family, seq, hd, R.seed_of(family, seq, hd))
    return q, k, v, R.ref64(q, k, v)


def _guarded(rows_cpu, fill=float("nan")):
    """`rows_cpu` on the device between two rows of `fill`: (buffer, view)."""
    buf = torch.full((rows_cpu.shape[0] + 2, rows_cpu.shape[1]), fill,
                     dtype=torch.bfloat16, device="cuda")
    buf[1:-1].copy_(rows_cpu)
    return buf, buf[1:-1]


def _launches():
    return {name: hotpath.timing_report(f"attn_{name}")[1]
            for name in (*hotpath.ATTN_RUNGS, "cls")}


def _run_fused(lib, q, k, v, force_rung):
    """cc_attn (force_rung None) or cc_attn_rung on guarded buffers, twice.
    Returns the output as [n, heads, seq, hd] on the CPU and the rung run."""
    n, heads, seq, hd = q.shape
    hidden, rows = heads * hd, n * seq
    planned = hotpath.attn_plan(n, seq, heads, hidden).rung
    rung = hotpath.ATTN_RUNGS[planned if force_rung is None else force_rung]
    qkv_buf, qkv = _guarded(R.fuse_qkv(q, k, v))
    assert torch.isnan(qkv_buf[0]).all() and torch.isnan(qkv_buf[-1]).all()
    stream = torch.cuda.current_stream().cuda_stream

    outs = []
    hotpath.timing_enable(True)
    try:
        for _ in range(2):
            out_buf = torch.full((rows + 2, hidden), SENTINEL, dtype=torch.bfloat16,
                                 device="cuda")
            out = out_buf[1:-1]
            assert qkv.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            args = (qkv.data_ptr(), out.data_ptr(), n, seq, heads, hidden,
                    ctypes.c_float(R.scale_of(hd)), stream)
            hotpath.check(lib.cc_attn(*args) if force_rung is None
                          else lib.cc_attn_rung(force_rung, *args))
            torch.cuda.synchronize()
            assert torch.all(out_buf[0] == SENTINEL), "wrote before the first output row"
            assert torch.all(out_buf[-1] == SENTINEL), "wrote past the last output row"
            outs.append(out)
        launches = _launches()
    finally:
        hotpath.timing_enable(False)
    assert launches == {r: 2 if r == rung else 0 for r in launches}
    assert torch.isfinite(outs[0].float()).all(), \
        "a pad chunk or a masked key reached the output"
    assert torch.equal(outs[0], outs[1]), "attention differs from run to run"
    return R.unfuse_out(outs[0].cpu(), n, heads, seq, hd), rung


def _check_fused(lib, label, seq, hd, family, force_rung):
    q, k, v, ref = _problem(family, seq, hd)
    got, rung = _run_fused(lib, q, k, v, force_rung)
    err = R.error(got, ref, v)
    print(f"attn_scores {label} ({rung}) seq {seq} hd {hd} {family}: "
          f"err {err:.5f} = {err / R.BOUND:.2f} x BOUND")
    assert err <= R.BOUND
    return rung


def _ids(cases):
    return [f"{seq}-{hd}-{family}" for _, seq, hd, family in cases]


def _rung_cases(name):
    return [c for c in R.RUNG_CASES if c[0] == name]


@pytest.mark.parametrize("case", _rung_cases("small"), ids=_ids(_rung_cases("small")))
def test_small_rung(lib, case):
    """k_attn_small: one key, a ragged tile, the full 64."""
    _, seq, hd, family = case
    _check_fused(lib, "small", seq, hd, family, force_rung=0)


@pytest.mark.parametrize("case", _rung_cases("mid"), ids=_ids(_rung_cases("mid")))
def test_mid_rung(lib, case):
    """k_attn_mid: one row into the second q-tile, three q-tiles, its last seq."""
    _, seq, hd, family = case
    _check_fused(lib, "mid", seq, hd, family, force_rung=1)


@pytest.mark.parametrize("case", _rung_cases("flash"), ids=_ids(_rung_cases("flash")))
def test_flash_rung(lib, case):
    """k_attn_flash: less than one KV tile (33); two Q and two KV tiles (65);
    three (129); one past mid's range (289); six KV tiles, the last with one
    row (321)."""
    _, seq, hd, family = case
    _check_fused(lib, "flash", seq, hd, family, force_rung=2)


@pytest.mark.parametrize("case", R.PLANNED_CASES, ids=_ids(R.PLANNED_CASES))
def test_planned_rung_every_head_dim(lib, case):
    """cc_attn's own choice at every head dim: the pad columns of a head are
    the next head's live data, and `neg_offset` and `last_key` are the
    families that a stray key or a lost one moves most."""
    _, seq, hd, family = case
    rung = _check_fused(lib, "planned", seq, hd, family, force_rung=None)
    assert rung == ("small" if seq == 50 else "flash")


@pytest.mark.parametrize("case", R.CLS_CASES, ids=_ids(R.CLS_CASES))
def test_cls(lib, case):
    """k_attn_cls: q is row 0 of each frame, K and V are the strided halves of
    one [n*seq, 2H] buffer; sentinel rows follow the n output rows."""
    _, seq, hd, family = case
    q, k, v, ref = _problem(family, seq, hd)
    n, heads = q.shape[:2]
    hidden = heads * hd
    ref0 = ref[:, :, :1]

    def rows(t):  # [n, heads, s, hd] -> [n*s, hidden]
        return t.permute(0, 2, 1, 3).reshape(-1, hidden)

    q_buf, q0 = _guarded(rows(q[:, :, :1]))
    kv_buf, kv = _guarded(torch.cat([rows(k), rows(v)], dim=1))
    kd, vd = kv[:, :hidden], kv[:, hidden:]
    assert kd.stride(0) == vd.stride(0) == 2 * hidden
    assert torch.isnan(kv_buf[0]).all() and torch.isnan(kv_buf[-1]).all()
    stream = torch.cuda.current_stream().cuda_stream

    outs = []
    hotpath.timing_enable(True)
    try:
        for _ in range(2):
            buf = torch.full((n + 2, hidden), SENTINEL, dtype=torch.bfloat16,
                             device="cuda")
            for p in (q0, kd, vd, buf):
                assert p.data_ptr() % 16 == 0
            hotpath.check(lib.cc_attn_cls(
                q0.data_ptr(), kd.data_ptr(), vd.data_ptr(), 2 * hidden,
                buf.data_ptr(), n, seq, heads, hidden,
                ctypes.c_float(R.scale_of(hd)), stream))
            torch.cuda.synchronize()
            assert torch.all(buf[n:] == SENTINEL), "wrote past the n output rows"
            outs.append(buf[:n])
        launches = _launches()
    finally:
        hotpath.timing_enable(False)
    assert launches == {r: 2 if r == "cls" else 0 for r in launches}
    assert torch.isfinite(outs[0].float()).all(), "a masked key reached the output"
    assert torch.equal(outs[0], outs[1]), "attn_cls differs from run to run"
    got = R.unfuse_out(outs[0].cpu(), n, heads, 1, hd)
    err = R.error(got, ref0, v)
    print(f"attn_scores cls seq {seq} hd {hd} {family}: "
          f"err {err:.5f} = {err / R.BOUND:.2f} x BOUND")
    assert err <= R.BOUND

    if seq <= R.TILE:
        # the same problem through the small rung: its row 0 is held to the
        # same reference
        full, _ = _run_fused(lib, q, k, v, force_rung=0)
        err0 = R.error(full[:, :, :1], ref0, v)
        print(f"attn_scores cls seq {seq} hd {hd} {family}: small rung's row 0 "
              f"err {err0:.5f} = {err0 / R.BOUND:.2f} x BOUND")
        assert err0 <= R.BOUND
