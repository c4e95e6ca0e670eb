"""The kernels the InternVideo2 tower added: the norm family at H = 1408,
RMSNorm (stand-alone, folded into a GEMM, and as QK-norm), the erf-GELU
epilogue, and cc_attn at the tower's head geometry.

1408 = 22 blocks of 64 columns = 5.5 steps of 256, so the wave-per-row
kernels run their last step on half a wave.  Inputs sit between NaN rows
and outputs between sentinel rows: an overrun by a row or a column shows as
a NaN or a broken sentinel, not as a fault.  Tolerances: rtol = atol = 2e-2
against torch f32 on the stored bf16 inputs (tests/test_gpu_gemm_ln.py); the
statistics to 1e-5 relative (tests/test_gpu_ln_1152.py).
"""

import ctypes

import pytest
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models.vit_encoder import fold_rmsnorm

pytestmark = pytest.mark.gpu

H = 1408
EPS = 1e-6
SENTINEL = -7.0  # exactly representable in bf16 and f32
CC_ERR_INVALID, CC_ERR_UNSUPPORTED = -1, -6  # include/cc_hotpath.h


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded_input(M, width, scale=2.0, offset=True):
    """[M, width] bf16 rows between two NaN rows."""
    buf = torch.full((M + 2, width), float("nan"), dtype=torch.bfloat16, device="cuda")
    x = torch.randn(M, width) * scale
    if offset:
        x = x + (0.5 + 1.5 * torch.rand(M, 1))
    buf[1:-1].copy_(x.to(torch.bfloat16))
    return buf, buf[1:-1]


def _guarded_output(M, width, dtype=torch.bfloat16):
    buf = torch.full((M + 2, width), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def _assert_guards(buf, what):
    assert torch.all(buf[0] == SENTINEL), f"{what}: wrote before the first row"
    assert torch.all(buf[-1] == SENTINEL), f"{what}: wrote past the last row"


def _rms_ref(x_bf16, w):
    """The kernel's own rounding order in f32: bf16(bf16(x * rstd) * w)."""
    xf = x_bf16.float()
    rstd = torch.rsqrt((xf * xf).mean(dim=-1, keepdim=True) + EPS)
    return ((xf * rstd).to(torch.bfloat16).float() * w).to(torch.bfloat16).float()


@pytest.mark.parametrize("width", [H, 768])
def test_rmsnorm(lib, width):
    M = 5  # one full workgroup of 4 waves plus one row
    torch.manual_seed(M + width)
    _, x = _guarded_input(M, width)
    w = (1.0 + 0.2 * torch.randn(width)).cuda()
    out_buf, out = _guarded_output(M, width)
    hotpath.check(lib.cc_rmsnorm_bf16(
        x.data_ptr(), w.data_ptr(), out.data_ptr(), M, width, EPS, _stream()))
    torch.cuda.synchronize()
    _assert_guards(out_buf, "rmsnorm")
    got = out.float()
    assert torch.isfinite(got).all(), "a NaN guard row reached the output"
    # same rounding order; rstd is rsqrtf on the device, so either of the
    # two roundings may fall the other way: two bf16 steps (2 * 2^-7).
    # And within the GEMM-level budget of the true f32 value
    want = _rms_ref(x, w)
    torch.testing.assert_close(got, want, rtol=2**-6, atol=1e-6)
    xf = x.float()
    true = xf * torch.rsqrt((xf * xf).mean(dim=-1, keepdim=True) + EPS) * w
    torch.testing.assert_close(got, true, rtol=2e-2, atol=2e-2)


def test_rmsnorm_refuses_other_widths(lib):
    x = torch.zeros(4, 3200, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(3200, device="cuda")
    out = torch.full_like(x, SENTINEL)
    rc = lib.cc_rmsnorm_bf16(x.data_ptr(), w.data_ptr(), out.data_ptr(), 4, 3200,
                             EPS, _stream())
    assert rc == CC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)


def test_layernorm_1408(lib):
    M = 5
    torch.manual_seed(M + H)
    _, x = _guarded_input(M, H)
    w = torch.randn(H).cuda()
    b = torch.randn(H).cuda()
    out_buf, out = _guarded_output(M, H)
    hotpath.check(lib.cc_layernorm_bf16(
        x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), M, H, EPS,
        _stream()))
    torch.cuda.synchronize()
    _assert_guards(out_buf, "layernorm")
    want = torch.nn.functional.layer_norm(x.float(), (H,), w, b, eps=EPS)
    torch.testing.assert_close(out.float(), want, rtol=2e-2, atol=2e-2)


def _stats(lib, x, M, width):
    buf, stats = _guarded_output(M, (width // 64) * 2, dtype=torch.float32)
    hotpath.check(lib.cc_ln_stats_bf16(x.data_ptr(), M, width, stats.data_ptr(),
                                       _stream()))
    torch.cuda.synchronize()
    _assert_guards(buf, "ln_stats")
    return stats.reshape(M, width // 64, 2)


def test_ln_stats_1408(lib):
    M = 5
    torch.manual_seed(M + H + 1)
    _, x = _guarded_input(M, H)
    runs = [_stats(lib, x, M, H) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]), "stats differ from run to run"
    assert torch.isfinite(runs[0]).all(), "a NaN guard row reached the stats"
    xb = x.float().reshape(M, H // 64, 64)
    s, ss = xb.sum(dim=2), (xb * xb).sum(dim=2)
    torch.testing.assert_close(runs[0][:, :, 0], s, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(runs[0][:, :, 1], ss, rtol=1e-5, atol=1e-4)
    # the half step: blocks 20 and 21, held by lanes 0..31 of the last step
    for blk in (20, 21):
        torch.testing.assert_close(runs[0][:, blk, 0], s[:, blk], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(runs[0][:, blk, 1], ss[:, blk], rtol=1e-5, atol=1e-4)


def test_rms_finalize(lib):
    """murstd = (0, rsqrt(sum x^2/H + eps)) of every row_step-th stats row."""
    rows, step = 10, 3
    M = (rows + step - 1) // step  # rows 0, 3, 6, 9
    torch.manual_seed(rows + H)
    _, x = _guarded_input(rows, H)
    stats = _stats(lib, x, rows, H)
    outs = []
    for _ in range(2):
        buf, out = _guarded_output(M, 2, dtype=torch.float32)
        hotpath.check(lib.cc_rms_finalize(
            stats.data_ptr(), M, H, step, EPS, out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        _assert_guards(buf, "rms_finalize")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert torch.all(outs[0][:, 0] == 0.0), "the mean column must be exactly 0"
    want = torch.rsqrt(stats[::step, :, 1].sum(dim=1) / H + EPS)
    torch.testing.assert_close(outs[0][:, 1], want, rtol=1e-5, atol=0)


def test_qk_rmsnorm(lib):
    M, ld = 5, 3 * H
    torch.manual_seed(M + ld)
    buf = torch.full((M + 2, ld), SENTINEL, dtype=torch.bfloat16, device="cuda")
    qkv = buf[1:-1]
    qkv.copy_((torch.randn(M, ld) * 2 + 0.5).to(torch.bfloat16))
    before = buf.clone()
    wq = (1.0 + 0.2 * torch.randn(H)).cuda()
    wk = (1.0 + 0.2 * torch.randn(H)).cuda()
    assert not torch.equal(wq, wk)  # a swapped weight must show
    hotpath.check(lib.cc_qk_rmsnorm_bf16(
        qkv.data_ptr(), M, H, ld, wq.data_ptr(), wk.data_ptr(), EPS, _stream()))
    torch.cuda.synchronize()
    # the guard rows and the v section: byte-equal to before the call
    assert torch.equal(buf[0], before[0]) and torch.equal(buf[-1], before[-1])
    assert torch.equal(qkv[:, 2 * H:], before[1:-1, 2 * H:]), "v was touched"
    x = before[1:-1]
    for name, sec, w, other in (("q", 0, wq, wk), ("k", 1, wk, wq)):
        got = qkv[:, sec * H:(sec + 1) * H].float()
        want = _rms_ref(x[:, sec * H:(sec + 1) * H], w)
        torch.testing.assert_close(got, want, rtol=2**-6, atol=1e-6,
                                   msg=lambda m: f"{name}: {m}")
        swapped = _rms_ref(x[:, sec * H:(sec + 1) * H], other)
        assert (got - swapped).abs().max() > 0.1, "the test cannot tell wq from wk"


def test_qk_rmsnorm_refuses_bad_ld(lib):
    qkv = torch.full((4, 3 * H), SENTINEL, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(H, device="cuda")
    for ld in (2 * H - 4, 3 * H + 1):
        rc = lib.cc_qk_rmsnorm_bf16(qkv.data_ptr(), 4, H, ld, w.data_ptr(),
                                    w.data_ptr(), EPS, _stream())
        assert rc == CC_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(qkv == SENTINEL)


def _gelu_erf(v):
    return torch.nn.functional.gelu(v, approximate="none")


@pytest.mark.parametrize(("M", "N", "body"), [(300, 256, 128), (300, 6144, 256)])
def test_gemm_erf_gelu(lib, M, N, body):
    K = H
    assert hotpath.gemm_plan(M, N, K, has_bias=True, act=3).body == body
    torch.manual_seed(M + N + K)
    _, a = _guarded_input(M, K, scale=1.0, offset=False)
    w = (0.5 * torch.randn(N, K) / K**0.5).to(torch.bfloat16).cuda()
    # pre-activations span [-6, 6]: both erf tails and the middle
    bias = torch.linspace(-6.0, 6.0, N).cuda()
    out_buf, out = _guarded_output(M, N)
    hotpath.check(lib.cc_gemm_bf16_ex(
        a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, bias.data_ptr(), 1, 3,
        None, _stream()))
    torch.cuda.synchronize()
    _assert_guards(out_buf, "gemm act 3")
    pre = torch.nn.functional.linear(a.float(), w.float(), bias)
    assert pre.min() < -5.5 and pre.max() > 5.5
    got = out.float()
    assert torch.isfinite(got).all()
    err = (got - _gelu_erf(pre)).abs()
    print(f"erf-gelu ({M},{N},{K}) body {body}: max abs err {err.max().item():.3e}")
    torch.testing.assert_close(got, _gelu_erf(pre), rtol=2e-2, atol=2e-2)
    # it is the erf form, not the tanh one: they differ by up to 4.7e-4
    # around |v| = 2, which bf16 resolves only where the value is small —
    # so compare in the left tail, where gelu itself is ~ -1e-3..-5e-2
    tail = (pre > -3.5) & (pre < -2.0)
    d_erf = (got - _gelu_erf(pre))[tail].abs().mean()
    d_tanh = (got - torch.nn.functional.gelu(pre, approximate="tanh"))[tail].abs().mean()
    assert d_erf < d_tanh


def test_gemm_act_values(lib):
    """act 3 with a residual or without a bias is not instantiated, and no
    value outside 0..3 is taken for "none"."""
    M, N, K = 64, 128, 128
    a = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(N, K, dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(N, device="cuda")
    res = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    out = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device="cuda")

    def call(act, bias_p, res_p):
        return lib.cc_gemm_bf16_ex(a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K,
                                   bias_p, 1, act, res_p, _stream())

    assert call(3, bias.data_ptr(), res.data_ptr()) == CC_ERR_UNSUPPORTED
    assert call(3, None, None) == CC_ERR_UNSUPPORTED
    assert call(4, bias.data_ptr(), None) == CC_ERR_INVALID
    assert call(-1, bias.data_ptr(), None) == CC_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL), "a refused call wrote a result"
    assert call(3, bias.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)


# M: the 128 body (M <= 128), the 256 body, and a 256 grid of more than 256
# tiles, where the persistent loop walks a second tile in some workgroups
@pytest.mark.parametrize(("M", "N", "act", "body", "tiles"), [
    (8, 4224, 0, 128, None), (300, 4224, 0, 256, 34), (3900, 4224, 0, 256, 272),
    (8, 6144, 3, 128, None), (300, 6144, 3, 256, 48), (2600, 6144, 3, 256, 264),
])
def test_gemm_rms(lib, M, N, act, body, tiles):
    K = H
    plan = hotpath.gemm_plan(M, N, K, has_bias=True, act=act)
    assert plan.body == body
    if tiles is not None:
        assert plan.tiles_x * plan.tiles_y == tiles
        assert (plan.grid < tiles) == (tiles > 256)
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K) + torch.linspace(-4.0, 4.0, M)[:, None]
    x[:, 5] = 20.0
    x[:, K - 3] = -20.0  # in the half step
    x_buf = torch.full((M + 2, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    x_buf[1:-1].copy_(x.to(torch.bfloat16))
    x = x_buf[1:-1]
    w = (torch.randn(N, K) / K**0.5).to(torch.bfloat16)
    b = 0.1 * torch.randn(N) if act else None  # qkv has no bias
    g = 1.0 + 0.2 * torch.randn(K)
    w_fold, zeros, cbias = (t.cuda() for t in fold_rmsnorm(w.float(), b, g))
    xf = x.float()
    normed = xf * torch.rsqrt((xf * xf).mean(dim=1, keepdim=True) + EPS) * g.cuda()
    want = torch.nn.functional.linear(
        normed, w.float().cuda(), None if b is None else b.cuda())
    if act:
        want = _gelu_erf(want)
    stats = _stats(lib, x, M, K)
    outs = []
    for _ in range(2):
        out_buf, out = _guarded_output(M, N)
        ws = torch.empty((M, 2), dtype=torch.float32, device="cuda")
        hotpath.check(lib.cc_gemm_bf16_rms(
            x.data_ptr(), 1, stats.data_ptr(), ws.data_ptr(), w_fold.data_ptr(),
            zeros.data_ptr(), cbias.data_ptr(), out.data_ptr(), M, N, K, act, EPS,
            _stream()))
        torch.cuda.synchronize()
        _assert_guards(out_buf, "gemm_rms")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "gemm_rms differs from run to run"
    got = outs[0].float()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    print(f"gemm_rms ({M},{N},{K}) act {act}: max abs err {err.max().item():.3e}")
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize(("M", "K", "body"), [(8, 1408, 128), (300, 1408, 128),
                                              (300, 6144, 256)])
def test_gemm_res_stats_n1408(lib, M, K, body):
    """Out-proj (N = K = 1408) gets the 128 body, which runs the stats
    kernel after the GEMM; fc2 (K = 6144) the 256 body's stats epilogue."""
    N = H
    assert hotpath.gemm_plan(M, N, K, has_bias=True, has_residual=True).body == body
    torch.manual_seed(M + N + K)
    _, a = _guarded_input(M, K, scale=1.0, offset=False)
    w = (torch.randn(N, K) / K**0.5).to(torch.bfloat16).cuda()
    bias = (0.1 * torch.randn(N)).cuda()
    _, res = _guarded_input(M, N, scale=1.0)
    ex = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    hotpath.check(lib.cc_gemm_bf16_ex(
        a.data_ptr(), w.data_ptr(), ex.data_ptr(), M, N, K, bias.data_ptr(), 1, 0,
        res.data_ptr(), _stream()))
    runs = []
    for _ in range(2):
        out_buf, out = _guarded_output(M, N)
        st_buf, stats = _guarded_output(M, (N // 64) * 2, dtype=torch.float32)
        hotpath.check(lib.cc_gemm_bf16_res_stats(
            a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, bias.data_ptr(),
            res.data_ptr(), stats.data_ptr(), _stream()))
        torch.cuda.synchronize()
        _assert_guards(out_buf, "res_stats C")
        _assert_guards(st_buf, "res_stats stats")
        assert torch.equal(out, ex), "C differs from cc_gemm_bf16_ex"
        runs.append(stats.reshape(M, N // 64, 2))
    assert torch.equal(runs[0], runs[1]), "stats differ from run to run"
    want = torch.nn.functional.linear(a.float(), w.float(), bias) + res.float()
    torch.testing.assert_close(ex.float(), want, rtol=2e-2, atol=8e-2)
    ref = _stats(lib, ex, M, N)
    if body == 128:  # the same kernel on the same C
        assert torch.equal(runs[0], ref)
    torch.testing.assert_close(runs[0], ref, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("seq", [33, 129, 1025])
def test_attn_hd88_16_heads(lib, seq):
    """cc_attn at the tower's geometry (16 heads of 88) and its sequence
    lengths: 33 (small rung), 129 and 1025 (flash; no multiple of 64)."""
    n, heads, hd = 2, 16, 88
    hidden = heads * hd
    rows = n * seq
    rung = hotpath.ATTN_RUNGS[hotpath.attn_plan(n, seq, heads, hidden).rung]
    assert rung == ("small" if seq == 33 else "flash")
    torch.manual_seed(1000 * hd + seq)
    qkv_buf = torch.full((rows + 2, 3 * hidden), float("nan"), dtype=torch.bfloat16,
                         device="cuda")
    qkv = qkv_buf[1:-1]
    qkv.copy_((torch.randn(rows, 3 * hidden) * 0.5).to(torch.bfloat16))
    scale = hd ** -0.5
    outs = []
    for _ in range(2):
        out_buf = torch.full((rows + 2, hidden), 7.0, dtype=torch.bfloat16, device="cuda")
        out = out_buf[1:-1]
        assert qkv.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        hotpath.check(lib.cc_attn(qkv.data_ptr(), out.data_ptr(), n, seq, heads, hidden,
                                  ctypes.c_float(scale), _stream()))
        torch.cuda.synchronize()
        assert torch.all(out_buf[0] == 7.0), "wrote before the first output row"
        assert torch.all(out_buf[-1] == 7.0), "wrote past the last output row"
        outs.append(out)
    got = outs[0].float()
    assert torch.isfinite(got).all(), "a pad chunk reached the scores or the output"
    assert torch.equal(outs[0], outs[1]), "attention differs from run to run"
    q, k, v = (qkv.reshape(n, seq, 3, heads, hd)[:, :, i].permute(0, 2, 1, 3).float()
               for i in range(3))
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale)
    want = want.permute(0, 2, 1, 3).reshape(rows, hidden)
    err = (got - want).abs()
    print(f"hd {hd} seq {seq} ({rung}): max abs err {err.max().item():.3e}")
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2)
