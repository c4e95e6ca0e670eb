"""The LayerNorm family at H = 1152 (SigLIP-so400m's hidden size).

1152 = 18 blocks of 64 columns = 4.5 steps of 256: the wave-per-row kernels
run their last step on half a wave.  Checked: the LN kernel, the row
statistics and their finalisation, and the two folded GEMMs (LN on the
input at K = 1152, statistics of the output at N = 1152) on both bodies.
Tolerances are those tests/test_gpu_vit.py and tests/test_gpu_gemm_ln.py
use for the same calls.
"""

import ctypes

import pytest
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models.vit_encoder import fold_layernorm

pytestmark = pytest.mark.gpu

H = 1152
EPS = 1e-6  # SigLIP's
SENTINEL = -7.0  # exactly representable in bf16 and f32


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows_with_offsets(M, width):
    """randn rows shifted so no row mean sits near zero (the statistics are
    checked with a relative tolerance only)."""
    off = 0.5 + 1.5 * torch.rand(M, 1)
    return (torch.randn(M, width) + off).to(torch.bfloat16).cuda()


def _finalize(lib, stats, M, width):
    out = torch.full((M + 1, 2), SENTINEL, dtype=torch.float32, device="cuda")
    hotpath.check(lib.cc_ln_finalize(
        stats.data_ptr(), M, width, 1, ctypes.c_float(EPS), out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert torch.all(out[M:] == SENTINEL), "finalize wrote past the M rows"
    return out[:M]


def _torch_mean_rstd(x_bf16):
    xf = x_bf16.float()
    return xf.mean(dim=1), torch.rsqrt(xf.var(dim=1, unbiased=False) + EPS)


def test_layernorm_1152(lib):
    M = 5  # not a multiple of the 4 rows per workgroup
    torch.manual_seed(M + H)
    x = (torch.randn(M, H) * 2).to(torch.bfloat16).cuda()
    w = torch.randn(H).float().cuda()
    b = torch.randn(H).float().cuda()
    out = torch.full((M + 1, H), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hotpath.check(lib.cc_layernorm_bf16(
        x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), M, H,
        ctypes.c_float(EPS), _stream()))
    torch.cuda.synchronize()
    assert torch.all(out[M:] == SENTINEL), "wrote past the M rows"
    want = torch.nn.functional.layer_norm(x.float(), (H,), w, b, eps=EPS)
    torch.testing.assert_close(out[:M].float(), want, rtol=2e-2, atol=2e-2)


def test_ln_stats_and_finalize_1152(lib):
    M = 5
    torch.manual_seed(M + H + 1)
    x = _rows_with_offsets(M, H)
    pad = 3
    runs = []
    for _ in range(2):
        stats = torch.full((M + pad, H // 64, 2), SENTINEL, dtype=torch.float32,
                           device="cuda")
        hotpath.check(lib.cc_ln_stats_bf16(x.data_ptr(), M, H, stats.data_ptr(),
                                           _stream()))
        torch.cuda.synchronize()
        assert torch.all(stats[M:] == SENTINEL), "wrote past the M stats rows"
        runs.append(stats)
    assert torch.equal(runs[0], runs[1]), "stats differ from run to run"
    xb = x.float().reshape(M, H // 64, 64)
    s, ss = xb.sum(dim=2), (xb * xb).sum(dim=2)
    torch.testing.assert_close(runs[0][:M, :, 0], s, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(runs[0][:M, :, 1], ss, rtol=1e-5, atol=1e-4)
    # k_layernorm_bf16's form, from the reference partials
    mean = s.sum(dim=1) / H
    rstd = torch.rsqrt(ss.sum(dim=1) / H - mean * mean + EPS)
    got = _finalize(lib, runs[0], M, H)
    torch.testing.assert_close(got[:, 0], mean, rtol=1e-4, atol=0)
    torch.testing.assert_close(got[:, 1], rstd, rtol=1e-4, atol=0)
    assert torch.equal(got, _finalize(lib, runs[1], M, H))


def _act(v, act):
    if act == 1:
        return v * torch.sigmoid(1.702 * v)
    if act == 2:
        return torch.nn.functional.gelu(v, approximate="tanh")
    return v


@pytest.mark.parametrize(("M", "N", "body"), [(8, 768, 128), (300, 1536, 256)])
def test_gemm_ln_k1152(lib, M, N, body):
    K = H
    torch.manual_seed(M + N + K)
    # row means up to 4 sigma, two large channels: the mean term matters
    x = torch.randn(M, K) + torch.linspace(-4.0, 4.0, M)[:, None]
    x[:, 5] = 20.0
    x[:, K - 3] = -20.0
    x = x.to(torch.bfloat16).cuda()
    w = (torch.randn(N, K) / K**0.5).to(torch.bfloat16)
    b = 0.1 * torch.randn(N)
    gamma = 1.0 + 0.2 * torch.randn(K)
    beta = 0.1 * torch.randn(K)
    w_fold, colsum, cbias = (t.cuda() for t in fold_layernorm(w.float(), b, gamma, beta))
    pre = torch.nn.functional.linear(
        torch.nn.functional.layer_norm(
            x.float(), (K,), gamma.cuda(), beta.cuda(), eps=EPS),
        w.float().cuda(), b.cuda())
    stats = torch.empty((M, K // 64, 2), dtype=torch.float32, device="cuda")
    hotpath.check(lib.cc_ln_stats_bf16(x.data_ptr(), M, K, stats.data_ptr(), _stream()))
    for act in (0, 1, 2):
        assert hotpath.gemm_plan(M, N, K, has_bias=True, act=act).body == body
        outs = []
        for _ in range(2):
            out = torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
            ws = torch.empty((M, 2), dtype=torch.float32, device="cuda")
            hotpath.check(lib.cc_gemm_bf16_ln(
                x.data_ptr(), 1, stats.data_ptr(), ws.data_ptr(), w_fold.data_ptr(),
                colsum.data_ptr(), cbias.data_ptr(), out.data_ptr(), M, N, K, act,
                ctypes.c_float(EPS), _stream()))
            torch.cuda.synchronize()
            assert torch.all(out[M:] == SENTINEL), "wrote past the M output rows"
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "gemm_ln differs from run to run"
        want = _act(pre, act)
        err = (outs[0][:M].float() - want).abs()
        print(f"gemm_ln ({M},{N},{K}) act {act}: max abs err {err.max().item():.3e}")
        torch.testing.assert_close(outs[0][:M].float(), want, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize(("M", "K", "body"), [(8, 1152, 128), (300, 1536, 256)])
def test_gemm_res_stats_n1152(lib, M, K, body):
    N = H
    assert hotpath.gemm_plan(M, N, K, has_bias=True, has_residual=True).body == body
    torch.manual_seed(M + N + K)
    a = torch.randn(M, K).to(torch.bfloat16).cuda()
    w = (torch.randn(N, K) / K**0.5).to(torch.bfloat16).cuda()
    bias = (0.1 * torch.randn(N)).cuda()
    res = _rows_with_offsets(M, N)
    ex = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    hotpath.check(lib.cc_gemm_bf16_ex(
        a.data_ptr(), w.data_ptr(), ex.data_ptr(), M, N, K, bias.data_ptr(), 1, 0,
        res.data_ptr(), _stream()))
    pad = 3
    runs = []
    for _ in range(2):
        out = torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
        stats = torch.full((M + pad, N // 64, 2), SENTINEL, dtype=torch.float32,
                           device="cuda")
        hotpath.check(lib.cc_gemm_bf16_res_stats(
            a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, bias.data_ptr(),
            res.data_ptr(), stats.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert torch.all(out[M:] == SENTINEL), "wrote past the M output rows"
        assert torch.equal(out[:M], ex), "C differs from cc_gemm_bf16_ex"
        assert torch.all(stats[M:] == SENTINEL), "wrote past the M stats rows"
        runs.append(stats)
    assert torch.equal(runs[0], runs[1]), "stats differ from run to run"
    # C is x @ w^T + b + r ...
    want = (torch.nn.functional.linear(a.float(), w.float(), bias) + res.float())
    torch.testing.assert_close(ex.float(), want, rtol=2e-2, atol=8e-2)
    # ... and the statistics are the block sums of the C that was stored
    cb = ex.float().reshape(M, N // 64, 64)
    torch.testing.assert_close(runs[0][:M, :, 0], cb.sum(dim=2), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(runs[0][:M, :, 1], (cb * cb).sum(dim=2), rtol=1e-5, atol=1e-4)
    got = _finalize(lib, runs[0], M, N)
    mean, rstd = _torch_mean_rstd(ex)
    torch.testing.assert_close(got[:, 0], mean, rtol=1e-4, atol=0)
    torch.testing.assert_close(got[:, 1], rstd, rtol=1e-4, atol=0)
