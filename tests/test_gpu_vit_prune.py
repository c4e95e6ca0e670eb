"""GPU parity for the last-layer CLS pruning: the cc_attn_cls kernel, the
row-strided GEMM entry point, and the pruned tower against the full one.
"""

import ctypes
import math

import pytest
import torch

from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

HD = 64
SENTINEL = -7.0  # exactly representable in bf16


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize(
    "n,seq,heads",
    [
        (3, 50, 12),   # ViT-B/32
        (2, 1, 1),     # a single key
        (1, 64, 3),    # exactly one full key chunk
        (2, 65, 2),    # one key into the second chunk
        (1, 257, 16),  # ViT-L/14
        (3, 50, 3),    # n*heads = 9 does not fill the last workgroup
    ],
)
def test_attn_cls_vs_torch_sdpa(lib, n, seq, heads):
    hidden = heads * HD
    scale = 1.0 / math.sqrt(HD)
    torch.manual_seed(n * 1000 + seq * 10 + heads)
    q = torch.randn(n, hidden).to(torch.bfloat16).cuda()
    # K and V as the two halves of one [n*seq, 2H] buffer (the K/V GEMM
    # output): strided views, row stride 2H
    kv = torch.randn(n * seq, 2 * hidden).to(torch.bfloat16).cuda()
    k, v = kv[:, :hidden], kv[:, hidden:]
    assert k.stride(0) == v.stride(0) == 2 * hidden
    pad = 2
    buf = torch.full((n + pad, hidden), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hotpath.check(
        lib.cc_attn_cls(q.data_ptr(), k.data_ptr(), v.data_ptr(), 2 * hidden,
                        buf.data_ptr(), n, seq, heads, hidden,
                        ctypes.c_float(scale), _stream())
    )
    torch.cuda.synchronize()
    got = buf[:n].float()
    assert torch.all(buf[n:] == SENTINEL), "wrote past the n output rows"

    def heads_first(t, rows):  # [n*rows, H] -> [n, heads, rows, hd] f32
        return t.reshape(n, rows, heads, HD).permute(0, 2, 1, 3).float()

    want = torch.nn.functional.scaled_dot_product_attention(
        heads_first(q, 1), heads_first(k, seq), heads_first(v, seq), scale=scale
    )
    want = want.permute(0, 2, 1, 3).reshape(n, hidden)
    print(f"attn_cls vs f32 sdpa ({n},{seq},{heads}): max abs diff "
          f"{(got - want).abs().max().item():.3e}")
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2)

    if seq <= 64:
        # same problem through cc_attn_small on the fused-qkv layout: our
        # q is row 0 of each frame, the other query rows are filler
        qkv = torch.randn(n, seq, 3, hidden).to(torch.bfloat16).cuda()
        qkv[:, 0, 0] = q
        qkv[:, :, 1] = k.reshape(n, seq, hidden)
        qkv[:, :, 2] = v.reshape(n, seq, hidden)
        full = torch.empty((n * seq, hidden), dtype=torch.bfloat16, device="cuda")
        hotpath.check(
            lib.cc_attn_small(qkv.data_ptr(), full.data_ptr(), n, seq, heads,
                              hidden, ctypes.c_float(scale), _stream())
        )
        torch.cuda.synchronize()
        small = full.reshape(n, seq, hidden)[:, 0].float()
        print(f"attn_cls vs attn_small row 0 ({n},{seq},{heads}): max abs diff "
              f"{(got - small).abs().max().item():.3e}")
        torch.testing.assert_close(got, small, rtol=2e-2, atol=2e-2)


def test_attn_cls_rejects_bad_args(lib):
    hidden = 2 * HD
    q = torch.zeros(1, hidden, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(4, 2 * hidden + 8, dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, hidden), SENTINEL, dtype=torch.bfloat16, device="cuda")
    args = lambda ldkv, hid, kp: (  # noqa: E731
        q.data_ptr(), kp, kv.data_ptr(), ldkv, out.data_ptr(), 1, 4, 2, hid,
        ctypes.c_float(0.125), _stream())
    assert lib.cc_attn_cls(*args(hidden - 8, hidden, kv.data_ptr())) != 0  # ldkv < H
    assert lib.cc_attn_cls(*args(2 * hidden + 4, hidden, kv.data_ptr())) != 0  # ldkv % 8
    assert lib.cc_attn_cls(*args(2 * hidden, hidden + 64, kv.data_ptr())) != 0  # hd != 64
    assert lib.cc_attn_cls(*args(2 * hidden, hidden, kv.data_ptr() + 2)) != 0  # alignment
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL), "a rejected call launched"


def _strided_gemm(lib, a, lda, b, M, N, K, bias, act, res, ldr):
    out = torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    rc = lib.cc_gemm_bf16_strided(
        a.data_ptr(), lda, b.data_ptr(), out.data_ptr(), M, N, K,
        bias.data_ptr(), 1, act, res.data_ptr() if res is not None else None,
        ldr, _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize(
    ("M", "N", "K"),
    [
        (5, 768, 768),
        (130, 64, 128),  # crosses a 128-row tile edge: row clamp with a stride
    ],
)
def test_strided_gemm_bit_identical_to_gathered(lib, M, N, K):
    seq = 50
    torch.manual_seed(M + N + K)
    a_all = torch.randn(M, seq, K).to(torch.bfloat16).cuda()
    r_all = torch.randn(M, seq, N).to(torch.bfloat16).cuda()
    b = (torch.randn(N, K) * 0.1).to(torch.bfloat16).cuda()
    bias = torch.randn(N).float().cuda()
    a_rows, r_rows = a_all[:, 0], r_all[:, 0]  # strided views
    a_gath, r_gath = a_rows.contiguous(), r_rows.contiguous()

    for act, use_res in ((0, True), (1, False), (0, False)):
        rc, got = _strided_gemm(
            lib, a_rows, seq * K, b, M, N, K, bias, act,
            r_rows if use_res else None, seq * N)
        hotpath.check(rc)
        rc, want = _strided_gemm(
            lib, a_gath, K, b, M, N, K, bias, act,
            r_gath if use_res else None, N)
        hotpath.check(rc)
        assert torch.all(got[M:] == SENTINEL), "wrote past the M output rows"
        assert torch.equal(got, want), (act, use_res)
        # and the dense launch is the unchanged cc_gemm_bf16_ex
        ex = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        hotpath.check(
            lib.cc_gemm_bf16_ex(a_gath.data_ptr(), b.data_ptr(), ex.data_ptr(),
                                M, N, K, bias.data_ptr(), 1, act,
                                r_gath.data_ptr() if use_res else None, _stream())
        )
        torch.cuda.synchronize()
        assert torch.equal(got[:M], ex), (act, use_res)

    # sanity against torch so "identical" cannot mean "identically wrong"
    ref = a_gath.float() @ b.float().T + bias + r_gath.float()
    rc, got = _strided_gemm(lib, a_rows, seq * K, b, M, N, K, bias, 0, r_rows, seq * N)
    hotpath.check(rc)
    torch.testing.assert_close(got[:M].float(), ref, rtol=2e-2, atol=5e-2)


def test_strided_gemm_rejects_bad_strides(lib):
    M, N, K = 5, 128, 128
    a = torch.zeros(M, 4 * K, dtype=torch.bfloat16, device="cuda")
    r = torch.zeros(M, 4 * N, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(N, K, dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(N, dtype=torch.float32, device="cuda")
    for lda, ldr in ((K - 8, N), (K, N - 8), (K + 4, N)):
        rc, out = _strided_gemm(lib, a, lda, b, M, N, K, bias, 0, r, ldr)
        assert rc != 0, (lda, ldr)
        assert torch.all(out == SENTINEL), "a rejected call launched"
    # ldr is ignored without a residual
    rc, _ = _strided_gemm(lib, a, K, b, M, N, K, bias, 0, None, 0)
    assert rc == 0


@pytest.mark.parametrize("model,n", [("vit_b32", 4), ("vit_l14", 2)])
def test_tower_pruned_matches_full(lib, model, n):
    from cosmos_curate_amd.models import clip_weights as cw
    from cosmos_curate_amd.models.clip_vit import ClipVisionTowerAMD

    cfg = cw.CONFIGS[model]
    tower = ClipVisionTowerAMD(cw.make_clip_vit_weights(cfg), cfg).cuda()
    assert tower.prune_last_layer  # pruned is the default
    torch.manual_seed(n)
    pixels = torch.randn(n, 3, cfg.image, cfg.image).to(torch.bfloat16).cuda()
    pruned = tower(pixels)
    again = tower(pixels)
    tower.prune_last_layer = False
    full = tower(pixels)
    torch.cuda.synchronize()
    assert torch.equal(pruned, again), "pruned tower is not run-to-run bit-identical"
    cos = torch.sum(pruned * full, dim=1)  # both unit-norm
    print(f"{model} per-frame cosine pruned vs full: {cos.tolist()}")
    assert torch.all(cos >= 0.9999), cos
