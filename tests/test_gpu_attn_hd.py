"""cc_attn above head dim 64 against f32 sdpa on the same bf16 QKV.

The MFMA shapes pad the head dim (QK^T in k-steps of 32, PV in fragments of
16 columns), and what lies past a head's last column is the next head, the
next Q/K/V section, the next row or the end of the buffer.  The guards catch
both ways that goes wrong without a fault: the QKV rows sit between two NaN
rows (a pad chunk that is loaded instead of zeroed turns scores into NaN —
within the buffer the pad of one head is live data of the next, which shows
as an error), and the output rows sit between rows of 7.0 in a buffer
pre-filled with 7.0 (a pad column that is stored lands in the next head, or
in the guard row after the last).

Three heads: the second head starts 144 bytes into a row at head dim 72 —
16-byte aligned, not 32.  Sequence lengths: both sides of each rung
threshold (64 | 65, 288 | 289), B/32's 50, L/14's 257 and so400m-384's 729.
"""

import ctypes

import pytest
import torch

from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

N, HEADS = 2, 3
HDS = [64, 72, 80, 88, 96, 104, 112, 120, 128]


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def _sdpa_on_fused_qkv(qkv, n, seq, heads, hd, scale):
    q, k, v = (
        qkv.reshape(n, seq, 3, heads, hd)[:, :, i].permute(0, 2, 1, 3).float()
        for i in range(3)
    )
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale)
    return want.permute(0, 2, 1, 3).reshape(n * seq, heads * hd)


def _check_guarded(lib, hd, seq, force_rung=None):
    """One attention call on guarded buffers, twice: cc_attn (the plan's
    rung), or cc_attn_rung(force_rung)."""
    hidden = HEADS * hd
    rows = N * seq
    planned = hotpath.attn_plan(N, seq, HEADS, hidden).rung
    rung = hotpath.ATTN_RUNGS[planned if force_rung is None else force_rung]
    torch.manual_seed(1000 * hd + seq)
    qkv_buf = torch.full((rows + 2, 3 * hidden), float("nan"), dtype=torch.bfloat16,
                         device="cuda")
    qkv = qkv_buf[1:-1]
    qkv.copy_((torch.randn(rows, 3 * hidden) * 0.5).to(torch.bfloat16))
    assert torch.isnan(qkv_buf[0]).all() and torch.isnan(qkv_buf[-1]).all()
    scale = hd ** -0.5
    stream = torch.cuda.current_stream().cuda_stream

    outs = []
    hotpath.timing_enable(True)
    try:
        for _ in range(2):
            out_buf = torch.full((rows + 2, hidden), 7.0, dtype=torch.bfloat16,
                                 device="cuda")
            out = out_buf[1:-1]
            assert qkv.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            args = (qkv.data_ptr(), out.data_ptr(), N, seq, HEADS, hidden,
                    ctypes.c_float(scale), stream)
            hotpath.check(lib.cc_attn(*args) if force_rung is None
                          else lib.cc_attn_rung(force_rung, *args))
            torch.cuda.synchronize()
            assert torch.all(out_buf[0] == 7.0), "wrote before the first output row"
            assert torch.all(out_buf[-1] == 7.0), "wrote past the last output row"
            outs.append(out)
        launches = {r: hotpath.timing_report(f"attn_{r}")[1] for r in hotpath.ATTN_RUNGS}
    finally:
        hotpath.timing_enable(False)
    assert launches == {r: 2 if r == rung else 0 for r in hotpath.ATTN_RUNGS}

    got = outs[0].float()
    assert torch.isfinite(got).all(), "a pad chunk reached the scores or the output"
    assert torch.equal(outs[0], outs[1]), "attention differs from run to run"
    want = _sdpa_on_fused_qkv(qkv, N, seq, HEADS, hd, scale)
    err = (got - want).abs()
    print(f"hd {hd} seq {seq} ({rung}): max abs err {err.max().item():.3e}")
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("seq", [50, 64, 65, 257, 288, 289, 729])
@pytest.mark.parametrize("hd", HDS)
def test_attn_hd_vs_sdpa(lib, hd, seq):
    """cc_attn: the rung the plan picks."""
    _check_guarded(lib, hd, seq)


@pytest.mark.parametrize("seq", [65, 257, 288])
@pytest.mark.parametrize("hd", HDS)
def test_attn_hd_mid_rung_vs_sdpa(lib, hd, seq):
    """Above head dim 64 the plan gives most of 65..288 to the flash rung
    (it measured faster, csrc/cc_attn_plan.hpp: below head dim 96 all of
    it); k_attn_mid stays launchable at every head dim through cc_attn_rung
    so the choice can be measured again, and is held to the same checks."""
    _check_guarded(lib, hd, seq, force_rung=1)


def test_attn_rung_entry_covers_what_it_can(lib):
    """cc_attn_rung, the A/B entry: any rung that can cover seq runs and
    agrees with the plan's choice within the sdpa tolerance; one that cannot
    is refused before any launch."""
    hd, seq = 72, 50
    hidden = HEADS * hd
    torch.manual_seed(7)
    qkv = (torch.randn(N * seq, 3 * hidden) * 0.5).to(torch.bfloat16).cuda()
    scale = ctypes.c_float(hd ** -0.5)
    stream = torch.cuda.current_stream().cuda_stream
    want = _sdpa_on_fused_qkv(qkv, N, seq, HEADS, hd, hd ** -0.5)
    for rung in range(3):  # seq 50: small, mid and flash all cover it
        out = torch.full((N * seq, hidden), 7.0, dtype=torch.bfloat16, device="cuda")
        hotpath.check(lib.cc_attn_rung(rung, qkv.data_ptr(), out.data_ptr(), N, seq,
                                       HEADS, hidden, scale, stream))
        torch.cuda.synchronize()
        torch.testing.assert_close(out.float(), want, rtol=2e-2, atol=2e-2)
    out = torch.full((N * 65, hidden), 7.0, dtype=torch.bfloat16, device="cuda")
    qkv65 = torch.zeros(N * 65, 3 * hidden, dtype=torch.bfloat16, device="cuda")
    for rung, seq_bad in ((0, 65), (3, 50), (-1, 50)):
        assert lib.cc_attn_rung(rung, qkv65.data_ptr(), out.data_ptr(), N, seq_bad,
                                HEADS, hidden, scale, stream) < 0
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
