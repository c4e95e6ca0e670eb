"""GPU parity for LayerNorm folded into the GEMMs: the row
statistics (stand-alone kernel and the residual GEMM's epilogue), the
consuming GEMM on both bodies and across the persistent walk, and whole
towers on the folded route against the fp32 oracle.
"""

import ctypes

import numpy as np
import pytest
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models.vit_encoder import fold_layernorm

pytestmark = pytest.mark.gpu

EPS = 1e-5
SENTINEL = -7.0  # exactly representable in bf16 and f32


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _finalize(lib, stats, M, H, row_step=1, eps=EPS):
    out = torch.empty((M, 2), dtype=torch.float32, device="cuda")
    hotpath.check(lib.cc_ln_finalize(
        stats.data_ptr(), M, H, row_step, ctypes.c_float(eps), out.data_ptr(),
        _stream()))
    return out


def _torch_mean_rstd(x_bf16, eps=EPS):
    xf = x_bf16.float()
    var = xf.var(dim=1, unbiased=False)
    return xf.mean(dim=1), torch.rsqrt(var + eps)


def _rows_with_offsets(M, H):
    """randn rows shifted so no row mean sits near zero (the stats are
    checked with a relative tolerance only)."""
    off = 0.5 + 1.5 * torch.rand(M, 1)
    return (torch.randn(M, H) + off).to(torch.bfloat16).cuda()


# one row short of / past the 4-rows-per-workgroup grid; every row-width
# family: the 2-per-lane H = 128 kernel, one, three and four 256-column steps
@pytest.mark.parametrize(("M", "H"), [(37, 128), (5, 256), (300, 768), (66, 1024)])
def test_ln_stats_kernel(lib, M, H):
    torch.manual_seed(M + H)
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
    # the partials are per 64-column block
    xb = x.float().reshape(M, H // 64, 64)
    torch.testing.assert_close(runs[0][:M, :, 0], xb.sum(dim=2), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(runs[0][:M, :, 1], (xb * xb).sum(dim=2), rtol=1e-5, atol=1e-4)
    got = _finalize(lib, runs[0], M, H)
    mean, rstd = _torch_mean_rstd(x)
    torch.testing.assert_close(got[:, 0], mean, rtol=1e-4, atol=0)
    torch.testing.assert_close(got[:, 1], rstd, rtol=1e-4, atol=0)


def _act(v, act):
    if act == 1:
        return v * torch.sigmoid(1.702 * v)
    if act == 2:
        return torch.nn.functional.gelu(v, approximate="tanh")
    return v


def _gemm_ln(lib, x, stats, folded, M, N, K, act, row_step=1):
    out = torch.full((M + 1, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty((M, 2), dtype=torch.float32, device="cuda")
    w_fold, colsum, cbias = folded
    rc = lib.cc_gemm_bf16_ln(
        x.data_ptr(), row_step, stats.data_ptr() if stats is not None else None,
        ws.data_ptr(), w_fold.data_ptr(), colsum.data_ptr(), cbias.data_ptr(),
        out.data_ptr(), M, N, K, act, ctypes.c_float(EPS), _stream())
    torch.cuda.synchronize()
    return rc, out


def _consumer_problem(M, N, K):
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
    folded = tuple(t.cuda() for t in fold_layernorm(w.float(), b, gamma, beta))
    pre = torch.nn.functional.linear(
        torch.nn.functional.layer_norm(
            x.float(), (K,), gamma.cuda(), beta.cuda(), eps=EPS),
        w.float().cuda(), b.cuda())
    stats = torch.empty((M, K // 64, 2), dtype=torch.float32, device="cuda")
    return x, stats, folded, pre


@pytest.mark.parametrize(
    ("M", "N", "K", "body"),
    [
        (300, 1536, 256, 256),    # 256² body, ragged M edge
        (100, 768, 256, 128),     # 128² body, ragged M edge
        (11008, 1536, 256, 256),  # 258 tiles: some workgroups walk two
    ],
)
def test_gemm_ln_vs_torch(lib, M, N, K, body):
    assert hotpath.gemm_plan(M, N, K, has_bias=True).body == body
    x, stats, folded, pre = _consumer_problem(M, N, K)
    hotpath.check(lib.cc_ln_stats_bf16(x.data_ptr(), M, K, stats.data_ptr(), _stream()))
    for act in (0, 1, 2):
        assert hotpath.gemm_plan(M, N, K, has_bias=True, act=act).body == body
        rc, out = _gemm_ln(lib, x, stats, folded, M, N, K, act)
        hotpath.check(rc)
        assert torch.all(out[M:] == SENTINEL), "wrote past the M output rows"
        want = _act(pre, act)
        err = (out[:M].float() - want).abs()
        print(f"gemm_ln ({M},{N},{K}) act {act}: max abs err {err.max().item():.3e}, "
              f"worst share of the budget "
              f"{(err / (2e-2 + 2e-2 * want.abs())).max().item():.3f}")
        torch.testing.assert_close(out[:M].float(), want, rtol=2e-2, atol=2e-2)
        rc, again = _gemm_ln(lib, x, stats, folded, M, N, K, act)
        hotpath.check(rc)
        assert torch.equal(out, again), "gemm_ln differs from run to run"


def test_gemm_ln_row_step_matches_gathered(lib):
    """The CLS-row form: every seq-th row of x and of its stats, in place."""
    n, seq, N, K = 5, 50, 768, 768
    torch.manual_seed(7)
    x, stats, folded, _ = _consumer_problem(n * seq, N, K)
    hotpath.check(lib.cc_ln_stats_bf16(x.data_ptr(), n * seq, K, stats.data_ptr(),
                                       _stream()))
    rc, got = _gemm_ln(lib, x, stats, folded, n, N, K, 1, row_step=seq)
    hotpath.check(rc)
    xg = x.reshape(n, seq, K)[:, 0].contiguous()
    sg = stats.reshape(n, seq, K // 64, 2)[:, 0].contiguous()
    rc, want = _gemm_ln(lib, xg, sg, folded, n, N, K, 1)
    hotpath.check(rc)
    assert torch.all(got[n:] == SENTINEL)
    assert torch.equal(got, want)


@pytest.mark.parametrize(
    ("M", "N", "K", "body"),
    [
        (300, 768, 1536, 256),    # 256² body: stats in the staged epilogue
        (300, 768, 768, 128),     # 128² body: stats kernel after the GEMM
        (22016, 768, 1536, 256),  # 258 tiles: persistent walk
    ],
)
def test_gemm_res_stats(lib, M, N, K, body):
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
    got = _finalize(lib, runs[0], M, N)
    mean, rstd = _torch_mean_rstd(ex)
    torch.testing.assert_close(got[:, 0], mean, rtol=1e-4, atol=0)
    torch.testing.assert_close(got[:, 1], rstd, rtol=1e-4, atol=0)


def test_new_entries_reject_bad_args(lib):
    M, H = 8, 256
    x = torch.zeros(M, H, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(H, H, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(H, dtype=torch.float32, device="cuda")
    stats = torch.full((M, H // 64, 2), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.full((M, 2), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((M, H), SENTINEL, dtype=torch.bfloat16, device="cuda")
    eps = ctypes.c_float(EPS)
    s = _stream()
    bad_h = 192  # a 64-multiple without LayerNorm kernels
    hotpath.timing_enable(True)
    try:
        assert lib.cc_ln_stats_bf16(x.data_ptr(), M, H, None, s) != 0
        assert lib.cc_ln_stats_bf16(x.data_ptr(), M, bad_h, stats.data_ptr(), s) != 0
        assert lib.cc_ln_finalize(None, M, H, 1, eps, ws.data_ptr(), s) != 0
        assert lib.cc_ln_finalize(stats.data_ptr(), M, bad_h, 1, eps, ws.data_ptr(), s) != 0
        assert lib.cc_ln_finalize(stats.data_ptr(), M, H, 0, eps, ws.data_ptr(), s) != 0
        res_args = lambda n, st: (  # noqa: E731
            x.data_ptr(), w.data_ptr(), out.data_ptr(), M, n, H, f.data_ptr(),
            out.data_ptr(), st, s)
        assert lib.cc_gemm_bf16_res_stats(*res_args(H, None)) != 0
        assert lib.cc_gemm_bf16_res_stats(*res_args(bad_h, stats.data_ptr())) != 0
        ln_args = lambda k, st: (  # noqa: E731
            x.data_ptr(), 1, st, ws.data_ptr(), w.data_ptr(), f.data_ptr(),
            f.data_ptr(), out.data_ptr(), M, H, k, 0, eps, s)
        assert lib.cc_gemm_bf16_ln(*ln_args(H, None)) != 0
        assert lib.cc_gemm_bf16_ln(*ln_args(bad_h, stats.data_ptr())) != 0
        assert lib.cc_last_error()
        torch.cuda.synchronize()
        for name in ("ln_stats", "ln_finalize", "gemm_bf16"):
            assert hotpath.timing_report(name)[1] == 0, name
    finally:
        hotpath.timing_enable(False)
    for t in (stats, ws, out):
        assert torch.all(t == SENTINEL), "a rejected call launched"


def _perturb_layernorms(sd, seed):
    """gamma = 1 + 0.2 randn, beta = 0.1 randn on every LayerNorm of the
    dict: the committed synthetic weights carry the identity LN, which
    would not exercise the fold."""
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if "norm" in k:
            noise = torch.randn(sd[k].shape, generator=g)
            sd[k] = (1.0 + 0.2 * noise) if k.endswith("weight") else 0.1 * noise
    return sd


def _clip_oracle(sd, cfg):
    from transformers import CLIPVisionConfig
    from transformers.models.clip.modeling_clip import CLIPVisionModelWithProjection

    ref = CLIPVisionModelWithProjection(CLIPVisionConfig(
        hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
        num_attention_heads=cfg.heads, intermediate_size=cfg.intermediate,
        patch_size=cfg.patch, projection_dim=cfg.proj, image_size=cfg.image))
    ref.load_state_dict(sd, strict=False)
    return ref.float().eval()


@pytest.mark.parametrize("model,n", [("vit_b32", 6), ("vit_l14", 2)])
def test_tower_folded_vs_oracle(lib, model, n):
    from cosmos_curate_amd.models import clip_weights as cw
    from cosmos_curate_amd.models.clip_vit import ClipVisionTowerAMD
    from oracle import vit as oracle_vit
    from oracle.color import clip_preprocess

    cfg = cw.CONFIGS[model]
    sd = _perturb_layernorms(cw.make_clip_vit_weights(cfg), n)
    rng = np.random.default_rng(n)
    pixels = clip_preprocess(
        rng.integers(0, 256, size=(n, cfg.image, cfg.image, 3), dtype=np.uint8))
    want = oracle_vit.embed_frames_fp32(_clip_oracle(sd, cfg), pixels)

    tower = ClipVisionTowerAMD(sd, cfg).cuda()
    assert tower.fold_ln and tower.prune_last_layer  # the defaults
    px = torch.from_numpy(pixels).cuda()
    hotpath.timing_enable(True)
    try:
        folded = tower(px)
        torch.cuda.synchronize()
        ln_launches = hotpath.timing_report("layernorm_bf16")[1]
        stats_launches = hotpath.timing_report("ln_stats")[1]
        finalize_launches = hotpath.timing_report("ln_finalize")[1]
    finally:
        hotpath.timing_enable(False)
    again = tower(px)
    tower.fold_ln = False
    unfolded = tower(px)
    torch.cuda.synchronize()
    # the LN kernel is left with LN2 on the CLS rows of the pruned last
    # layer and the post-LN; the Q GEMM reads the CLS rows' statistics in
    # place, so LN1 of the last layer is gone too
    kept = 2
    assert kept != 2 * cfg.layers + 1
    assert ln_launches == kept, ln_launches
    # the stats kernel: once at the encoder entry, and after each residual
    # GEMM of a full layer that the plan gives to the 128² body (at the
    # bench batch none is; at this test's M the out-proj may be)
    M = n * ((cfg.image // cfg.patch) ** 2 + 1)
    on_128 = sum(
        hotpath.gemm_plan(M, cfg.hidden, k, has_bias=True, has_residual=True).body == 128
        for k in (cfg.hidden, cfg.intermediate))
    assert stats_launches == 1 + on_128 * (cfg.layers - 1), stats_launches
    assert finalize_launches == 2 * cfg.layers, finalize_launches
    assert torch.equal(folded, again), "folded tower is not run-to-run bit-identical"

    cos_f = np.sum(want * folded.cpu().numpy(), axis=1)
    cos_u = np.sum(want * unfolded.cpu().numpy(), axis=1)
    cos_fu = torch.sum(folded * unfolded, dim=1)
    print(f"{model} per-frame cosine vs fp32 oracle, folded:   {cos_f.tolist()}")
    print(f"{model} per-frame cosine vs fp32 oracle, unfolded: {cos_u.tolist()}")
    print(f"{model} per-frame cosine folded vs unfolded: {cos_fu.tolist()}, "
          f"max abs diff {(folded - unfolded).abs().max().item():.3e}")
    assert np.all(cos_f >= 0.999), cos_f


def test_siglip_tiny_folded_vs_oracle(lib):
    """hidden 256, head dim 64, gelu_tanh, eps 1e-6 through the folded route."""
    from cosmos_curate_amd.models import clip_weights as cw
    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD
    from oracle.vit import build_reference_siglip_vision, siglip_embed_frames_fp32

    image = 64
    cfg = cw.VitConfig("siglip_tiny256", hidden=256, layers=2, heads=4,
                       intermediate=512, patch=16, proj=256, image=image,
                       has_cls=False, act="gelu_tanh", ln_eps=1e-6)
    sd = _perturb_layernorms(cw.make_siglip_weights(cfg), 3)
    ref = build_reference_siglip_vision(
        sd, dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                 num_attention_heads=4, image_size=image, patch_size=16))
    torch.manual_seed(image)
    pix = torch.rand(3, 3, image, image) * 2 - 1
    want = siglip_embed_frames_fp32(ref, pix)
    tower = SiglipVisionTowerAMD(sd, cfg).cuda()
    assert tower.fold_ln
    px = pix.cuda().to(torch.bfloat16)
    hotpath.timing_enable(True)
    try:
        got = tower(px).cpu().numpy()
        torch.cuda.synchronize()
        ln_launches = hotpath.timing_report("layernorm_bf16")[1]
    finally:
        hotpath.timing_enable(False)
    assert ln_launches == 1, ln_launches  # the post-LN only
    tower.fold_ln = False
    unfolded = tower(px).cpu().numpy()
    cos = (got * want).sum(axis=1)
    print("siglip tiny per-frame cosine vs fp32 oracle, folded:  ", cos.tolist())
    print("siglip tiny per-frame cosine vs fp32 oracle, unfolded:",
          (unfolded * want).sum(axis=1).tolist())
    assert np.all(cos >= 0.999), cos
