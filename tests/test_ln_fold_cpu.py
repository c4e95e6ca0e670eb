"""LayerNorm folded into the linear layer it feeds (vit_encoder.fold_layernorm),
on the CPU: the arithmetic the folded GEMM route performs, emulated in
torch, against float64 linear(layer_norm(x)).

The emulation takes the rounding points of the GPU route:
bf16 x, W' rounded to bf16, f32 accumulation, row statistics in f32 from
the bf16 x in the var = sum(x^2)/H - mean^2 form, and a bf16 result.  The
committed synthetic weights carry gamma = 1, beta = 0, which would not
exercise the fold, so gamma and beta are perturbed here.
"""

import pytest
import torch

from cosmos_curate_amd.models import clip_weights as cw
from cosmos_curate_amd.models.vit_encoder import VitEncoderAMD, fold_layernorm

EPS = 1e-5
TOL = 2e-2  # rtol = atol on the bf16 result (tests/test_gpu_vit.py's LN bound)


def _inputs(family: str, M: int, K: int) -> torch.Tensor:
    x = torch.randn(M, K)
    if family == "row_means":  # row means up to 16 sigma either way
        x = x + torch.linspace(-16.0, 16.0, M)[:, None]
    elif family == "massive_channels":  # two outlier channels, every row
        x[:, 3] = 60.0
        x[:, K // 2 + 1] = 60.0
    return x.to(torch.bfloat16)


def _folded_forward(x_bf16, w_fold, colsum, cbias):
    """What cc_gemm_bf16_ln computes, in torch f32."""
    xf = x_bf16.float()
    H = xf.shape[1]
    acc = xf @ w_fold.float().T
    mean = xf.sum(dim=1) / H
    var = (xf * xf).sum(dim=1) / H - mean * mean
    rstd = torch.rsqrt(var + EPS)
    return (rstd[:, None] * (acc - mean[:, None] * colsum) + cbias).to(torch.bfloat16)


@pytest.mark.parametrize("family", ["plain", "row_means", "massive_channels"])
@pytest.mark.parametrize(("K", "N"), [(768, 768), (256, 512)])
def test_fold_matches_float64_layernorm_linear(family, K, N):
    M = 300
    torch.manual_seed(K + N + len(family))
    x = _inputs(family, M, K)
    w = torch.randn(N, K) / K**0.5
    b = 0.1 * torch.randn(N)
    gamma = 1.0 + 0.2 * torch.randn(K)
    beta = 0.1 * torch.randn(K)

    w_fold, colsum, cbias = fold_layernorm(w, b, gamma, beta)
    assert w_fold.dtype == torch.bfloat16 and w_fold.shape == (N, K)
    assert colsum.dtype == cbias.dtype == torch.float32
    # s is the sum of the ROUNDED W' (what the MFMA multiplies)
    torch.testing.assert_close(
        colsum, w_fold.double().sum(dim=1).float(), rtol=0, atol=0)

    got = _folded_forward(x, w_fold, colsum, cbias).double()
    want = torch.nn.functional.linear(
        torch.nn.functional.layer_norm(
            x.double(), (K,), gamma.double(), beta.double(), eps=EPS),
        w.double(), b.double())
    err = (got - want).abs()
    worst = (err / (TOL + TOL * want.abs())).max().item()
    print(f"{family} K={K} N={N}: max abs err {err.max().item():.3e}, "
          f"worst share of the budget {worst:.3f}")
    torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)


def test_identity_layernorm_folds_to_the_plain_weight():
    """gamma = 1, beta = 0: W' is the bf16 weight and c the bias."""
    torch.manual_seed(0)
    w, b = torch.randn(64, 128), torch.randn(64)
    w_fold, colsum, cbias = fold_layernorm(w, b, torch.ones(128), torch.zeros(128))
    assert torch.equal(w_fold, w.to(torch.bfloat16))
    assert torch.equal(cbias, b)


def test_encoder_registers_folded_buffers_with_qkv_row_order():
    cfg = cw.VitConfig("tiny", hidden=128, layers=2, heads=2, intermediate=256,
                       patch=16, proj=128, image=32, has_cls=False,
                       act="gelu_tanh", ln_eps=1e-6)
    sd = cw.make_siglip_weights(cfg)
    torch.manual_seed(1)
    for k in sd:
        if "layer_norm1" in k or "layer_norm2" in k:
            sd[k] = sd[k] + 0.1 * torch.randn_like(sd[k])
    enc = VitEncoderAMD(sd, cfg, "")
    H = cfg.hidden
    for i in range(cfg.layers):
        q = f"encoder.layers.{i}."
        for j, name in enumerate("qkv"):
            want = fold_layernorm(
                sd[q + f"self_attn.{name}_proj.weight"],
                sd[q + f"self_attn.{name}_proj.bias"],
                sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"])
            rows = slice(j * H, (j + 1) * H)
            for pre, t in zip(("wf", "s", "c"), want):
                got = getattr(enc, f"{pre}_qkv_{i}")[rows]
                assert got.is_contiguous()
                if pre == "wf":
                    assert torch.equal(got, t), (i, name)
                else:  # f64 reductions may block differently per call
                    torch.testing.assert_close(got, t, rtol=1e-6, atol=1e-7)
        want = fold_layernorm(
            sd[q + "mlp.fc1.weight"], sd[q + "mlp.fc1.bias"],
            sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"])
        for pre, t in zip(("wf", "s", "c"), want):
            torch.testing.assert_close(
                getattr(enc, f"{pre}_fc1_{i}"), t, rtol=1e-6, atol=1e-7)
    # derived buffers stay out of the checkpoint; the plain ones remain
    assert not any(k.startswith(("wf_", "s_", "c_")) for k in enc.state_dict())
    assert "w_qkv_0" in enc.state_dict() and "ln1_w_0" in enc.state_dict()
    assert VitEncoderAMD.fold_ln
