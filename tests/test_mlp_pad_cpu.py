"""The MLP width padded once at construction (no GPU).

cc_gemm needs K % 64 == 0 and SigLIP-so400m's MLP is 4304 wide, so
VitEncoderAMD pads fc1 / fc2 (and the folded fc1) to the next multiple of 64
with zeros.  Pinned here at hidden 128, intermediate 200 -> 256: the pads
are exactly zero, the rest is the unpadded construction, and a layer
computes what the unpadded tensors compute.
"""

import pytest
import torch

from cosmos_curate_amd.models import clip_weights as cw
from cosmos_curate_amd.models.vit_encoder import VitEncoderAMD, fold_layernorm

HIDDEN, INTER, PADDED, HEADS = 128, 200, 256, 2
Q = "encoder.layers.0."


@pytest.fixture(scope="module")
def sd():
    cfg = _cfg()
    sd = cw.make_siglip_weights(cfg)
    g = torch.Generator().manual_seed(11)
    for k in sd:  # the synthetic LayerNorms are the identity: perturb them
        if "layer_norm" in k:
            noise = torch.randn(sd[k].shape, generator=g)
            sd[k] = (1.0 + 0.2 * noise) if k.endswith("weight") else 0.1 * noise
    return sd


def _cfg():
    return cw.VitConfig("pad_tiny", hidden=HIDDEN, layers=1, heads=HEADS,
                        intermediate=INTER, patch=16, proj=HIDDEN, image=32,
                        has_cls=False, act="gelu_tanh", ln_eps=1e-6)


def _torch_linear(self, x, w, b, act=0, residual=None):
    y = torch.nn.functional.linear(x.float(), w.float(), b.float() if b is not None else None)
    if act == 1:
        y = y * torch.sigmoid(1.702 * y)
    if act == 2:
        y = torch.nn.functional.gelu(y, approximate="tanh")
    if residual is not None:
        y = y + residual.float()
    return y.to(torch.bfloat16)


def test_mlp_buffers_padded_with_zeros(sd):
    enc = VitEncoderAMD(sd, _cfg(), "")
    assert enc.intermediate == PADDED
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    w1, b1, w2 = sd[Q + "mlp.fc1.weight"], sd[Q + "mlp.fc1.bias"], sd[Q + "mlp.fc2.weight"]
    wf, s, c = fold_layernorm(w1, b1.float(), sd[Q + "layer_norm2.weight"].float(),
                              sd[Q + "layer_norm2.bias"].float())
    # (buffer, its unpadded construction, the padded axis)
    for name, want, axis in (
        ("w_fc1_0", bf(w1), 0), ("b_fc1_0", b1.float(), 0), ("w_fc2_0", bf(w2), 1),
        ("wf_fc1_0", wf, 0), ("s_fc1_0", s, 0), ("c_fc1_0", c, 0),
    ):
        got = getattr(enc, name)
        assert got.shape[axis] == PADDED and got.is_contiguous(), name
        assert got.dtype == want.dtype, name
        live, pad = got.split([INTER, PADDED - INTER], dim=axis)
        assert torch.equal(live, want), name
        assert torch.count_nonzero(pad) == 0, name
    # nothing else changed shape
    assert enc.b_fc2_0.shape == (HIDDEN,)
    assert enc.w_qkv_0.shape == (3 * HIDDEN, HIDDEN)


def test_multiple_of_64_is_not_padded():
    cfg = cw.VitConfig("nopad_tiny", hidden=HIDDEN, layers=1, heads=HEADS,
                       intermediate=256, patch=16, proj=HIDDEN, image=32,
                       has_cls=False, act="gelu_tanh", ln_eps=1e-6)
    sd = cw.make_siglip_weights(cfg)
    enc = VitEncoderAMD(sd, cfg, "")
    assert enc.intermediate == 256
    assert torch.equal(enc.w_fc1_0, sd[Q + "mlp.fc1.weight"].to(torch.bfloat16))
    assert torch.equal(enc.w_fc2_0, sd[Q + "mlp.fc2.weight"].to(torch.bfloat16))


def test_padded_layer_equals_unpadded_by_hand(sd, monkeypatch):
    monkeypatch.setattr(VitEncoderAMD, "_linear", _torch_linear)
    cfg = _cfg()
    enc = VitEncoderAMD(sd, cfg, "")
    n, seq = 2, 5
    torch.manual_seed(3)
    h = torch.randn(n, seq, HIDDEN).to(torch.bfloat16)
    got = enc._layer(h, 0, n, seq)

    # the same layer from the unpadded checkpoint tensors
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    F = torch.nn.functional
    ln = lambda x, k: F.layer_norm(  # noqa: E731
        x.float(), (HIDDEN,), sd[Q + k + ".weight"].float(),
        sd[Q + k + ".bias"].float(), eps=cfg.ln_eps).to(torch.bfloat16)
    lin = lambda x, k, **kw: _torch_linear(  # noqa: E731
        None, x, bf(sd[Q + k + ".weight"]), sd[Q + k + ".bias"].float(), **kw)
    hd = HIDDEN // HEADS
    x = h.reshape(n * seq, HIDDEN)
    y = ln(x, "layer_norm1")
    q, k, v = (
        lin(y, f"self_attn.{p}_proj").reshape(n, seq, HEADS, hd).permute(0, 2, 1, 3)
        for p in "qkv")
    attn = F.scaled_dot_product_attention(q, k, v, scale=hd ** -0.5)
    attn = attn.permute(0, 2, 1, 3).reshape(n * seq, HIDDEN)
    x = lin(attn, "self_attn.out_proj", residual=x)
    y = lin(ln(x, "layer_norm2"), "mlp.fc1", act=2)
    assert y.shape == (n * seq, INTER)
    want = lin(y, "mlp.fc2", residual=x).reshape(n, seq, HIDDEN)
    torch.testing.assert_close(got, want)
