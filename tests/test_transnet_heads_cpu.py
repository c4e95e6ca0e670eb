"""Native TransNetV2 heads: everything that needs no GPU.

Weight packing, the CPU restatement of the head kernels
(tests/transnet_heads_ref.py) against ``_TransNetV2.heads``, the band against
the gathered T x T matrix, the library's host-side argument checks, and the
option's way from the command line to the model.  The kernels themselves are
pinned in test_gpu_transnet_heads.py.
"""

from __future__ import annotations

import argparse

import numpy as np
import pytest
import torch

import transnet_bf16_ref as trunk_ref
import transnet_heads_ref as ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models.transnetv2 import (
    TransNetV2,
    _TransNetV2,
    _window_gather,
    make_transnetv2_weights,
)
from cosmos_curate_amd.models.transnetv2_native import pack_heads
from cosmos_curate_amd.pipelines.video.clipping.transnetv2_extraction_stages import (
    TransNetV2ClipExtractionStage,
)

CC_ERR_INVALID, CC_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def net():
    n = _TransNetV2()
    n.load_state_dict(make_transnetv2_weights(), strict=True)
    return n.eval()


@pytest.fixture(scope="module")
def packed(net):
    return pack_heads(net.state_dict())


# ---- 1. weight packing -------------------------------------------------------

def test_pack_heads_shapes_and_split(net, packed):
    sd = net.state_dict()
    assert packed.proj_wt.shape == (448, 128) and packed.proj_b.shape == (128,)
    assert packed.sim_fc_wt.shape == packed.hist_fc_wt.shape == (101, 128)
    assert packed.sim_fc_b.shape == packed.hist_fc_b.shape == (128,)
    assert packed.fc1_hi.shape == packed.fc1_lo.shape == (1024, 256 + 4608)
    assert packed.fc1_hi.dtype == packed.fc1_lo.dtype == torch.bfloat16
    assert packed.fc1_b.shape == packed.cls_w.shape == (1024,)
    assert all(t.is_contiguous() for t in (packed.proj_wt, packed.sim_fc_wt,
                                           packed.hist_fc_wt, packed.fc1_hi, packed.fc1_lo))
    torch.testing.assert_close(packed.proj_wt, sd["frame_sim_layer.projection.weight"].T,
                               rtol=0, atol=0)
    torch.testing.assert_close(packed.sim_fc_wt, sd["frame_sim_layer.fc.weight"].T,
                               rtol=0, atol=0)
    torch.testing.assert_close(packed.hist_fc_wt, sd["color_hist_layer.fc.weight"].T,
                               rtol=0, atol=0)
    torch.testing.assert_close(packed.cls_w, sd["cls_layer1.weight"][0], rtol=0, atol=0)
    assert packed.cls_b == float(sd["cls_layer1.bias"][0])

    w = sd["fc1.weight"].double()
    back = packed.fc1_hi.double() + packed.fc1_lo.double()
    excess = (back - w).abs() - 2.0 ** -16 * w.abs()
    print(f"fc1 hi+lo: worst |hi+lo-w|/|w| {float(((back - w).abs() / w.abs()).max()):.3e}")
    assert float(excess.max()) <= 0
    # one bf16 alone would not do
    assert float(((packed.fc1_hi.double() - w).abs() - 2.0 ** -16 * w.abs()).max()) > 0


def test_pack_heads_rejects_bad_state_dicts(net):
    with pytest.raises(ValueError, match="no heads"):
        pack_heads({k: v for k, v in net.state_dict().items() if k.startswith("SDDCNN.")})
    sd = dict(net.state_dict())
    sd["color_hist_layer.fc.weight"] = torch.zeros(128, 51)
    with pytest.raises(ValueError, match="color_hist_layer.fc.weight"):
        pack_heads(sd)
    sd = dict(net.state_dict())
    sd["fc1.weight"] = torch.zeros(1024, 256 + 4600)
    with pytest.raises(ValueError, match="fc1.weight"):
        pack_heads(sd)


# ---- 2. the restatement against the module -------------------------------------

def _inputs(golden_dir):
    golden = torch.from_numpy(np.load(golden_dir / "transnetv2_golden.npz")["input"])
    gen = torch.Generator().manual_seed(11)
    rand = torch.randint(0, 256, (2, 30, 27, 48, 3), generator=gen, dtype=torch.uint8)
    return {"golden": golden, "random B=2 T=30": rand}


@pytest.mark.parametrize("which", ["golden", "random B=2 T=30"])
def test_restatement_matches_the_module_heads(net, packed, golden_dir, which):
    """Reference against reference: measured 4.8e-7 (golden) and 4.2e-7
    (random) when the split was chosen; ten times that covers torch's own
    summation order."""
    frames = _inputs(golden_dir)[which]
    feats = [trunk_ref.rb(f) for f in trunk_ref.trunk_f32(net, frames)]  # (B,C,T,h,w)
    want = net.heads(frames, feats)
    got = ref.heads(packed, frames, [f.permute(0, 2, 3, 4, 1).contiguous() for f in feats])
    assert got.shape == want.shape == (*frames.shape[:2], 1)
    err = float((got - want).abs().max())
    print(f"{which}: max |restatement - module heads| {err:.3e}")
    assert err <= 5e-6


@pytest.mark.parametrize("t", [1, 51, 100, 130])
def test_band_equals_the_gathered_matrix(t):
    """Small integers in f64: both sides are exact, so they are equal."""
    gen = torch.Generator().manual_seed(t)
    x = torch.randint(-4, 5, (2, t, 16), generator=gen).double()
    want = _window_gather(torch.bmm(x, x.transpose(1, 2)), 101)
    got = ref.band(x)
    assert got.shape == (2, t, 101)
    np.testing.assert_array_equal(got.numpy(), want.numpy())
    assert float(got.abs().max()) > 0


def test_hist_restatement_matches_the_module():
    gen = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (1, 5, 27, 48, 3), generator=gen, dtype=torch.uint8)
    from cosmos_curate_amd.models.transnetv2 import ColorHistograms

    want = ColorHistograms._histograms(frames)[0].numpy()
    got = ref.hist512(frames.reshape(5, -1, 3).numpy())
    np.testing.assert_allclose(got, want, rtol=4 * 2.0 ** -24, atol=0)


# ---- 3. host validation, no device ---------------------------------------------

P = 0x10000  # an aligned address nothing dereferences: every call below is rejected first


def _rejected(call, *args, code: int, word: str) -> None:
    with pytest.raises(RuntimeError, match=f"cc error {code}: {word}"):
        call(*args)


def _hist(frames=P, out=P, n=5, pixels=1296):
    return (frames, out, n, pixels, 0)


def _embed(x0=P, x1=P, x2=P, wt=P, b=P, out=P, n=3, out_dim=128, c2=256, maps=3):
    return ([(x0, 312, 64), (x1, 72, 128), (x2, 18, c2)][:maps], wt, b, out, n, out_dim, 0)


def _simband(x=P, wt=P, b=P, out=P, nb=2, t=100, d=512, ldo=256, col=0):
    return (x, wt, b, out, nb, t, d, ldo, col, 0)


def _fc1(hd=P, feat=P, hi=P, lo=P, bias=P, y=P, m=100, kh=256, kf=4608, n=1024):
    return (hd, feat, hi, lo, bias, y, m, kh, kf, n, 0)


def _cls(y=P, w=P, b=0.5, p=P, m=70, n=1024):
    return (y, w, b, p, m, n, 0)


def test_null_pointers_are_invalid():
    for kw in ("frames", "out"):
        _rejected(hotpath.tn_hist512_u8, *_hist(**{kw: 0}), code=CC_ERR_INVALID, word="tn_hist512")
    for kw in ("x0", "x1", "x2", "wt", "b", "out"):
        _rejected(hotpath.tn_framesim_embed, *_embed(**{kw: 0}), code=CC_ERR_INVALID,
                  word="tn_framesim_embed")
    for kw in ("x", "wt", "b", "out"):
        _rejected(hotpath.tn_simband_fc, *_simband(**{kw: 0}), code=CC_ERR_INVALID,
                  word="tn_simband_fc")
    for kw in ("hd", "feat", "hi", "lo", "bias", "y"):
        _rejected(hotpath.tn_fc1_relu, *_fc1(**{kw: 0}), code=CC_ERR_INVALID, word="tn_fc1_relu")
    for kw in ("y", "w", "p"):
        _rejected(hotpath.tn_cls_sigmoid, *_cls(**{kw: 0}), code=CC_ERR_INVALID,
                  word="tn_cls_sigmoid")


def test_misaligned_pointers_are_invalid():
    _rejected(hotpath.tn_hist512_u8, *_hist(out=P + 4), code=CC_ERR_INVALID, word="tn_hist512")
    for kw in ("x0", "x1", "x2", "wt", "b", "out"):
        _rejected(hotpath.tn_framesim_embed, *_embed(**{kw: P + 8}), code=CC_ERR_INVALID,
                  word="tn_framesim_embed")
    for kw in ("x", "wt", "b", "out"):
        _rejected(hotpath.tn_simband_fc, *_simband(**{kw: P + 8}), code=CC_ERR_INVALID,
                  word="tn_simband_fc")
    for kw in ("hd", "feat", "hi", "lo", "bias", "y"):
        _rejected(hotpath.tn_fc1_relu, *_fc1(**{kw: P + 8}), code=CC_ERR_INVALID,
                  word="tn_fc1_relu")
    for kw, off in (("y", 8), ("w", 8), ("p", 2)):
        _rejected(hotpath.tn_cls_sigmoid, *_cls(**{kw: P + off}), code=CC_ERR_INVALID,
                  word="tn_cls_sigmoid")


def test_non_positive_sizes_are_invalid():
    _rejected(hotpath.tn_hist512_u8, *_hist(n=0), code=CC_ERR_INVALID, word="tn_hist512")
    _rejected(hotpath.tn_hist512_u8, *_hist(pixels=0), code=CC_ERR_INVALID, word="tn_hist512")
    _rejected(hotpath.tn_framesim_embed, *_embed(n=0), code=CC_ERR_INVALID,
              word="tn_framesim_embed")
    _rejected(hotpath.tn_framesim_embed, *_embed(c2=0), code=CC_ERR_INVALID,
              word="tn_framesim_embed")
    for kw in ({"t": 0}, {"t": -3}, {"nb": 0}, {"ldo": 200, "col": 128}, {"col": -1}):
        _rejected(hotpath.tn_simband_fc, *_simband(**kw), code=CC_ERR_INVALID,
                  word="tn_simband_fc")
    for kw in ({"m": 0}, {"kh": 0}, {"kf": -32}, {"n": 0}):
        _rejected(hotpath.tn_fc1_relu, *_fc1(**kw), code=CC_ERR_INVALID, word="tn_fc1_relu")
    for kw in ({"m": 0}, {"n": 0}):
        _rejected(hotpath.tn_cls_sigmoid, *_cls(**kw), code=CC_ERR_INVALID,
                  word="tn_cls_sigmoid")


def test_sizes_outside_the_stated_set_are_unsupported():
    _rejected(hotpath.tn_hist512_u8, *_hist(pixels=4097), code=CC_ERR_UNSUPPORTED,
              word="tn_hist512")
    _rejected(hotpath.tn_framesim_embed, *_embed(c2=384), code=CC_ERR_UNSUPPORTED,
              word="tn_framesim_embed")  # 64 + 128 + 384 > 512
    _rejected(hotpath.tn_framesim_embed, *_embed(c2=260), code=CC_ERR_UNSUPPORTED,
              word="tn_framesim_embed")  # no multiple of 8
    _rejected(hotpath.tn_framesim_embed, *_embed(out_dim=64), code=CC_ERR_UNSUPPORTED,
              word="tn_framesim_embed")
    _rejected(hotpath.tn_framesim_embed, *_embed(maps=0), code=CC_ERR_UNSUPPORTED,
              word="tn_framesim_embed")
    for d in (96, 256, 0):
        _rejected(hotpath.tn_simband_fc, *_simband(d=d), code=CC_ERR_UNSUPPORTED,
                  word="tn_simband_fc")
    for kw in ({"kh": 48}, {"kf": 4600}, {"n": 24}):
        _rejected(hotpath.tn_fc1_relu, *_fc1(**kw), code=CC_ERR_UNSUPPORTED, word="tn_fc1_relu")


# ---- 4. the option, from the command line to the model --------------------------

def test_heads_option_defaults_and_pairing():
    assert TransNetV2().heads == "torch"
    assert TransNetV2(backend="native").heads == "torch"
    assert TransNetV2(backend="native", heads="native").heads == "native"
    with pytest.raises(ValueError, match="backend='native'"):
        TransNetV2(backend="torch", heads="native")
    with pytest.raises(ValueError):
        TransNetV2(backend="native", heads="hip")
    assert TransNetV2ClipExtractionStage().heads == "torch"
    stage = TransNetV2ClipExtractionStage(backend="native", heads="native")
    assert (stage.model.backend, stage.model.heads) == ("native", "native")
    with pytest.raises(ValueError):
        TransNetV2ClipExtractionStage(heads="native")


def _split_args(tmp_path, *extra):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _setup_parser

    (tmp_path / "in").mkdir(exist_ok=True)
    p = argparse.ArgumentParser()
    _setup_parser(p)
    return p.parse_args(["--input-video-path", str(tmp_path / "in"),
                         "--output-clip-path", str(tmp_path / "out"),
                         "--splitting-algorithm", "transnetv2", *extra])


def _transnet_stage(stages):
    inner = [st.stage if hasattr(st, "stage") else st for st in stages]
    (stage,) = [s for s in inner if isinstance(s, TransNetV2ClipExtractionStage)]
    return stage


def test_cli_hands_the_setting_to_the_stage(tmp_path):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _assemble_stages

    assert _split_args(tmp_path).transnetv2_heads == "torch"
    for extra, want in (((), ("torch", "torch")),
                        (("--transnetv2-backend", "native"), ("native", "torch")),
                        (("--transnetv2-backend", "native", "--transnetv2-heads", "native"),
                         ("native", "native"))):
        stage = _transnet_stage(_assemble_stages(_split_args(tmp_path, *extra)))
        assert (stage.backend, stage.heads) == want
        assert (stage.model.backend, stage.model.heads) == want
    with pytest.raises(SystemExit):
        _split_args(tmp_path, "--transnetv2-heads", "hip")


def test_cli_rejects_native_heads_on_the_torch_backend(tmp_path):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _assemble_stages, split

    for extra in (("--transnetv2-heads", "native"),
                  ("--transnetv2-heads", "native", "--transnetv2-backend", "torch")):
        with pytest.raises(ValueError, match="--transnetv2-backend native"):
            _assemble_stages(_split_args(tmp_path, *extra))
        with pytest.raises(ValueError, match="--transnetv2-backend native"):
            split(_split_args(tmp_path, "--dry-run", *extra))


def test_cli_dry_run_shows_the_option(tmp_path, capsys):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import split

    split(_split_args(tmp_path, "--dry-run", "--transnetv2-backend", "native"))
    quiet = capsys.readouterr().out.splitlines()
    assert "TransNetV2ClipExtractionStage" in quiet
    assert not any("heads" in line for line in quiet)
    split(_split_args(tmp_path, "--dry-run", "--transnetv2-backend", "native",
                      "--transnetv2-heads", "native"))
    shown = capsys.readouterr().out.splitlines()
    assert "TransNetV2ClipExtractionStage heads=native" in shown
    assert len(shown) == len(quiet)
    assert sum("heads" in line for line in shown) == 1
