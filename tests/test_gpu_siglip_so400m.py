"""SigLIP-so400m-shaped towers on the GPU: head dim 72, LayerNorm at 1152,
the MLP width 4304 padded to 4352 — against transformers fp32.

Two layers instead of 27 and small images keep it to seconds; every width
the real tower has is the real one.  Images of 56, 126 and 266 pixels give
16, 81 and 361 tokens at patch 14.  At head dim 72 the plan as built sends
16 to the small rung and both 81 and 361 to flash (below head dim 96 no
length runs the mid rung, csrc/cc_attn_plan.hpp; tests/test_gpu_attn_hd.py
covers that rung at head dim 72).
The full-depth config is covered without constructing it: every GEMM shape
and the attention shape of siglip_so400m_14_224 pass the launch plans.
"""

import numpy as np
import pytest
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models import clip_weights as cw

LAYERS, N = 2, 2
SO400M = cw.CONFIGS["siglip_so400m_14_224"]


def _tiny_cfg(image):
    return cw.VitConfig(
        f"so400m_tiny_{image}", hidden=SO400M.hidden, layers=LAYERS,
        heads=SO400M.heads, intermediate=SO400M.intermediate, patch=SO400M.patch,
        proj=SO400M.proj, image=image, has_cls=False, act=SO400M.act,
        ln_eps=SO400M.ln_eps)


def _perturb_layernorms(sd, seed):
    """gamma = 1 + 0.2 randn, beta = 0.1 randn on every LayerNorm: the
    synthetic weights carry the identity LN, which would not exercise the
    fold."""
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if "norm" in k:
            noise = torch.randn(sd[k].shape, generator=g)
            sd[k] = (1.0 + 0.2 * noise) if k.endswith("weight") else 0.1 * noise
    return sd


@pytest.mark.gpu
@pytest.mark.parametrize(("image", "rung"), [(56, "small"), (126, "flash"), (266, "flash")])
def test_so400m_tiny_gpu_vs_oracle_cosine(image, rung):
    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD
    from oracle.vit import build_reference_siglip_vision, siglip_embed_frames_fp32

    hotpath.require_gpu()
    cfg = _tiny_cfg(image)
    seq = (image // cfg.patch) ** 2
    assert hotpath.ATTN_RUNGS[
        hotpath.attn_plan(N, seq, cfg.heads, cfg.hidden).rung] == rung
    sd = _perturb_layernorms(cw.make_siglip_weights(cfg), image)
    ref = build_reference_siglip_vision(
        sd, dict(hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                 num_hidden_layers=LAYERS, num_attention_heads=cfg.heads,
                 image_size=image, patch_size=cfg.patch))
    torch.manual_seed(image)
    pix = torch.rand(N, 3, image, image) * 2 - 1  # SigLIP-normalized range
    want = siglip_embed_frames_fp32(ref, pix)

    tower = SiglipVisionTowerAMD(sd, cfg).cuda()
    assert tower.fold_ln and not tower.force_sdpa  # the defaults
    assert tower.intermediate == 4352
    px = pix.cuda().to(torch.bfloat16)
    hotpath.timing_enable(True)
    try:
        native = tower(px)
        torch.cuda.synchronize()
        attn = {r: hotpath.timing_report(f"attn_{r}")[1] for r in hotpath.ATTN_RUNGS}
        finalize = hotpath.timing_report("ln_finalize")[1]
        ln = hotpath.timing_report("layernorm_bf16")[1]
    finally:
        hotpath.timing_enable(False)
    # native attention on the rung the plan names, LN1/LN2 folded away
    assert attn == {r: LAYERS if r == rung else 0 for r in hotpath.ATTN_RUNGS}, attn
    assert finalize == 2 * LAYERS, finalize
    assert ln == 1, ln  # the post-LN only

    tower.force_sdpa = True
    hotpath.timing_enable(True)
    try:
        sdpa = tower(px)
        torch.cuda.synchronize()
        attn_forced = sum(hotpath.timing_report(f"attn_{r}")[1] for r in hotpath.ATTN_RUNGS)
    finally:
        hotpath.timing_enable(False)
    assert attn_forced == 0, "force_sdpa still launched cc_attn"

    assert native.shape == (N, cfg.proj)
    cos = (native.cpu().numpy() * want).sum(axis=1)
    cos_sdpa = (sdpa.cpu().numpy() * want).sum(axis=1)
    agree = torch.sum(native * sdpa, dim=1)
    print(f"so400m tiny {image}px per-frame cosine vs fp32 oracle, native: {cos.tolist()}")
    print(f"so400m tiny {image}px per-frame cosine vs fp32 oracle, sdpa:   {cos_sdpa.tolist()}")
    print(f"so400m tiny {image}px native vs sdpa: {agree.tolist()}")
    assert np.all(cos >= 0.999), cos
    assert torch.all(agree >= 0.9999), agree


def test_so400m_full_config_shapes_pass_the_plans():
    """siglip_so400m_14_224 at one frame: every GEMM the tower issues and its
    attention call are launchable (host-only plans; nothing is built)."""
    from cosmos_curate_amd import build as cc_build

    cc_build.build(verbose=False)
    cfg = SO400M
    seq = (cfg.image // cfg.patch) ** 2
    assert seq == 256 and cfg.hidden // cfg.heads == 72
    H = cfg.hidden
    inter = (cfg.intermediate + 63) // 64 * 64
    patch_k = (3 * cfg.patch * cfg.patch + 63) // 64 * 64
    assert (inter, patch_k) == (4352, 640)
    M = seq
    # (M, N, K, bias, act, residual)
    gemms = {
        "patch": (M, H, patch_k, True, 0, False),
        "qkv (LN folded)": (M, 3 * H, H, True, 0, False),
        "out-proj": (M, H, H, True, 0, True),
        "fc1 (LN folded)": (M, inter, H, True, 2, False),
        "fc2": (M, H, inter, True, 0, True),
    }
    for name, (m, n, k, bias, act, res) in gemms.items():
        p = hotpath.gemm_plan(m, n, k, has_bias=bias, act=act, has_residual=res)
        assert p.body in (128, 256) and p.grid > 0, name
    # fc2 takes the 256-tile body at the padded width; the raw width is
    # what the GEMM refuses
    assert hotpath.gemm_plan(M, H, inter, has_bias=True, has_residual=True).body == 256
    with pytest.raises(RuntimeError):
        hotpath.gemm_plan(M, H, cfg.intermediate, has_bias=True, has_residual=True)
    p = hotpath.attn_plan(1, seq, cfg.heads, H)
    assert (hotpath.ATTN_RUNGS[p.rung], p.grid) == ("flash", 4 * cfg.heads)
