"""The towers' pooling heads on cc_attn_pool (``native_pool = True``) against
their torch f32 heads (per-frame cosine >= 0.9999, the bar for native against
force_sdpa) and against the fp32 oracles of test_gpu_siglip_so400m.py and
test_gpu_iv2_tower.py (>= 0.999), on two-layer stand-in towers.
"""

import dataclasses

import numpy as np
import pytest
import torch

import iv2_ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models import clip_weights as cw
from cosmos_curate_amd.models import internvideo2_weights as iw
from test_gpu_siglip_so400m import _perturb_layernorms

pytestmark = pytest.mark.gpu

N = 2


def _siglip_cfg(base, image):
    b = cw.CONFIGS[base]
    return cw.VitConfig(
        f"{base}_tiny_{image}", hidden=b.hidden, layers=2, heads=b.heads,
        intermediate=b.intermediate, patch=b.patch, proj=b.proj, image=image,
        has_cls=False, act=b.act, ln_eps=b.ln_eps)


def _both_heads(tower, px):
    """(torch head, native head, attn_pool launches of each) for one input."""
    outs, launches = [], []
    for flag in (False, True):
        tower.native_pool = flag
        hotpath.timing_enable(True)
        try:
            outs.append(tower(px).cpu())
            torch.cuda.synchronize()
            launches.append(hotpath.timing_report("attn_pool")[1])
        finally:
            hotpath.timing_enable(False)
    assert launches[0] == 0 and launches[1] > 0, launches
    return outs


def _check(label, torch_head, native, want):
    cos = lambda a, b: torch.nn.functional.cosine_similarity(  # noqa: E731
        a.double(), b.double(), dim=-1)
    agree, vs_oracle = cos(native, torch_head), cos(native, want)
    print(f"{label}: native vs torch head {agree.tolist()}, native vs fp32 oracle "
          f"{vs_oracle.tolist()}, torch head vs oracle {cos(torch_head, want).tolist()}")
    assert agree.min() >= 0.9999, agree
    assert vs_oracle.min() >= 0.999, vs_oracle


# so400m widths at 16 and 256 tokens, L16-256 widths at 16 tokens
@pytest.mark.parametrize(("base", "image"), [
    ("siglip_so400m_14_224", 56), ("siglip_so400m_14_224", 224), ("siglip_l16_256", 64)])
def test_siglip_map_head_native(base, image):
    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD
    from oracle.vit import build_reference_siglip_vision, siglip_embed_frames_fp32

    cfg = _siglip_cfg(base, image)
    sd = _perturb_layernorms(cw.make_siglip_weights(cfg), image)
    ref = build_reference_siglip_vision(
        sd, dict(hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                 num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                 image_size=image, patch_size=cfg.patch))
    torch.manual_seed(image)
    pix = torch.rand(N, 3, image, image) * 2 - 1
    want = torch.from_numpy(np.asarray(siglip_embed_frames_fp32(ref, pix)))
    tower = SiglipVisionTowerAMD(sd, cfg).cuda()
    assert not tower.native_pool  # the default
    torch_head, native = _both_heads(tower, pix.cuda().to(torch.bfloat16))
    _check(f"{base} {image}px", torch_head, native, want)


@pytest.mark.parametrize("fold_ln", [True, False])
def test_internvideo2_pool_native(fold_ln):
    from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD

    cfg = dataclasses.replace(iw.INTERNVIDEO2_1B, layers=2, num_frames=2, image=56)
    sd = iw.make_internvideo2_weights(cfg)
    px = torch.randn(N, 2, 3, 56, 56, generator=torch.Generator().manual_seed(56))
    px = px.to(torch.bfloat16).float().cuda()  # bf16 values, for oracle and tower alike
    want = iv2_ref.InternVideo2Ref(sd, cfg).cuda()(px).cpu()
    tower = InternVideo2VisionTowerAMD(sd, cfg).cuda()
    tower.fold_ln = fold_ln
    torch_head, native = _both_heads(tower, px)
    _check(f"internvideo2 fold_ln={fold_ln}", torch_head, native, want)


def test_stages_hand_the_flag_to_their_tower(monkeypatch):
    from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD
    from cosmos_curate_amd.pipelines.video.embedding.clip_stages import ClipEmbeddingStage
    from cosmos_curate_amd.pipelines.video.embedding.internvideo2_stages import (
        InternVideo2EmbeddingStage)

    monkeypatch.setitem(cw.CONFIGS, "siglip_tiny", _siglip_cfg("siglip_so400m_14_224", 56))
    for pool, flag in (("torch", False), ("native", True)):
        stage = ClipEmbeddingStage(variant="siglip_tiny", pool_head=pool)
        stage.model.setup()
        assert stage.model._model.tower.native_pool is flag
    with pytest.raises(ValueError, match="attention-pooling head"):
        ClipEmbeddingStage(variant="vit_b32", pool_head="native")

    cfg = dataclasses.replace(iw.INTERNVIDEO2_1B, layers=1, num_frames=2, image=56)
    stage = InternVideo2EmbeddingStage.with_pool_head("native")
    # a one-block tower in place of the 40 blocks setup() would build
    stage.model._tower = InternVideo2VisionTowerAMD(iw.make_internvideo2_weights(cfg), cfg)
    stage.model.setup()
    assert stage.model._tower.native_pool is True
