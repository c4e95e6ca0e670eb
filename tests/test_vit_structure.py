"""Product ViT arithmetic vs the transformers oracle (CPU, no GPU).

Pins the *structure* of ClipVisionTowerAMD (patch-GEMM flattening, fused
QKV ordering, quick-gelu, LN placement, projection, L2 norm) against the
reference's own arithmetic (transformers CLIPVisionModelWithProjection,
models/clip.py:64-74) by monkeypatching the one contraction primitive
(_linear) to torch on CPU.  The MFMA kernel itself is pinned on the GPU in
tests/test_gpu_vit.py; this test makes a GPU failure attributable to the
kernel alone.  The SigLIP and the InternVideo2 tower (the latter against
tests/iv2_ref.py) are pinned the same way.
"""

import dataclasses
import functools

import numpy as np
import pytest
import torch

import iv2_ref
from cosmos_curate_amd.models import internvideo2_weights as iw
from cosmos_curate_amd.models.clip_vit import ClipVisionTowerAMD
from cosmos_curate_amd.models.clip_weights import make_clip_vit_b32_weights
from oracle import vit as oracle_vit
from oracle.color import clip_preprocess


@pytest.fixture(scope="module")
def weights():
    return make_clip_vit_b32_weights()


def _torch_linear(self, x, w, b, act=0, residual=None):
    y = torch.nn.functional.linear(x.float(), w.float(), b.float() if b is not None else None)
    if act == 1:
        y = y * torch.sigmoid(1.702 * y)
    if act == 2:
        y = torch.nn.functional.gelu(y, approximate="tanh")
    if act == 3:
        y = torch.nn.functional.gelu(y, approximate="none")
    if residual is not None:
        y = y + residual.float()
    return y.to(torch.bfloat16)


def test_weights_deterministic(weights):
    again = make_clip_vit_b32_weights()
    for k, v in weights.items():
        assert torch.equal(v, again[k]), k


def test_tower_l14_matches_transformers_fp32(monkeypatch):
    """ViT-L/14 geometry (the reference's own CLIP model, clip.py:33):
    patch-K padding (588->640) + 24-layer tower vs transformers fp32."""
    pytest.importorskip("transformers")
    from transformers import CLIPVisionConfig
    from transformers.models.clip.modeling_clip import CLIPVisionModelWithProjection

    from cosmos_curate_amd.models import clip_weights as cw

    weights = cw.make_clip_vit_weights(cw.VIT_L14)
    cfg = CLIPVisionConfig(
        hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
        intermediate_size=4096, patch_size=14, projection_dim=768,
    )
    ref = CLIPVisionModelWithProjection(cfg)
    missing, unexpected = ref.load_state_dict(weights, strict=False)
    assert not [m for m in missing if "position_ids" not in m] and not unexpected
    ref = ref.float().eval()

    rng = np.random.default_rng(0x14)
    frames = rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)
    pixels = clip_preprocess(frames)
    with torch.no_grad():
        want = ref(pixel_values=torch.from_numpy(pixels)).image_embeds
        want = (want / torch.linalg.vector_norm(want, dim=-1, keepdim=True)).numpy()

    monkeypatch.setattr(ClipVisionTowerAMD, "_linear", _torch_linear)
    tower = ClipVisionTowerAMD(weights, cw.VIT_L14)
    got = tower(torch.from_numpy(pixels)).float().numpy()
    assert got.shape == (1, 768)
    cos = float(np.sum(want * got))
    assert cos >= 0.999, cos


def test_tower_matches_transformers_fp32(weights, monkeypatch):
    transformers = pytest.importorskip("transformers")  # noqa: F841
    ref = oracle_vit.build_reference_clip_vision(weights)

    rng = np.random.default_rng(0xC11F)
    frames = rng.integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    pixels = clip_preprocess(frames)  # (2,3,224,224) f32

    want = oracle_vit.embed_frames_fp32(ref, pixels)

    monkeypatch.setattr(ClipVisionTowerAMD, "_linear", _torch_linear)
    tower = ClipVisionTowerAMD(weights)
    got = tower(torch.from_numpy(pixels)).float().numpy()

    assert want.shape == got.shape == (2, 512)
    cos = np.sum(want * got, axis=1)  # both unit-norm
    assert np.all(cos >= 0.999), f"cosine too low: {cos}"
    # unit norm
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-3)


def test_siglip_weights_load_into_transformers():
    """make_siglip_weights keys match SiglipVisionModel exactly and the
    fp32 oracle produces unit-norm pooled embeddings (tiny geometry)."""
    import torch

    from cosmos_curate_amd.models.clip_weights import VitConfig, make_siglip_weights
    from oracle.vit import build_reference_siglip_vision, siglip_embed_frames_fp32

    tiny = VitConfig("siglip_l16_256", hidden=128, layers=2, heads=2,
                     intermediate=256, patch=16, proj=128, image=32,
                     has_cls=False, act="gelu_tanh")
    sd = make_siglip_weights(tiny)
    ref = build_reference_siglip_vision(
        sd, dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                 num_attention_heads=2, image_size=32, patch_size=16))
    e = siglip_embed_frames_fp32(ref, torch.randn(2, 3, 32, 32))
    assert e.shape == (2, 128)
    import numpy as np

    np.testing.assert_allclose((e ** 2).sum(axis=1), 1.0, rtol=1e-5)


def _tiny_siglip(image):
    """(cfg, weights) of a 2-layer, 2-head (hd 64) SigLIP tower."""
    from cosmos_curate_amd.models.clip_weights import VitConfig, make_siglip_weights

    cfg = VitConfig("siglip_tiny", hidden=128, layers=2, heads=2,
                    intermediate=256, patch=16, proj=128, image=image,
                    has_cls=False, act="gelu_tanh", ln_eps=1e-6)
    return cfg, make_siglip_weights(cfg)


@pytest.mark.parametrize("image", [32, 144])  # seq 4 and 81
def test_siglip_tower_matches_transformers_fp32(monkeypatch, image):
    """SiglipVisionTowerAMD's own arithmetic (patch bias, position add, the
    shared encoder at act 2 / eps 1e-6, post-LN, MAP head) vs transformers
    SiglipVisionModel fp32, _linear patched to torch."""
    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD

    cfg, sd = _tiny_siglip(image)
    ref = oracle_vit.build_reference_siglip_vision(
        sd, dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                 num_attention_heads=2, image_size=image, patch_size=16))
    torch.manual_seed(image)
    pixels = torch.rand(2, 3, image, image) * 2 - 1  # SigLIP-normalized range
    want = oracle_vit.siglip_embed_frames_fp32(ref, pixels)

    monkeypatch.setattr(SiglipVisionTowerAMD, "_linear", _torch_linear)
    got = SiglipVisionTowerAMD(sd, cfg)(pixels).numpy()
    assert want.shape == got.shape == (2, 128)
    cos = np.sum(want * got, axis=1)  # both unit-norm
    print("per-frame cosine vs fp32 oracle:", cos.tolist())
    assert np.all(cos >= 0.999), cos


def test_siglip_tower_linear_calls(monkeypatch):
    """The shared layer loop as SigLIP drives it: the patch GEMM (with its
    bias) and 4 GEMMs per layer, every one on all n*seq rows; the fc1
    epilogue carries the tanh-gelu code and nothing else an activation."""
    from cosmos_curate_amd.models.siglip_vit import SiglipVisionTowerAMD

    cfg, sd = _tiny_siglip(32)
    calls = []

    def counting(self, x, w, b, act=0, residual=None):
        calls.append((x.shape[0], b is not None, act, residual is not None))
        return _torch_linear(self, x, w, b, act, residual)

    monkeypatch.setattr(SiglipVisionTowerAMD, "_linear", counting)
    n, seq = 3, 4
    SiglipVisionTowerAMD(sd, cfg)(torch.randn(n, 3, 32, 32))
    rows = n * seq
    layer = [(rows, True, 0, False), (rows, True, 0, True),   # qkv, out+res
             (rows, True, 2, False), (rows, True, 0, True)]   # fc1, fc2+res
    assert calls == [(rows, True, 0, False)] + layer * cfg.layers
    assert len(calls) == 1 + 4 * cfg.layers


def test_siglip_config_geometry():
    from cosmos_curate_amd.models.clip_weights import SIGLIP_L16_256

    cfg = SIGLIP_L16_256
    assert cfg.num_pos == 256  # no CLS token
    assert cfg.hidden // cfg.heads == 64  # attn_mid head-dim contract
    assert (3 * cfg.patch * cfg.patch) % 64 == 0


# ---- InternVideo2 on the shared layer: RMSNorm, QK-norm, no QKV bias -----

def _iv2_case(case):
    """(cfg, weights): the tiny geometry, or the real widths at 2 blocks,
    T = 2, image 56 (33 tokens), plain or with outlier channels."""
    if case == "tiny":
        from test_iv2_cpu import TINY

        return TINY, iw.make_internvideo2_weights(TINY)
    cfg = dataclasses.replace(iw.INTERNVIDEO2_1B, layers=2, num_frames=2, image=56)
    make = (iw.make_internvideo2_weights_stress if case == "real_stress"
            else iw.make_internvideo2_weights)
    return cfg, make(cfg)


@functools.lru_cache(maxsize=None)
def _iv2_run(case):
    """(cfg, fp32 reference, the tower on CPU with _linear patched to torch,
    its _linear calls), once per case.  Two clips that share their first
    frame, as in tests/test_gpu_iv2_tower.py."""
    from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD

    cfg, sd = _iv2_case(case)
    g = torch.Generator().manual_seed(1000 * cfg.num_frames + cfg.image)
    px = torch.randn(2, cfg.num_frames, 3, cfg.image, cfg.image, generator=g)
    px[1, 0] = px[0, 0]
    px = px.to(torch.bfloat16).float()
    want = iv2_ref.InternVideo2Ref(sd, cfg)(px)
    calls = []

    def counting(self, x, w, b, act=0, residual=None):
        calls.append((x.shape[0], b is not None, act, residual is not None))
        return _torch_linear(self, x, w, b, act, residual)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(InternVideo2VisionTowerAMD, "_linear", counting)
        got = InternVideo2VisionTowerAMD(sd, cfg)(px)
    return cfg, want, got, calls


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


@pytest.mark.parametrize("case", ["tiny", "real", "real_stress"])
def test_iv2_tower_matches_fp32_reference(case):
    """InternVideo2VisionTowerAMD's arithmetic (patch bias, CLS + position
    add, the shared layer with RMSNorm / QK-norm / erf-GELU and the folded
    LayerScale, the pooling head) vs tests/iv2_ref.py in fp32 on the same
    state dict.  The bound is BASELINE.json's tower cosine."""
    cfg, want, got, _ = _iv2_run(case)
    assert got.shape == want.shape == (2, cfg.proj) and got.dtype == torch.float32
    torch.testing.assert_close(
        torch.linalg.vector_norm(got, dim=-1), torch.ones(2), rtol=0, atol=1e-5)
    cos = _cos(got, want)
    print(f"{case}: per-clip cosine vs fp32 reference {cos.tolist()}")
    assert cos.min() >= 0.999, cos


def test_iv2_tower_linear_calls():
    """The shared layer loop as InternVideo2 drives it: the patch GEMM with
    its bias, 4 GEMMs per block on all n*seq rows — QKV without a bias, the
    erf-GELU code on fc1 and nowhere else — and the pooling head's K and V."""
    cfg, _, _, calls = _iv2_run("tiny")
    rows = 2 * cfg.num_pos
    block = [(rows, False, 0, False), (rows, True, 0, True),   # qkv, out+res
             (rows, True, 3, False), (rows, True, 0, True)]    # fc1, fc2+res
    assert len(calls) == 4 * cfg.layers + 3
    assert calls == ([(rows - 2, True, 0, False)] + block * cfg.layers
                     + [(rows, True, 0, False)] * 2)


@pytest.mark.parametrize("case", ["tiny", "real"])
def test_iv2_tower_reads_every_frame(case):
    """The two clips share their first frame.  A tower that ignored time
    would pass the parity check with one embedding for both
    (test_gpu_iv2_tower.test_tower_reads_every_frame, on the CPU route)."""
    _, want, got, _ = _iv2_run(case)
    ref_between = float(_cos(want[0], want[1]))
    got_between = float(_cos(got[0], got[1]))
    print(f"{case}: cosine between the clips, fp32 {ref_between:.6f}, "
          f"tower {got_between:.6f}")
    assert ref_between < 0.999, "the reference cannot tell the clips apart"
    assert not torch.equal(got[0], got[1])
    assert got_between < 0.9999
