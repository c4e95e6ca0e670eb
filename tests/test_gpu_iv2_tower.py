"""InternVideo2 tower parity on the GPU, and its two stages end to end.

2-block towers at the real widths (hidden 1408, 16 heads of 88, MLP 6144,
pool to 768, projection 512) on stand-in weights, against tests/iv2_ref.py
in fp32 on the same state dict.  Three geometries, one per attention path
and sequence length class:

    T = 2, image 56    33 tokens   (small rung)
    T = 2, image 112   129 tokens  (flash rung)
    T = 4, image 224   1025 tokens (the pipeline's geometry)

Tolerances are BASELINE.json's tower cosine >= 0.999; the folded and the
unfolded route compute the same function and are held to 0.9999.
"""

import dataclasses
import functools
import pathlib
import uuid

import numpy as np
import pytest
import torch

import iv2_ref
from cosmos_curate_amd.models import internvideo2_weights as iw

pytestmark = pytest.mark.gpu

GEOMETRIES = {"t2_i56": (2, 56), "t2_i112": (2, 112), "t4_i224": (4, 224)}
CLIPS = 2


def _cfg(T, image):
    return dataclasses.replace(iw.INTERNVIDEO2_1B, layers=2, num_frames=T, image=image)


def _pixels(T, image):
    """Two clips of normalised-pixel-like values, already bf16 values.  At
    T = 2 the clips differ in their second frame only."""
    g = torch.Generator().manual_seed(1000 * T + image)
    px = torch.randn(CLIPS, T, 3, image, image, generator=g)
    if T == 2:
        px[1, 0] = px[0, 0]
    return px.to(torch.bfloat16).float()


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


def _tower(sd, cfg):
    from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD

    return InternVideo2VisionTowerAMD(sd, cfg).cuda()


@functools.lru_cache(maxsize=None)
def _run(geometry, stress=False):
    """(reference fp32, folded, folded again, unfolded) embeddings, once."""
    T, image = GEOMETRIES[geometry]
    cfg = _cfg(T, image)
    sd = (iw.make_internvideo2_weights_stress if stress
          else iw.make_internvideo2_weights)(cfg)
    px = _pixels(T, image).cuda()
    want = iv2_ref.InternVideo2Ref(sd, cfg).cuda()(px).cpu()
    tower = _tower(sd, cfg)
    folded = tower(px).cpu()
    again = tower(px).cpu()
    tower.fold_ln = False
    unfolded = tower(px).cpu()
    return want, folded, again, unfolded


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_tower_vs_fp32_reference(geometry):
    want, folded, again, unfolded = _run(geometry)
    assert folded.shape == (CLIPS, 512) and folded.dtype == torch.float32
    torch.testing.assert_close(
        torch.linalg.vector_norm(folded, dim=-1), torch.ones(CLIPS), rtol=0, atol=1e-5)
    cos, cos_u, cos_fu = _cos(folded, want), _cos(unfolded, want), _cos(folded, unfolded)
    print(f"{geometry}: folded vs fp32 {cos.tolist()}, unfolded vs fp32 "
          f"{cos_u.tolist()}, folded vs unfolded {cos_fu.tolist()}")
    assert cos.min() >= 0.999, cos
    assert cos_u.min() >= 0.999, cos_u
    assert cos_fu.min() >= 0.9999, cos_fu
    assert torch.equal(folded, again), "the tower differs from run to run"


@pytest.mark.parametrize("geometry", ["t2_i56", "t2_i112"])
def test_tower_reads_every_frame(geometry):
    """The two clips share their first frame.  A tower that ignored time
    would pass every parity check above with one embedding for both."""
    want, folded, _, _ = _run(geometry)
    ref_between = float(_cos(want[0], want[1]))
    got_between = float(_cos(folded[0], folded[1]))
    print(f"{geometry}: cosine between the clips, fp32 {ref_between:.6f}, "
          f"native {got_between:.6f}")
    assert ref_between < 0.999, "the reference cannot tell the clips apart"
    assert not torch.equal(folded[0], folded[1])
    assert got_between < 0.9999


def test_tower_outlier_channels():
    """Two LayerScale channels and two norm weights per block at 8.0."""
    want, folded, _, unfolded = _run("t2_i112", stress=True)
    cos, cos_u = _cos(folded, want), _cos(unfolded, want)
    print(f"stress: folded vs fp32 {cos.tolist()}, unfolded vs fp32 {cos_u.tolist()}")
    assert cos.min() >= 0.999, cos
    assert cos_u.min() >= 0.999, cos_u


def test_tower_refuses_what_is_out_of_scope():
    cfg = _cfg(2, 56)
    sd = iw.make_internvideo2_weights(cfg)
    with pytest.raises(ValueError, match="position table"):
        _tower(sd, dataclasses.replace(cfg, num_frames=4))
    with pytest.raises(NotImplementedError, match="single-image"):
        _tower(sd, dataclasses.replace(cfg, num_frames=1))
    tower = _tower(sd, cfg)
    with pytest.raises(ValueError, match="expected"):
        tower(torch.zeros(1, 3, 3, 56, 56, device="cuda"))


# ---- the two stages, on raw-NV12 payload clips --------------------------

def _clip_video(secs_per_clip):
    from cosmos_curate_amd.pipelines.video.utils import raw_backend
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        Clip, SplitPipeTask, Video, VideoMetadata)

    h, w, fps = 64, 96, 30
    v = Video(input_video=pathlib.Path("/synthetic/iv2.nv12"),
              metadata=VideoMetadata(size=1, height=h, width=w, framerate=float(fps),
                                     num_frames=fps * max(secs_per_clip),
                                     duration=float(max(secs_per_clip)),
                                     video_codec="raw"))
    for i, secs in enumerate(secs_per_clip):
        raw = raw_backend.make_synthetic_clip(fps * secs, h, w, fps, seed=40 + i)
        v.clips.append(Clip(uuid=uuid.uuid5(uuid.NAMESPACE_URL, f"iv2_{i}"),
                            source_video="s", span=(0.0, float(secs)),
                            encoded_data=np.frombuffer(raw, dtype=np.uint8)))
    return SplitPipeTask(videos=[v])


def test_stages_end_to_end():
    from cosmos_curate_amd.core.interfaces import SequentialRunner, run_pipeline
    from cosmos_curate_amd.models.internvideo2 import InternVideo2MultiModality
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        ClipFrameExtractionStage)
    from cosmos_curate_amd.pipelines.video.embedding.internvideo2_stages import (
        InternVideo2EmbeddingStage, InternVideo2FrameCreationStage)

    cfg = _cfg(4, 224)
    tower = _tower(iw.make_internvideo2_weights(cfg), cfg)
    # 4 s at 2 fps: 9 frames.  1 s at 2 fps: 3 frames < T = 4, re-extracted
    # at 4 fps: 5 frames
    task = _clip_video([4, 1])
    out = run_pipeline(
        [task],
        [ClipFrameExtractionStage(target_fps=[2], target_res=(224, 224)),
         InternVideo2FrameCreationStage(target_fps=2.0)],
        runner=SequentialRunner())
    clips = out[0].video.clips
    inputs = []
    for clip in clips:
        assert not clip.errors, clip.errors
        iv2 = clip.intern_video_2_frames.resolve()
        assert iv2.shape == (1, 4, 3, 224, 224) and iv2.dtype == torch.float32
        assert iv2.is_cuda
        inputs.append(iv2)
    stage = InternVideo2EmbeddingStage(batch_size=8)
    stage._model = InternVideo2MultiModality(tower=tower)  # 2 blocks: seconds
    out = run_pipeline(out, [stage], runner=SequentialRunner())
    want = tower(torch.cat(inputs, dim=0)).cpu().numpy()
    for clip, w in zip(out[0].video.clips, want):
        assert not clip.errors, clip.errors
        e = clip.intern_video_2_embedding
        assert e.shape == (512,) and e.dtype == np.float32
        np.testing.assert_allclose(np.linalg.norm(e), 1.0, atol=1e-5)
        np.testing.assert_array_equal(e, w)
        assert clip.intern_video_2_frames is None  # dropped by its last consumer
        assert clip.clip_embedding is None


def test_u8_frames_match_prepared_tensor():
    """encode_batched_videos on (B, T, 224, 224, 3) u8 frames — normalise
    and patch extraction fused in one kernel — against the prepared float
    tensor of the same frames."""
    from cosmos_curate_amd.models import internvideo2_prep as prep
    from cosmos_curate_amd.models.internvideo2 import InternVideo2MultiModality

    cfg = _cfg(4, 224)
    tower = _tower(iw.make_internvideo2_weights(cfg), cfg)
    model = InternVideo2MultiModality(tower=tower)
    g = torch.Generator().manual_seed(9)
    u8 = torch.randint(0, 256, (CLIPS, 4, 224, 224, 3), generator=g,
                       dtype=torch.uint8).cuda()
    prepared = torch.cat([prep.formulate_input_frames(c, fnum=4) for c in u8])
    a = model.encode_batched_videos(u8)
    b = model.encode_batched_videos(prepared, batch_size=1)
    assert a.shape == (CLIPS, 512)
    assert _cos(a.cpu(), b.cpu()).min() >= 0.9999
