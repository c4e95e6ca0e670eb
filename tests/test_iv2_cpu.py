"""InternVideo2 on the CPU: the fp32 reference on a tiny geometry, the
arithmetic of the two folds the tower makes at construction, the pinned
geometry and checkpoint key names, the pipeline switch and the writer.
"""

import argparse
import dataclasses
import uuid

import numpy as np
import pytest
import torch

import iv2_ref
from cosmos_curate_amd.models import internvideo2_weights as iw
from cosmos_curate_amd.models.internvideo2_vit import fold_layerscale
from cosmos_curate_amd.models.vit_encoder import fold_rmsnorm

TINY = iw.InternVideo2Config(
    "iv2_tiny", hidden=128, layers=2, heads=2, intermediate=256, patch=14,
    pool_dim=64, proj=32, image=28, num_frames=2, pool_heads=2)
EPS = 1e-6
TOL = 2e-2  # rtol = atol on the bf16 result, tests/test_ln_fold_cpu.py's bound


# ---- the reference ------------------------------------------------------

def _tiny_pixels(B=3):
    g = torch.Generator().manual_seed(5)
    return torch.randn(B, TINY.num_frames, 3, TINY.image, TINY.image, generator=g)


def test_ref_tiny_shape_norm_determinism():
    sd = iw.make_internvideo2_weights(TINY)
    px = _tiny_pixels()
    ref = iv2_ref.InternVideo2Ref(sd, TINY)
    out = ref(px)
    assert out.shape == (3, TINY.proj) and out.dtype == torch.float32
    torch.testing.assert_close(
        torch.linalg.vector_norm(out, dim=-1), torch.ones(3), rtol=0, atol=1e-6)
    again = iv2_ref.InternVideo2Ref(iw.make_internvideo2_weights(TINY), TINY)(px)
    assert torch.equal(out, again)
    # a batch is its clips
    torch.testing.assert_close(ref(px[1:2]), out[1:2], rtol=1e-5, atol=1e-6)


def test_ref_zero_layerscale_bypasses_the_blocks():
    """With every LayerScale gamma at 0 both branches of every block vanish:
    the output no longer depends on any block weight.  With the stand-in
    gammas it does — the residuals are wired through the gammas."""
    px = _tiny_pixels(2)

    def run(zero_gammas, scramble):
        sd = iw.make_internvideo2_weights(TINY)
        for k in sd:
            if ".blocks." not in k:
                continue
            if k.endswith(".gamma"):
                if zero_gammas:
                    sd[k] = torch.zeros_like(sd[k])
            elif scramble:
                sd[k] = sd[k].flip(0) * 1.5
        return iv2_ref.InternVideo2Ref(sd, TINY)(px)

    assert torch.equal(run(True, False), run(True, True))
    assert not torch.allclose(run(False, False), run(False, True), atol=1e-3)
    assert not torch.allclose(run(False, False), run(True, False), atol=1e-3)


def test_ref_reads_time():
    px = _tiny_pixels(1)
    swapped = px.flip(1)  # the same frames in the other order
    ref = iv2_ref.InternVideo2Ref(iw.make_internvideo2_weights(TINY), TINY)
    assert not torch.allclose(ref(px), ref(swapped), atol=1e-4)


# ---- the RMS fold -------------------------------------------------------

def _inputs(family, M, K):
    x = torch.randn(M, K)
    if family == "row_means":  # row means up to 16 sigma either way
        x = x + torch.linspace(-16.0, 16.0, M)[:, None]
    elif family == "massive_channels":  # two outlier channels, every row
        x[:, 3] = 60.0
        x[:, K // 2 + 1] = 60.0
    return x.to(torch.bfloat16)


def _folded_rms_forward(x_bf16, w_fold, zeros, cbias):
    """What cc_gemm_bf16_rms computes, in torch f32: bf16 x, W' rounded to
    bf16, f32 accumulation, rstd in f32 from the bf16 x, the LN_IN epilogue
    rstd * (acc - mean * s) + c with mean = 0, a bf16 result."""
    xf = x_bf16.float()
    acc = xf @ w_fold.float().T
    rstd = torch.rsqrt((xf * xf).sum(dim=1) / xf.shape[1] + EPS)
    mean = torch.zeros_like(rstd)
    return (rstd[:, None] * (acc - mean[:, None] * zeros) + cbias).to(torch.bfloat16)


@pytest.mark.parametrize("family", ["plain", "row_means", "massive_channels"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize(("K", "N"), [(1408, 256), (256, 512)])
def test_rms_fold_matches_float64(family, bias, K, N):
    M = 300
    torch.manual_seed(K + N + len(family))
    x = _inputs(family, M, K)
    w = torch.randn(N, K) / K**0.5
    b = 0.1 * torch.randn(N) if bias else None
    g = 1.0 + 0.2 * torch.randn(K)
    w_fold, zeros, cbias = fold_rmsnorm(w, b, g)
    assert w_fold.dtype == torch.bfloat16 and w_fold.shape == (N, K)
    assert zeros.dtype == cbias.dtype == torch.float32
    assert torch.all(zeros == 0) and zeros.shape == (N,)
    assert torch.equal(cbias, b if bias else torch.zeros(N))
    got = _folded_rms_forward(x, w_fold, zeros, cbias).double()
    xd = x.double()
    normed = xd * torch.rsqrt((xd * xd).mean(dim=1, keepdim=True) + EPS) * g.double()
    want = torch.nn.functional.linear(
        normed, w.double(), None if b is None else b.double())
    err = (got - want).abs()
    worst = (err / (TOL + TOL * want.abs())).max().item()
    print(f"{family} K={K} N={N} bias={bias}: max abs err {err.max().item():.3e}, "
          f"worst share of the budget {worst:.3f}")
    torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)


# ---- the LayerScale fold ------------------------------------------------

def test_layerscale_fold_is_exact_to_f32_roundoff():
    torch.manual_seed(3)
    N, K, M = 96, 160, 17
    x, w, b = torch.randn(M, K), torch.randn(N, K) / K**0.5, torch.randn(N)
    gamma = 0.5 + torch.rand(N)
    gamma[7] = 8.0
    folded = torch.nn.functional.linear(x, gamma[:, None] * w, gamma * b)
    want = gamma * torch.nn.functional.linear(x, w, b)
    torch.testing.assert_close(folded, want, rtol=1e-5, atol=1e-5)
    # the tower's helper: that scaling in f32, then one cast of the weight
    w_bf, b_f32 = fold_layerscale(w, b, gamma)
    assert torch.equal(w_bf, (gamma[:, None] * w).to(torch.bfloat16))
    assert torch.equal(b_f32, gamma * b) and b_f32.dtype == torch.float32


# ---- geometry, key names, stand-in values -------------------------------

def test_config_geometry_pinned():
    c = iw.INTERNVIDEO2_1B
    assert (c.hidden, c.layers, c.heads, c.intermediate, c.patch, c.image,
            c.pool_dim, c.proj) == (1408, 40, 16, 6144, 14, 224, 768, 512)
    assert c.hidden // c.heads == 88 and c.pool_heads == 16
    assert c.num_frames == 4 and c.num_pos == 1025
    assert dataclasses.replace(c, num_frames=8).num_pos == 2049
    assert c.rms_eps == 1e-6 and c.pool_ln_eps == 1e-5
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.hidden = 1
    # not one of the image towers --embedding-model chooses from
    from cosmos_curate_amd.models import clip_weights as cw
    assert c.name not in cw.CONFIGS


def test_weight_dict_key_names_and_shapes():
    cfg = dataclasses.replace(iw.INTERNVIDEO2_1B, layers=2)
    sd = iw.make_internvideo2_weights(cfg)
    H, I = 1408, 6144
    want = {
        "vision_encoder.patch_embed.proj.weight": (H, 3, 1, 14, 14),
        "vision_encoder.patch_embed.proj.bias": (H,),
        "vision_encoder.cls_token": (1, 1, H),
        "vision_encoder.pos_embed": (1, 1025, H),
        "vision_encoder.clip_projector.norm1_q.weight": (H,),
        "vision_encoder.clip_projector.norm1_q.bias": (H,),
        "vision_encoder.clip_projector.norm1_k.weight": (H,),
        "vision_encoder.clip_projector.norm1_k.bias": (H,),
        "vision_encoder.clip_projector.norm1_v.weight": (H,),
        "vision_encoder.clip_projector.norm1_v.bias": (H,),
        "vision_encoder.clip_projector.cross_attn.q.weight": (H, H),
        "vision_encoder.clip_projector.cross_attn.k.weight": (H, H),
        "vision_encoder.clip_projector.cross_attn.v.weight": (H, H),
        "vision_encoder.clip_projector.cross_attn.q_bias": (H,),
        "vision_encoder.clip_projector.cross_attn.k_bias": (H,),
        "vision_encoder.clip_projector.cross_attn.v_bias": (H,),
        "vision_encoder.clip_projector.cross_attn.proj.weight": (768, H),
        "vision_encoder.clip_projector.cross_attn.proj.bias": (768,),
        "vision_proj.weight": (512, 768),
        "vision_proj.bias": (512,),
    }
    for i in range(2):
        b = f"vision_encoder.blocks.{i}."
        want.update({
            b + "norm1.weight": (H,), b + "norm2.weight": (H,),
            b + "attn.qkv.weight": (3 * H, H),
            b + "attn.q_norm.weight": (H,), b + "attn.k_norm.weight": (H,),
            b + "attn.proj.weight": (H, H), b + "attn.proj.bias": (H,),
            b + "ls1.gamma": (H,), b + "ls2.gamma": (H,),
            b + "mlp.fc1.weight": (I, H), b + "mlp.fc1.bias": (I,),
            b + "mlp.fc2.weight": (H, I), b + "mlp.fc2.bias": (H,),
        })
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert not any("qkv.bias" in k for k in sd)  # qkv has no bias
    for k, v in sd.items():
        if k.endswith(".gamma"):  # of order one, never the initial 1e-5
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5, k
        if "norm" in k and k.endswith(".weight"):  # a spread, not ones
            assert 0.1 < float(v.std()) < 0.3 and abs(float(v.mean()) - 1) < 0.05, k
    again = iw.make_internvideo2_weights(cfg)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    stress = iw.make_internvideo2_weights_stress(cfg)
    for i in range(2):
        b = f"vision_encoder.blocks.{i}."
        for key in ("ls1.gamma", "ls2.gamma", "norm1.weight", "norm2.weight"):
            assert int((stress[b + key] == 8.0).sum()) == 1
            assert int((stress[b + key] != sd[b + key]).sum()) == 1


def test_tower_construction_refusals_need_no_gpu():
    from cosmos_curate_amd.models.internvideo2_vit import InternVideo2VisionTowerAMD

    sd = iw.make_internvideo2_weights(TINY)
    with pytest.raises(ValueError, match="position table"):
        InternVideo2VisionTowerAMD(sd, dataclasses.replace(TINY, num_frames=4))
    with pytest.raises(NotImplementedError, match="single-image"):
        InternVideo2VisionTowerAMD(sd, dataclasses.replace(TINY, num_frames=1))
    tower = InternVideo2VisionTowerAMD(sd, TINY)
    # LayerScale went into the out-proj / fc2 buffers, the norms into wf_*
    b = "vision_encoder.blocks.1."
    assert torch.equal(tower.w_fc2_1, (sd[b + "ls2.gamma"][:, None]
                                       * sd[b + "mlp.fc2.weight"]).to(torch.bfloat16))
    assert torch.equal(tower.b_out_1, sd[b + "ls1.gamma"] * sd[b + "attn.proj.bias"])
    assert torch.equal(tower.wf_qkv_1, (sd[b + "attn.qkv.weight"]
                                        * sd[b + "norm1.weight"][None, :]).to(torch.bfloat16))
    assert torch.all(tower.c_qkv_1 == 0) and torch.equal(tower.c_fc1_1, sd[b + "mlp.fc1.bias"])
    assert tower.wf_pool_kv.shape == (2 * TINY.hidden, TINY.hidden)
    assert not any(k.startswith(("wf_", "s_", "c_")) for k in tower.state_dict())


# ---- parser, assembly, writer -------------------------------------------

def _parse(argv):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _setup_parser

    p = argparse.ArgumentParser()
    _setup_parser(p)
    return p.parse_args(["--input-video-path", "/in", "--output-clip-path", "/out", *argv])


def _stage_names(args):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _assemble_stages

    return [type(getattr(s, "stage", s)).__name__ for s in _assemble_stages(args)]


def test_embedding_algorithm_switch():
    default = _stage_names(_parse([]))
    assert default == [
        "VideoDownloader", "FixedStrideExtractorStage", "ClipTranscodingStage",
        "ClipFrameExtractionStage", "ClipFrameCreationStage", "ClipEmbeddingStage",
        "ClipWriterStage"]
    # free text stays free text: any other value keeps that assembly
    assert _stage_names(_parse(["--embedding-algorithm", "anything"])) == default
    iv2 = _stage_names(_parse(["--embedding-algorithm", "internvideo2",
                               "--embedding-model", "vit_l14"]))
    assert iv2 == [
        "VideoDownloader", "FixedStrideExtractorStage", "ClipTranscodingStage",
        "ClipFrameExtractionStage", "InternVideo2FrameCreationStage",
        "InternVideo2EmbeddingStage", "ClipWriterStage"]
    assert not any(n.startswith("Clip") and "Embedding" in n for n in iv2)
    no_emb = _stage_names(_parse(["--embedding-algorithm", "internvideo2",
                                  "--no-embeddings"]))
    assert not any("InternVideo2" in n for n in no_emb)


def test_stage_signatures_and_texts_to_verify():
    import inspect

    from cosmos_curate_amd.pipelines.video.embedding.internvideo2_stages import (
        InternVideo2EmbeddingStage, InternVideo2FrameCreationStage)

    sig = inspect.signature(InternVideo2FrameCreationStage.__init__).parameters
    assert list(sig)[1:] == ["target_fps", "verbose", "log_stats"]
    assert sig["target_fps"].default == 2.0
    sig = inspect.signature(InternVideo2EmbeddingStage.__init__).parameters
    assert list(sig)[1:] == ["num_gpus_per_worker", "batch_size", "verbose",
                             "log_stats", "texts_to_verify"]
    assert (sig["num_gpus_per_worker"].default, sig["batch_size"].default) == (0.25, 8)
    stage = InternVideo2EmbeddingStage()
    assert stage.resources.gpus == 0.25
    assert stage.model.conda_env_name == "unified"
    with pytest.raises(NotImplementedError, match="texts_to_verify"):
        InternVideo2EmbeddingStage(texts_to_verify=["a cat"])
    with pytest.raises(NotImplementedError):
        stage.model.get_text_embedding("a cat")


def test_clip_fields_default_to_none():
    from cosmos_curate_amd.pipelines.video.utils.data_model import Clip

    c = Clip(uuid=uuid.uuid4(), source_video="s", span=(0.0, 1.0))
    assert c.intern_video_2_frames is None and c.intern_video_2_embedding is None


def test_writer_round_trip_iv2_embd(tmp_path):
    from cosmos_curate_amd.pipelines.video.dedup_pipeline import load_embeddings
    from cosmos_curate_amd.pipelines.video.read_write.metadata_writer_stage import (
        ClipWriterStage, write_split_summary)
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        Clip, SplitPipeTask, Video)

    rng = np.random.default_rng(0)
    embs = rng.standard_normal((3, 512)).astype(np.float32)
    embs /= np.linalg.norm(embs, axis=1, keepdims=True)
    v = Video(input_video="v.mp4")
    for i in range(4):
        c = Clip(uuid=uuid.uuid5(uuid.NAMESPACE_URL, f"c{i}"), source_video="v.mp4",
                 span=(float(i), float(i + 1)))
        if i < 3:
            c.intern_video_2_embedding = embs[i]
        else:  # an image embedding is not what this run writes
            c.clip_embedding = np.ones(512, dtype=np.float32)
        v.clips.append(c)
    task = SplitPipeTask(videos=[v])
    stage = ClipWriterStage(str(tmp_path), embedding_algorithm="internvideo2")
    stage.stage_setup()
    stage.process_data([task])
    assert sorted(p.name for p in tmp_path.glob("*_embd")) == ["iv2_embd"]
    ids, got = load_embeddings(tmp_path)
    assert got.shape == (3, 512) and got.shape[1] % 64 == 0
    order = [ids.index(str(c.uuid)) for c in v.clips[:3]]
    np.testing.assert_array_equal(got[order], embs)
    import json

    metas = {c.uuid: json.loads((tmp_path / "metas" / "v0" / f"{c.uuid}.json").read_text())
             for c in v.clips}
    assert [metas[c.uuid]["has_embedding"] for c in v.clips] == [True, True, True, False]
    assert v.clip_stats.num_with_embeddings == 3
    summary = write_split_summary(str(tmp_path), [task], embedding_algorithm="internvideo2")
    assert summary["num_clips_with_embeddings"] == 3
    # the default algorithm is untouched: clip_embd/, the image embedding
    other = tmp_path / "clip_run"
    stage = ClipWriterStage(str(other))
    stage.stage_setup()
    stage.process_data([SplitPipeTask(videos=[v])])
    assert sorted(p.name for p in other.glob("*_embd")) == ["clip_embd"]
    assert load_embeddings(other)[1].shape == (1, 512)
