"""What the cosmos-embed1-* embedder rests on that needs no GPU: the parser
and the stage assembly, the writer's routing and the stages' refusals."""

import argparse
import uuid

import numpy as np
import pytest

VARIANTS = ("224p", "336p", "448p")


def _parse(argv):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _setup_parser

    p = argparse.ArgumentParser()
    _setup_parser(p)
    return p.parse_args(["--input-video-path", "/in", "--output-clip-path", "/out", *argv])


def test_parser_default_is_unchanged():
    assert _parse([]).embedding_algorithm == "clip"


@pytest.mark.parametrize("variant", VARIANTS)
def test_assembly_and_writer_routing(variant):
    from cosmos_curate_amd.pipelines.video.read_write.metadata_writer_stage import (
        clip_embedding_of, embd_stem)
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _assemble_stages
    from cosmos_curate_amd.pipelines.video.utils.data_model import Clip

    algorithm = f"cosmos-embed1-{variant}"
    args = _parse(["--embedding-algorithm", algorithm])
    assert args.embedding_algorithm == algorithm
    stages = [getattr(s, "stage", s) for s in _assemble_stages(args)]
    assert [type(s).__name__ for s in stages[-3:]] == [
        "CosmosEmbed1FrameCreationStage", "CosmosEmbed1EmbeddingStage",
        "ClipWriterStage"]
    assert not any("Clip" in type(s).__name__ and "Embedding" in type(s).__name__
                   for s in stages)
    for stage in stages[-3:-1]:
        assert stage.model.variant == variant
        assert stage.model.model_id_names == [f"nvidia/Cosmos-Embed1-{variant}"]
        assert stage.model.get_target_num_frames() == 8
    assert stages[-1]._embedding_algorithm == algorithm

    assert embd_stem(algorithm) == f"ce1_embd_{variant}"
    clip = Clip(uuid=uuid.uuid4(), source_video="s", span=(0.0, 1.0))
    assert clip.cosmos_embed1_frames is None
    assert clip_embedding_of(clip, algorithm) is None
    clip.cosmos_embed1_embedding = np.ones(4, np.float32)
    clip.clip_embedding = np.zeros(4, np.float32)
    assert clip_embedding_of(clip, algorithm) is clip.cosmos_embed1_embedding
    assert clip_embedding_of(clip, "clip") is clip.clip_embedding


def test_text_side_and_unknown_variant_are_refused():
    from cosmos_curate_amd.pipelines.video.embedding.cosmos_embed1_stages import (
        CosmosEmbed1EmbeddingStage)

    stage = CosmosEmbed1EmbeddingStage("224p")
    assert stage.resources.gpus == 0.25
    with pytest.raises(NotImplementedError, match="texts_to_verify"):
        CosmosEmbed1EmbeddingStage("224p", texts_to_verify=["a cat"])
    with pytest.raises(NotImplementedError):
        stage.model.get_text_embedding("a cat")
    with pytest.raises(ValueError, match="variant"):
        CosmosEmbed1EmbeddingStage("512p")
