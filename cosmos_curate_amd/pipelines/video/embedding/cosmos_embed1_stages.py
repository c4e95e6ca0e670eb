"""Cosmos-Embed1 embedding stages — the ``cosmos-embed1-*`` video embedder.

Counterpart of the reference's pipelines/video/embedding/
cosmos_embed1_stages.py: ``CosmosEmbed1FrameCreationStage`` turns a clip's
extracted frames into the model's input (8 frames, subsampled
``[::len//8][:8]``, resized to the variant's resolution and normalised on
the device) and ``CosmosEmbed1EmbeddingStage`` runs the tower over batches
of clips and stores a unit-norm ``clip.cosmos_embed1_embedding`` (256 wide at
224p, 768 at 336p and 448p).  Constructor signatures, defaults and error keys
are the reference's.

The text side is not implemented: ``texts_to_verify`` raises at
construction.
"""

from __future__ import annotations

from cosmos_curate_amd.core.interfaces.model_interface import ModelInterface
from cosmos_curate_amd.core.interfaces.stage_interface import (
    CuratorStage,
    CuratorStageResource,
)
from cosmos_curate_amd.core.utils.lazy_data import LazyData
from cosmos_curate_amd.core.utils.performance_utils import StageTimer
from cosmos_curate_amd.core.utils.roctx import annotate
from cosmos_curate_amd.models.cosmos_embed1 import CosmosEmbed1
from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
    extract_frames,
)
from cosmos_curate_amd.pipelines.video.utils.data_model import SplitPipeTask
from cosmos_curate_amd.pipelines.video.utils.decoder_utils import (
    FrameExtractionPolicy,
    FrameExtractionSignature,
)

_MAX_FPS = 20  # re-extraction stops doubling here
_BATCH = 8     # clips per forward


class CosmosEmbed1FrameCreationStage(CuratorStage):
    """Create the Cosmos-Embed1 input frames of every clip."""

    def __init__(
        self,
        variant: str = "336p",
        target_fps: float = 2.0,
        *,
        verbose: bool = False,
        log_stats: bool = False,
    ) -> None:
        self._timer = StageTimer(self)
        self._target_fps = target_fps
        self._frame_extraction_signature = FrameExtractionSignature(
            FrameExtractionPolicy.sequence, self._target_fps
        ).to_str()
        # utils_only: frame preparation without the tower
        self._model = CosmosEmbed1(variant=variant, utils_only=True)
        self._verbose = verbose
        self._log_stats = log_stats

    @property
    def model(self) -> ModelInterface:
        return self._model

    @property
    def resources(self) -> CuratorStageResource:
        return CuratorStageResource(cpus=1.0)

    @annotate("CosmosEmbed1FrameCreationStage")
    def process_data(self, tasks: list[SplitPipeTask]) -> list[SplitPipeTask] | None:
        sig = self._frame_extraction_signature
        for task in tasks:
            self._timer.reinit(self, task.get_major_size())
            for video in task.videos:
                for clip in video.clips:
                    data = clip.encoded_data.resolve()
                    if data is None:
                        clip.errors["encoded_data"] = "empty"
                        continue
                    ef = clip.extracted_frames.resolve()
                    if ef is None or sig not in ef:
                        clip.errors[f"frames-{sig}"] = "missing"
                        continue
                    with self._timer.time_process():
                        try:
                            frames = ef[sig]
                            # frame-count guarantee: re-extract at doubling
                            # fps; out of headroom, keep what there is
                            target = self._model.get_target_num_frames()
                            regen_fps = self._target_fps
                            while frames.shape[0] < target:
                                regen_fps *= 2
                                if regen_fps > _MAX_FPS:
                                    break
                                frames = extract_frames(data, sample_rate_fps=regen_fps)
                            ce1 = self._model.formulate_input_frames(frames)
                        except Exception as e:  # recorded, not raised
                            clip.errors["cosmos_embed1_frames"] = str(e)
                            continue
                        clip.cosmos_embed1_frames = LazyData(
                            value=ce1, nbytes=ce1.numel() * ce1.element_size())
            if self._log_stats:
                name, stats = self._timer.log_stats()
                task.stage_perf[name] = stats
        return tasks


class CosmosEmbed1EmbeddingStage(CuratorStage):
    """Embed the Cosmos-Embed1 input frames of every clip."""

    def __init__(
        self,
        variant: str = "336p",
        num_gpus_per_worker: float = 0.25,
        *,
        verbose: bool = False,
        log_stats: bool = False,
        texts_to_verify: list[str] | None = None,
    ) -> None:
        if texts_to_verify is not None:
            msg = ("texts_to_verify needs the Cosmos-Embed1 text tower, which "
                   "is not implemented")
            raise NotImplementedError(msg)
        self._timer = StageTimer(self)
        self._num_gpus_per_worker = num_gpus_per_worker
        self._verbose = verbose
        self._log_stats = log_stats
        self._model = CosmosEmbed1(variant=variant)

    @property
    def model(self) -> ModelInterface:
        return self._model

    @property
    def resources(self) -> CuratorStageResource:
        return CuratorStageResource(gpus=self._num_gpus_per_worker)

    @annotate("CosmosEmbed1EmbeddingStage")
    def process_data(self, tasks: list[SplitPipeTask]) -> list[SplitPipeTask] | None:
        for task in tasks:
            self._timer.reinit(self, task.get_major_size())
            with self._timer.time_process():
                for video in task.videos:
                    clips, inputs = [], []
                    for clip in video.clips:
                        ce1 = (clip.cosmos_embed1_frames.resolve()
                               if clip.cosmos_embed1_frames is not None else None)
                        if ce1 is None or ce1.numel() == 0:
                            clip.errors["cosmos_embed1_frames"] = "empty"
                        else:
                            clips.append(clip)
                            inputs.append(ce1)
                    # one forward per _BATCH clips; a failing batch is
                    # recorded on its clips and the others go on
                    for i in range(0, len(clips), _BATCH):
                        part = clips[i : i + _BATCH]
                        try:
                            emb = self._model.encode_video_frames(
                                inputs[i : i + _BATCH], _BATCH)
                            emb = emb.float().cpu().numpy()
                        except Exception as e:
                            for clip in part:
                                clip.errors["cosmos_embed1_embedding"] = str(e)
                            continue
                        for clip, e in zip(part, emb):
                            clip.cosmos_embed1_embedding = e
                    for clip in video.clips:
                        clip.cosmos_embed1_frames = None  # last consumer
            if self._log_stats:
                name, stats = self._timer.log_stats()
                task.stage_perf[name] = stats
        return tasks
