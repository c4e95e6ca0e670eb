"""Stage + runner integration on CPU (SequentialRunner, no GPU).

Mirrors the reference's test approach: real stages driven by
a SequentialRunner mini-pipeline; golden expectations from
test_fixed_stride_extraction.py (30 s video -> 3 x 10 s clips, etc.).
"""

import pathlib
import uuid

import numpy as np
import pytest

from cosmos_curate_amd.core.interfaces import (
    CuratorStage,
    CuratorStageSpec,
    PipelineExecutionError,
    SequentialRunner,
    WorkerPoolRunner,
    run_pipeline,
)
from cosmos_curate_amd.pipelines.video.clipping.clip_extraction_stages import (
    FixedStrideExtractorStage,
)
from cosmos_curate_amd.pipelines.video.utils.data_model import (
    SplitPipeTask,
    Video,
    VideoMetadata,
)


def make_task(duration_s: float = 30.0, fps: float = 24.0) -> SplitPipeTask:
    n = int(duration_s * fps)
    v = Video(
        input_video=pathlib.Path("/data/test_video.mp4"),
        metadata=VideoMetadata(
            size=1000, height=480, width=854, framerate=fps, num_frames=n,
            duration=duration_s, video_codec="h264",
        ),
        timestamps=(np.arange(n) / fps).astype(np.float32),
    )
    return SplitPipeTask(videos=[v])


def test_fixed_stride_default_parameters():
    """test_fixed_stride_extraction.py:100-141 golden: 3 clips 0-10/10-20/20-30."""
    stage = FixedStrideExtractorStage(log_stats=True)
    assert stage.clip_len_s == 10 and stage.clip_stride_s == 10
    assert stage.min_clip_length_s == 10 and stage._limit_clips == 0
    assert stage.resources.cpus == 1.0 and stage.resources.gpus == 0

    out = run_pipeline([make_task()], [stage], runner=SequentialRunner())
    assert len(out) == 1
    video = out[0].video
    assert len(video.clips) == 3
    expected = [(0.0, 10.0), (10.0, 20.0), (20.0, 30.0)]
    for clip, (s, e) in zip(video.clips, expected):
        assert clip.span[0] == pytest.approx(s, abs=0.01)
        assert clip.span[1] == pytest.approx(e, abs=0.01)
    assert "FixedStrideExtractorStage" in out[0].stage_perf


def test_fixed_stride_5s():
    """test_fixed_stride_extraction.py:146-186 golden: 6 clips of 5 s."""
    stage = FixedStrideExtractorStage(
        clip_len_s=5.0, clip_stride_s=5.0, min_clip_length_s=5.0
    )
    out = run_pipeline([make_task()], [stage], runner=SequentialRunner())
    assert len(out[0].video.clips) == 6


def test_fixed_stride_uuid_determinism():
    """UUID formula: uuid5(NAMESPACE_URL, f"{session}_{s}_{e}") with
    session = input path (test_fixed_stride_extraction.py:406 pattern)."""
    out1 = run_pipeline([make_task()], [FixedStrideExtractorStage()], runner=SequentialRunner())
    out2 = run_pipeline([make_task()], [FixedStrideExtractorStage()], runner=SequentialRunner())
    u1 = [c.uuid for c in out1[0].video.clips]
    u2 = [c.uuid for c in out2[0].video.clips]
    assert u1 == u2
    assert u1[0] == uuid.uuid5(uuid.NAMESPACE_URL, "/data/test_video.mp4_0.0_10.0")


def test_invalid_duration_records_error_not_raise():
    t = make_task()
    t.video.metadata.num_frames = 0
    out = run_pipeline([t], [FixedStrideExtractorStage()], runner=SequentialRunner())
    assert out[0].video.errors  # recorded, not raised (§8b error convention)
    assert not out[0].video.clips


def test_run_pipeline_wraps_failures():
    class Boom(CuratorStage):
        def process_data(self, tasks):
            raise RuntimeError("boom")

    with pytest.raises(PipelineExecutionError):
        run_pipeline([make_task()], [Boom()], runner=SequentialRunner())


def test_spec_defaults_gpu_lifetime():
    class G(CuratorStage):
        @property
        def resources(self):
            from cosmos_curate_amd.core.interfaces import CuratorStageResource

            return CuratorStageResource(gpus=1)

    from cosmos_curate_amd.core.interfaces.pipeline_interface import (
        _build_pipeline_stage_specs,
    )

    specs = _build_pipeline_stage_specs([G()])
    assert specs[0].worker_max_lifetime_m == 120  # pipeline_interface.py:187-219
    assert specs[0].worker_restart_interval_m == 5


def test_worker_pool_runner_shards():
    tasks = [make_task() for _ in range(7)]
    r0 = WorkerPoolRunner(rank=0, world_size=2)
    r1 = WorkerPoolRunner(rank=1, world_size=2)
    s0 = r0.shard(tasks)
    s1 = r1.shard(tasks)
    assert len(s0) == 4 and len(s1) == 3
    assert {id(t) for t in s0} | {id(t) for t in s1} == {id(t) for t in tasks}
    out = r0.run(tasks, [CuratorStageSpec(FixedStrideExtractorStage())])
    assert len(out) == 4


def test_retry_attempts():
    calls = {"n": 0}

    class Flaky(CuratorStage):
        def process_data(self, tasks):
            calls["n"] += 1
            if calls["n"] < 3:
                raise RuntimeError("transient")
            return tasks

    spec = CuratorStageSpec(Flaky(), num_run_attempts_python=3)
    out = run_pipeline([make_task()], [spec], runner=SequentialRunner())
    assert calls["n"] == 3 and len(out) == 1


def test_multicam_alignment_checks():
    """data_model.py:595-687 multicam contract: aligned spans pass,
    misalignment and count mismatch are loud."""
    import uuid as uuid_mod

    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        Clip,
        assert_video_clip_alignment,
        check_clip_time_alignment,
    )

    def cam(spans):
        v = make_task().video
        v.clips = [
            Clip(uuid=uuid_mod.uuid4(), source_video="s", span=s) for s in spans
        ]
        return v

    a = cam([(0.0, 10.0), (10.0, 20.0)])
    b = cam([(0.0, 10.0), (10.0, 20.0)])
    assert check_clip_time_alignment([a.clips, b.clips]) == []
    assert_video_clip_alignment([a, b])  # no raise

    c = cam([(0.0, 10.0), (10.0, 21.0)])
    assert check_clip_time_alignment([a.clips, c.clips]) == [1]
    with pytest.raises(ValueError, match="misaligned spans"):
        assert_video_clip_alignment([a, c])

    d = cam([(0.0, 10.0)])
    with pytest.raises(ValueError, match="different clip counts"):
        check_clip_time_alignment([a.clips, d.clips])


def test_multicam_fixed_stride_shares_spans_and_uuids():
    """Multicam: FixedStrideExtractorStage gives every camera the same
    spans AND the same clip uuids (clip_extraction_stages.py:654-661)."""
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        assert_time_alignment,
    )

    t = make_task()
    t.videos.append(make_task().video)  # second camera
    out = run_pipeline([t], [FixedStrideExtractorStage()], runner=SequentialRunner())
    cams = out[0].videos
    assert len(cams) == 2
    assert [c.span for c in cams[0].clips] == [c.span for c in cams[1].clips]
    assert [c.uuid for c in cams[0].clips] == [c.uuid for c in cams[1].clips]
    assert_time_alignment(out)


def test_lazy_data_prefetch_resolve_as_ready():
    """ref_resolver surface (prefetch/resolve_as_ready): 1:1 mapping,
    empty items yield (key, None)."""
    from cosmos_curate_amd.core.utils.lazy_data import (
        LazyData,
        prefetch,
        resolve_as_ready,
    )

    a = LazyData(value=b"abc", nbytes=3)
    b = LazyData()
    prefetch([a, b])  # no-op, must not raise
    out = list(resolve_as_ready([("a", a), ("b", b), ("c", None)]))
    assert out == [("a", b"abc"), ("b", None), ("c", None)]


def test_timestamps_integration_real_mp4(tmp_path):
    """Mirror of the reference test_timestamps_integration.py sanity
    battery: populate_metadata/populate_timestamps on a real MP4 ->
    monotonic finite f32 within duration; major-size delta ==
    timestamps.nbytes; downloader -> fixed-stride on the 30 s sample
    yields 3 clips.  Uses the reference's own 30 s fixture (committed
    with its slice payload blanked, tests/golden_videos.py)."""
    import numpy as np

    from cosmos_curate_amd.pipelines.video.utils.data_model import Video
    from golden_videos import video_bytes

    src = tmp_path / "test_video_30s.mp4"
    src.write_bytes(video_bytes("test_video_30s"))
    v = Video(input_video=src, encoded_data=np.frombuffer(src.read_bytes(), dtype=np.uint8))
    v.populate_metadata()
    size_before = v.get_major_size()
    v.populate_timestamps()
    ts = v.timestamps
    assert ts is not None and len(ts) > 0 and ts.dtype == np.float32
    assert np.all(ts >= 0.0) and np.all(np.isfinite(ts))
    assert np.all(np.diff(ts) >= 0)
    assert v.metadata.duration is not None
    assert float(ts[-1]) <= v.metadata.duration + 0.1
    assert v.get_major_size() == size_before + ts.nbytes

    # downloader -> fixed-stride chain: 30 s -> 3 clips (reference
    # test_downloader_then_fixed_stride_real_mp4...)
    from cosmos_curate_amd.pipelines.video.read_write.download_stages import (
        VideoDownloader,
    )

    v2 = Video(input_video=src)
    t = SplitPipeTask(videos=[v2])
    VideoDownloader(input_path=str(tmp_path)).process_data([t])
    assert "timestamps" not in v2.errors and v2.timestamps is not None
    out = run_pipeline([t], [FixedStrideExtractorStage()], runner=SequentialRunner())
    assert len(out[0].video.clips) == 3


def test_frame_creation_reextraction_passes_target_res(monkeypatch):
    """min_frames re-extraction must regenerate at the stage's target_res
    (it previously omitted it, regenerating source-resolution
    frames that failed downstream)."""
    import numpy as np

    from cosmos_curate_amd.pipelines.video.embedding import clip_stages
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        Clip,
        LazyData,
        SplitPipeTask,
        Video,
    )
    from cosmos_curate_amd.pipelines.video.utils.decoder_utils import (
        FrameExtractionPolicy,
        FrameExtractionSignature,
    )

    seen_kwargs = {}

    def fake_extract_frames(data, *, sample_rate_fps, target_res=(-1, -1), to_host=False):
        seen_kwargs["target_res"] = target_res
        return np.zeros((8, target_res[0], target_res[1], 3), dtype=np.uint8)

    monkeypatch.setattr(clip_stages, "extract_frames", fake_extract_frames)

    sig = FrameExtractionSignature(FrameExtractionPolicy.sequence, 2.0).to_str()
    few = np.zeros((2, 64, 64, 3), dtype=np.uint8)
    clip = Clip(uuid="u", source_video="s", span=(0.0, 10.0))
    clip.extracted_frames = LazyData(value={sig: few}, nbytes=few.nbytes)
    clip.encoded_data = LazyData(value=b"payload", nbytes=7)
    stage = clip_stages.ClipFrameCreationStage(
        target_fps=2.0, min_frames=8, target_res=(64, 64))
    stage.process_data([SplitPipeTask(videos=[Video(input_video="v", clips=[clip])])])
    assert seen_kwargs.get("target_res") == (64, 64)
    assert len(clip.clip_embedding_frames.resolve()) == 8


def test_vcn_slot_map_bframe_reordering():
    """The VCN path's pts->slot mapping on a B-frame-style decode order
    (decode order != presentation order), against sample_closest's
    sorted-timeline contract."""
    import numpy as np

    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        vcn_slot_map,
    )
    from cosmos_curate_amd.pipelines.video.utils.decoder_utils import sample_closest

    # decode order: I P B B P B B ... (pts ticks at 512/frame, shifted)
    pres_ticks = 1024 + 512 * np.arange(12, dtype=np.int64)
    # pts_ticks[k] = presentation tick of the k-th frame in DECODE order
    decode_order = np.array([0, 3, 1, 2, 6, 4, 5, 9, 7, 8, 11, 10])
    pts_ticks = pres_ticks[decode_order]
    # presentation-sorted seconds timeline (timescale 12288)
    ts = np.sort((pts_ticks / 12288.0).astype(np.float32))
    idx, counts, _ = sample_closest(ts, sample_rate=12288.0 / 512 / 2)

    m = vcn_slot_map(pts_ticks, idx)
    # the mapping must point each WANTED presentation position's tick at
    # its output slot, regardless of decode order
    assert len(m) == len(idx)
    for j, i in enumerate(idx):
        tick = int(round(float(ts[i]) * 12288))
        assert m[tick] == j
    # and ticks NOT sampled are absent (frames get skipped, not written)
    all_ticks = set(int(t) for t in pts_ticks)
    assert set(m).issubset(all_ticks)


def test_corrupt_clip_payload_records_error_not_crash(tmp_path):
    """A clip whose payload is truncated/corrupted mid-pipeline records a
    per-clip error (reference record-don't-raise convention) and the
    pipeline completes for the healthy clips."""
    import argparse

    from cosmos_curate_amd.core.interfaces import SequentialRunner
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _setup_parser, split
    from cosmos_curate_amd.pipelines.video.utils import raw_backend

    inp = tmp_path / "in"
    inp.mkdir()
    good = raw_backend.make_synthetic_clip(600, 32, 48, 30, seed=1)
    (inp / "good.nv12").write_bytes(good)
    # corrupt: valid magic+header but body truncated to half a frame
    bad = good[: raw_backend.HEADER_SIZE + (32 * 48 + 16 * 48) // 2]
    (inp / "bad.nv12").write_bytes(bad)
    out = tmp_path / "out"
    p = argparse.ArgumentParser()
    _setup_parser(p)
    summary = split(p.parse_args([
        "--input-video-path", str(inp), "--output-clip-path", str(out),
        "--no-embeddings",
    ]), runner=SequentialRunner())
    # the good video's 2 clips complete; the bad one errors, not raises
    assert summary["num_clips"] >= 2
    metas = list((out / "metas" / "v0").glob("*.json"))
    assert len(metas) >= 2


def test_raw_header_fuzz_never_crashes():
    """Random corruption of the raw-NV12 header is rejected or parsed
    bounded — never a crash (mirror of the mp4 fuzz discipline)."""
    import numpy as np

    from cosmos_curate_amd.pipelines.video.utils import raw_backend

    base = raw_backend.make_synthetic_clip(30, 16, 16, 30, seed=0)
    rng = np.random.default_rng(7)
    arr = bytearray(base)
    for _ in range(300):
        i = int(rng.integers(0, min(64, len(arr))))
        b = bytearray(arr)
        b[i] = int(rng.integers(0, 256))
        data = bytes(b)
        try:
            if raw_backend.is_raw_nv12(data):
                n, h, w, fps = raw_backend.parse_header(data)
                # bounded: parsing must not allocate absurd shapes before
                # validation by consumers
                assert 0 <= n < 2 ** 32 and 0 <= h < 2 ** 32
        except (AssertionError, ValueError, Exception):
            pass  # loud rejection is fine; crash/hang is not
