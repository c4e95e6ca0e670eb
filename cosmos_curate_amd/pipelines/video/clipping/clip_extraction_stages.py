"""Fixed-stride clip extraction.

Mirror of /root/reference/cosmos_curate/pipelines/video/clipping/
clip_extraction_stages.py, hot-path subset:
- ``_make_spans_fixed_stride``      (:512-551)
- ``_make_clip_uuids``              (:554-565)  uuid5 contract
- ``_populate_clips_fixed_stride``  (:568-661)
- ``FixedStrideExtractorStage``     (:664-744)  same constructor signature,
  defaults (10 s len/stride/min, limit 0) and resources (1 CPU).

Bit-exact span + UUID parity vs oracle/spans.py is pinned in
tests/test_product_vs_oracle.py; golden expectations in
tests/golden/spans_kats.json.
Also here (same module as upstream):
- ``slice_video_clips`` / ``chunk_tasks``  (:42-164)  fan-out of transcoded
  clips into <=num_clips_per_chunk*8 subtasks (the task-count change point,
  SURVEY.md appendix);
- ``ClipTranscodingStage``  (:167-441)  per-clip source -> standalone clip
  payloads.  The reference shells out to ffmpeg (libopenh264/h264_nvenc)
  to RE-ENCODE each span; no encoder library exists in this image, so the
  rebuild extracts clips by STREAM COPY: raw-NV12 payloads are sliced
  frame-exact; H.264 mp4 spans are remuxed sample-exact via the in-repo
  demuxer+writer when the span starts on a sync sample (else a per-clip
  error is recorded - loud, no silent re-encode).  Clip boundaries and
  frame indices — the bit-exact contracts — are
  preserved exactly; re-encoding is a rate-control concern the hot path
  does not need.
"""

from __future__ import annotations

import copy
import math
import uuid

import numpy as np

from cosmos_curate_amd.core.interfaces.stage_interface import (
    CuratorStage,
    CuratorStageResource,
)
from cosmos_curate_amd.core.utils.lazy_data import LazyData
from cosmos_curate_amd.core.utils.performance_utils import StageTimer
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import (
    Clip,
    SplitPipeTask,
    Video,
)


def _make_spans_fixed_stride(
    start_s: float,
    end_s: float,
    clip_len_s: float,
    clip_stride_s: float,
    min_clip_length_s: float,
) -> list[tuple[float, float]]:
    """Fixed-stride spans (clip_extraction_stages.py:512-551)."""
    spans: list[tuple[float, float]] = []
    pos = start_s
    while pos < end_s:
        end = min(pos + clip_len_s, end_s)
        if (end - pos) >= min_clip_length_s:
            spans.append((pos, end))
        pos += clip_stride_s
    return spans


def _make_clip_uuids(session_id: str, spans: list[tuple[float, float]]) -> list[uuid.UUID]:
    """uuid5(NAMESPACE_URL, f"{session}_{s}_{e}") (clip_extraction_stages.py:554-565)."""
    return [uuid.uuid5(uuid.NAMESPACE_URL, f"{session_id}_{s}_{e}") for (s, e) in spans]


def _get_videos_durations(videos: list[Video]) -> list[float]:
    """num_frames/framerate duration convention (clip_extraction_stages.py:486-509)."""

    def one(v: Video) -> float:
        nf, fr = v.metadata.num_frames, v.metadata.framerate
        if nf is None or fr is None or fr <= 0:
            return -1.0
        return float(nf / fr)

    return [one(v) for v in videos]


def _populate_clips_fixed_stride(
    videos: list[Video],
    session_id: str,
    clip_len_s: float,
    clip_stride_s: float,
    min_clip_length_s: float,
    *,
    limit_clips: int = 0,
) -> None:
    """Populate video.clips in place (clip_extraction_stages.py:568-661).

    Preserves the reference's start=0 convention: spans run over
    [0, min(durations)) regardless of first-PTS offset (:633-635).
    """
    durations = _get_videos_durations(videos)
    if any(d <= 0 for d in durations):
        msg = "Some videos have invalid (zero or negative) duration"
        raise ValueError(msg)
    for v in videos:
        if v.timestamps is None or len(v.timestamps) == 0:
            msg = f"Video {v.input_path} has no timestamps"
            raise ValueError(msg)
    end_s = min(durations)
    spans = _make_spans_fixed_stride(0.0, end_s, clip_len_s, clip_stride_s, min_clip_length_s)
    if limit_clips > 0:
        spans = spans[:limit_clips]
    clip_uuids = _make_clip_uuids(session_id, spans)
    for span, cu in zip(spans, clip_uuids):
        for video in videos:
            video.clips.append(
                Clip(uuid=cu, source_video=str(video.input_video), span=span)
            )


class FixedStrideExtractorStage(CuratorStage):
    """clip_extraction_stages.py:664-744: split videos into fixed clips."""

    def __init__(
        self,
        clip_len_s: float = 10,
        clip_stride_s: float = 10,
        min_clip_length_s: float = 10,
        limit_clips: int = 0,
        *,
        verbose: bool = False,
        log_stats: bool = False,
    ) -> None:
        self._timer = StageTimer(self)
        self.clip_len_s = clip_len_s
        self.clip_stride_s = clip_stride_s
        self.min_clip_length_s = min_clip_length_s
        self._limit_clips = limit_clips
        self._verbose = verbose
        self._log_stats = log_stats

    @property
    def resources(self) -> CuratorStageResource:
        return CuratorStageResource(cpus=1.0)

    def process_data(self, tasks: list[SplitPipeTask]) -> list[SplitPipeTask] | None:
        for task in tasks:
            self._timer.reinit(self, task.get_major_size())
            with self._timer.time_process():
                try:
                    session_id = task.session_id or task.video.input_path
                    _populate_clips_fixed_stride(
                        task.videos,
                        session_id,
                        self.clip_len_s,
                        self.clip_stride_s,
                        self.min_clip_length_s,
                        limit_clips=self._limit_clips,
                    )
                except Exception as e:  # per-item error convention (§8b)
                    for video in task.videos:
                        video.errors[type(self).__name__] = str(e)
            if self._log_stats:
                name, stats = self._timer.log_stats()
                task.stage_perf[name] = stats
        return tasks


def slice_video_clips(
    video: Video, start: int, end: int, chunk_index: int, num_chunks: int
) -> Video:
    """New Video carrying clips[start:end] (clip_extraction_stages.py:42-89)."""
    if end < start:
        msg = f"End index {end} is less than start index {start}"
        raise ValueError(msg)
    if start < 0 or end > len(video.clips):
        msg = f"Invalid slice [{start}:{end}] for {len(video.clips)} clips"
        raise ValueError(msg)
    sliced = copy.copy(video)
    sliced.clips = video.clips[start:end]
    sliced.filtered_clips = []
    sliced.num_total_clips = len(video.clips)
    sliced.num_clip_chunks = num_chunks
    sliced.clip_chunk_index = chunk_index
    return sliced


def chunk_tasks(
    tasks: list[SplitPipeTask], num_clips_per_chunk: int, *, verbose: bool = False
) -> list[SplitPipeTask]:
    """Fan each task out into contiguous clip-index chunks (:92-164).

    Chunk size = num_clips_per_chunk * 8 clips (the reference groups by
    clip count through grouping.split_by_chunk_size with that bound).
    """
    if num_clips_per_chunk <= 0:
        msg = f"num_clips_per_chunk must be positive, got {num_clips_per_chunk}"
        raise ValueError(msg)
    per_chunk = num_clips_per_chunk * 8
    out: list[SplitPipeTask] = []
    for task in tasks:
        primary = task.videos[0].clips
        num_chunks = max(1, math.ceil(len(primary) / per_chunk))
        start = 0
        for idx in range(num_chunks):
            end = min(start + per_chunk, len(primary))
            videos = [slice_video_clips(v, start, end, idx, num_chunks) for v in task.videos]
            sub = SplitPipeTask(
                session_id=task.session_id,
                videos=videos,
                stage_perf=copy.deepcopy(task.stage_perf) if idx == 0 else {},
            )
            out.append(sub)
            start = end
    # multicam chunking must preserve time alignment (reference :163)
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        assert_time_alignment,
    )

    assert_time_alignment(out)
    return out


def _slice_raw_clip(raw: bytes | np.ndarray, span: tuple[float, float]) -> np.ndarray:
    """Frame-exact raw NV12/P016 span slice: frames with i/fps in [start, end).

    Zero-copy when the span covers the whole source; otherwise one
    header+body concatenation (frames are contiguous in the payload), no
    per-frame gather — raw payloads are ~93 MB per second of video, so
    every avoided pass shows up in the driver-level throughput
    (profiles/r02_driver_bench.log vs r01's 5.3 s transcode stage).
    """
    n, h, w, fps = raw_backend.parse_header(raw)
    first = int(math.ceil(span[0] * fps - 1e-6))
    last = int(math.ceil(span[1] * fps - 1e-6))  # exclusive
    first = max(0, min(first, n))
    last = max(first, min(last, n))
    buf = np.frombuffer(raw, dtype=np.uint8)
    if first == 0 and last == n:
        return buf  # span covers the whole source: zero-copy payload
    fsz = raw_backend.frame_nbytes(raw)
    num = int(round(fps))
    depth, matrix, full_range, _ = raw_backend.parse_format(raw)
    hdr = raw_backend.pack_header(last - first, h, w, num, 1, bit_depth=depth,
                                  matrix=matrix, full_range=full_range,
                                  transfer=raw_backend.parse_transfer(raw))
    body = buf[raw_backend.HEADER_SIZE + first * fsz:
               raw_backend.HEADER_SIZE + last * fsz]
    return np.concatenate([np.frombuffer(hdr, dtype=np.uint8), body])


def _remux_mp4_clip(raw: bytes, span: tuple[float, float]) -> bytes:
    """Sample-exact H.264 mp4 span remux (cc_demux_remux_clip).

    Requires the span's first sample to be a sync sample; otherwise the
    library fails with CC_ERR_UNSUPPORTED (recorded per clip upstream) —
    no silent re-encode.
    """
    from cosmos_curate_amd import hotpath

    with hotpath.Demuxer(raw) as d:
        return d.remux_clip(span[0], span[1])


class ClipTranscodingStage(CuratorStage):
    """Per-clip payload extraction (clip_extraction_stages.py:167-311).

    Keeps the reference constructor surface; `encoder` names are accepted
    for compatibility but the rebuild stream-copies (module docstring).
    Fans tasks out through chunk_tasks afterwards, exactly like the
    reference (:301).
    """

    def __init__(
        self,
        num_cpus_per_worker: float = 6.0,
        encoder: str = "libopenh264",
        encoder_threads: int = 1,
        encode_batch_size: int = 16,
        nb_streams_per_gpu: int = 3,
        num_clips_per_chunk: int = 32,
        *,
        use_hwaccel: bool = False,
        use_input_bit_rate: bool = False,
        verbose: bool = False,
        log_stats: bool = False,
    ) -> None:
        if encoder not in {"libopenh264", "h264_nvenc", "copy"}:
            msg = f"Expected encoder of `libopenh264`, `h264_nvenc` or `copy`. Got {encoder}"
            raise ValueError(msg)
        self._timer = StageTimer(self)
        self._num_cpus_per_worker = num_cpus_per_worker
        self._encoder = encoder
        self._encoder_threads = encoder_threads
        self._encode_batch_size = encode_batch_size
        self._num_clips_per_chunk = num_clips_per_chunk
        self._verbose = verbose
        self._log_stats = log_stats

    @property
    def resources(self) -> CuratorStageResource:
        return CuratorStageResource(cpus=self._num_cpus_per_worker)

    def _process_video(self, video: Video) -> None:
        data = video.encoded_data.resolve()
        if data is None:
            video.errors["transcode"] = "no encoded data"
            return
        is_raw = raw_backend.is_raw_nv12(data)
        video.was_remuxed = not is_raw  # mp4 spans get new containers
        # raw payloads stay numpy end to end (no bytes() copy of the
        # ~GB source); mp4 payloads (real-codec sized) go through the
        # demuxer, which wants bytes
        mp4_bytes = None if is_raw else (
            data if isinstance(data, bytes) else bytes(data))
        for clip in video.clips:
            try:
                payload = (_slice_raw_clip(data, clip.span) if is_raw
                           else _remux_mp4_clip(mp4_bytes, clip.span))
                arr = np.frombuffer(payload, dtype=np.uint8)
                clip.encoded_data = LazyData(value=arr, nbytes=arr.nbytes)
                video.clip_stats.num_transcoded += 1
            except Exception as e:
                clip.errors["transcode"] = str(e) or type(e).__name__

    def process_data(self, tasks: list[SplitPipeTask]) -> list[SplitPipeTask] | None:
        for task in tasks:
            self._timer.reinit(self, task.get_major_size())
            for video in task.videos:
                with self._timer.time_process():
                    try:
                        self._process_video(video)
                        # source bytes no longer needed once clips carry their own
                        video.encoded_data.drop()
                    except Exception as e:
                        video.errors[type(self).__name__] = str(e)
            if self._log_stats:
                name, stats = self._timer.log_stats()
                task.stage_perf[name] = stats
        return chunk_tasks(tasks, self._num_clips_per_chunk, verbose=self._verbose)
