"""Motion-vector estimation — the first half of the motion filter.

Takes the place of the reference's ``MotionVectorDecodeStage`` /
``decode_for_motion`` (motion_vector_backend.py:169-250), which reads the
vectors an H.264 entropy decoder leaves in its side data.  No decoder on
this platform exposes that side data, so the per-block displacement field
is ESTIMATED from the luma the device path already carries: full-search
block matching between neighbouring frames on the GPU
(csrc/cc_motion.hip, ``cc_motion_estimate``).  The output has the
reference's shape — per-frame ``(n, 10)`` float32 MV arrays in a
``DecodedMotionData`` — so ``MotionFilterStage`` scores it unchanged.

Estimated vectors are not codec vectors (DESIGN.md "Motion estimation"):
every 16x16 block gets exactly one full-pel vector, zero vectors included,
and blocks tile the frame without overlap.
"""

from __future__ import annotations

import numpy as np
import numpy.typing as npt
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces.stage_interface import (
    CuratorStage,
    CuratorStageResource,
)
from cosmos_curate_amd.core.utils.performance_utils import StageTimer
from cosmos_curate_amd.pipelines.video.filtering.motion.motion_filter_stages import (
    DecodedMotionData,
)
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import SplitPipeTask

BLOCK = 16
MIN_SIDE = 256  # the per-patch-256 score needs at least one whole patch


class VideoResolutionTooSmallError(Exception):
    """Frame smaller than 256 pixels on a side (reference name)."""


def blocks_to_mv_rows(
    mv: npt.NDArray[np.int16], h: int, w: int
) -> npt.NDArray[np.float32]:
    """(nby, nbx, 2) block vectors (dx, dy) of an ``h`` x ``w`` frame ->
    (nby*nbx, 10) float32 rows in raster order, columns
    [w, h, src_x, src_y, dst_x, dst_y, flags, motion_x, motion_y,
    motion_scale]: 16x16 blocks centred on dst, src = dst + (dx, dy),
    motion in the quarter-pel units codec side data carries (scale 4)."""
    nby, nbx = -(-h // BLOCK), -(-w // BLOCK)
    if mv.shape != (nby, nbx, 2):
        msg = f"mv shape {mv.shape} does not match a {h}x{w} frame ({nby}x{nbx} blocks)"
        raise ValueError(msg)
    by, bx = np.mgrid[0:nby, 0:nbx]
    d = mv.astype(np.float32)
    out = np.zeros((nby, nbx, 10), dtype=np.float32)
    out[..., 0] = BLOCK
    out[..., 1] = BLOCK
    out[..., 4] = BLOCK * bx + BLOCK // 2
    out[..., 5] = BLOCK * by + BLOCK // 2
    out[..., 2] = out[..., 4] + d[..., 0]
    out[..., 3] = out[..., 5] + d[..., 1]
    out[..., 7] = 4.0 * d[..., 0]
    out[..., 8] = 4.0 * d[..., 1]
    out[..., 9] = 4.0
    return out.reshape(nby * nbx, 10)


def motion_sample_pairs(
    n_frames: int, fps: float, target_fps: float = 2.0,
    target_duration_ratio: float = 0.5,
) -> list[tuple[int, int]]:
    """(reference frame, current frame) index pairs to match, following
    decode_for_motion's sampling with the payload header as stream info.

    Frames i = 0, step, 2*step, ... are sampled; frame 0 contributes
    nothing (in the reference it is the keyframe, which carries no
    vectors) and each later one is matched against its immediate
    predecessor i-1, because codec vectors — and the filter's thresholds —
    measure motion per source-frame interval.  At most ``max_frames``
    pairs.
    """
    if n_frames <= 0 or fps <= 0 or target_fps <= 0:
        msg = f"bad stream info: n_frames={n_frames} fps={fps} target_fps={target_fps}"
        raise ValueError(msg)
    duration = n_frames / fps
    max_frames = max(10, round(target_fps * duration * target_duration_ratio))
    step = max(1, round(fps / target_fps))
    return [(i - 1, i) for i in range(step, n_frames, step)][:max_frames]


def estimate_clip_motion(
    data: bytes | npt.NDArray[np.uint8], *,
    target_fps: float = 2.0, target_duration_ratio: float = 0.5,
    search_range: int = 16, mv_lambda: int = 4,
) -> DecodedMotionData:
    """Raw payload (version 1 or 2) -> per-sampled-frame MV arrays.

    One host gather of the luma planes the pairs need, one upload, one
    kernel launch for all pairs on the current stream, one copy back.
    """
    n_frames, h, w, fps = raw_backend.parse_header(data)
    if h < MIN_SIDE or w < MIN_SIDE:
        msg = f"video resolution {w}x{h} is below {MIN_SIDE} on a side"
        raise VideoResolutionTooSmallError(msg)
    pairs = motion_sample_pairs(n_frames, fps, target_fps, target_duration_ratio)
    if not pairs:
        return DecodedMotionData(frames=[], frame_size=(h, w))
    depth, _, _, bps = raw_backend.parse_format(data)

    hotpath.require_gpu()
    # consecutive pairs share frames (ref of one is cur of the previous):
    # upload each frame once and let cur = ref + one frame; otherwise the
    # pairs are disjoint and are laid out ref, cur, ref, cur, ...
    if all(p[1] == q[0] for p, q in zip(pairs, pairs[1:])):
        frames = [pairs[0][0]] + [c for _, c in pairs]
        stride_frames = 1
    else:
        frames = [i for p in pairs for i in p]
        stride_frames = 2
    ys, _ = raw_backend.frame_planes(data, np.asarray(frames, dtype=np.int32))
    dev = torch.device("cuda", torch.cuda.current_device())
    y_dev = torch.from_numpy(ys.view(np.uint8)).to(dev, non_blocking=True)
    stream = torch.cuda.current_stream(dev).cuda_stream

    n = len(pairs)
    nby, nbx = -(-h // BLOCK), -(-w // BLOCK)
    plane = h * w * bps
    mv = torch.empty((n, nby, nbx, 2), dtype=torch.int16, device=dev)
    hotpath.estimate_motion(
        y_dev.data_ptr() + plane, y_dev.data_ptr(), n, h, w, w * bps,
        mv.data_ptr(), stream, frame_stride_bytes=stride_frames * plane,
        bit_depth=depth, search_range=search_range, mv_lambda=mv_lambda,
    )
    mv_host = mv.cpu().numpy()  # synchronises the stream
    return DecodedMotionData(
        frames=[blocks_to_mv_rows(m, h, w) for m in mv_host], frame_size=(h, w)
    )


class MotionVectorEstimationStage(CuratorStage):
    """Role and error vocabulary of the reference MotionVectorDecodeStage
    (motion_filter_stages.py:40-125): fills ``clip.decoded_motion_data``
    for ``MotionFilterStage``; failures are per-clip ``errors`` entries and
    the clip stays in ``video.clips``."""

    def __init__(
        self,
        num_cpus_per_worker: float = 1.0,
        *,
        verbose: bool = False,
        log_stats: bool = False,
        target_fps: float = 2.0,
        target_duration_ratio: float = 0.5,
        search_range: int = 16,
        mv_lambda: int = 4,
        num_gpus_per_worker: float = 0.25,
    ) -> None:
        self._timer = StageTimer(self)
        self._num_cpus = num_cpus_per_worker
        self._num_gpus = num_gpus_per_worker
        self._verbose = verbose
        self._log_stats = log_stats
        self._target_fps = target_fps
        self._target_duration_ratio = target_duration_ratio
        self._search_range = search_range
        self._mv_lambda = mv_lambda

    @property
    def resources(self) -> CuratorStageResource:
        return CuratorStageResource(cpus=self._num_cpus, gpus=self._num_gpus)

    def _process_clip(self, clip) -> None:
        data = clip.encoded_data.resolve()
        if data is None:
            clip.errors["encoded_data"] = "empty"
            return
        # the two header-only outcomes are decided before the GPU is touched
        if not raw_backend.is_raw_nv12(data):
            # mp4 needs a decode session to get at the luma (DESIGN.md
            # "Motion estimation", follow-up)
            clip.errors["motion_decode"] = "decode_unavailable"
            return
        try:
            clip.decoded_motion_data = estimate_clip_motion(
                data,
                target_fps=self._target_fps,
                target_duration_ratio=self._target_duration_ratio,
                search_range=self._search_range,
                mv_lambda=self._mv_lambda,
            )
        except VideoResolutionTooSmallError:
            clip.errors["motion_decode"] = "resolution_too_small"
            return
        except Exception as e:  # per-clip error convention
            if self._verbose:
                print(f"[{type(self).__name__}] clip {clip.uuid}: {e}")
            clip.decoded_motion_data = None
            clip.errors["motion_decode"] = "decode_failed"
            return
        if not clip.decoded_motion_data.frames:
            clip.decoded_motion_data = None
            clip.errors["motion_decode"] = "no_motion_frames"

    def process_data(self, tasks: list[SplitPipeTask]) -> list[SplitPipeTask] | None:
        for task in tasks:
            self._timer.reinit(self, task.get_major_size())
            with self._timer.time_process():
                for video in task.videos:
                    for clip in video.clips:
                        self._process_clip(clip)
            if self._log_stats:
                name, stats = self._timer.log_stats()
                task.stage_perf[name] = stats
        return tasks
