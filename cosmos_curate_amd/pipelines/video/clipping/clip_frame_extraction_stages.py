"""Per-clip GPU frame extraction — the heart of the rebuilt hot path.

Mirror of /root/reference/cosmos_curate/pipelines/video/clipping/
clip_frame_extraction_stages.py:43-192 (``ClipFrameExtractionStage``: same
constructor signature and defaults — policies=(sequence,), target_fps=[2],
target_res=(-1,-1), 3 CPUs — same LCM-of-fps decode trick :116-137, same
``clip.extracted_frames[signature]`` output contract :157, same per-clip
error convention :160-165), with the decode/resize pipeline replaced by the
MI355X path:

    demux (cc_demux_* / null-raw header)             [host]
    sample_closest on PTS                            [host, §8 row a2]
    NV12 surfaces -> HBM (rocDecode | raw upload)    [device]
    fused YUV->RGB + bilinear resize kernel          [device, §2b rows 3-5]
      (cc_yuv420sp_to_rgb_resize for every depth and colour standard;
       8-bit BT.601 limited gives the bits of cc_nv12_to_rgb_resize;
       cc_yuv420sp_hdr_to_rgb_resize for PQ clips under hdr="tonemap")
    duplicate-count broadcast (cc_gather_frames_u8)  [device]

Output frames live on DEVICE as torch uint8 NHWC tensors keyed by
``FrameExtractionSignature.to_str()`` — mirroring the reference's GPU
route, where PyNvcFrameExtractor hands downstream stages torch cuda
tensors (nvcodec_utils.py:313-380).  ``to_host=True`` gives the CPU-path
numpy payloads instead.

No CPU decode fallback: an mp4 clip without rocDecode records
``errors["frame_extraction"] = "decode_unavailable"`` (reference records
``video_decode_failed`` on its own decode errors, :162).
"""

from __future__ import annotations

import ctypes
import math
from functools import reduce

import numpy as np
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces.stage_interface import (
    CuratorStage,
    CuratorStageResource,
)
from cosmos_curate_amd.core.utils.lazy_data import LazyData
from cosmos_curate_amd.core.utils.performance_utils import StageTimer
from cosmos_curate_amd.core.utils.roctx import annotate
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import SplitPipeTask, Video
from cosmos_curate_amd.pipelines.video.utils.decoder_utils import (
    FrameExtractionPolicy,
    FrameExtractionSignature,
    sample_closest,
)


# color_standard -> conversion-kernel matrix code (cc_yuv420sp_to_rgb*)
_FORCED_MATRIX = {"bt601": 0, "bt709": 1, "bt2020": 2}
# H.273 matrix_coefficients -> kernel matrix code; everything else
# (unspecified = 2 included) converts as BT.601
_H273_MATRIX = {1: 1, 5: 0, 6: 0, 9: 2}
_H273_TRANSFER_PQ = 16  # SMPTE ST 2084
# colour_primaries under which a PQ stream is tone-mapped: BT.2020, or
# nothing signalled (0 reserved, 2 unspecified) — BT.2100 content
_H273_PQ_PRIMARIES = (0, 2, 9)
_HDR_MODES = ("off", "tonemap")


class ClipFrameExtractionStage(CuratorStage):
    """clip_frame_extraction_stages.py:43-192, GPU-native inside.

    ``color_standard`` picks the YUV->RGB matrix: ``"bt601"`` (default;
    BT.601 limited range for every input, what the reference's fixed
    cvcuda conversion does), ``"bt709"`` / ``"bt2020"`` (that matrix,
    limited range), or ``"stream"`` (matrix and range the clip signals:
    the decoder's sequence header, or the raw payload's header).

    ``hdr`` says what to do with clips that signal the PQ transfer function
    (HDR10): ``"off"`` (default) converts them like any other clip,
    ``"tonemap"`` maps them to SDR BT.709 in the same kernel (inverse PQ,
    BT.2020 -> BT.709, extended Reinhard up to ``hdr_peak_nits`` with
    diffuse white at ``hdr_reference_white_nits``, display gamma 2.4).
    Their matrix and range are then the ones the clip signals, whatever
    ``color_standard`` says, and BT.2020-NCL when it signals none.  Every
    other clip takes the same call as under ``"off"``.
    """

    def __init__(
        self,
        extraction_policies: tuple[FrameExtractionPolicy, ...] = (
            FrameExtractionPolicy.sequence,
        ),
        target_fps: list[float | int] | None = None,
        target_res: tuple[int, int] | None = None,
        *,
        num_cpus_per_worker: float = 3.0,
        verbose: bool = False,
        log_stats: bool = False,
        to_host: bool = False,
        color_standard: str = "bt601",
        hdr: str = "off",
        hdr_peak_nits: float = 1000.0,
        hdr_reference_white_nits: float = 203.0,
    ) -> None:
        if color_standard != "stream" and color_standard not in _FORCED_MATRIX:
            msg = (f"color_standard must be one of bt601, bt709, bt2020, "
                   f"stream; got {color_standard!r}")
            raise ValueError(msg)
        if hdr not in _HDR_MODES:
            msg = f"hdr must be one of off, tonemap; got {hdr!r}"
            raise ValueError(msg)
        for name, nits in (("hdr_peak_nits", hdr_peak_nits),
                           ("hdr_reference_white_nits", hdr_reference_white_nits)):
            if isinstance(nits, bool) or not isinstance(nits, (int, float)) \
                    or not math.isfinite(nits) or nits <= 0:
                msg = f"{name} must be a positive finite number; got {nits!r}"
                raise ValueError(msg)
        if hdr_peak_nits < hdr_reference_white_nits:
            msg = (f"hdr_peak_nits ({hdr_peak_nits}) must not be below "
                   f"hdr_reference_white_nits ({hdr_reference_white_nits})")
            raise ValueError(msg)
        if target_fps is None:
            target_fps = [2]
        if target_res is None:
            target_res = (-1, -1)
        self._timer = StageTimer(self)
        self._extraction_policies = extraction_policies
        self._target_fps = target_fps
        self._target_res = target_res
        self._num_cpus = num_cpus_per_worker
        self._verbose = verbose
        self._log_stats = log_stats
        self._to_host = to_host
        self._color_standard = color_standard
        self._hdr = hdr
        self._hdr_peak_nits = float(hdr_peak_nits)
        self._hdr_white_nits = float(hdr_reference_white_nits)

    @property
    def resources(self) -> CuratorStageResource:
        return CuratorStageResource(cpus=self._num_cpus, gpus=0.5)

    def lcm_multiple(self, fps: list[float | int]) -> float | int:
        """LCM of fps targets (clip_frame_extraction_stages.py:94-100)."""

        def lcm(a, b):
            return abs(a * b) // math.gcd(int(a), int(b))

        return reduce(lcm, fps)

    def _color(self, matrix: int, full_range: bool) -> tuple[int, bool]:
        """(kernel matrix code, full_range) to convert with, given what the
        clip signals (already as a kernel matrix code)."""
        if self._color_standard == "stream":
            return matrix, full_range
        return _FORCED_MATRIX[self._color_standard], False

    def _convert_resize(
        self, y: int, uv: int, n: int, src_h: int, src_w: int, pitch: int,
        out_rgb: int, out_h: int, out_w: int, stream: int, *,
        bit_depth: int, matrix: int, full_range: bool, pq: bool,
    ) -> None:
        """The one conversion launch of both routes: the tone-mapping entry
        for a PQ clip under ``hdr="tonemap"`` (``pq``), else the SDR one."""
        if not pq:
            hotpath.yuv_to_rgb_resize(
                y, uv, n, src_h, src_w, pitch, out_rgb, out_h, out_w, stream,
                bit_depth=bit_depth, matrix=matrix, full_range=full_range,
            )
            return
        tables = hotpath.hdr_tables(hotpath.HDR_TRANSFER_PQ, self._hdr_white_nits)
        hotpath.yuv_hdr_to_rgb_resize(
            y, uv, n, src_h, src_w, pitch, out_rgb, out_h, out_w, stream,
            tables=tables.data_ptr(),
            inv_w2=hotpath.hdr_inv_w2(self._hdr_peak_nits, self._hdr_white_nits),
            bit_depth=bit_depth, matrix=matrix, full_range=full_range,
        )

    # ---- device pipeline -------------------------------------------------
    def _extract_clip_frames(
        self, data: bytes, sample_rate_fps: float
    ) -> torch.Tensor:
        """Decode+sample+resize one clip -> (T, th, tw, 3) u8 device tensor."""
        lib = hotpath.require_gpu()
        if raw_backend.is_raw_nv12(data):
            ts = raw_backend.timestamps(data)
            n_frames, src_h, src_w, _ = raw_backend.parse_header(data)
            depth, sig_matrix, sig_full, bps = raw_backend.parse_format(data)
            pq = (self._hdr == "tonemap"
                  and raw_backend.parse_transfer(data) == raw_backend.TRANSFER_PQ)
            if pq:  # BT.2100 content: the signalled matrix, never a forced one
                matrix, full_range = sig_matrix, sig_full
            else:
                matrix, full_range = self._color(sig_matrix, sig_full)
        else:
            rc = lib.cc_rocdecode_available()
            if rc != 0:
                raise RuntimeError("decode_unavailable")
            return self._extract_clip_frames_vcn(data, sample_rate_fps)

        idx, counts, _ = sample_closest(ts, sample_rate=sample_rate_fps)
        th, tw = self._target_res
        if th <= 0 or tw <= 0:
            th, tw = src_h, src_w

        # host gather of the unique selected NV12/P016 frames, then one h2d
        ys, uvs = raw_backend.frame_planes(data, idx)
        dev = torch.device("cuda")
        # uploaded as bytes: P016 planes are u16, the kernels take pointers
        y_dev = torch.from_numpy(ys.view(np.uint8)).to(dev, non_blocking=True)
        uv_dev = torch.from_numpy(uvs.view(np.uint8)).to(dev, non_blocking=True)
        stream = torch.cuda.current_stream(dev).cuda_stream

        n_sel = len(idx)
        rgb = torch.empty((n_sel, th, tw, 3), dtype=torch.uint8, device=dev)
        self._convert_resize(
            y_dev.data_ptr(), uv_dev.data_ptr(), n_sel, src_h, src_w,
            src_w * bps, rgb.data_ptr(), th, tw, stream,
            bit_depth=depth, matrix=matrix, full_range=full_range, pq=pq,
        )
        total = int(counts.sum())
        if total == n_sel and np.all(counts == 1):
            return rgb
        out = torch.empty((total, th, tw, 3), dtype=torch.uint8, device=dev)
        # after host gather the selected frames are 0..n_sel-1 in order
        local_idx = np.arange(n_sel, dtype=np.int32)
        hotpath.check(
            lib.cc_gather_frames_u8(
                rgb.data_ptr(), n_sel, th * tw * 3,
                local_idx.ctypes.data_as(ctypes.c_void_p),
                counts.ctypes.data_as(ctypes.c_void_p),
                n_sel, total, out.data_ptr(), stream,
            )
        )
        return out

    def _extract_clip_frames_vcn(
        self, data: bytes, sample_rate_fps: float
    ) -> torch.Tensor:
        """mp4 clip -> frames via the VCN/rocDecode session
        (csrc/cc_decode.cpp; NvVideoDecoder flow, nvcodec_utils.py:199-313).

        Packets are fed in decode order; mapped display-order surfaces
        whose pts matches a sampled frame are converted straight from the
        decoder's surface pool with the fused NV12->RGB(+resize) kernel,
        then recycled after a stream synchronize (the surfaces are reused
        by the VCN once marked).  Selection math is sample_closest on the
        demuxer's PTS — identical to the raw-NV12 path (§8 row a2).
        """
        lib = hotpath.require_gpu()
        if not isinstance(data, bytes):
            data = bytes(data)  # demuxer ABI wants bytes; mp4 payloads are small
        d = hotpath.Demuxer(data)
        try:
            info = d.probe()
            ts = d.timestamps()
            idx, counts, _ = sample_closest(ts, sample_rate=sample_rate_fps)
            th, tw = self._target_res
            # decode-order walk collecting each sample's pts tick, so the
            # display-order mapping below can match pts -> sample index
            n_samples = info.num_samples
            pts_ticks = np.empty(n_samples, dtype=np.int64)
            pkts: list[bytes] = []
            for s in range(n_samples):
                pkt, tick, _ = d.packet(s)
                pkts.append(pkt)
                pts_ticks[s] = tick
            # sampled presentation indices -> wanted pts ticks -> slots
            slot_by_tick = vcn_slot_map(pts_ticks, idx)

            dev = torch.device("cuda")
            stream = torch.cuda.current_stream(dev).cuda_stream
            n_sel = len(idx)
            rgb: torch.Tensor | None = None
            filled = np.zeros(n_sel, dtype=bool)
            sess = hotpath.DecodeSession(0, int(info.codec))
            try:
                def drain() -> None:
                    nonlocal rgb
                    frames = sess.map_frames()
                    if not frames:
                        return
                    # one query per batch of mapped frames, not per stream:
                    # a mid-stream bit-depth change recreates the decoder
                    # (NV12 <-> P016) only between batches, so every frame
                    # of this batch has this format
                    fmt = sess.stream_format()
                    pq = False
                    if self._hdr == "tonemap":
                        transfer, primaries = sess.stream_transfer()
                        pq = (transfer == _H273_TRANSFER_PQ
                              and primaries in _H273_PQ_PRIMARIES)
                    if pq:
                        # the stream's own matrix and range; PQ with none
                        # signalled is BT.2100: BT.2020-NCL
                        matrix = _H273_MATRIX.get(int(fmt.matrix_coefficients), 2)
                        full_range = bool(fmt.full_range)
                    else:
                        matrix, full_range = self._color(
                            _H273_MATRIX.get(int(fmt.matrix_coefficients), 0),
                            bool(fmt.full_range))
                    launched = False
                    for f in frames:
                        slot = slot_by_tick.get(int(f.pts))
                        if slot is None:
                            continue
                        fh, fw = int(f.height), int(f.width)
                        oh, ow = (th, tw) if th > 0 and tw > 0 else (fh, fw)
                        if rgb is None:
                            rgb = torch.empty((n_sel, oh, ow, 3),
                                              dtype=torch.uint8, device=dev)
                        elif rgb.shape[1:3] != (oh, ow):
                            # mid-stream resolution change with no target
                            # resolution: no consistent output shape exists
                            msg = (f"mid-clip resolution change "
                                   f"{tuple(rgb.shape[1:3])} -> {(oh, ow)} "
                                   "with target_res unset")
                            raise RuntimeError(msg)
                        self._convert_resize(
                            f.y, f.uv, 1, fh, fw, f.pitch,
                            rgb[slot].data_ptr(), oh, ow, stream,
                            bit_depth=int(fmt.bit_depth), matrix=matrix,
                            full_range=full_range, pq=pq,
                        )
                        filled[slot] = True
                        launched = True
                    if launched:
                        torch.cuda.current_stream(dev).synchronize()
                    sess.recycle()

                for s in range(n_samples):
                    sess.submit(pkts[s], int(pts_ticks[s]))
                    drain()
                sess.submit(None)  # flush
                drain()
            finally:
                sess.close()
        finally:
            d.close()
        if rgb is None or not filled.all():
            # a dropped/duplicate-pts frame would otherwise leave an
            # UNINITIALIZED slot in the output — fail loudly instead
            missing = int(n_sel - int(filled.sum()))
            msg = f"decoder did not produce {missing}/{n_sel} sampled frames"
            raise RuntimeError(msg)
        total = int(counts.sum())
        if total == n_sel and np.all(counts == 1):
            return rgb
        oh, ow = rgb.shape[1], rgb.shape[2]
        out = torch.empty((total, oh, ow, 3), dtype=torch.uint8, device=dev)
        local_idx = np.arange(n_sel, dtype=np.int32)
        hotpath.check(
            lib.cc_gather_frames_u8(
                rgb.data_ptr(), n_sel, oh * ow * 3,
                local_idx.ctypes.data_as(ctypes.c_void_p),
                counts.ctypes.data_as(ctypes.c_void_p),
                n_sel, total, out.data_ptr(), stream,
            )
        )
        return out

    def _process_video(self, video: Video) -> None:
        for clip in video.clips:
            data = clip.encoded_data.resolve()
            if data is None:
                clip.errors["encoded_data"] = "empty"
                continue
            # raw payloads stay numpy (raw_backend consumes any buffer);
            # the VCN path converts to bytes itself for the demuxer
            raw = data
            try:
                local_frames: dict[str, torch.Tensor | np.ndarray] = {}
                for policy in self._extraction_policies:
                    use_lcm = len(self._target_fps) > 1 and all(
                        (f.is_integer() if isinstance(f, float) else isinstance(f, int))
                        for f in self._target_fps
                    )
                    if use_lcm:
                        lcm = self.lcm_multiple(self._target_fps)
                        frames = self._extract_clip_frames(raw, float(lcm))
                        for fps in self._target_fps:
                            sig = FrameExtractionSignature(policy, fps).to_str()
                            local_frames[sig] = frames[:: int(lcm / fps)]
                    else:
                        for fps in self._target_fps:
                            frames = self._extract_clip_frames(raw, float(fps))
                            sig = FrameExtractionSignature(policy, fps).to_str()
                            local_frames[sig] = frames
                if self._to_host:
                    local_frames = {
                        k: v.cpu().numpy() for k, v in local_frames.items()
                    }
                nbytes = sum(
                    (v.nbytes if isinstance(v, np.ndarray) else v.numel())
                    for v in local_frames.values()
                )
                clip.extracted_frames = LazyData(value=local_frames, nbytes=nbytes)
            except Exception as e:  # per-clip error convention (:160-165)
                clip.errors["frame_extraction"] = (
                    "decode_unavailable"
                    if "decode_unavailable" in str(e)
                    else "video_decode_failed"
                )
                clip.encoded_data.drop()
                continue

    @annotate("ClipFrameExtractionStage")  # reference: nvtx, clip_frame_extraction_stages.py:167
    def process_data(self, tasks: list[SplitPipeTask]) -> list[SplitPipeTask] | None:
        for task in tasks:
            self._timer.reinit(self, task.get_major_size())
            for video in task.videos:
                with self._timer.time_process():
                    try:
                        self._process_video(video)
                    except Exception as e:
                        video.errors[type(self).__name__] = str(e)
            if self._log_stats:
                name, stats = self._timer.log_stats()
                task.stage_perf[name] = stats
        return tasks


def vcn_slot_map(pts_ticks: "np.ndarray", sampled_idx: "np.ndarray") -> dict[int, int]:
    """Map pts tick -> output slot for sampled PRESENTATION indices.

    ``pts_ticks`` are per-sample pts in DECODE order (cc_demux_packet
    walk); ``sampled_idx`` indexes the SORTED presentation timeline
    (sample_closest's contract over get_video_timestamps).  The VCN
    session emits frames in display order tagged with their pts, so the
    lookup key is the tick value itself.  Pure function, unit-tested
    against B-frame-style reorderings (test_stages_cpu)."""
    order = np.argsort(pts_ticks, kind="stable")  # presentation order
    return {int(pts_ticks[order[i]]): j for j, i in enumerate(sampled_idx)}


def extract_frames(
    data: bytes,
    *,
    sample_rate_fps: float,
    target_res: tuple[int, int] = (-1, -1),
    to_host: bool = False,
    hdr: str = "off",
    hdr_peak_nits: float = 1000.0,
    hdr_reference_white_nits: float = 203.0,
) -> "torch.Tensor | np.ndarray":
    """One-off frame extraction (reference decoder_utils.extract_frames
    shape, used by the embedding stage's doubling-fps re-extraction,
    internvideo2_stages.py:157-175)."""
    stage = ClipFrameExtractionStage(
        target_res=target_res, to_host=to_host, hdr=hdr,
        hdr_peak_nits=hdr_peak_nits,
        hdr_reference_white_nits=hdr_reference_white_nits)
    frames = stage._extract_clip_frames(data, float(sample_rate_fps))
    return frames.cpu().numpy() if to_host else frames
