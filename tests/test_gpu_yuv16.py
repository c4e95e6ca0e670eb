"""cc_yuv420sp_to_rgb / cc_yuv420sp_to_rgb_resize on the MI355X: bit-exact
against tests/yuv_ref.py over depth x matrix x range, at the shapes where
the kernel changes path (scalar-only, vector body + row tail, pure vector
body), plus the stages that route 10/12-bit payloads through them.

Every rejected call below returns before any launch; nothing here hands a
kernel a bad pointer or size.
"""

from __future__ import annotations

import pathlib
import uuid

import numpy as np
import pytest
import torch

import yuv_ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from oracle import color as ocolor
from oracle import sampling as osampling

pytestmark = pytest.mark.gpu

# (n, h, w, pitch in bytes at 16 bit); depth 8 halves the pitch
SHAPES = [
    (2, 6, 10, 20),     # tail only; rows not 16-byte aligned -> scalar kernel
    (1, 34, 66, 256),   # vector body + 2-pixel row tail, padded rows
    (3, 16, 64, 128),   # pure vector body, several frames
]
GRID = [(d, m, r) for d in yuv_ref.DEPTHS for m in yuv_ref.MATRICES for r in (0, 1)]


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def _dev(arr: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8)).cuda()


def rand_planes(rng, n, h, w, depth):
    """Random samples over the full code range (junk low bits included)."""
    if depth == 8:
        return (rng.integers(0, 256, size=(n, h, w), dtype=np.uint8),
                rng.integers(0, 256, size=(n, h // 2, w), dtype=np.uint8))
    return (rng.integers(0, 1 << 16, size=(n, h, w), dtype=np.uint16),
            rng.integers(0, 1 << 16, size=(n, h // 2, w), dtype=np.uint16))


def pitched(plane: np.ndarray, pitch_bytes: int) -> np.ndarray:
    """(n, rows, w) samples -> the same rows laid out with `pitch_bytes`
    stride, padding filled with 0xA5 so a stray read would show."""
    n, rows, w = plane.shape
    per = pitch_bytes // plane.itemsize
    buf = np.full((n, rows, per), 0xA5A5 if plane.itemsize == 2 else 0xA5,
                  dtype=plane.dtype)
    buf[:, :, :w] = plane
    return buf


def convert(lib, y, uv, pitch_bytes, depth, matrix, full_range):
    n, h, w = y.shape
    yd, uvd = _dev(pitched(y, pitch_bytes)), _dev(pitched(uv, pitch_bytes))
    out = torch.full((n, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda")
    hotpath.check(lib.cc_yuv420sp_to_rgb(
        yd.data_ptr(), uvd.data_ptr(), n, h, w, pitch_bytes, depth, matrix,
        full_range, out.data_ptr(), 0))
    torch.cuda.synchronize()
    return out


def convert_resize(lib, y, uv, pitch_bytes, depth, matrix, full_range, oh, ow):
    n, h, w = y.shape
    yd, uvd = _dev(pitched(y, pitch_bytes)), _dev(pitched(uv, pitch_bytes))
    out = torch.full((n, oh, ow, 3), 0x5A, dtype=torch.uint8, device="cuda")
    hotpath.check(lib.cc_yuv420sp_to_rgb_resize(
        yd.data_ptr(), uvd.data_ptr(), n, h, w, pitch_bytes, depth, matrix,
        full_range, out.data_ptr(), oh, ow, 0))
    torch.cuda.synchronize()
    return out


def equiv16(rng, a8: np.ndarray, depth: int) -> np.ndarray:
    junk = rng.integers(0, 1 << (16 - depth), size=a8.shape, dtype=np.uint16)
    return (a8.astype(np.uint16) << np.uint16(8)) | junk.astype(np.uint16)


# ---- 1. bit-exact over the whole grid ----------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["tail-unaligned", "body+tail", "body"])
def test_bitexact_grid(lib, shape):
    n, h, w, pitch16 = shape
    rng = np.random.default_rng(100 + w)
    planes = {d: rand_planes(rng, n, h, w, d) for d in yuv_ref.DEPTHS}
    for depth, matrix, full_range in GRID:
        y, uv = planes[depth]
        pitch = pitch16 // 2 if depth == 8 else pitch16
        got = convert(lib, y, uv, pitch, depth, matrix, full_range).cpu().numpy()
        want = yuv_ref.yuv420sp_to_rgb_batch(y, uv, depth, matrix, full_range)
        np.testing.assert_array_equal(
            got, want, err_msg=f"depth {depth} matrix {matrix} full {full_range}")


# ---- 2. extremes: both clamps ------------------------------------------------

@pytest.mark.parametrize("depth", yuv_ref.DEPTHS)
def test_extremes(lib, depth):
    n, h, w, pitch16 = SHAPES[1]
    dtype, top = (np.uint8, 0xFF) if depth == 8 else (np.uint16, 0xFFFF)
    pitch = pitch16 // 2 if depth == 8 else pitch16
    cases = {"zero": (0, 0), "max": (top, top), "ymax-cmin": (top, 0)}
    lo, hi = 255, 0
    for name, (yv, cv) in cases.items():
        y = np.full((n, h, w), yv, dtype=dtype)
        uv = np.full((n, h // 2, w), cv, dtype=dtype)
        for matrix in yuv_ref.MATRICES:
            for full_range in (0, 1):
                got = convert(lib, y, uv, pitch, depth, matrix, full_range).cpu().numpy()
                want = yuv_ref.yuv420sp_to_rgb_batch(y, uv, depth, matrix, full_range)
                np.testing.assert_array_equal(got, want, err_msg=f"{name} {depth} "
                                              f"{matrix} {full_range}")
                lo, hi = min(lo, int(want.min())), max(hi, int(want.max()))
    assert (lo, hi) == (0, 255)  # the cases do reach both clamps


# ---- 3. cross-checks against the existing 8-bit kernels ----------------------

def test_depth8_bt601_equals_nv12_kernels(lib):
    """The cc_nv12_* entries are the yuv420sp launcher at (8, bt601, limited),
    so entry-point equality compares a kernel with itself; the independent
    truth is oracle/color.py, on the same pitched planes."""
    rng = np.random.default_rng(5)
    for n, h, w, pitch16 in SHAPES:
        pitch = pitch16 // 2
        y, uv = rand_planes(rng, n, h, w, 8)
        yd, uvd = _dev(pitched(y, pitch)), _dev(pitched(uv, pitch))
        old = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        hotpath.check(lib.cc_nv12_to_rgb(yd.data_ptr(), uvd.data_ptr(), n, h, w,
                                         pitch, old.data_ptr(), 0))
        new = convert(lib, y, uv, pitch, 8, 0, 0)
        assert torch.equal(old, new), (n, h, w)
        want = np.stack([ocolor.nv12_to_rgb(y[i], uv[i].reshape(h // 2, w // 2, 2))
                         for i in range(n)])
        np.testing.assert_array_equal(old.cpu().numpy(), want, err_msg=str((n, h, w)))
        for oh, ow in ((7, 9), (2 * h + 1, 2 * w - 3)):
            old_r = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
            hotpath.check(lib.cc_nv12_to_rgb_resize(
                yd.data_ptr(), uvd.data_ptr(), n, h, w, pitch, old_r.data_ptr(),
                oh, ow, 0))
            new_r = convert_resize(lib, y, uv, pitch, 8, 0, 0, oh, ow)
            assert torch.equal(old_r, new_r), (n, h, w, oh, ow)
            want_r = np.stack([ocolor.resize_bilinear_u8(f, oh, ow) for f in want])
            np.testing.assert_array_equal(old_r.cpu().numpy(), want_r,
                                          err_msg=str((n, h, w, oh, ow)))


@pytest.mark.parametrize("depth", (8, 10))
def test_misaligned_base_takes_the_scalar_kernel(lib, depth):
    """Planes 8- but not 16-byte aligned, rows a multiple of 8 pixels at a
    16-byte-multiple pitch: only the base-alignment test keeps the call off
    the vector kernel's 16-byte loads.  Depth 8 goes through cc_nv12_to_rgb,
    which depends on that dispatch since it shares the launcher."""
    n, h, w = 1, 4, 16
    pitch = 16 if depth == 8 else 32
    rng = np.random.default_rng(8 + depth)
    y, uv = rand_planes(rng, n, h, w, depth)

    def carve(plane):  # the plane's bytes at offset 8 of a 0xA5-filled buffer
        raw = torch.from_numpy(np.ascontiguousarray(plane).view(np.uint8).reshape(-1))
        buf = torch.full((raw.numel() + 24,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[8:8 + raw.numel()] = raw.cuda()
        assert buf.data_ptr() % 16 == 0
        return buf, buf.data_ptr() + 8

    ybuf, yp = carve(y)
    uvbuf, uvp = carve(uv)
    nbytes, guard = n * h * w * 3, 64
    out = torch.full((nbytes + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    if depth == 8:
        hotpath.check(lib.cc_nv12_to_rgb(yp, uvp, n, h, w, pitch, out.data_ptr(), 0))
    else:
        hotpath.check(lib.cc_yuv420sp_to_rgb(yp, uvp, n, h, w, pitch, depth, 0, 0,
                                             out.data_ptr(), 0))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = yuv_ref.yuv420sp_to_rgb_batch(y, uv, depth, 0, 0)
    np.testing.assert_array_equal(got[:nbytes].reshape(n, h, w, 3), want)
    assert (got[nbytes:] == 0x5A).all()  # guard bytes untouched


def test_nv12_entries_keep_their_timing_names(lib):
    n, h, w, _ = SHAPES[0]  # 6x10: the scalar kernel alone
    y, uv = rand_planes(np.random.default_rng(9), n, h, w, 8)
    yd, uvd = _dev(y), _dev(uv)
    full = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    small = torch.empty((n, 3, 5, 3), dtype=torch.uint8, device="cuda")
    hotpath.timing_enable(True)
    try:
        hotpath.check(lib.cc_nv12_to_rgb_resize(
            yd.data_ptr(), uvd.data_ptr(), n, h, w, w, small.data_ptr(), 3, 5, 0))
        hotpath.check(lib.cc_nv12_to_rgb(yd.data_ptr(), uvd.data_ptr(), n, h, w, w,
                                         full.data_ptr(), 0))
        torch.cuda.synchronize()
        assert hotpath.timing_report("nv12_to_rgb_resize")[1] == 1
        assert hotpath.timing_report("nv12_to_rgb")[1] >= 1  # body and/or row tail
        assert hotpath.timing_report("yuv420sp_to_rgb")[1] == 0
    finally:
        hotpath.timing_enable(False)


@pytest.mark.parametrize("depth", (10, 12))
def test_8bit_equivalent_16bit_input_equals_nv12_kernel(lib, depth):
    rng = np.random.default_rng(6)
    n, h, w, pitch16 = SHAPES[1]
    y8, uv8 = rand_planes(rng, n, h, w, 8)
    y8.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    uv8.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    yd, uvd = _dev(y8), _dev(uv8)
    old = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    hotpath.check(lib.cc_nv12_to_rgb(yd.data_ptr(), uvd.data_ptr(), n, h, w, w,
                                     old.data_ptr(), 0))
    new = convert(lib, equiv16(rng, y8, depth), equiv16(rng, uv8, depth), pitch16,
                  depth, 0, 0)
    assert torch.equal(old, new)


# ---- 4. fused resize ----------------------------------------------------------

@pytest.mark.parametrize("case", [(1, 34, 66, 256, 7, 9), (2, 6, 10, 20, 13, 17)],
                         ids=["down", "up"])
def test_fused_resize(lib, case):
    n, h, w, pitch16, oh, ow = case
    rng = np.random.default_rng(7)
    planes = {d: rand_planes(rng, n, h, w, d) for d in yuv_ref.DEPTHS}
    for depth, matrix, full_range in GRID:
        y, uv = planes[depth]
        pitch = pitch16 // 2 if depth == 8 else pitch16
        got = convert_resize(lib, y, uv, pitch, depth, matrix, full_range, oh, ow)
        rgb = yuv_ref.yuv420sp_to_rgb_batch(y, uv, depth, matrix, full_range)
        want = np.stack([ocolor.resize_bilinear_u8(rgb[i], oh, ow) for i in range(n)])
        np.testing.assert_array_equal(
            got.cpu().numpy(), want,
            err_msg=f"depth {depth} matrix {matrix} full {full_range}")
        # == the full-resolution kernel followed by cc_resize_bilinear_u8
        full = convert(lib, y, uv, pitch, depth, matrix, full_range)
        two = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
        hotpath.check(lib.cc_resize_bilinear_u8(full.data_ptr(), n, h, w,
                                                two.data_ptr(), oh, ow, 0))
        torch.cuda.synchronize()
        assert torch.equal(got, two), (depth, matrix, full_range)


# ---- 5. error paths: rejected before any launch ------------------------------

def test_rejections_leave_the_output_untouched(lib):
    n, h, w, pitch = 1, 4, 8, 16
    y = torch.zeros(h * pitch, dtype=torch.uint8, device="cuda")
    uv = torch.zeros(h // 2 * pitch, dtype=torch.uint8, device="cuda")
    out = torch.full((n, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda")
    yp, uvp, op = y.data_ptr(), uv.data_ptr(), out.data_ptr()
    good = dict(y=yp, uv=uvp, n=n, h=h, w=w, pitch=pitch, depth=10, matrix=1, full=0,
                out=op)
    bad = {
        "odd h": dict(h=3), "odd w": dict(w=7),
        "depth 9": dict(depth=9), "depth 16": dict(depth=16),
        "matrix -1": dict(matrix=-1), "matrix 3": dict(matrix=3),
        "full 2": dict(full=2), "full -1": dict(full=-1),
        "pitch < row bytes": dict(pitch=14),
        "pitch < row bytes (8 bit)": dict(depth=8, pitch=6),
        "odd pitch at 16 bit": dict(pitch=17),
        "null y": dict(y=None), "null uv": dict(uv=None), "null out": dict(out=None),
        "n 0": dict(n=0), "h 0": dict(h=0), "w -2": dict(w=-2),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        rc = lib.cc_yuv420sp_to_rgb(a["y"], a["uv"], a["n"], a["h"], a["w"], a["pitch"],
                                    a["depth"], a["matrix"], a["full"], a["out"], 0)
        assert rc == -1, name  # CC_ERR_INVALID
        assert lib.cc_last_error().decode(), name
        rc = lib.cc_yuv420sp_to_rgb_resize(
            a["y"], a["uv"], a["n"], a["h"], a["w"], a["pitch"], a["depth"],
            a["matrix"], a["full"], a["out"], 2, 2, 0)
        assert rc == -1, name + " (resize)"
        assert lib.cc_last_error().decode(), name
    for oh, ow in ((0, 2), (2, -1)):
        rc = lib.cc_yuv420sp_to_rgb_resize(yp, uvp, n, h, w, pitch, 10, 1, 0, op, oh, ow, 0)
        assert rc == -1 and lib.cc_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    # the unchanged arguments are accepted
    hotpath.check(lib.cc_yuv420sp_to_rgb(yp, uvp, n, h, w, pitch, 10, 1, 0, op, 0))
    torch.cuda.synchronize()
    assert not bool((out == 0x5A).all())


# ---- 6. stages ----------------------------------------------------------------

FPS, NFRAMES, H, W = 30, 60, 32, 48


def _task(data: bytes):
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        Clip, SplitPipeTask, Video, VideoMetadata,
    )

    arr = np.frombuffer(data, dtype=np.uint8)
    video = Video(
        input_video=pathlib.Path("/synthetic/yuv16.bin"),
        metadata=VideoMetadata(size=len(data), height=H, width=W, framerate=FPS,
                               num_frames=NFRAMES, duration=NFRAMES / FPS,
                               video_codec="raw"),
    )
    video.clips.append(Clip(uuid=uuid.uuid5(uuid.NAMESPACE_URL, "yuv16"),
                            source_video="synthetic", span=(0.0, NFRAMES / FPS),
                            encoded_data=arr))
    return SplitPipeTask(videos=[video]), video


def _host_pipeline(data: bytes, fps: float, matrix: int, full_range: int, oh: int, ow: int):
    depth = raw_backend.parse_format(data)[0]
    ts = raw_backend.timestamps(data)
    idx, counts, _ = osampling.sample_closest(ts, fps)
    ys, uvs = raw_backend.frame_planes(data, idx)
    rgb = yuv_ref.yuv420sp_to_rgb_batch(ys, uvs, depth, matrix, full_range)
    sel = np.stack([ocolor.resize_bilinear_u8(f, oh, ow) for f in rgb])
    return osampling.broadcast_selected(sel, np.arange(len(idx), dtype=np.int32), counts)


@pytest.fixture(scope="module")
def clip10_bt709() -> bytes:
    return raw_backend.make_synthetic_clip_p016(NFRAMES, H, W, FPS, seed=11,
                                                bit_depth=10, matrix=1)


@pytest.mark.parametrize("standard,matrix", [("bt601", 0), ("bt709", 1), ("stream", 1)])
def test_clip_frame_extraction_stage_10bit(lib, clip10_bt709, standard, matrix):
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        ClipFrameExtractionStage,
    )

    task, video = _task(clip10_bt709)
    stage = ClipFrameExtractionStage(target_fps=[2], target_res=(16, 24),
                                     to_host=True, color_standard=standard)
    stage.process_data([task])
    clip = video.clips[0]
    assert not clip.errors and not video.errors, (clip.errors, video.errors)
    (got,) = clip.extracted_frames.resolve().values()
    want = _host_pipeline(clip10_bt709, 2.0, matrix, 0, 16, 24)
    np.testing.assert_array_equal(got, want)


def test_stream_standard_follows_the_full_range_flag(lib):
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        extract_frames, ClipFrameExtractionStage,
    )

    data = raw_backend.make_synthetic_clip_p016(NFRAMES, H, W, FPS, seed=12,
                                                bit_depth=12, matrix=2, full_range=True)
    stage = ClipFrameExtractionStage(target_res=(16, 24), color_standard="stream")
    got = stage._extract_clip_frames(data, 2.0).cpu().numpy()
    np.testing.assert_array_equal(got, _host_pipeline(data, 2.0, 2, 1, 16, 24))
    # the default standard ignores the signalling
    got601 = extract_frames(data, sample_rate_fps=2.0, target_res=(16, 24), to_host=True)
    np.testing.assert_array_equal(got601, _host_pipeline(data, 2.0, 0, 0, 16, 24))


def test_8bit_equivalent_version2_clip_matches_its_nv12_twin(lib):
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        extract_frames,
    )

    v1 = raw_backend.make_synthetic_clip(NFRAMES, H, W, FPS, seed=13)
    ys, uvs = raw_backend.frame_planes(v1, np.arange(NFRAMES, dtype=np.int32))
    v2 = raw_backend.encode_raw_p016(ys.astype(np.uint16) << 8, uvs.astype(np.uint16) << 8,
                                     FPS, bit_depth=10)
    a = extract_frames(v1, sample_rate_fps=2.0, target_res=(16, 24), to_host=True)
    b = extract_frames(v2, sample_rate_fps=2.0, target_res=(16, 24), to_host=True)
    np.testing.assert_array_equal(a, b)


def test_whole_video_frame_extraction_stage_10bit(lib, clip10_bt709):
    from cosmos_curate_amd.core.utils.lazy_data import LazyData
    from cosmos_curate_amd.pipelines.video.clipping.transnetv2_extraction_stages import (
        VideoFrameExtractionStage,
    )

    task, video = _task(clip10_bt709)
    arr = np.frombuffer(clip10_bt709, dtype=np.uint8)
    video.encoded_data = LazyData(value=arr, nbytes=arr.nbytes)
    VideoFrameExtractionStage().process_data([task])
    assert not video.errors, video.errors
    got = video.frame_array.resolve()
    ys, uvs = raw_backend.frame_planes(clip10_bt709, np.arange(NFRAMES, dtype=np.int32))
    rgb = yuv_ref.yuv420sp_to_rgb_batch(ys, uvs, 10, 0, 0)  # BT.601 limited
    want = np.stack([ocolor.resize_bilinear_u8(f, 27, 48) for f in rgb])
    np.testing.assert_array_equal(got, want)
