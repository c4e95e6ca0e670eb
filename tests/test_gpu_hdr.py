"""cc_yuv420sp_hdr_to_rgb / cc_yuv420sp_hdr_to_rgb_resize on the MI355X:
bit-exact against tests/hdr_ref.py fed the library's own tables (so no libm
detail can enter), at the shapes where the kernel changes path (vector body
+ row tail, whole-frame scalar, pure vector body), plus the stage that
routes PQ payloads through them.

Every conversion below runs on guarded buffers: the input planes sit between
rows of 0xFFFF (padding columns too) and the output between rows of 7, so a
stray read changes the result and a stray write shows in a guard, without a
fault.  Every call runs twice and must give the same bytes.  Every rejected
call returns before any launch; nothing here hands a kernel a bad pointer or
size.
"""

from __future__ import annotations

import pathlib
import uuid

import numpy as np
import pytest
import torch

import hdr_ref
import yuv_ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from oracle import color as ocolor
from oracle import sampling as osampling

pytestmark = pytest.mark.gpu

PEAKS = (1000.0, 4000.0)
WHITE = 203.0
# (matrix, full_range): BT.2020-NCL limited (what HDR10 is), BT.709 full
COLOURS = ((2, 0), (1, 1))
# (n, h, w, pitch in bytes at 16 bit)
SHAPES = [
    (2, 6, 26, 64),  # vector body of 24 columns + 2-column tail, aligned pitch
    (2, 6, 26, 52),  # pitch 2*w, not 16-byte aligned: whole-frame scalar path
    (2, 6, 8, 16),   # pure vector body, no tail
]


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


@pytest.fixture(scope="module")
def tabs(lib):
    """The library's tables: (device tensor, tin, tout)."""
    dev = hotpath.hdr_tables(hotpath.HDR_TRANSFER_PQ, WHITE)
    assert dev.dtype == torch.uint8 and dev.numel() == hotpath.HDR_TABLE_BYTES
    assert hotpath.hdr_tables(hotpath.HDR_TRANSFER_PQ, WHITE) is dev  # uploaded once
    tin, tout = hdr_ref.split_image(dev.cpu().numpy())
    host = hdr_ref.split_image(hotpath.hdr_tables_build(hotpath.HDR_TRANSFER_PQ, WHITE))
    np.testing.assert_array_equal(tin, host[0])
    np.testing.assert_array_equal(tout, host[1])
    return dev, tin, tout


def guarded_plane(plane: np.ndarray, pitch_bytes: int) -> tuple[torch.Tensor, int]:
    """(n, rows, w) samples -> a device buffer holding a guard row, the rows
    at `pitch_bytes` stride, a guard row; everything that is not a sample is
    0xFF bytes.  Returns (buffer, pointer to the first sample row)."""
    n, rows, w = plane.shape
    buf = np.full((n * rows + 2, pitch_bytes), 0xFF, dtype=np.uint8)
    body = np.ascontiguousarray(plane.reshape(n * rows, w)).view(np.uint8)
    buf[1:-1, :body.shape[1]] = body
    dev = torch.from_numpy(buf).cuda()
    return dev, dev.data_ptr() + pitch_bytes


def run_guarded(launch, y, uv, pitch_bytes, out_shape):
    """launch(y_ptr, uv_ptr, out_ptr) twice on guarded buffers -> the output
    as numpy, after checking the guards and that both launches agree."""
    ybuf, yp = guarded_plane(y, pitch_bytes)
    uvbuf, uvp = guarded_plane(uv, pitch_bytes)
    n, oh, ow, _ = out_shape
    row = ow * 3
    outs = []
    for _ in range(2):
        obuf = torch.full((n * oh + 2, row), 7, dtype=torch.uint8, device="cuda")
        launch(yp, uvp, obuf.data_ptr() + row)
        torch.cuda.synchronize()
        got = obuf.cpu().numpy()
        assert (got[0] == 7).all() and (got[-1] == 7).all(), "output guard row written"
        outs.append(got[1:-1].reshape(out_shape))
    np.testing.assert_array_equal(outs[0], outs[1], err_msg="two launches differ")
    assert bool((ybuf.cpu().numpy()[[0, -1]] == 0xFF).all())  # inputs are read-only
    return outs[0]


def convert(lib, tabs, y, uv, pitch, depth, matrix, full_range, peak):
    n, h, w = y.shape
    iw2 = float(hdr_ref.inv_w2(peak, WHITE))
    return run_guarded(
        lambda yp, uvp, op: hotpath.check(lib.cc_yuv420sp_hdr_to_rgb(
            yp, uvp, n, h, w, pitch, depth, matrix, full_range, tabs[0].data_ptr(),
            iw2, op, 0)),
        y, uv, pitch, (n, h, w, 3))


def convert_resize(lib, tabs, y, uv, pitch, depth, matrix, full_range, peak, oh, ow):
    n, h, w = y.shape
    iw2 = float(hdr_ref.inv_w2(peak, WHITE))
    return run_guarded(
        lambda yp, uvp, op: hotpath.check(lib.cc_yuv420sp_hdr_to_rgb_resize(
            yp, uvp, n, h, w, pitch, depth, matrix, full_range, tabs[0].data_ptr(),
            iw2, op, oh, ow, 0)),
        y, uv, pitch, (n, oh, ow, 3))


def reference(tabs, y, uv, depth, matrix, full_range, peak):
    return hdr_ref.yuv420sp_hdr_to_rgb_batch(
        y, uv, depth, matrix, full_range, tabs[1], tabs[2], hdr_ref.inv_w2(peak, WHITE))


def content(rng, h, w, depth, phase=0):
    """Two frames of MSB-aligned samples whose ignored low bits are nonzero
    noise.  Frame 0: a luma ramp over the whole code range, neutral chroma.
    Frame 1: random luma and chroma over all 16 bits, so sub-black and
    super-white R'G'B' occur and every clamp of the chain fires."""
    if depth == 8:
        top, dtype, shift = 256, np.uint8, 0
    else:
        top, dtype, shift = 1 << depth, np.uint16, 16 - depth
    npx = h * w
    ramp = (phase + np.arange(npx) * (top // npx + 1)) % top
    ramp[-1] = top - 1
    y = np.empty((2, h, w), dtype=np.int64)
    uv = np.empty((2, h // 2, w), dtype=np.int64)
    y[0] = ramp.reshape(h, w) << shift
    uv[0] = (top // 2) << shift
    y[1] = rng.integers(0, top, size=(h, w)) << shift
    uv[1] = rng.integers(0, top, size=(h // 2, w)) << shift
    if shift:
        y |= rng.integers(1, 1 << shift, size=y.shape)
        uv |= rng.integers(1, 1 << shift, size=uv.shape)
    return y.astype(dtype), uv.astype(dtype)


# ---- 1. full resolution, bit-exact ---------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["body+tail", "scalar-unaligned", "body"])
def test_bitexact_full_resolution(lib, tabs, shape):
    n, h, w, pitch = shape
    rng = np.random.default_rng(2084 + pitch)
    clamps = np.zeros(4, dtype=bool)
    for k, depth in enumerate((10, 12)):
        for matrix, full_range in COLOURS:
            y, uv = content(rng, h, w, depth, phase=37 * k + 11 * matrix)
            assert y.shape == (n, h, w)
            for peak in PEAKS:
                got = convert(lib, tabs, y, uv, pitch, depth, matrix, full_range, peak)
                want = reference(tabs, y, uv, depth, matrix, full_range, peak)
                np.testing.assert_array_equal(
                    got, want, err_msg=f"depth {depth} matrix {matrix} full "
                    f"{full_range} peak {peak}")
            # what the random frame exercises (peak 1000: w^2 = 24.3 < 49.3)
            p8 = hdr_ref.rgb_prime(y[1], uv[1], depth, matrix, full_range)
            lin = tabs[1][hdr_ref._pq_index(p8)].astype(np.float64)
            mapped = lin @ np.array(hdr_ref.GAMUT).T
            clamps |= [(p8 < 0).any(), (p8 > 255).any(), (mapped < 0).any(),
                       (mapped.max(axis=-1) > (PEAKS[0] / WHITE) ** 2).any()]
    assert clamps.all(), clamps  # index low/high, gamut floor, tone-map ceiling


def test_every_table_index(lib, tabs):
    """All 4096 luma codes of a 12-bit full-range ramp with neutral chroma:
    every one of the 4081 inverse-PQ entries is read, on the vector path."""
    n, h, w, pitch = 1, 64, 64, 128
    rng = np.random.default_rng(12)
    y = (np.arange(4096).reshape(n, h, w) << 4) | rng.integers(1, 16, size=(n, h, w))
    uv = np.full((n, h // 2, w), 2048 << 4) | rng.integers(1, 16, size=(n, h // 2, w))
    y, uv = y.astype(np.uint16), uv.astype(np.uint16)
    idx = hdr_ref._pq_index(hdr_ref.rgb_prime(y[0], uv[0], 12, 1, 1))
    assert np.array_equal(np.unique(idx), np.arange(hdr_ref.N_IN))
    for peak in PEAKS:
        got = convert(lib, tabs, y, uv, pitch, 12, 1, 1, peak)
        want = reference(tabs, y, uv, 12, 1, 1, peak)
        np.testing.assert_array_equal(got, want, err_msg=f"peak {peak}")
        grey = want[0].reshape(-1, 3).astype(int)
        assert (np.diff(grey[:, 1]) >= 0).all() and grey[0].tolist() == [0, 0, 0]
        assert grey[-1].tolist() == [255, 255, 255]


def test_depth8_instantiation(lib, tabs):
    """PQ at 8 bit is legal: the u8 instantiations, body + tail and scalar."""
    rng = np.random.default_rng(8)
    for pitch in (32, 26):
        y, uv = content(rng, 6, 26, 8)
        got = convert(lib, tabs, y, uv, pitch, 8, 2, 0, 1000.0)
        np.testing.assert_array_equal(got, reference(tabs, y, uv, 8, 2, 0, 1000.0))
        small = convert_resize(lib, tabs, y, uv, pitch, 8, 2, 0, 1000.0, 5, 7)
        want = np.stack([ocolor.resize_bilinear_u8(f, 5, 7) for f in got])
        np.testing.assert_array_equal(small, want)


def test_other_reference_white(lib, tabs):
    """Tables for another diffuse white are their own upload."""
    dev = hotpath.hdr_tables(hotpath.HDR_TRANSFER_PQ, 100.0)
    tin, tout = hdr_ref.split_image(dev.cpu().numpy())
    assert dev is not tabs[0] and not np.array_equal(tin, tabs[1])
    y, uv = content(np.random.default_rng(100), 6, 26, 10)
    iw2 = float(hdr_ref.inv_w2(1000.0, 100.0))
    got = run_guarded(
        lambda yp, uvp, op: hotpath.yuv_hdr_to_rgb(
            yp, uvp, 2, 6, 26, 64, op, 0, tables=dev.data_ptr(), inv_w2=iw2,
            bit_depth=10, matrix=2, full_range=False),
        y, uv, 64, (2, 6, 26, 3))
    want = hdr_ref.yuv420sp_hdr_to_rgb_batch(y, uv, 10, 2, 0, tin, tout, np.float32(iw2))
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, reference(tabs, y, uv, 10, 2, 0, 1000.0))


# ---- 2. fused resize -------------------------------------------------------------

@pytest.mark.parametrize("case", [(2, 18, 34, 80, 7, 9), (2, 6, 26, 64, 6, 26)],
                         ids=["down", "identity"])
def test_fused_resize(lib, tabs, case):
    n, h, w, pitch, oh, ow = case
    rng = np.random.default_rng(7 + h)
    for depth in (10, 12):
        for matrix, full_range in COLOURS:
            y, uv = content(rng, h, w, depth, phase=5 * depth)
            for peak in PEAKS:
                tag = f"depth {depth} matrix {matrix} full {full_range} peak {peak}"
                got = convert_resize(lib, tabs, y, uv, pitch, depth, matrix, full_range,
                                     peak, oh, ow)
                rgb = reference(tabs, y, uv, depth, matrix, full_range, peak)
                want = np.stack([ocolor.resize_bilinear_u8(f, oh, ow) for f in rgb])
                np.testing.assert_array_equal(got, want, err_msg=tag)
                if (oh, ow) == (h, w):
                    np.testing.assert_array_equal(got, rgb, err_msg=tag)  # identity taps
                # == the full-resolution kernel followed by cc_resize_bilinear_u8
                full = convert(lib, tabs, y, uv, pitch, depth, matrix, full_range, peak)
                np.testing.assert_array_equal(full, rgb, err_msg=tag)
                full_dev = torch.from_numpy(full).cuda()
                two = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
                hotpath.check(lib.cc_resize_bilinear_u8(
                    full_dev.data_ptr(), n, h, w, two.data_ptr(), oh, ow, 0))
                torch.cuda.synchronize()
                np.testing.assert_array_equal(got, two.cpu().numpy(), err_msg=tag)


# ---- 3. SDR entries are untouched --------------------------------------------------

def test_sdr_entry_still_equals_yuv_ref(lib, tabs):
    """The HDR instantiations share templates with the SDR kernels: the same
    planes through cc_yuv420sp_to_rgb still give yuv_ref's bytes, and differ
    from the tone-mapped ones."""
    y, uv = content(np.random.default_rng(3), 6, 26, 10)
    sdr = run_guarded(
        lambda yp, uvp, op: hotpath.check(lib.cc_yuv420sp_to_rgb(
            yp, uvp, 2, 6, 26, 64, 10, 2, 0, op, 0)),
        y, uv, 64, (2, 6, 26, 3))
    np.testing.assert_array_equal(sdr, yuv_ref.yuv420sp_to_rgb_batch(y, uv, 10, 2, 0))
    assert not np.array_equal(sdr, convert(lib, tabs, y, uv, 64, 10, 2, 0, 1000.0))


def test_timing_names(lib, tabs):
    y, uv = content(np.random.default_rng(4), 6, 26, 10)
    hotpath.timing_enable(True)
    try:
        convert(lib, tabs, y, uv, 64, 10, 2, 0, 1000.0)  # two calls: body + tail each
        convert_resize(lib, tabs, y, uv, 64, 10, 2, 0, 1000.0, 3, 5)
        assert hotpath.timing_report("yuv420sp_hdr_to_rgb")[1] == 4
        assert hotpath.timing_report("yuv420sp_hdr_to_rgb_resize")[1] == 2
        assert hotpath.timing_report("yuv420sp_to_rgb")[1] == 0
    finally:
        hotpath.timing_enable(False)


# ---- 4. error paths: rejected before any launch --------------------------------------

def test_rejections_leave_the_output_untouched(lib, tabs):
    n, h, w, pitch = 1, 4, 8, 16
    y = torch.zeros(h * pitch, dtype=torch.uint8, device="cuda")
    uv = torch.zeros(h // 2 * pitch, dtype=torch.uint8, device="cuda")
    out = torch.full((n, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(y=y.data_ptr(), uv=uv.data_ptr(), n=n, h=h, w=w, pitch=pitch, depth=10,
                matrix=2, full=0, tables=tabs[0].data_ptr(), iw2=0.04, out=out.data_ptr())
    bad = {
        "null tables": dict(tables=None),
        "tables not 16-byte aligned": dict(tables=tabs[0].data_ptr() + 4),
        "negative inv_w2": dict(iw2=-0.04),
        "nan inv_w2": dict(iw2=float("nan")),
        "inf inv_w2": dict(iw2=float("inf")),
        "odd w": dict(w=7), "odd h": dict(h=3),
        "depth 9": dict(depth=9), "matrix 3": dict(matrix=3), "full 2": dict(full=2),
        "pitch < row bytes": dict(pitch=14), "odd pitch": dict(pitch=17),
        "null y": dict(y=None), "null uv": dict(uv=None), "null out": dict(out=None),
        "n 0": dict(n=0),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        rc = lib.cc_yuv420sp_hdr_to_rgb(
            a["y"], a["uv"], a["n"], a["h"], a["w"], a["pitch"], a["depth"], a["matrix"],
            a["full"], a["tables"], a["iw2"], a["out"], 0)
        assert rc == -1, name  # CC_ERR_INVALID
        assert lib.cc_last_error().decode(), name
        rc = lib.cc_yuv420sp_hdr_to_rgb_resize(
            a["y"], a["uv"], a["n"], a["h"], a["w"], a["pitch"], a["depth"], a["matrix"],
            a["full"], a["tables"], a["iw2"], a["out"], 2, 2, 0)
        assert rc == -1, name + " (resize)"
        assert lib.cc_last_error().decode(), name
    a = good
    rc = lib.cc_yuv420sp_hdr_to_rgb_resize(
        a["y"], a["uv"], n, h, w, pitch, 10, 2, 0, a["tables"], a["iw2"], a["out"], 0, 2, 0)
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    # the unchanged arguments are accepted; inv_w2 = 0 (no peak) is legal
    for iw2 in (0.04, 0.0):
        hotpath.check(lib.cc_yuv420sp_hdr_to_rgb(
            a["y"], a["uv"], n, h, w, pitch, 10, 2, 0, a["tables"], iw2, a["out"], 0))
    torch.cuda.synchronize()
    assert not bool((out == 0x5A).all())


# ---- 5. stage, end to end --------------------------------------------------------------

FPS, NFRAMES, H, W = 4, 8, 64, 96


def _task(data: bytes):
    from cosmos_curate_amd.pipelines.video.utils.data_model import (
        Clip, SplitPipeTask, Video, VideoMetadata,
    )

    arr = np.frombuffer(data, dtype=np.uint8)
    video = Video(
        input_video=pathlib.Path("/synthetic/hdr.bin"),
        metadata=VideoMetadata(size=len(data), height=H, width=W, framerate=FPS,
                               num_frames=NFRAMES, duration=NFRAMES / FPS,
                               video_codec="raw"),
    )
    video.clips.append(Clip(uuid=uuid.uuid5(uuid.NAMESPACE_URL, "hdr"),
                            source_video="synthetic", span=(0.0, NFRAMES / FPS),
                            encoded_data=arr))
    return SplitPipeTask(videos=[video]), video


def _host_pipeline(data: bytes, fps: float, convert_batch, oh: int, ow: int):
    ts = raw_backend.timestamps(data)
    idx, counts, _ = osampling.sample_closest(ts, fps)
    ys, uvs = raw_backend.frame_planes(data, idx)
    rgb = convert_batch(ys, uvs)
    sel = np.stack([ocolor.resize_bilinear_u8(f, oh, ow) for f in rgb])
    return osampling.broadcast_selected(sel, np.arange(len(idx), dtype=np.int32), counts)


def _stage_frames(data: bytes, **kw):
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        ClipFrameExtractionStage,
    )

    task, video = _task(data)
    stage = ClipFrameExtractionStage(target_fps=[2], target_res=(16, 16), to_host=True,
                                     **kw)
    stage.process_data([task])
    clip = video.clips[0]
    assert not clip.errors and not video.errors, (clip.errors, video.errors)
    (got,) = clip.extracted_frames.resolve().values()
    return got


@pytest.fixture(scope="module")
def clip_pq() -> bytes:
    data = raw_backend.make_synthetic_clip_p016(NFRAMES, H, W, FPS, seed=21, bit_depth=10,
                                                matrix=2, transfer=1)
    assert raw_backend.parse_transfer(data) == 1 and data[10] == 3
    return data


@pytest.mark.parametrize("peak", PEAKS)
def test_stage_tonemaps_a_pq_clip(lib, tabs, clip_pq, peak):
    got = _stage_frames(clip_pq, hdr="tonemap", hdr_peak_nits=peak)
    want = _host_pipeline(
        clip_pq, 2.0,
        lambda ys, uvs: reference(tabs, ys, uvs, 10, 2, 0, peak), 16, 16)
    assert got.shape == want.shape and got.shape[1:] == (16, 16, 3)
    np.testing.assert_array_equal(got, want)
    if peak == 1000.0:
        # the signalled matrix is used whatever color_standard forces
        forced = _stage_frames(clip_pq, hdr="tonemap", color_standard="bt709")
        np.testing.assert_array_equal(forced, want)
        from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
            extract_frames,
        )

        one_off = extract_frames(clip_pq, sample_rate_fps=2.0, target_res=(16, 16),
                                 to_host=True, hdr="tonemap")
        np.testing.assert_array_equal(one_off, want)


def test_stage_hdr_off_keeps_todays_path(lib, clip_pq):
    """The PQ clip under the default: converted as if gamma-encoded, with the
    stage's present matrix choice (BT.601 limited unless told otherwise)."""
    for kw, (matrix, full_range) in (({}, (0, 0)),
                                     ({"hdr": "off"}, (0, 0)),
                                     ({"hdr": "off", "color_standard": "stream"}, (2, 0))):
        got = _stage_frames(clip_pq, **kw)
        want = _host_pipeline(
            clip_pq, 2.0,
            lambda ys, uvs: yuv_ref.yuv420sp_to_rgb_batch(ys, uvs, 10, matrix, full_range),
            16, 16)
        np.testing.assert_array_equal(got, want, err_msg=str(kw))


def test_stage_tonemap_leaves_sdr_clips_alone(lib):
    sdr = raw_backend.make_synthetic_clip_p016(NFRAMES, H, W, FPS, seed=21, bit_depth=10,
                                               matrix=2)
    assert sdr[10] == 2 and raw_backend.parse_transfer(sdr) == 0
    v1 = raw_backend.make_synthetic_clip(NFRAMES, H, W, FPS, seed=22)
    for data in (sdr, v1):
        off = _stage_frames(data)
        np.testing.assert_array_equal(_stage_frames(data, hdr="tonemap"), off)
    want = _host_pipeline(
        sdr, 2.0, lambda ys, uvs: yuv_ref.yuv420sp_to_rgb_batch(ys, uvs, 10, 0, 0), 16, 16)
    np.testing.assert_array_equal(_stage_frames(sdr, hdr="tonemap"), want)
