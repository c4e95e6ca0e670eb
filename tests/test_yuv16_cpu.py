"""10/12-bit and BT.709/BT.2020 YUV->RGB: everything that needs no GPU.

The arithmetic reference (tests/yuv_ref.py) against the 8-bit oracle, the
version-2 raw payload, the decode session against the mocked librocdecode
(10/12-bit streams -> P016 surfaces, stream-format query) and the stage
constructor.  The kernels themselves are pinned in test_gpu_yuv16.py.
"""

from __future__ import annotations

import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import yuv_ref
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from oracle import color as ocolor

ROOT = pathlib.Path(__file__).resolve().parent.parent
MOCK_SRC = ROOT / "tools" / "mock_rocdecode.cpp"

BT601_LIMITED = (1.1643835, 1.5960267, -0.8129676, -0.3917623, 2.0172321)


def equiv16(rng, a8: np.ndarray, depth: int) -> np.ndarray:
    """16-bit samples whose top 8 bits are a8: the rest of the depth's bits
    are zero, the ignored low 16-depth bits are random junk."""
    junk = rng.integers(0, 1 << (16 - depth), size=a8.shape, dtype=np.uint16)
    return (a8.astype(np.uint16) << np.uint16(8)) | junk.astype(np.uint16)


def rand_p016(rng, shape, depth: int) -> np.ndarray:
    """True `depth`-bit content, MSB-aligned, with junk in the ignored bits."""
    return rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)


# ---- 1. coefficient table --------------------------------------------------

def test_bt601_limited_row_is_the_existing_literals():
    row = yuv_ref.coefficients(8, 0, 0)
    assert row[0] == np.float32(16.0)
    assert row[1:] == tuple(np.float32(c) for c in BT601_LIMITED)
    # the oracle's own constants, bit for bit
    assert row[1:] == (ocolor._CY, ocolor._CVR, ocolor._CVG, ocolor._CUG, ocolor._CUB)
    for depth in (10, 12):
        assert yuv_ref.coefficients(depth, 0, 0) == row


@pytest.mark.parametrize("depth", yuv_ref.DEPTHS)
@pytest.mark.parametrize("matrix", yuv_ref.MATRICES)
@pytest.mark.parametrize("full_range", (0, 1))
def test_rows_within_one_ulp_of_formula(depth, matrix, full_range):
    got = yuv_ref.coefficients(depth, matrix, full_range)
    want = yuv_ref.formula(depth, matrix, full_range)
    for g, w in zip(got, want):
        ulp = float(np.spacing(np.float32(abs(w)))) if w else 0.0
        if (matrix, full_range) == (0, 0):
            # the pinned literals: CVR and CVG are the f32 NEIGHBOUR of the
            # rounded formula (one ulp between f32 values), the rest equal it
            assert abs(float(g) - float(np.float32(w))) <= ulp, (depth, g, w)
        else:
            # every other row is the formula rounded to f32
            assert abs(float(g) - w) <= ulp, (depth, matrix, full_range, g, w)
            assert g == np.float32(w), (depth, matrix, full_range, g, w)


# ---- 2. equivalence with the 8-bit oracle ------------------------------------

@pytest.mark.parametrize("depth", (10, 12))
def test_8bit_equivalent_input_matches_oracle(depth):
    rng = np.random.default_rng(20 + depth)
    h, w = 64, 96
    y8 = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    uv8 = rng.integers(0, 256, size=(h // 2, w), dtype=np.uint8)
    y8.flat[:256] = np.arange(256, dtype=np.uint8)  # every code at least once
    uv8.flat[:256] = np.arange(256, dtype=np.uint8)
    got = yuv_ref.yuv420sp_to_rgb(equiv16(rng, y8, depth), equiv16(rng, uv8, depth),
                                  depth, 0, 0)
    want = ocolor.nv12_to_rgb(y8, uv8.reshape(h // 2, w // 2, 2))
    np.testing.assert_array_equal(got, want)
    # and depth 8 through the reference is the oracle itself
    np.testing.assert_array_equal(yuv_ref.yuv420sp_to_rgb(y8, uv8, 8, 0, 0), want)


# ---- 3. discrimination -----------------------------------------------------

def test_true_10bit_and_bt709_are_really_different():
    rng = np.random.default_rng(3)
    h, w = 64, 96
    y = rand_p016(rng, (h, w), 10)
    uv = rand_p016(rng, (h // 2, w), 10)
    ref = yuv_ref.yuv420sp_to_rgb(y, uv, 10, 0, 0)
    trunc = ocolor.nv12_to_rgb((y >> 8).astype(np.uint8),
                               (uv >> 8).astype(np.uint8).reshape(h // 2, w // 2, 2))
    frac_depth = float(np.mean(ref != trunc))
    frac_matrix = float(np.mean(ref != yuv_ref.yuv420sp_to_rgb(y, uv, 10, 1, 0)))
    print(f"10-bit vs truncated 8-bit: {frac_depth:.3f}; bt709 vs bt601: {frac_matrix:.3f}")
    assert frac_depth >= 0.20
    assert frac_matrix >= 0.30


# ---- 4. raw backend --------------------------------------------------------

# encode_raw_nv12(y, uv, 30000, 1001) of the input below, captured from the
# commit before version 2 existed
V1_LITERAL = bytes.fromhex(
    "43434e56313252415700010002000000020000000400000030750000e9030000"
    "030a11181f262d34646f7a853b424950575e656c909ba6b1")
V1_HEADER_LITERAL = bytes.fromhex(
    "43434e5631325241570001000500000006000000080000001900000001000000")


def test_version1_bytes_unchanged():
    y = (np.arange(16, dtype=np.uint8) * 7 + 3).reshape(2, 2, 4)
    uv = (np.arange(8, dtype=np.uint8) * 11 + 100).reshape(2, 1, 4)
    assert raw_backend.encode_raw_nv12(y, uv, 30000, 1001) == V1_LITERAL
    assert raw_backend.pack_header(5, 6, 8, 25) == V1_HEADER_LITERAL
    assert raw_backend.parse_format(V1_LITERAL) == (8, 0, False, 1)
    assert raw_backend.parse_header(V1_LITERAL) == (2, 2, 4, 30000 / 1001)
    assert raw_backend.frame_nbytes(V1_LITERAL) == 12
    ys, uvs = raw_backend.frame_planes(V1_LITERAL, np.array([1, 0], dtype=np.int32))
    assert ys.dtype == np.uint8
    np.testing.assert_array_equal(ys, y[[1, 0]])
    np.testing.assert_array_equal(uvs, uv[[1, 0]])


@pytest.mark.parametrize("depth,matrix,full_range", [(10, 1, False), (12, 2, True)])
def test_version2_round_trip(depth, matrix, full_range):
    rng = np.random.default_rng(4)
    n, h, w = 5, 6, 10
    y = rand_p016(rng, (n, h, w), depth)
    uv = rand_p016(rng, (n, h // 2, w), depth)
    data = raw_backend.encode_raw_p016(y, uv, 30000, 1001, bit_depth=depth,
                                       matrix=matrix, full_range=full_range)
    assert raw_backend.HEADER_SIZE == 32
    assert len(data) == 32 + n * (h * w + h // 2 * w) * 2
    assert data[:32] == raw_backend.pack_header(
        n, h, w, 30000, 1001, bit_depth=depth, matrix=matrix, full_range=full_range)
    assert raw_backend.is_raw_nv12(data)
    assert raw_backend.parse_header(data) == (n, h, w, 30000 / 1001)
    assert raw_backend.parse_format(data) == (depth, matrix, full_range, 2)
    assert raw_backend.frame_nbytes(data) == (h * w + h // 2 * w) * 2
    idx = np.array([4, 0, 2], dtype=np.int32)
    ys, uvs = raw_backend.frame_planes(data, idx)
    assert ys.dtype == np.uint16 and uvs.dtype == np.uint16
    np.testing.assert_array_equal(ys, y[idx])
    np.testing.assert_array_equal(uvs, uv[idx])
    # planes are little-endian u16 in the body
    assert data[32:34] == int(y[0, 0, 0]).to_bytes(2, "little")
    ts = raw_backend.timestamps(data)
    want_ts = np.arange(n, dtype=np.float32) / np.float32(30000 / 1001)
    np.testing.assert_array_equal(ts, want_ts.astype(np.float32))


def test_pack_header_rejects_what_it_cannot_hold():
    with pytest.raises(ValueError):
        raw_backend.pack_header(1, 2, 2, 30, bit_depth=9)
    with pytest.raises(ValueError):
        raw_backend.pack_header(1, 2, 2, 30, bit_depth=10, matrix=3)
    with pytest.raises(ValueError):
        raw_backend.pack_header(1, 2, 2, 30, matrix=1)  # version 1 has no room


def test_synthetic_p016_clip_is_true_10bit():
    data = raw_backend.make_synthetic_clip_p016(4, 16, 24, 30, seed=1, bit_depth=10,
                                                matrix=1)
    assert raw_backend.parse_format(data) == (10, 1, False, 2)
    ys, uvs = raw_backend.frame_planes(data, np.arange(4, dtype=np.int32))
    for plane in (ys, uvs):
        assert not np.any(plane & 0x3F)            # MSB-aligned: low 6 bits clear
        assert np.any((plane >> 6) & 0x3)          # the two bits 8-bit lacks are used


def test_slice_raw_clip_version2_is_frame_exact_and_keeps_format():
    from cosmos_curate_amd.pipelines.video.clipping.clip_extraction_stages import (
        _slice_raw_clip,
    )

    data = raw_backend.make_synthetic_clip_p016(60, 8, 12, 30, seed=2, bit_depth=12,
                                                matrix=2, full_range=True)
    # the whole span is the payload itself (zero-copy)
    whole = _slice_raw_clip(data, (0.0, 2.0))
    assert bytes(whole) == data
    part = bytes(_slice_raw_clip(data, (0.5, 1.2)))  # frames 15..35
    assert raw_backend.parse_header(part) == (21, 8, 12, 30.0)
    assert raw_backend.parse_format(part) == (12, 2, True, 2)
    want = raw_backend.frame_planes(data, np.arange(15, 36, dtype=np.int32))
    got = raw_backend.frame_planes(part, np.arange(21, dtype=np.int32))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    # version 1 still slices to version-1 bytes
    v1 = raw_backend.make_synthetic_clip(60, 8, 12, 30, seed=2)
    part1 = bytes(_slice_raw_clip(v1, (0.5, 1.2)))
    assert part1[:32] == raw_backend.pack_header(21, 8, 12, 30)
    assert part1[32:] == v1[32 + 15 * 144: 32 + 36 * 144]


def test_download_stage_names_the_pixel_format():
    from cosmos_curate_amd.pipelines.video.read_write.download_stages import (
        VideoDownloader,
    )
    from cosmos_curate_amd.pipelines.video.utils.data_model import Video, VideoMetadata

    for depth, name in ((10, "p010le"), (12, "p012le")):
        v = Video(input_video=pathlib.Path("/synthetic/x"), metadata=VideoMetadata())
        data = raw_backend.make_synthetic_clip_p016(3, 4, 4, 30, seed=0, bit_depth=depth)
        VideoDownloader._populate_raw(None, v, data)
        assert v.metadata.pixel_format == name
        assert (v.metadata.height, v.metadata.width, v.metadata.num_frames) == (4, 4, 3)
    v = Video(input_video=pathlib.Path("/synthetic/x"), metadata=VideoMetadata())
    VideoDownloader._populate_raw(None, v, raw_backend.make_synthetic_clip(3, 4, 4, 30, seed=0))
    assert v.metadata.pixel_format == "nv12"


# ---- 5. decode session against the mock --------------------------------------

@pytest.fixture(scope="module")
def mock_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("mock_rocdecode16")
    subprocess.run(
        ["g++", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
         "-I/opt/rocm/include", str(MOCK_SRC), "-o", str(d / "librocdecode.so")],
        check=True,
    )
    return d


DRIVER = r"""
import ctypes
import json
import sys

sys.path.insert(0, ".")
from cosmos_curate_amd import hotpath

lib = hotpath.load()
assert lib.cc_rocdecode_available() == 0, lib.cc_last_error().decode()
mock = ctypes.CDLL("librocdecode.so")

out = {}
s = hotpath.DecodeSession(device=0, codec=1)
try:
    s.stream_format()
    out["format_before_sps"] = "returned"
except RuntimeError as e:
    out["format_before_sps"] = str(e)
try:
    for i in range(3):
        s.submit(b"\x00\x00\x00\x01\x26" + bytes([i]) * 16, pts=1000 * (i + 1))
    frames = s.map_frames(cap=8)
    f = s.stream_format()
    out.update(
        n=len(frames),
        fmt=[f.bit_depth, f.chroma_format, f.matrix_coefficients, f.full_range,
             f.bytes_per_sample],
        pitch=[fr.pitch for fr in frames],
        uv_minus_y=[fr.uv - fr.y for fr in frames],
        wh=[[fr.width, fr.height] for fr in frames],
        output_format=mock.mock_output_format(),
    )
    s.recycle()
except RuntimeError as e:
    out["error"] = str(e)
s.close()
print(json.dumps(out))
"""


def run_mock(mock_dir, **env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MOCK_ROCDEC_")}
    env["LD_LIBRARY_PATH"] = str(mock_dir)
    env.update({k: str(v) for k, v in env_extra.items()})
    r = subprocess.run([sys.executable, "-c", DRIVER], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


P016, NV12, CHROMA_420 = 1, 0, 1  # rocDecVideoSurfaceFormat / ChromaFormat values


def test_session_10bit_bt709_maps_p016(mock_dir):
    out = run_mock(mock_dir, MOCK_ROCDEC_BIT_DEPTH=10, MOCK_ROCDEC_MATRIX=1)
    assert "error" not in out, out
    assert "cc error -1" in out["format_before_sps"]  # CC_ERR_INVALID before the SPS
    assert out["output_format"] == P016
    assert out["fmt"] == [10, CHROMA_420, 1, 0, 2]
    assert out["n"] == 3
    assert out["pitch"] == [128] * 3
    # the mock puts the UV plane pitch x coded height (32 rows) after Y
    assert out["uv_minus_y"] == [128 * 32] * 3
    assert out["wh"] == [[48, 30]] * 3


def test_session_12bit_full_range_bt2020(mock_dir):
    out = run_mock(mock_dir, MOCK_ROCDEC_BIT_DEPTH=12, MOCK_ROCDEC_MATRIX=9,
                   MOCK_ROCDEC_FULL_RANGE=1)
    assert "error" not in out, out
    assert out["output_format"] == P016
    assert out["fmt"] == [12, CHROMA_420, 9, 1, 2]
    assert out["pitch"] == [128] * 3


def test_session_14bit_is_loudly_unsupported(mock_dir):
    out = run_mock(mock_dir, MOCK_ROCDEC_BIT_DEPTH=14)
    assert "cc error -6" in out["error"], out  # CC_ERR_UNSUPPORTED
    assert "14" in out["error"]
    assert "n" not in out


def test_session_default_is_still_8bit_nv12(mock_dir):
    out = run_mock(mock_dir)
    assert "error" not in out, out
    assert out["output_format"] == NV12
    assert out["fmt"] == [8, CHROMA_420, 0, 0, 1]
    assert out["pitch"] == [64] * 3
    assert out["uv_minus_y"] == [0x8000] * 3


# ---- 6. stage constructor --------------------------------------------------

def test_color_standard_is_validated():
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        ClipFrameExtractionStage,
    )

    with pytest.raises(ValueError):
        ClipFrameExtractionStage(color_standard="nope")
    for ok in ("bt601", "bt709", "bt2020", "stream"):
        ClipFrameExtractionStage(color_standard=ok)
    s = ClipFrameExtractionStage(color_standard="stream")
    assert s._color(2, True) == (2, True)
    assert ClipFrameExtractionStage()._color(2, True) == (0, False)
    assert ClipFrameExtractionStage(color_standard="bt709")._color(0, True) == (1, False)
