"""PQ (HDR10) -> SDR tone mapping: everything that needs no GPU.

The table builder against the numpy restatement (tests/hdr_ref.py), the f32
table chain against the float64 closed form, the version-3 raw payload, the
stage and CLI arguments, and the decode session's transfer query against the
mocked librocdecode.  The kernels themselves are pinned in test_gpu_hdr.py.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import hdr_ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.pipelines.video.utils import raw_backend

ROOT = pathlib.Path(__file__).resolve().parent.parent
MOCK_SRC = ROOT / "tools" / "mock_rocdecode.cpp"

CC_ERR_INVALID, CC_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def lib_tables():
    """(tin, tout) of cc_hdr_tables_build(PQ, 203)."""
    return hdr_ref.split_image(hotpath.hdr_tables_build(hotpath.HDR_TRANSFER_PQ, 203.0))


# ---- 1. tables ---------------------------------------------------------------

def _ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in f32 steps between non-negative f32 arrays."""
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("white", (203.0, 100.0))
def test_tables_match_the_numpy_restatement(white):
    img = hotpath.hdr_tables_build(hotpath.HDR_TRANSFER_PQ, white)
    assert img.dtype == np.uint8 and img.shape == (hotpath.HDR_TABLE_BYTES,)
    assert hotpath.HDR_TABLE_BYTES == hdr_ref.TABLE_BYTES == 20480
    tin, tout = hdr_ref.split_image(img)
    want_in, want_out = hdr_ref.tables(white)
    assert int(_ulp_distance(tin, want_in).max()) <= 1
    assert int(np.abs(tout.astype(np.int32) - want_out.astype(np.int32)).max()) <= 1
    used = tin[:hdr_ref.N_IN]
    assert (np.diff(used) >= 0).all() and (np.diff(tout.astype(np.int32)) >= 0).all()
    assert tin[0] == 0 and tout[0] == 0 and tout[4095] == 255
    assert (tin[hdr_ref.N_IN:] == 0).all() and tin[hdr_ref.N_IN:].size == 15
    # the last used entry is the PQ peak over reference white
    assert abs(float(used[-1]) - 10000.0 / white) <= 1e-6 * 10000.0 / white


def test_tables_reject_what_they_cannot_build():
    lib = hotpath.load()
    buf = np.full(hotpath.HDR_TABLE_BYTES, 0x5A, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for transfer in (0, 2, 16, 18, -1):  # only code 1 (PQ) has tables; HLG does not
        assert lib.cc_hdr_tables_build(transfer, 203.0, p) == CC_ERR_UNSUPPORTED, transfer
        assert lib.cc_last_error().decode()
    for white in (0.0, -203.0, float("inf"), float("nan")):
        assert lib.cc_hdr_tables_build(1, white, p) == CC_ERR_INVALID, white
        assert lib.cc_last_error().decode()
    assert lib.cc_hdr_tables_build(1, 203.0, None) == CC_ERR_INVALID
    assert (buf == 0x5A).all()  # nothing written by a rejected call
    with pytest.raises(RuntimeError):
        hotpath.hdr_tables_build(18, 203.0)


# ---- 2. accuracy of the f32 table chain --------------------------------------

@pytest.fixture(scope="module")
def triples() -> np.ndarray:
    """Fixed-seed R'G'B' triples on the 8-bit scale: 1M over [-5, 260]^3
    (sub-black and super-white included) plus 0.5M near-neutral."""
    rng = np.random.default_rng(2084)
    wide = rng.uniform(-5.0, 260.0, (1_000_000, 3))
    grey = rng.uniform(0.0, 255.0, (500_000, 1)) + rng.normal(0.0, 3.0, (500_000, 3))
    return np.concatenate([wide, grey]).astype(np.float32)


@pytest.mark.parametrize("peak", (1000.0, 4000.0))
def test_f32_chain_against_the_float64_closed_form(lib_tables, triples, peak):
    """Bounds from the CPU prototype of the chain: the f32 table chain stays
    within 0.55 code of the unrounded float64 value (0.5 of that is the
    output rounding itself), so 0.6 here, and never more than one code from
    the rounded float64 value."""
    tin, tout = lib_tables
    got = hdr_ref.chain_f32(triples, tin, tout, hdr_ref.inv_w2(peak)).astype(np.float64)
    want = hdr_ref.chain_f64(triples, peak)
    off_rounded = np.abs(got - np.floor(want + 0.5))
    off_exact = np.abs(got - want)
    print(f"peak {peak:g}: max |f32 - round(f64)| {off_rounded.max():g} codes, "
          f"share differing {np.mean(off_rounded > 0):.4f}, "
          f"max |f32 - f64| {off_exact.max():.4f} codes")
    assert off_rounded.max() <= 1.0
    assert off_exact.max() <= 0.6
    assert got.min() == 0 and got.max() == 255  # the sample reaches both ends


def test_inv_w2_is_the_f32_of_the_double_value():
    assert hotpath.hdr_inv_w2(1000.0, 203.0) == float(hdr_ref.inv_w2(1000.0, 203.0))
    assert hotpath.hdr_inv_w2(4000.0) == float(np.float32(1.0 / (4000.0 / 203.0) ** 2))
    with pytest.raises(ValueError):
        hotpath.hdr_inv_w2(0.0)


def test_a_pixel_at_peak_maps_to_white(lib_tables):
    """Extended Reinhard: luminance `peak` on a neutral pixel gives 1.0,
    reference white stays well below it."""
    tin, tout = lib_tables
    for peak in (1000.0, 4000.0):
        codes = np.arange(hdr_ref.N_IN) / 16.0
        grey = np.repeat(codes[:, None], 3, axis=1).astype(np.float32)
        out = hdr_ref.chain_f32(grey, tin, tout, hdr_ref.inv_w2(peak))[:, 0].astype(int)
        assert (np.diff(out) >= 0).all()
        nits = hdr_ref.pq_eotf_nits(np.arange(hdr_ref.N_IN) / 4080.0)
        at_peak = int(np.searchsorted(nits, peak))
        assert out[at_peak] >= 254 and out[-1] == 255
        # L = 1 gives 255*((1 + inv_w2)/2)^(1/2.4): 191 (peak -> inf) to 195
        assert 189 <= out[int(np.searchsorted(nits, 203.0))] <= 197


# ---- 3. raw payload, version 3 -----------------------------------------------

# pack_header(...) of the arguments below, captured from the commit before
# version 3 existed
V1_HEADER_LITERAL = bytes.fromhex(
    "43434e5631325241570001000500000006000000080000001900000001000000")
V2_HEADER_10_BT709 = bytes.fromhex(
    "43434e56313252415700020005000000060000000800000030750000e9030a01")
V2_HEADER_12_BT2020_FULL = bytes.fromhex(
    "43434e56313252415700020007000000040000000c0000001900000001000c82")


def test_version1_and_version2_bytes_unchanged():
    assert raw_backend.pack_header(5, 6, 8, 25) == V1_HEADER_LITERAL
    assert raw_backend.pack_header(5, 6, 8, 25, transfer=0) == V1_HEADER_LITERAL
    assert raw_backend.pack_header(
        5, 6, 8, 30000, 1001, bit_depth=10, matrix=1) == V2_HEADER_10_BT709
    assert raw_backend.pack_header(
        5, 6, 8, 30000, 1001, bit_depth=10, matrix=1, transfer=0) == V2_HEADER_10_BT709
    assert raw_backend.pack_header(
        7, 4, 12, 25, bit_depth=12, matrix=2, full_range=True,
        transfer=0) == V2_HEADER_12_BT2020_FULL
    for hdr, fmt in ((V1_HEADER_LITERAL, (8, 0, False, 1)),
                     (V2_HEADER_10_BT709, (10, 1, False, 2)),
                     (V2_HEADER_12_BT2020_FULL, (12, 2, True, 2))):
        assert raw_backend.parse_format(hdr) == fmt
        assert raw_backend.parse_transfer(hdr) == 0


@pytest.mark.parametrize("depth,matrix,full_range", [(10, 2, False), (12, 1, True)])
def test_version3_round_trip(depth, matrix, full_range):
    rng = np.random.default_rng(3)
    n, h, w = 4, 6, 10
    y = rng.integers(0, 1 << 16, size=(n, h, w), dtype=np.uint16)
    uv = rng.integers(0, 1 << 16, size=(n, h // 2, w), dtype=np.uint16)
    kw = dict(bit_depth=depth, matrix=matrix, full_range=full_range)
    data = raw_backend.encode_raw_p016(y, uv, 30000, 1001, transfer=1, **kw)
    v2 = raw_backend.encode_raw_p016(y, uv, 30000, 1001, **kw)
    assert len(data) == len(v2) == 32 + n * (h * w + h // 2 * w) * 2
    assert data[:32] == raw_backend.pack_header(n, h, w, 30000, 1001, transfer=1, **kw)
    # version 3 = version 2 + the version number + bits 2..3 of the colour byte
    assert data[10:12] == (3).to_bytes(2, "little") and v2[10:12] == (2).to_bytes(2, "little")
    assert data[31] == v2[31] | (1 << 2)
    assert data[:10] == v2[:10] and data[12:31] == v2[12:31] and data[32:] == v2[32:]
    assert raw_backend.is_raw_nv12(data)
    assert raw_backend.parse_transfer(data) == 1 and raw_backend.parse_transfer(v2) == 0
    fmt = raw_backend.parse_format(data)
    assert fmt == (depth, matrix, full_range, 2) and len(fmt) == 4
    assert raw_backend.parse_header(data) == (n, h, w, 30000 / 1001)
    assert raw_backend.frame_nbytes(data) == raw_backend.frame_nbytes(v2)
    idx = np.array([3, 0], dtype=np.int32)
    ys, uvs = raw_backend.frame_planes(data, idx)
    np.testing.assert_array_equal(ys, y[idx])
    np.testing.assert_array_equal(uvs, uv[idx])
    np.testing.assert_array_equal(raw_backend.timestamps(data), raw_backend.timestamps(v2))


def test_bad_transfer_is_rejected():
    for transfer in (2, 3, -1, 16):
        with pytest.raises(ValueError):
            raw_backend.pack_header(1, 2, 2, 30, bit_depth=10, transfer=transfer)
    with pytest.raises(ValueError):
        raw_backend.pack_header(1, 2, 2, 30, transfer=1)  # version 1 has no room
    good = bytearray(raw_backend.pack_header(1, 2, 2, 30, bit_depth=10, matrix=2,
                                             transfer=1))
    assert raw_backend.parse_transfer(bytes(good)) == 1
    for value in (2, 3):  # transfers no payload may carry
        bad = bytearray(good)
        bad[31] = (bad[31] & ~0x0C) | (value << 2)
        for parse in (raw_backend.parse_transfer, raw_backend.parse_format,
                      raw_backend.parse_header):
            with pytest.raises(AssertionError):
                parse(bytes(bad))
    # a version-2 header has no transfer bits: set, they are a bad matrix
    v2 = bytearray(raw_backend.pack_header(1, 2, 2, 30, bit_depth=10))
    v2[31] |= 1 << 2
    with pytest.raises(AssertionError):
        raw_backend.parse_format(bytes(v2))
    bad_version = bytearray(good)
    bad_version[10] = 4
    with pytest.raises(AssertionError):
        raw_backend.parse_transfer(bytes(bad_version))


def test_synthetic_clip_and_slice_keep_the_transfer():
    from cosmos_curate_amd.pipelines.video.clipping.clip_extraction_stages import (
        _slice_raw_clip,
    )

    kw = dict(bit_depth=10, matrix=2)
    pq = raw_backend.make_synthetic_clip_p016(60, 8, 12, 30, seed=2, transfer=1, **kw)
    sdr = raw_backend.make_synthetic_clip_p016(60, 8, 12, 30, seed=2, **kw)
    assert raw_backend.parse_transfer(pq) == 1 and raw_backend.parse_transfer(sdr) == 0
    assert pq[32:] == sdr[32:]  # the transfer only labels the samples
    part = bytes(_slice_raw_clip(pq, (0.5, 1.2)))  # frames 15..35
    assert raw_backend.parse_header(part) == (21, 8, 12, 30.0)
    assert raw_backend.parse_format(part) == (10, 2, False, 2)
    assert raw_backend.parse_transfer(part) == 1
    part_sdr = bytes(_slice_raw_clip(sdr, (0.5, 1.2)))
    assert raw_backend.parse_transfer(part_sdr) == 0 and part_sdr[32:] == part[32:]


# ---- 4. stage and CLI ----------------------------------------------------------

def test_stage_hdr_arguments_are_validated():
    from cosmos_curate_amd.pipelines.video.clipping.clip_frame_extraction_stages import (
        ClipFrameExtractionStage,
    )

    s = ClipFrameExtractionStage()
    assert (s._hdr, s._hdr_peak_nits, s._hdr_white_nits) == ("off", 1000.0, 203.0)
    s = ClipFrameExtractionStage(hdr="tonemap", hdr_peak_nits=4000,
                                 hdr_reference_white_nits=100.0)
    assert (s._hdr, s._hdr_peak_nits, s._hdr_white_nits) == ("tonemap", 4000.0, 100.0)
    for bad in ("on", "hlg", "", None, True):
        with pytest.raises(ValueError):
            ClipFrameExtractionStage(hdr=bad)
    for bad in (0, -1000.0, float("inf"), float("nan"), "1000", None, True):
        with pytest.raises(ValueError):
            ClipFrameExtractionStage(hdr="tonemap", hdr_peak_nits=bad)
        with pytest.raises(ValueError):
            ClipFrameExtractionStage(hdr="tonemap", hdr_reference_white_nits=bad)
    with pytest.raises(ValueError):  # a peak below diffuse white
        ClipFrameExtractionStage(hdr="tonemap", hdr_peak_nits=100.0)
    # validated under "off" too, like color_standard
    with pytest.raises(ValueError):
        ClipFrameExtractionStage(hdr_peak_nits=-1.0)


def test_extract_frames_takes_the_hdr_arguments():
    import inspect

    from cosmos_curate_amd.pipelines.video.clipping import clip_frame_extraction_stages as m

    params = inspect.signature(m.extract_frames).parameters
    assert params["hdr"].default == "off"
    assert params["hdr_peak_nits"].default == 1000.0
    assert params["hdr_reference_white_nits"].default == 203.0
    with pytest.raises(ValueError):  # reaches the stage constructor's checks
        m.extract_frames(b"", sample_rate_fps=1.0, hdr="nope")


def _split_args(tmp_path, *extra):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _setup_parser

    (tmp_path / "in").mkdir(exist_ok=True)
    p = argparse.ArgumentParser()
    _setup_parser(p)
    return p.parse_args(["--input-video-path", str(tmp_path / "in"),
                         "--output-clip-path", str(tmp_path / "out"), *extra])


def test_cli_hdr_off_builds_todays_stage_list(tmp_path):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _assemble_stages

    def names(args):
        return [type(st.stage if hasattr(st, "stage") else st).__name__
                for st in _assemble_stages(args)]

    today = ["VideoDownloader", "FixedStrideExtractorStage", "ClipTranscodingStage",
             "ClipFrameExtractionStage", "ClipFrameCreationStage", "ClipEmbeddingStage",
             "ClipWriterStage"]
    default = _split_args(tmp_path)
    assert (default.hdr, default.hdr_peak_nits) == ("off", 1000.0)
    assert names(default) == today
    assert names(_split_args(tmp_path, "--hdr", "off")) == today
    assert names(_split_args(tmp_path, "--hdr", "tonemap")) == today
    with pytest.raises(SystemExit):
        _split_args(tmp_path, "--hdr", "hlg")
    stage = _assemble_stages(_split_args(tmp_path, "--hdr", "tonemap",
                                         "--hdr-peak-nits", "4000"))[3]
    stage = stage.stage if hasattr(stage, "stage") else stage
    assert (stage._hdr, stage._hdr_peak_nits) == ("tonemap", 4000.0)


def test_cli_dry_run_shows_the_option(tmp_path, capsys):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import split

    summary = split(_split_args(tmp_path, "--dry-run", "--hdr", "tonemap",
                                "--hdr-peak-nits", "4000"))
    assert summary["dry_run"] and summary["num_stages"] == 7
    shown = capsys.readouterr().out.splitlines()
    assert "ClipFrameExtractionStage hdr=tonemap hdr_peak_nits=4000" in shown
    split(_split_args(tmp_path, "--dry-run", "--hdr", "off"))
    off = capsys.readouterr().out.splitlines()
    assert "ClipFrameExtractionStage" in off and not any("hdr" in line for line in off)
    assert len(off) == len(shown) == 7


# ---- 5. decode session against the mock ----------------------------------------

@pytest.fixture(scope="module")
def mock_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("mock_rocdecode_hdr")
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

out = {}
s = hotpath.DecodeSession(device=0, codec=1)
tc, cp = ctypes.c_int32(-7), ctypes.c_int32(-7)
out["rc_before_sps"] = lib.cc_decode_stream_transfer(s._h, ctypes.byref(tc), ctypes.byref(cp))
out["untouched_before_sps"] = [tc.value, cp.value]
try:
    s.stream_transfer()
    out["before_sps"] = "returned"
except RuntimeError as e:
    out["before_sps"] = str(e)
for i in range(2):
    s.submit(b"\x00\x00\x00\x01\x26" + bytes([i]) * 16, pts=1000 * (i + 1))
frames = s.map_frames(cap=8)
f = s.stream_format()
out["transfer"] = list(s.stream_transfer())
out["fmt"] = [f.bit_depth, f.chroma_format, f.matrix_coefficients, f.full_range,
              f.bytes_per_sample]
out["sizeof_format"] = ctypes.sizeof(hotpath.StreamFormat)
# either output may be omitted
out["rc_null_outputs"] = lib.cc_decode_stream_transfer(s._h, None, None)
out["rc_null_session"] = lib.cc_decode_stream_transfer(None, ctypes.byref(tc), ctypes.byref(cp))
s.recycle()
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


def test_session_reports_pq_and_bt2020(mock_dir):
    out = run_mock(mock_dir, MOCK_ROCDEC_BIT_DEPTH=10, MOCK_ROCDEC_MATRIX=9,
                   MOCK_ROCDEC_TRANSFER=16, MOCK_ROCDEC_PRIMARIES=9)
    assert out["rc_before_sps"] == CC_ERR_INVALID
    assert out["untouched_before_sps"] == [-7, -7]
    assert "cc error -1" in out["before_sps"]
    assert out["transfer"] == [16, 9]
    assert out["fmt"] == [10, 1, 9, 0, 2]  # cc_stream_format as before
    assert out["sizeof_format"] == 20      # and its layout
    assert out["rc_null_outputs"] == 0
    assert out["rc_null_session"] == CC_ERR_INVALID


def test_session_defaults_leave_the_transfer_unset(mock_dir):
    out = run_mock(mock_dir)
    assert out["transfer"] == [0, 0]
    assert out["fmt"] == [8, 1, 0, 0, 1]
    out = run_mock(mock_dir, MOCK_ROCDEC_TRANSFER=18, MOCK_ROCDEC_PRIMARIES=1)
    assert out["transfer"] == [18, 1]  # HLG is reported, not tone-mapped
