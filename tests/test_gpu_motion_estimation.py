"""cc_motion_estimate on the MI355X: bit-exact against tests/motion_est_ref.py
at the smallest shapes where each path can break, then the Python layer and
the two motion stages end to end on real kernel output.

Every rejected call below returns before any launch; nothing here hands a
kernel a bad pointer or size.
"""

from __future__ import annotations

import pathlib
import uuid

import numpy as np
import pytest
import torch

import motion_est_ref as ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces import SequentialRunner, run_pipeline
from cosmos_curate_amd.pipelines.video.filtering.motion import motion_estimation as me
from cosmos_curate_amd.pipelines.video.filtering.motion.motion_filter_stages import (
    MotionFilterStage,
    check_if_small_motion,
)
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import (
    Clip,
    SplitPipeTask,
    Video,
)
from oracle import motion as omotion

pytestmark = pytest.mark.gpu

MV_SENTINEL, COST_SENTINEL = 0x7B7B, 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def pitched(planes: np.ndarray, pitch_bytes: int | None) -> np.ndarray:
    """(n, h, w) samples -> the same rows `pitch_bytes` apart, padding
    filled with 0xA5 so a stray read would show."""
    n, h, w = planes.shape
    if pitch_bytes is None:
        return np.ascontiguousarray(planes)
    per = pitch_bytes // planes.itemsize
    buf = np.full((n, h, per), 0xA5A5 if planes.itemsize == 2 else 0xA5,
                  dtype=planes.dtype)
    buf[:, :, :w] = planes
    return buf


def _dev(arr: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def outputs(n: int, h: int, w: int) -> tuple[torch.Tensor, torch.Tensor]:
    nby, nbx = -(-h // 16), -(-w // 16)
    mv = torch.full((n, nby, nbx, 2), MV_SENTINEL, dtype=torch.int16, device="cuda")
    cost = torch.full((n, nby, nbx), COST_SENTINEL, dtype=torch.int32, device="cuda")
    return mv, cost


def launch(lib, cur_ptr, ref_ptr, n, h, w, pitch, stride, bps, rng_, lam):
    mv, cost = outputs(n, h, w)
    hotpath.check(lib.cc_motion_estimate(
        cur_ptr, ref_ptr, n, h, w, pitch, stride, bps, rng_, lam,
        mv.data_ptr(), cost.data_ptr(), 0))
    torch.cuda.synchronize()
    return mv.cpu().numpy(), cost.cpu().numpy().view(np.uint32)


def estimate(lib, cur: np.ndarray, rf: np.ndarray, search_range: int, lam: int,
             pitch_bytes: int | None = None):
    """Separate cur / ref allocations, rows `pitch_bytes` apart."""
    n, h, w = cur.shape
    bps = cur.itemsize
    pitch = pitch_bytes or w * bps
    cd, rd = _dev(pitched(cur, pitch_bytes)), _dev(pitched(rf, pitch_bytes))
    return launch(lib, cd.data_ptr(), rd.data_ptr(), n, h, w, pitch, pitch * h, bps,
                  search_range, lam)


def assert_matches_ref(got, cur, rf, search_range, lam, msg=""):
    want_mv, want_cost = ref.estimate(cur, rf, search_range, lam)
    np.testing.assert_array_equal(got[0], want_mv, err_msg=f"mv {msg}")
    np.testing.assert_array_equal(got[1], want_cost, err_msg=f"cost {msg}")


def rand8(seed: int, *shape: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---- 1. bit-exact at the shapes where a path can break ------------------------

@pytest.mark.parametrize("search_range", [1, 32])
def test_one_block_whole_window_is_replicated_edge(lib, search_range):
    f = rand8(10, 2, 1, 16, 16)
    got = estimate(lib, f[0], f[1], search_range, 4)
    assert_matches_ref(got, f[0], f[1], search_range, 4)


@pytest.mark.parametrize("lam", [0, 9])
def test_partial_blocks_odd_range_unaligned_rows(lib, lam):
    f = rand8(11, 2, 1, 18, 34)
    got = estimate(lib, f[0], f[1], 7, lam, pitch_bytes=40)
    assert_matches_ref(got, f[0], f[1], 7, lam)


def test_odd_pitch_and_odd_base_address(lib):
    """Nothing beyond sample alignment is assumed: 8-bit rows 35 bytes
    apart, off an odd base address."""
    f = rand8(12, 2, 1, 18, 34)
    cd = _dev(np.concatenate([[np.uint8(0xA5)], pitched(f[0], 35).reshape(-1)]))
    rd = _dev(np.concatenate([[np.uint8(0xA5)], pitched(f[1], 35).reshape(-1)]))
    got = launch(lib, cd.data_ptr() + 1, rd.data_ptr() + 1, 1, 18, 34, 35, 35 * 18,
                 1, 7, 3)
    assert_matches_ref(got, f[0], f[1], 7, 3)


def test_several_blocks_and_frames(lib):
    f = rand8(13, 2, 3, 48, 80)
    got = estimate(lib, f[0], f[1], 16, 4, pitch_bytes=128)
    assert_matches_ref(got, f[0], f[1], 16, 4)


def test_overlapping_frames_in_one_allocation(lib):
    """cur = ref advanced by one frame: pair f is (frame f+1, frame f)."""
    f = rand8(14, 4, 48, 80)
    buf = _dev(pitched(f, 128))
    got = launch(lib, buf.data_ptr() + 128 * 48, buf.data_ptr(), 3, 48, 80, 128,
                 128 * 48, 1, 16, 4)
    assert_matches_ref(got, f[1:], f[:-1], 16, 4)


def test_16bit_samples_equal_the_8bit_result_on_the_high_byte(lib):
    s = np.random.default_rng(15).integers(0, 1 << 16, size=(2, 2, 24, 40),
                                           dtype=np.uint16)
    got16 = estimate(lib, s[0], s[1], 16, 4)
    assert_matches_ref(got16, s[0], s[1], 16, 4)
    hi = (s >> 8).astype(np.uint8)
    got8 = estimate(lib, hi[0], hi[1], 16, 4)
    np.testing.assert_array_equal(got16[0], got8[0])
    np.testing.assert_array_equal(got16[1], got8[1])
    # pitched 16-bit rows off a 2-byte (not 8-byte) aligned pitch
    got16p = estimate(lib, s[0], s[1], 16, 4, pitch_bytes=86)
    np.testing.assert_array_equal(got16p[0], got16[0])
    np.testing.assert_array_equal(got16p[1], got16[1])


def test_tie_breaks_on_device(lib):
    c = np.full((1, 18, 34), 93, dtype=np.uint8)
    got = estimate(lib, c, c, 7, 0)
    assert not got[0].any() and not got[1].any()
    assert_matches_ref(got, c, c, 7, 0, "constant")
    s = ref.stripes(32, 48, period=8)[None]
    cur = np.roll(s, 4, axis=2)
    got = estimate(lib, cur, s, 16, 0)
    assert (got[0][0, :, 1] == np.array([-4, 0], dtype=np.int16)).all()
    assert_matches_ref(got, cur, s, 16, 0, "stripes")


def test_smooth_content_with_near_ties(lib):
    clip = raw_backend.make_synthetic_clip(3, 48, 80, 30, seed=16)
    ys, _ = raw_backend.frame_planes(clip, np.arange(3, dtype=np.int32))
    got = estimate(lib, ys[1:], ys[:-1], 16, 4)
    assert_matches_ref(got, ys[1:], ys[:-1], 16, 4)


def test_same_call_twice_gives_identical_bytes(lib):
    f = rand8(17, 2, 3, 48, 80)
    a = estimate(lib, f[0], f[1], 16, 4, pitch_bytes=128)
    b = estimate(lib, f[0], f[1], 16, 4, pitch_bytes=128)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_cost_output_is_optional(lib):
    f = rand8(18, 2, 1, 18, 34)
    cd, rd = _dev(f[0]), _dev(f[1])
    mv, _ = outputs(1, 18, 34)
    hotpath.estimate_motion(cd.data_ptr(), rd.data_ptr(), 1, 18, 34, 34,
                            mv.data_ptr(), 0, search_range=7, mv_lambda=9)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mv.cpu().numpy(), ref.estimate(f[0], f[1], 7, 9)[0])


# ---- 2. error paths: rejected before any launch ------------------------------

def test_rejections_leave_the_outputs_untouched(lib):
    n, h, w, pitch = 2, 18, 34, 80
    buf = torch.zeros(n * h * pitch + 8, dtype=torch.uint8, device="cuda")
    mv, cost = outputs(n, h, w)
    good = dict(cur=buf.data_ptr(), ref=buf.data_ptr(), n=n, h=h, w=w, pitch=pitch,
                stride=pitch * h, bps=2, R=16, lam=4, mv=mv.data_ptr(),
                cost=cost.data_ptr())
    invalid = {
        "null cur": dict(cur=None), "null ref": dict(ref=None), "null mv": dict(mv=None),
        "n 0": dict(n=0), "h 0": dict(h=0), "w -3": dict(w=-3),
        "range 0": dict(R=0), "range 33": dict(R=33),
        "lambda -1": dict(lam=-1), "lambda 256": dict(lam=256),
        "bps 0": dict(bps=0), "bps 3": dict(bps=3), "bps 4": dict(bps=4),
        "pitch < row bytes": dict(pitch=66, stride=66 * h),
        "pitch < row bytes (8 bit)": dict(bps=1, pitch=33, stride=33 * h),
        "stride < plane": dict(stride=pitch * h - 2),
        "odd pitch at 16 bit": dict(pitch=81, stride=81 * h + 1),
        "odd stride at 16 bit": dict(stride=pitch * h + 1),
        "odd cur at 16 bit": dict(cur=buf.data_ptr() + 1),
        "odd ref at 16 bit": dict(ref=buf.data_ptr() + 1),
    }
    unsupported = {
        "too many pairs": dict(n=65536),
        "too many block rows": dict(h=16 * 65535 + 1, stride=pitch * (16 * 65535 + 1)),
        "too many blocks": dict(n=4096, h=16 * 64, w=16 * 64, pitch=2048,
                                stride=2048 * 1024),
    }
    for want_rc, table in ((-1, invalid), (-6, unsupported)):
        for name, change in table.items():
            a = dict(good, **change)
            rc = lib.cc_motion_estimate(
                a["cur"], a["ref"], a["n"], a["h"], a["w"], a["pitch"], a["stride"],
                a["bps"], a["R"], a["lam"], a["mv"], a["cost"], 0)
            assert rc == want_rc, name
            assert lib.cc_last_error().decode(), name
    torch.cuda.synchronize()
    assert bool((mv == MV_SENTINEL).all()) and bool((cost == COST_SENTINEL).all())
    # the unchanged arguments are accepted
    a = good
    hotpath.check(lib.cc_motion_estimate(
        a["cur"], a["ref"], a["n"], a["h"], a["w"], a["pitch"], a["stride"], a["bps"],
        a["R"], a["lam"], a["mv"], a["cost"], 0))
    torch.cuda.synchronize()
    assert not bool((mv == MV_SENTINEL).any()) and not bool((cost == COST_SENTINEL).any())


# ---- 3. the Python layer and the stages ---------------------------------------

N_FRAMES, SIDE, FPS = 31, 256, 30
PAIRS = [(14, 15), (29, 30)]


def nv12_payload(y: np.ndarray) -> bytes:
    uv = np.full((y.shape[0], y.shape[1] // 2, y.shape[2]), 128, dtype=np.uint8)
    return raw_backend.encode_raw_nv12(y, uv, FPS)


@pytest.fixture(scope="module")
def moving() -> np.ndarray:
    return ref.translating(N_FRAMES, SIDE, SIDE, seed=20, step=(3, -2))


@pytest.fixture(scope="module")
def moving_rows(moving) -> list[np.ndarray]:
    """Reference expansion for the sampled pairs, computed once."""
    return [ref.rows(ref.estimate_pair(moving[c], moving[p], 16, 4)[0])
            for p, c in PAIRS]


def check_clip(md, want_rows):
    assert md.frame_size == (SIDE, SIDE) and len(md.frames) == 2
    for got, want in zip(md.frames, want_rows):
        assert got.shape == (256, 10) and got.dtype == np.float32
        np.testing.assert_array_equal(got, want)
    small, patch_min, gmean = check_if_small_motion(md.frames, md.frame_size)
    small_o, patch_o, gmean_o = omotion.check_if_small_motion(md.frames, md.frame_size)
    assert small == small_o
    assert gmean == pytest.approx(gmean_o, rel=1e-5)
    assert patch_min == pytest.approx(patch_o, rel=1e-5)


def test_estimate_clip_motion_8bit(lib, moving, moving_rows):
    assert me.motion_sample_pairs(N_FRAMES, FPS) == PAIRS
    check_clip(me.estimate_clip_motion(nv12_payload(moving)), moving_rows)


def test_estimate_clip_motion_10bit(lib, moving, moving_rows):
    # the same content as 10-bit codes (<< 2), MSB-aligned (<< 6)
    y = (moving.astype(np.uint16) << 2) << 6
    uv = np.full((N_FRAMES, SIDE // 2, SIDE), 512 << 6, dtype=np.uint16)
    data = raw_backend.encode_raw_p016(y, uv, FPS, bit_depth=10)
    check_clip(me.estimate_clip_motion(data), moving_rows)


def test_estimate_clip_motion_chained_pairs(lib):
    """fps == target fps: consecutive pairs share frames (cur = ref + one
    frame on the device)."""
    f = ref.translating(4, SIDE, SIDE, seed=21, step=(-1, 2))
    uv = np.full((4, SIDE // 2, SIDE), 128, dtype=np.uint8)
    md = me.estimate_clip_motion(raw_backend.encode_raw_nv12(f, uv, 2))
    assert len(md.frames) == 3
    for k, got in enumerate(md.frames):
        np.testing.assert_array_equal(
            got, ref.rows(ref.estimate_pair(f[k + 1], f[k], 16, 4)[0]))


def test_stages_end_to_end(lib, moving):
    def clip(name: str, y: np.ndarray) -> Clip:
        return Clip(uuid=uuid.uuid5(uuid.NAMESPACE_URL, name), source_video="s",
                    span=(0.0, N_FRAMES / FPS),
                    encoded_data=np.frombuffer(nv12_payload(y), dtype=np.uint8))

    video = Video(input_video=pathlib.Path("/synthetic/motion.bin"))
    video.clips = [clip("moving", moving),
                   clip("static", ref.static_with_noise(N_FRAMES, SIDE, SIDE, seed=22))]
    out = run_pipeline(
        [SplitPipeTask(videos=[video])],
        [me.MotionVectorEstimationStage(), MotionFilterStage()],
        runner=SequentialRunner())
    v = out[0].video
    assert len(v.clips) == 1 and len(v.filtered_clips) == 1
    kept, dropped = v.clips[0], v.filtered_clips[0]
    assert kept.uuid == uuid.uuid5(uuid.NAMESPACE_URL, "moving")
    assert kept.motion_score_global_mean > 0.00098
    assert dropped.motion_score_global_mean == 0.0
    assert v.clip_stats.num_filtered_by_motion == 1
    for c in (kept, dropped):
        assert "motion" not in c.errors and "motion_decode" not in c.errors, c.errors
