"""Motion estimation without a GPU: the numpy reference's own sanity, the
MV row expansion, the sampling rule, the stage's header-only error paths
and the driver's stage list."""

from __future__ import annotations

import argparse
import math
import pathlib
import uuid

import numpy as np
import pytest
import torch

import motion_est_ref as ref
from cosmos_curate_amd.pipelines.video.filtering.motion import motion_estimation as me
from cosmos_curate_amd.pipelines.video.filtering.motion.motion_filter_stages import (
    MotionFilterStage,
    motion_vectors_to_flowfield,
)
from cosmos_curate_amd.pipelines.video.splitting_pipeline import (
    _assemble_stages,
    _setup_parser,
    split,
)
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import (
    Clip,
    SplitPipeTask,
    Video,
)
from oracle import motion as omotion


def interior(a: np.ndarray) -> np.ndarray:
    """Blocks not in the first or last block row or column."""
    return a[1:-1, 1:-1]


# ---- reference self-checks ----------------------------------------------------

def test_reference_recovers_a_translation():
    f = ref.translating(2, 256, 256, seed=1, step=(3, -2))
    mv, _ = ref.estimate_pair(f[1], f[0], 16, 4)
    assert mv.shape == (16, 16, 2)
    assert (interior(mv) == np.array([-3, 2], dtype=np.int16)).all()
    rows = me.blocks_to_mv_rows(mv, 256, 256)
    small, _, gmean = omotion.check_if_small_motion([rows], (256, 256))
    assert gmean == pytest.approx(math.sqrt(13) / 512, rel=1e-6)
    assert small is False


def test_reference_static_content_with_noise_is_zero_motion():
    f = ref.static_with_noise(2, 256, 256, seed=1)
    assert (f[0] != f[1]).any()
    mv, _ = ref.estimate_pair(f[1], f[0], 16, 4)
    assert not mv.any()
    small, patch_min, gmean = omotion.check_if_small_motion(
        [me.blocks_to_mv_rows(mv, 256, 256)], (256, 256))
    assert (small, patch_min, gmean) == (True, 0.0, 0.0)


def test_reference_constant_frame_ties_resolve_to_zero():
    c = np.full((18, 34), 93, dtype=np.uint8)
    mv, cost = ref.estimate_pair(c, c, 7, 0)
    assert mv.shape == (2, 3, 2) and not mv.any() and not cost.any()


def test_reference_equal_length_ties_resolve_to_smaller_dx():
    s = ref.stripes(32, 48, period=8)
    mv, cost = ref.estimate_pair(np.roll(s, 4, axis=1), s, 16, 0)
    # period 8 rolled by 4: dx = -4 and +4 (and +-12) match equally, every
    # dy matches (the content is constant along y, so every block row is
    # interior to it); the middle block column is clear of the border
    assert (mv[:, 1] == np.array([-4, 0], dtype=np.int16)).all()
    assert not cost[:, 1].any()


def test_reference_16bit_ignores_low_bits():
    rng = np.random.default_rng(2)
    a8 = rng.integers(0, 256, size=(2, 24, 40), dtype=np.uint8)
    junk = rng.integers(0, 256, size=a8.shape).astype(np.uint16)
    a16 = (a8.astype(np.uint16) << 8) | junk
    for got, want in zip(ref.estimate_pair(a16[1], a16[0], 5, 3),
                         ref.estimate_pair(a8[1], a8[0], 5, 3)):
        np.testing.assert_array_equal(got, want)


# ---- blocks_to_mv_rows ----------------------------------------------------------

FIELD = np.array([[[0, 0], [3, -2], [-16, 16]],
                  [[1, 0], [0, -1], [7, 7]]], dtype=np.int16)


@pytest.mark.parametrize("size", [(32, 48), (20, 37)], ids=["multiple", "partial"])
def test_blocks_to_mv_rows(size):
    h, w = size
    rows = me.blocks_to_mv_rows(FIELD, h, w)
    assert rows.shape == (6, 10) and rows.dtype == np.float32
    np.testing.assert_array_equal(rows, ref.rows(FIELD))
    # raster order and columns, written out for block (by=0, bx=1) and (1, 2)
    np.testing.assert_array_equal(rows[1], [16, 16, 27, 6, 24, 8, 0, 12, -8, 4])
    np.testing.assert_array_equal(rows[5], [16, 16, 47, 31, 40, 24, 0, 28, 28, 4])
    got = motion_vectors_to_flowfield(torch.from_numpy(rows).unsqueeze(0), (h, w))[0]
    want = omotion.motion_vectors_to_flowfield(rows, (h, w))
    np.testing.assert_array_equal(got.numpy(), want)
    # the paint shows content displacement reference -> current: (-dx, -dy)
    np.testing.assert_array_equal(want[0, 16], [-3.0, 2.0])


def test_blocks_to_mv_rows_rejects_a_wrong_grid():
    with pytest.raises(ValueError, match="blocks"):
        me.blocks_to_mv_rows(FIELD, 64, 48)


# ---- sampling rule --------------------------------------------------------------

def test_sample_pairs():
    assert me.motion_sample_pairs(31, 30.0, 2.0, 0.5) == [(14, 15), (29, 30)]
    assert me.motion_sample_pairs(5, 30.0) == []
    # fps == target: consecutive pairs, capped at max_frames = max(10, round(2*30*0.5))
    assert me.motion_sample_pairs(60, 2.0, 2.0, 0.5) == [(i - 1, i) for i in range(1, 31)]
    # ... and at the floor of 10 for a short clip
    assert me.motion_sample_pairs(14, 2.0, 2.0, 0.5) == [(i - 1, i) for i in range(1, 11)]
    # Python round: 25 fps at target 2 -> step round(12.5) = 12
    assert me.motion_sample_pairs(30, 25.0)[:2] == [(11, 12), (23, 24)]
    with pytest.raises(ValueError):
        me.motion_sample_pairs(10, 0.0)


# ---- stage error paths that never touch the GPU --------------------------------

def _run_stage(payload) -> Clip:
    clip = Clip(uuid=uuid.uuid4(), source_video="s", span=(0.0, 1.0),
                encoded_data=payload)
    video = Video(input_video=pathlib.Path("/m.bin"))
    video.clips = [clip]
    me.MotionVectorEstimationStage().process_data([SplitPipeTask(videos=[video])])
    assert video.clips == [clip] and clip.decoded_motion_data is None
    return clip


def test_stage_error_paths_without_gpu():
    mp4 = np.frombuffer(b"\x00\x00\x00\x18ftypisom" + bytes(64), dtype=np.uint8)
    assert _run_stage(mp4).errors == {"motion_decode": "decode_unavailable"}
    small = raw_backend.pack_header(4, 128, 384, 30) + bytes(4 * 128 * 384 * 3 // 2)
    assert _run_stage(np.frombuffer(small, dtype=np.uint8)).errors == {
        "motion_decode": "resolution_too_small"}
    assert _run_stage(None).errors == {"encoded_data": "empty"}


def test_stage_resources_and_defaults():
    st = me.MotionVectorEstimationStage()
    assert (st.resources.cpus, st.resources.gpus) == (1.0, 0.25)
    st = me.MotionVectorEstimationStage(2.0, num_gpus_per_worker=0.5)
    assert (st.resources.cpus, st.resources.gpus) == (2.0, 0.5)


def test_estimate_clip_motion_header_only_outcomes():
    with pytest.raises(me.VideoResolutionTooSmallError):
        me.estimate_clip_motion(raw_backend.pack_header(31, 256, 255, 30))
    # no pairs: an object with no frames, before the GPU is asked for
    md = me.estimate_clip_motion(raw_backend.pack_header(5, 256, 256, 30))
    assert md.frames == [] and md.frame_size == (256, 256)


def test_hotpath_wrapper_rejects_a_bad_bit_depth():
    from cosmos_curate_amd import hotpath

    with pytest.raises(ValueError, match="bit_depth"):
        hotpath.estimate_motion(0, 0, 1, 16, 16, 16, 0, 0, bit_depth=9)


def test_launcher_rejects_bad_arguments_before_touching_a_device():
    """Validation runs before the first HIP call, so it can be checked
    here: the pointers are host addresses nothing dereferences."""
    from cosmos_curate_amd import hotpath

    lib = hotpath.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    good = dict(cur=p, ref=p, n=1, h=18, w=34, pitch=80, stride=80 * 18, bps=2,
                R=16, lam=4, mv=p, cost=p)
    cases = {
        "null cur": (dict(cur=None), -1), "null mv": (dict(mv=None), -1),
        "n 0": (dict(n=0), -1), "w -3": (dict(w=-3), -1),
        "range 0": (dict(R=0), -1), "range 33": (dict(R=33), -1),
        "lambda 256": (dict(lam=256), -1), "bps 3": (dict(bps=3), -1),
        "pitch < row bytes": (dict(pitch=66, stride=66 * 18), -1),
        "stride < plane": (dict(stride=80 * 18 - 2), -1),
        "odd pitch at 16 bit": (dict(pitch=81, stride=81 * 18 + 1), -1),
        "odd ref at 16 bit": (dict(ref=p + 1), -1),
        "too many pairs": (dict(n=65536), -6),
    }
    for name, (change, want_rc) in cases.items():
        a = dict(good, **change)
        rc = lib.cc_motion_estimate(
            a["cur"], a["ref"], a["n"], a["h"], a["w"], a["pitch"], a["stride"],
            a["bps"], a["R"], a["lam"], a["mv"], a["cost"], 0)
        assert rc == want_rc, name
        assert b"motion_estimate" in lib.cc_last_error(), name
    assert not buf.any()


# ---- driver ---------------------------------------------------------------------

def _parse(argv):
    p = argparse.ArgumentParser()
    _setup_parser(p)
    return p.parse_args(["--input-video-path", "/i", "--output-clip-path", "/o", *argv])


def _names(args) -> list[str]:
    return [type(s.stage if hasattr(s, "stage") else s).__name__
            for s in _assemble_stages(args)]


def test_flag_defaults():
    a = _parse([])
    assert a.motion_vector_backend == "none"
    assert a.motion_decode_target_fps == 2.0
    assert a.motion_decode_target_duration_ratio == 0.5
    assert a.motion_search_range == 16
    assert a.motion_estimate_lambda == 4


def test_stage_list():
    base = _names(_parse(["--motion-filter", "enable"]))
    assert "MotionVectorEstimationStage" not in base
    est = _names(_parse(["--motion-filter", "enable",
                         "--motion-vector-backend", "estimate"]))
    i = est.index("MotionFilterStage")
    assert est[i - 1] == "MotionVectorEstimationStage"
    assert est[: i - 1] + est[i:] == base
    # the filter disabled: the backend flag alone adds nothing
    assert _names(_parse(["--motion-vector-backend", "estimate"])) == _names(_parse([]))
    # flags reach the stage
    args = _parse(["--motion-filter", "score-only", "--motion-vector-backend",
                   "estimate", "--motion-search-range", "8",
                   "--motion-estimate-lambda", "2",
                   "--motion-decode-target-fps", "4"])
    st = next(s for s in _assemble_stages(args)
              if isinstance(s, me.MotionVectorEstimationStage))
    assert (st._search_range, st._mv_lambda, st._target_fps) == (8, 2, 4.0)
    assert isinstance(_assemble_stages(args)[_names(args).index("MotionFilterStage")],
                      MotionFilterStage)


def test_dry_run_lists_the_estimation_stage(tmp_path, capsys):
    (tmp_path / "in").mkdir()
    p = argparse.ArgumentParser()
    _setup_parser(p)
    args = p.parse_args([
        "--input-video-path", str(tmp_path / "in"),
        "--output-clip-path", str(tmp_path / "out"), "--dry-run",
        "--motion-filter", "enable", "--motion-vector-backend", "estimate"])
    assert split(args)["dry_run"]
    printed = capsys.readouterr().out.split()
    i = printed.index("MotionFilterStage")
    assert printed[i - 1] == "MotionVectorEstimationStage"
