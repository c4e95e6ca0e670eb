"""The motion score kernels (csrc/cc_motionscore.hip) against the float64
reference (tests/motion_score_ref.py) on MI355X.

Tolerance, derived: inputs are f32 and the reference is f64 on the same f32
values.  A pixel's f32 chain (one divide, two multiplies and an add, a square
root, one divide) errs by a few ulp, about 3 * 6e-8 relative; f64 sums of
non-negative terms keep that relative bound; the f32 rounding of the temporal
mean and the f32 blend add a few ulp more.  rtol = 2e-6 is more than 5x the
bound; atol = 0, and where the reference is exactly 0 so is the kernel.
"""

import functools
import pathlib
import uuid

import motion_score_ref as ref
import numpy as np
import pytest
import torch

from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces import SequentialRunner, run_pipeline
from cosmos_curate_amd.pipelines.video.filtering.motion import motion_estimation as me
from cosmos_curate_amd.pipelines.video.filtering.motion.motion_filter_stages import (
    BLOCK_OPTIONS,
    DecodedMotionData,
    MotionFilterStage,
    check_if_small_motion,
    score_clips_native,
)
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import Clip, SplitPipeTask, Video

pytestmark = pytest.mark.gpu
RTOL = 2e-6


def _rows(rng, n, xr, yr, sizes=BLOCK_OPTIONS, taps=None):
    """n rows of random sizes out of `sizes`, integer dst in xr x yr; with
    taps=(h, w), the first oh * ow of them are moved onto the centres of the
    256-patches, where the bilinear taps lie, so that per_patch_min is not 0
    (later rows may still own those pixels)."""
    mv = np.zeros((n, 10), dtype=np.float32)
    mv[:, 0:2] = np.asarray(sizes, dtype=np.float32)[rng.integers(len(sizes), size=n)]
    mv[:, 4] = rng.integers(*xr, size=n)
    mv[:, 5] = rng.integers(*yr, size=n)
    mv[:, 7:9] = rng.integers(-64, 65, size=(n, 2))
    mv[:, 9] = 4.0
    if taps and n:
        (h, w), (oh, ow) = taps, hotpath.motion_patch_grid(*taps)
        ys, xs = np.mgrid[0:oh, 0:ow]
        mv[:oh * ow, 0:2] = 16
        mv[:oh * ow, 4] = (xs.ravel() + 0.5) * w // ow
        mv[:oh * ow, 5] = (ys.ravel() + 0.5) * h // oh
    return mv


def _build(name):
    """Clips [(frames, (h, w))] of a case, seeded."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "sizes":  # off-tile frames; oh, ow = (1,1), (2,2) half-even, (1,2)
        return [([_rows(rng, 60, (0, w), (0, h), taps=(h, w)) for _ in range(2)], (h, w))
                for h, w in ((270, 330), (384, 640), (300, 520))]
    h, w = 270, 330
    if name == "overlap":  # dense: same-size and cross-size overlaps decide pixels
        return [([_rows(rng, 400, (110, 220), (90, 180)) for _ in range(3)], (h, w))]
    if name == "outside":  # dst past every side; every edge and tile boundary
        mv = _rows(rng, 500, (-24, w + 24), (-24, h + 24))
        far = _rows(rng, 4, (0, 1), (0, 1))
        far[:, 4:6] = [(-1000, 50), (w + 1000, 50), (50, -1000), (64, h + 1000)]
        return [([np.concatenate([mv, far])], (h, w))]
    if name == "nothing":  # unsupported sizes, zero rows, scale 0
        mv = _rows(rng, 300, (0, w), (0, h),
                   sizes=((8, 8), (4, 4), (16, 4), (0, 0), (16, 16), (8.5, 8), (32, 32)),
                   taps=(h, w))
        mv[5::5] = 0.0
        mv[1::7, 9] = 0.0
        return [([mv, np.zeros((40, 10), np.float32)], (h, w))]
    if name == "deep":  # 70 000 rows in two tiles: bin depth, > 16 bits of row
        # pixels x 64..190, y 96..127: tiles (1, 3) and (2, 3), the tap row 127
        return [([_rows(rng, 70_000, (72, 184), (104, 121), sizes=((8, 8), (16, 16)))],
                 (256, 256))]
    if name == "clips":  # unequal frame counts, no frames, a frame without rows
        counts = ([50, 0, 30], [], [20], [40, 40])
        return [([_rows(rng, n, (0, w), (0, h), taps=(h, w)) for n in c], (h, w)) for c in counts]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    clips = _build(name)
    want = [ref.score(f, h, w, *hotpath.motion_patch_grid(h, w)) for f, (h, w) in clips]
    return clips, want


def _assert_close(got, want):
    for g, x in zip(got, want):
        print(f"got {g!r} want {x!r} rel {abs(g - x) / x if x else 0.0:.3e}")
        assert g == 0.0 if x == 0.0 else abs(g - x) <= RTOL * abs(x)


@pytest.mark.parametrize("name", ["sizes", "overlap", "outside", "nothing", "deep", "clips"])
def test_score_rows_matches_reference(name):
    clips, want = _case(name)
    data = [DecodedMotionData(f, size) for f, size in clips]
    got = score_clips_native(data)
    assert len(got) == len(want)
    for g, x in zip(got, want):
        _assert_close(g, x)
    assert all(x[0] > 0 and x[1] > 0 for f, x in zip(data, want) if f.frames)
    if name == "clips":
        assert got[1] == (0.0, 0.0)
    if name == "overlap":  # bit-identical run to run
        assert score_clips_native(data) == got
    frames, size = clips[0]
    small, patch_min, gmean = check_if_small_motion(frames, size, backend="native")
    assert (patch_min, gmean) == got[0]
    assert small == (want[0][1] < 0.00098 or want[0][0] < 0.000001)


@pytest.mark.parametrize(("h", "w", "n"), [(256, 256, 1), (270, 330, 3), (1080, 1920, 2)])
def test_score_blocks_matches_rows_reference(h, w, n):
    rng = np.random.default_rng(h + w)
    field = rng.integers(-32, 33, size=(n, -(-h // 16), -(-w // 16), 2)).astype(np.int16)
    frames = [me.blocks_to_mv_rows(m, h, w) for m in field]
    want = ref.score(frames, h, w, *hotpath.motion_patch_grid(h, w))
    got = me.score_blocks_native(torch.from_numpy(field).cuda(), h, w)
    _assert_close(got, want)
    assert want[0] > 0 and want[1] > 0


def test_stage_native_filters_what_torch_filters():
    def videos():
        v = Video(input_video=pathlib.Path("/m.mp4"))
        v.clips = []
        for i, moving in enumerate((True, False, True)):
            c = Clip(uuid=uuid.UUID(int=i), source_video="s", span=(float(i), i + 1.0))
            row = [16, 16, 0, 0, 0, 64, 0, 40 + i, 40, 4.0]
            mv = np.array([row[:4] + [x] + row[5:] for x in range(8, 384, 16)], np.float32)
            c.decoded_motion_data = DecodedMotionData(
                [mv if moving else np.zeros((0, 10), np.float32)] * 10, (128, 384))
            v.clips.append(c)
        return v

    out = {}
    for backend in ("torch", "native"):
        task = run_pipeline([SplitPipeTask(videos=[videos()])],
                            [MotionFilterStage(score_backend=backend)],
                            runner=SequentialRunner())[0]
        out[backend] = task.video
    for attr in ("clips", "filtered_clips"):
        ids = {b: [c.uuid for c in getattr(v, attr)] for b, v in out.items()}
        assert ids["native"] == ids["torch"]
    assert len(out["native"].clips) == 2 and len(out["native"].filtered_clips) == 1
    for a, b in zip(out["native"].clips, out["torch"].clips):
        assert a.motion_score_global_mean == pytest.approx(b.motion_score_global_mean, rel=1e-5)
        assert a.decoded_motion_data is None


def test_estimate_into_score_stays_on_device_and_stages_run_native():
    """cc_motion_estimate -> cc_motion_score_blocks equals scoring the rows the
    estimate expands to, and the two motion stages run with the native score."""
    h, w = 256, 330
    raw = raw_backend.make_synthetic_clip(4, h, w, 2, seed=5)  # 3 chained pairs
    md = me.estimate_clip_motion(raw)
    want = ref.score(md.frames, h, w, *hotpath.motion_patch_grid(h, w))
    assert len(md.frames) == 3 and want[1] > 0
    _assert_close(me.score_clip_motion(raw), want)
    video = Video(input_video=pathlib.Path("/synthetic/motion.bin"))
    video.clips = [Clip(uuid=uuid.UUID(int=7), source_video="s", span=(0.0, 2.0),
                        encoded_data=np.frombuffer(raw, dtype=np.uint8))]
    out = run_pipeline(
        [SplitPipeTask(videos=[video])],
        [me.MotionVectorEstimationStage(), MotionFilterStage(score_backend="native", score_only=True)],
        runner=SequentialRunner())
    clip = out[0].video.clips[0]
    assert not clip.errors, clip.errors
    _assert_close((clip.motion_score_per_patch_min_256, clip.motion_score_global_mean), want)
