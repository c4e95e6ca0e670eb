"""The motion score's launch rule, pinned through cc_motion_score_plan (no GPU).

cc::motion_score_plan (csrc/cc_motionscore_plan.hpp) is the only validation of
the shapes cc_motion_score_rows and cc_motion_score_blocks take; the GPU side
(tests/test_gpu_motion_score.py) checks what the kernels compute.
"""

import argparse

import pytest

from cosmos_curate_amd import build as cc_build
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.pipelines.video.splitting_pipeline import (
    _assemble_stages,
    _setup_parser,
)

CC_ERR_INVALID = -1
CC_ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def lib():
    cc_build.build(verbose=False)
    return hotpath.load()


def _a16(b):
    return -(-b // 16) * 16


@pytest.mark.parametrize(
    ("frames", "rows", "clips", "h", "w", "tiles_x", "tiles_y", "est_partials"),
    [(10, 81600, 1, 1080, 1920, 30, 34, 8),   # 1080 is 33.75 tiles high
     (3, 70000, 2, 256, 256, 4, 8, 1),
     (5, 0, 3, 270, 330, 6, 9, 1)],           # frames without rows
)
def test_motion_score_plan_table(lib, frames, rows, clips, h, w, tiles_x, tiles_y,
                                 est_partials):
    oh, ow = hotpath.motion_patch_grid(h, w)
    p = hotpath.motion_score_plan(frames, rows, clips, h, w, oh, ow)
    t = tiles_x * tiles_y
    assert (p.tile_w, p.tile_h, p.block, p.scan_block) == (64, 32, 256, 1024)
    assert (p.tiles_x, p.tiles_y, p.tiles_per_frame) == (tiles_x, tiles_y, t)
    assert p.taps_per_frame == 4 * oh * ow
    assert (p.zero_grid, p.bin_grid) == (-(-frames * t // 256), -(-rows // 256))
    assert (p.scan_grid, p.paint_grid, p.finish_grid) == (frames, frames * t, clips)
    assert (p.est_partials, p.est_grid) == (est_partials, frames * est_partials)
    taps = _a16(frames * 4 * oh * ow * 4)
    # f64 partials, f32 taps, int32 counts and starts, 4 int32 bin slots a row
    assert p.workspace_bytes == (_a16(frames * t * 8) + taps + _a16(frames * t * 4)
                                 + _a16(frames * (t + 1) * 4) + 16 * rows)
    assert p.est_workspace_bytes == _a16(frames * est_partials * 8) + taps


def test_motion_patch_grid_rounds_half_to_even():
    assert hotpath.motion_patch_grid(384, 640) == (2, 2)  # round(1.5), round(2.5)
    assert hotpath.motion_patch_grid(128, 384) == (1, 2)  # max(1, round(0.5))


@pytest.mark.parametrize(
    ("args", "code"),
    [
        ((-1, 10, 1, 256, 256, 1, 1), CC_ERR_INVALID),
        ((1, -1, 1, 256, 256, 1, 1), CC_ERR_INVALID),
        ((1, 10, 0, 256, 256, 1, 1), CC_ERR_INVALID),
        ((1, 10, 1, 0, 256, 1, 1), CC_ERR_INVALID),
        ((1, 10, 1, 256, -4, 1, 1), CC_ERR_INVALID),
        ((1, 10, 1, 256, 256, 0, 1), CC_ERR_INVALID),
        ((1, 10, 1, 256, 256, 1, 257), CC_ERR_INVALID),
        ((1, 10, 1, 16385, 256, 1, 1), CC_ERR_UNSUPPORTED),
        ((1, 2**28, 1, 256, 256, 1, 1), CC_ERR_UNSUPPORTED),   # key: 28 row bits
        ((2**26, 10, 1, 256, 256, 1, 1), CC_ERR_UNSUPPORTED),  # 2^31 paint groups
        ((1, 10, 2**31, 256, 256, 1, 1), CC_ERR_UNSUPPORTED),
    ],
)
def test_motion_score_plan_rejects(lib, args, code):
    assert lib.cc_motion_score_plan(*args, hotpath.MotionScorePlan()) == code
    assert lib.cc_last_error().decode()
    with pytest.raises(RuntimeError):
        hotpath.motion_score_plan(*args)
    assert lib.cc_motion_score_plan(1, 10, 1, 256, 256, 1, 1, None) == CC_ERR_INVALID


def test_score_backend_flag_reaches_the_stage():
    parser = argparse.ArgumentParser()
    _setup_parser(parser)
    base = ["--input-video-path", "/i", "--output-clip-path", "/o", "--motion-filter", "enable"]
    for argv, want in (([], "torch"), (["--motion-score-backend", "native"], "native")):
        stages = [getattr(s, "stage", s) for s in _assemble_stages(parser.parse_args(base + argv))]
        (stage,) = [s for s in stages if type(s).__name__ == "MotionFilterStage"]
        assert stage._score_backend == want
