// Launch plan of the motion-filter score (cc_motion_score_rows,
// cc_motion_score_blocks; cc_motionscore.hip): the pixel tile, the tiles of a
// frame, the grid and block of every kernel and the workspace.  Everything is
// a function of (n_frames, n_rows, n_clips, h, w, oh, ow) alone: the frame and
// clip offsets live on the device and are never read back.  Host-only, no HIP
// types, so the rule can be evaluated (tests/test_motion_score_plan_cpu.py)
// without a device.  The launchers execute exactly what this returns.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

// The pixel tile one paint workgroup owns: 64 x 32.  A block is at most 16
// pixels on a side, so a row's clamped extent touches at most 2 x 2 tiles of
// either candidate size.  64 x 32 against 128 x 32:
// - the owner map is 10 KB of LDS (32 rows of 64 keys, padded to 80), so a CU
//   holds its full complement of 256-thread workgroups; 128 x 32 doubles it
//   and halves the workgroups of a frame (510 at 1080p, two per CU on 256 CUs,
//   against 1020 here), which is what a single clip of 10 frames needs to fill
//   the device;
// - a wave of the resolve pass covers one 64-pixel tile row, 256 B of keys
//   and consecutive banks, whichever size is picked;
// - a row that straddles a tile edge is binned once a tile: 16-pixel blocks
//   that start on multiples of 8 average (1 + 1/8)(1 + 1/4) = 1.41 bin
//   entries a row here against (1 + 1/16)(1 + 1/4) = 1.33 at 128 x 32, 4 B
//   each; macroblock-aligned 16 x 16 blocks straddle nothing at either size.
constexpr int MS_TILE_W = 64;
constexpr int MS_TILE_H = 32;
constexpr int MS_BLOCK = 256;       // every kernel: 4 waves
constexpr int MS_SCAN_BLOCK = 1024;  // one workgroup scans a frame's tiles
// key = (pass + 1) << 28 | row in frame; the plan sees only the total, so it
// rejects a call that COULD hold a frame the key cannot index
constexpr int MS_KEY_ROW_BITS = 28;
constexpr int64_t MS_ROWS_MAX = (1LL << MS_KEY_ROW_BITS) - 1;
constexpr int64_t MS_SIDE_MAX = 16384;  // h + w exact in f32, 4*oh*ow in int32
constexpr int64_t MS_GRID_MAX = 0x7fffffffLL;
// estimated-block path: 16 x 16 blocks, 4 a thread
constexpr int MS_EST_BLOCK = 16;
constexpr int MS_EST_PER_WG = 4 * MS_BLOCK;

inline int64_t ms_align16(int64_t b) { return (b + 15) / 16 * 16; }

// Returns CC_OK and fills *p, or sets the error and returns its code.
inline int motion_score_plan(int64_t n_frames, int64_t n_rows, int64_t n_clips,
                             int64_t h, int64_t w, int64_t oh, int64_t ow,
                             cc_motion_score_plan_info* p) {
  if (n_frames < 0 || n_rows < 0 || n_clips <= 0 || h <= 0 || w <= 0)
    return set_error(CC_ERR_INVALID,
                     "bad motion_score args (frames %lld, rows %lld, clips "
                     "%lld, %lld x %lld)",
                     (long long)n_frames, (long long)n_rows, (long long)n_clips,
                     (long long)h, (long long)w);
  if (oh < 1 || ow < 1 || oh > h || ow > w)
    return set_error(CC_ERR_INVALID,
                     "motion_score patch grid %lld x %lld of a %lld x %lld frame",
                     (long long)oh, (long long)ow, (long long)h, (long long)w);
  if (h > MS_SIDE_MAX || w > MS_SIDE_MAX)
    return set_error(CC_ERR_UNSUPPORTED,
                     "motion_score takes frames up to %lld on a side (%lld x %lld)",
                     (long long)MS_SIDE_MAX, (long long)h, (long long)w);
  if (n_rows > MS_ROWS_MAX)
    return set_error(CC_ERR_UNSUPPORTED,
                     "motion_score key holds %d bits of row index (%lld rows)",
                     MS_KEY_ROW_BITS, (long long)n_rows);
  const int64_t tx = (w + MS_TILE_W - 1) / MS_TILE_W;
  const int64_t ty = (h + MS_TILE_H - 1) / MS_TILE_H;
  const int64_t T = tx * ty;
  const int64_t nb = ((h + MS_EST_BLOCK - 1) / MS_EST_BLOCK) *
                     ((w + MS_EST_BLOCK - 1) / MS_EST_BLOCK);
  const int64_t P = (nb + MS_EST_PER_WG - 1) / MS_EST_PER_WG;
  if (n_frames > MS_GRID_MAX || n_clips > MS_GRID_MAX ||
      n_frames * T > MS_GRID_MAX)
    return set_error(CC_ERR_UNSUPPORTED,
                     "motion_score grid overflows (%lld frames of %lld tiles, "
                     "%lld clips)",
                     (long long)n_frames, (long long)T, (long long)n_clips);
  const int64_t taps = 4 * oh * ow;
  p->tile_w = MS_TILE_W;
  p->tile_h = MS_TILE_H;
  p->tiles_x = (int32_t)tx;
  p->tiles_y = (int32_t)ty;
  p->tiles_per_frame = (int32_t)T;
  p->taps_per_frame = (int32_t)taps;
  p->block = MS_BLOCK;
  p->zero_grid = (int32_t)((n_frames * T + MS_BLOCK - 1) / MS_BLOCK);
  p->bin_grid = (int32_t)((n_rows + MS_BLOCK - 1) / MS_BLOCK);
  p->scan_grid = (int32_t)n_frames;
  p->scan_block = MS_SCAN_BLOCK;
  p->paint_grid = (int32_t)(n_frames * T);
  p->finish_grid = (int32_t)n_clips;
  p->est_partials = (int32_t)P;
  p->est_grid = (int32_t)(n_frames * P);
  // f64 partials [frames][T], f32 taps [frames][2 oh][2 ow], int32 counts
  // [frames][T], int32 starts [frames][T + 1], int32 bins [4 n_rows]: a frame
  // owns the bins from 4 * its first row, 4 per row being the most tiles a
  // row's extent can touch
  p->partial_bytes = ms_align16(n_frames * T * 8);
  p->tap_bytes = ms_align16(n_frames * taps * 4);
  p->count_bytes = ms_align16(n_frames * T * 4);
  p->start_bytes = ms_align16(n_frames * (T + 1) * 4);
  p->workspace_bytes = p->partial_bytes + p->tap_bytes + p->count_bytes +
                       p->start_bytes + ms_align16(n_rows * 16);
  // estimated blocks: f64 partials [frames][P], then the taps
  p->est_partial_bytes = ms_align16(n_frames * P * 8);
  p->est_workspace_bytes = p->est_partial_bytes + p->tap_bytes;
  if (p->workspace_bytes < 16) p->workspace_bytes = 16;
  if (p->est_workspace_bytes < 16) p->est_workspace_bytes = 16;
  return CC_OK;
}

}  // namespace cc
