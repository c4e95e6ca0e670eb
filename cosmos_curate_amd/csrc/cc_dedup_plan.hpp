// Launch plan of the segmented pruning scan (cc_pairwise_max_earlier_seg;
// cc_dedupseg.hip): which shapes it takes, the tile, how far a j-tile's
// i-range is cut into work items, the persistent grid and the workspace.
// Everything is a function of (m, d, k) alone: the segment lengths live on
// the device and are never read back.  Host-only, no HIP types, so the rule
// can be evaluated (tests/test_dedup_plan_cpu.py) without a device.  The
// launcher executes exactly what this returns.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

// One tile edge for both operands: a work item multiplies 128 scan positions
// (j, the columns that get an answer) by 128 earlier positions (i) at a time,
// the k-means assign tile.  A 64-column tile would waste less on the diagonal
// (11.5 % of the MFMAs at 1000 rows a segment against 18 %) but halves the
// MFMAs per byte staged, and the j-rows cannot stay resident in LDS beside a
// double-buffered i-tile at d = 1152 either way.
constexpr int PS_TILE = 128;
constexpr int PS_DK = 32;      // columns of d staged per step
constexpr int PS_BLOCK = 256;  // 4 waves, 2 (i halves) x 2 (j halves)
// A j-tile's i-range is cut into work items of at most C i-tiles, C the
// smallest value >= PS_CHUNK_MIN that cuts no j-tile into more than
// PS_MAX_CHUNKS items.  The floor keeps an item long enough (8 tiles x d/32
// steps) to amortise its prologue; the cap bounds the partials to
// PS_MAX_CHUNKS (value, index) pairs a row whatever the segment lengths are
// (fixed C = 8 would need m^2 / 256 bytes for one segment of m rows: 3.9 GB at
// 1M).  One segment of 900k rows among 1M is still 54k items of at most 489
// tiles each.
constexpr int PS_CHUNK_MIN = 8;
constexpr int PS_MAX_CHUNKS = 16;
// Two workgroups a CU (75.8 KB of LDS each) on 256 CUs; the grid walks the
// work list with a stride and is never sized from the offsets.
constexpr int PS_GRID = 512;
constexpr int PS_PREFIX_BLOCK = 1024;
constexpr int PS_COMBINE_BLOCK = 256;
constexpr int PS_D_STEP = 64;
constexpr int PS_D_MIN = 64;
constexpr int PS_D_MAX = 1152;
constexpr int64_t PS_K_MAX = 1LL << 30;
constexpr int64_t PS_M_MAX = 0x7fffffffLL;  // order and offsets are int32

// Returns CC_OK and fills *p, or sets the error and returns its code.
inline int pairwise_seg_plan(int64_t m, int64_t d, int64_t k,
                             cc_pairwise_seg_plan_info* p) {
  if (m <= 0 || k <= 0 || d <= 0)
    return set_error(CC_ERR_INVALID,
                     "bad pairwise_seg args (m %lld, d %lld, k %lld)",
                     (long long)m, (long long)d, (long long)k);
  if (d < PS_D_MIN || d > PS_D_MAX || d % PS_D_STEP != 0)
    return set_error(CC_ERR_UNSUPPORTED,
                     "pairwise_seg needs d a multiple of %d in [%d, %d] (d %lld)",
                     PS_D_STEP, PS_D_MIN, PS_D_MAX, (long long)d);
  if (m > PS_M_MAX)
    return set_error(CC_ERR_INVALID,
                     "pairwise_seg takes at most 2^31-1 rows (%lld)",
                     (long long)m);
  if (k > PS_K_MAX)
    return set_error(CC_ERR_INVALID,
                     "pairwise_seg takes at most 2^30 segments (%lld)",
                     (long long)k);
  const int64_t tiles = (m + PS_TILE - 1) / PS_TILE;  // of the longest segment
  const int64_t fit = (tiles + PS_MAX_CHUNKS - 1) / PS_MAX_CHUNKS;
  const int64_t C = fit > PS_CHUNK_MIN ? fit : PS_CHUNK_MIN;
  const int64_t chunks = (tiles + C - 1) / C;
  p->tile = PS_TILE;
  p->d_chunks = (int32_t)(d / PS_DK);
  p->chunk_tiles = (int32_t)C;
  p->max_chunks = (int32_t)chunks;
  // without cuts there are at most tiles + k items; with cuts m is large
  p->grid = (int32_t)(tiles + k < PS_GRID ? tiles + k : PS_GRID);
  p->block = PS_BLOCK;
  p->prefix_block = PS_PREFIX_BLOCK;
  p->combine_grid = (int32_t)((m + PS_COMBINE_BLOCK - 1) / PS_COMBINE_BLOCK);
  p->combine_block = PS_COMBINE_BLOCK;
  p->prefix_bytes = ((k + 1) * (int64_t)sizeof(int64_t) + 15) / 16 * 16;
  // partial values f32 [chunks][m], then indices int32 [chunks][m]; a j-tile
  // that is one item writes its answer directly, so one chunk needs none
  const int64_t slices = chunks > 1 ? chunks : 0;
  p->workspace_bytes = p->prefix_bytes + slices * ((m + 3) / 4 * 4) * 8;
  return CC_OK;
}

}  // namespace cc
