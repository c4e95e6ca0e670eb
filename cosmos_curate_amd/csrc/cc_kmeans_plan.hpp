// Launch plan of the k-means step (cc_kmeans_assign, cc_kmeans_accumulate;
// cc_kmeans.hip): which shapes it takes, how rows and centroids are tiled,
// how the sorted rows are cut into pieces and how much workspace the pieces'
// open ends need.  Host-only, no HIP types, so the rule can be evaluated
// (tests/test_kmeans_plan_cpu.py) without a device.  The launchers execute
// exactly what this returns.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

// Known loss against torch (`(e @ cent.T).argmax(1)`, not routed around):
// assign at (m, d, k) = (100k, 1152, 1000), 2.475 vs 1.858 ms.  Its 782
// workgroups are 1.53 rounds of the 512 a device holds, two a CU, so the
// second round runs half empty; at 1M rows (7813 workgroups) assign ties
// torch at k = 1000 and wins at k = 100, and the step (assign + accumulate)
// wins at all four measured shapes.  Not built: a 64-row
// tile for small m.
constexpr int KM_TILE_ROWS = 128;   // rows of e a workgroup owns
constexpr int KM_TILE_CENTS = 128;  // centroids per tile it marches over
constexpr int KM_DK = 32;           // columns of d staged per step
constexpr int KM_BLOCK = 256;       // 4 waves, 2 (centroids) x 2 (rows)
constexpr int KM_D_STEP = 64;
constexpr int KM_D_MIN = 64;
constexpr int KM_D_MAX = 1152;
// labels and centroid indices are int32; one tile of slack for the padded
// index of the last tile
constexpr int64_t KM_K_MAX = 1LL << 30;
constexpr int64_t KM_ACC_M_MAX = 0x7fffffffLL;  // order and offsets are int32
// Rows of the sorted order one accumulate workgroup walks.  A piece is one
// serial chain of f64 adds per column, so its length is the kernel's latency
// floor (512 rows, 8 loads in flight: 64 round trips), while every piece adds
// up to two open ends (2 d doubles written and read back, against 512 d
// floats read) and one step to its cluster's serial combine.
constexpr int KM_PIECE = 512;
constexpr int KM_COMBINE_BLOCK = 256;  // columns per combine workgroup

constexpr bool kmeans_d_supported(int64_t d) {
  return d >= KM_D_MIN && d <= KM_D_MAX && d % KM_D_STEP == 0;
}

// threads of an accumulate workgroup: one float4 of columns each, whole waves
constexpr int kmeans_acc_block(int64_t d) {
  return (int)((d / 4 + 63) / 64 * 64);
}

// Returns CC_OK and fills *p, or sets the error and returns its code.
inline int kmeans_plan(int64_t m, int64_t d, int64_t k,
                       cc_kmeans_plan_info* p) {
  if (m <= 0 || k <= 0 || d <= 0)
    return set_error(CC_ERR_INVALID, "bad kmeans args (m %lld, d %lld, k %lld)",
                     (long long)m, (long long)d, (long long)k);
  if (!kmeans_d_supported(d))
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_kmeans needs d a multiple of %d in [%d, %d] (d %lld)",
                     KM_D_STEP, KM_D_MIN, KM_D_MAX, (long long)d);
  if (k > KM_K_MAX)
    return set_error(CC_ERR_INVALID, "kmeans takes at most 2^30 clusters (%lld)",
                     (long long)k);
  // the assign grid is the larger of the two; accumulate's int32 row indices
  // bound m further (KM_ACC_M_MAX), checked by its entry
  if (m > (int64_t)KM_TILE_ROWS * 0x7fffffffLL)
    return set_error(CC_ERR_INVALID, "kmeans grid too large (m %lld)",
                     (long long)m);
  p->tile_rows = KM_TILE_ROWS;
  p->tile_cents = KM_TILE_CENTS;
  p->cent_tiles = (int32_t)((k + KM_TILE_CENTS - 1) / KM_TILE_CENTS);
  p->d_chunks = (int32_t)(d / KM_DK);
  p->assign_grid = (int32_t)((m + KM_TILE_ROWS - 1) / KM_TILE_ROWS);
  p->assign_block = KM_BLOCK;
  p->piece_rows = KM_PIECE;
  p->pieces = (int32_t)((m + KM_PIECE - 1) / KM_PIECE);
  p->acc_block = kmeans_acc_block(d);
  p->combine_grid_y = (int32_t)((d + KM_COMBINE_BLOCK - 1) / KM_COMBINE_BLOCK);
  // head[pieces][d] then tail[pieces][d], f64
  p->workspace_bytes = 2 * (int64_t)p->pieces * d * (int64_t)sizeof(double);
  return CC_OK;
}

}  // namespace cc
