// Launch plan of cc_attn_pool (one-query attention pooling, cc_attnpool.hip):
// which widths it takes, how a frame's tokens are cut into splits and how
// much workspace the partials need.  Host-only, no HIP types, so the rule can
// be evaluated (tests/test_attn_pool_cpu.py) without a device.  The launcher
// executes exactly what this returns.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

constexpr int POOL_HEADS_MAX = 16;  // one MFMA dimension
constexpr int POOL_H_STEP = 128;    // 8 waves x one 16-column k-step
constexpr int POOL_H_MAX = 1408;    // the X chunk at 1408 is 90.6 KB of LDS
constexpr int POOL_CHUNK = 32;      // tokens staged per pass
constexpr int POOL_BLOCK = 512;     // 8 waves
constexpr int POOL_SPLITS_MAX = 256;
// The plan's own choice of splits aims at one workgroup per compute unit of
// an MI355X.  A split that is not the only one writes (m, l, sum c, Z[16][H])
// f32, as many bytes as one chunk it reads, and the combine reads them back,
// so the plan gives a split no fewer than POOL_MIN_CHUNKS chunks.
constexpr int POOL_DEVICE_CUS = 256;
constexpr int POOL_MIN_CHUNKS = 4;

constexpr bool attn_pool_supported(int heads, int H) {
  return heads >= 1 && heads <= POOL_HEADS_MAX && H >= POOL_H_STEP &&
         H <= POOL_H_MAX && H % POOL_H_STEP == 0;
}

// f32 elements of one (frame, split) partial: m[16], l[16], sum c[16], Z[16][H]
constexpr int64_t attn_pool_partial_floats(int H) {
  return 3 * POOL_HEADS_MAX + (int64_t)POOL_HEADS_MAX * H;
}

// Returns CC_OK and fills *p, or sets the error and returns its code.
// `splits` 0 asks for the plan's choice; an explicit value is taken as given
// (splits past the last chunk stay empty and weigh nothing in the combine).
inline int attn_pool_plan(int64_t n, int seq, int heads, int H, int splits,
                          cc_attn_pool_plan_info* p) {
  if (n <= 0 || seq <= 0 || splits < 0)
    return set_error(CC_ERR_INVALID,
                     "bad attn_pool args (n %lld, seq %d, splits %d)",
                     (long long)n, seq, splits);
  if (!attn_pool_supported(heads, H))
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_attn_pool needs heads <= %d and H a multiple of %d up "
                     "to %d (heads %d, H %d)",
                     POOL_HEADS_MAX, POOL_H_STEP, POOL_H_MAX, heads, H);
  if (splits > POOL_SPLITS_MAX)
    return set_error(CC_ERR_INVALID, "attn_pool takes at most %d splits (%d)",
                     POOL_SPLITS_MAX, splits);
  const int chunks = (int)(((int64_t)seq + POOL_CHUNK - 1) / POOL_CHUNK);
  int per;
  if (splits == 0) {
    const int64_t want = (POOL_DEVICE_CUS + n - 1) / n;
    const int most = chunks / POOL_MIN_CHUNKS > 0 ? chunks / POOL_MIN_CHUNKS : 1;
    splits = (int)(want < most ? want : most);
    per = (chunks + splits - 1) / splits;
    splits = (chunks + per - 1) / per;  // no empty split
  } else {
    per = (chunks + splits - 1) / splits;
  }
  if (n > 0x7fffffffLL / splits)
    return set_error(CC_ERR_INVALID, "attn_pool grid too large (n %lld x %d)",
                     (long long)n, splits);
  p->splits = splits;
  p->chunk = POOL_CHUNK;
  p->chunks_per_split = per;
  p->grid = (int32_t)(n * splits);
  p->block = POOL_BLOCK;
  p->workspace_floats =
      splits == 1 ? 0 : n * splits * attn_pool_partial_floats(H);
  return CC_OK;
}

}  // namespace cc
