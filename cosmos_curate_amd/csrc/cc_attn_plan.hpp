// Attention launch plan: the single statement of which rung of the ladder
// (k_attn_small / k_attn_mid / k_attn_flash) a cc_attn call runs and how it
// is launched.  Host-only, no HIP types, so the rule can be evaluated (and
// is pinned, tests/test_attn_plan_cpu.py) without a device.  cc_attn.hip's
// launcher executes exactly what this returns.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

constexpr int ATTN_HD = 64;         // head dim of every attention kernel
constexpr int ATTN_SMALL_MAX = 64;  // k_attn_small: one padded 64-row tile
constexpr int ATTN_MID_MAX = 288;   // k_attn_mid: 18 x 16-col S fragments
constexpr int ATTN_QTILE = 64;      // k_attn_flash: q rows per workgroup

// Returns CC_OK and fills *p, or sets the error and returns its code.
inline int attn_plan(int64_t n_frames, int seq, int heads, int hidden,
                     cc_attn_plan_info* p) {
  if (n_frames <= 0 || seq <= 0 || heads <= 0)
    return set_error(CC_ERR_INVALID,
                     "bad attn args (n_frames %lld, seq %d, heads %d)",
                     (long long)n_frames, seq, heads);
  if ((int64_t)hidden != (int64_t)heads * ATTN_HD)
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_attn needs hd == %d (hidden %d, heads %d)", ATTN_HD,
                     hidden, heads);
  // small and mid: one workgroup per (frame, head); flash: one per
  // (frame, head, 64-row q-tile)
  const int rung = seq <= ATTN_SMALL_MAX ? CC_ATTN_SMALL
                   : seq <= ATTN_MID_MAX ? CC_ATTN_MID
                                         : CC_ATTN_FLASH;
  const int64_t per_frame =
      rung == CC_ATTN_FLASH
          ? heads * (((int64_t)seq + ATTN_QTILE - 1) / ATTN_QTILE)
          : heads;
  if (n_frames > 0x7fffffffLL / per_frame)
    return set_error(CC_ERR_INVALID,
                     "attn grid too large (n_frames %lld x %lld workgroups "
                     "per frame)",
                     (long long)n_frames, (long long)per_frame);
  p->rung = rung;
  p->grid = (int32_t)(n_frames * per_frame);
  p->block = 256;
  return CC_OK;
}

}  // namespace cc
