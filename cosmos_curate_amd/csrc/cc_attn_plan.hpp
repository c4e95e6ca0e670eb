// Attention launch plan: the single statement of which rung of the ladder
// (k_attn_small / k_attn_mid / k_attn_flash) a cc_attn call runs and how it
// is launched.  Host-only, no HIP types, so the rule can be evaluated (and
// is pinned, tests/test_attn_plan_cpu.py, tests/test_attn_hd_plan_cpu.py)
// without a device.  cc_attn.hip's launcher executes exactly what this
// returns.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

// Head dims cc_attn takes: every multiple of 8 in [64, 128] (one kernel
// instantiation per value and rung).  A multiple of 8 keeps every head
// offset 16-byte aligned and every 8-element fragment chunk wholly inside
// or wholly outside the head (cc_attn.hip).
constexpr int ATTN_HD_MIN = 64;
constexpr int ATTN_HD_MAX = 128;
constexpr int ATTN_HD_STEP = 8;
constexpr int ATTN_CLS_HD = 64;     // k_attn_cls: head dim 64 only
constexpr int ATTN_SMALL_MAX = 64;  // k_attn_small: one padded 64-row tile
constexpr int ATTN_MID_MAX = 288;   // k_attn_mid: 18 x 16-col S fragments
constexpr int ATTN_QTILE = 64;      // k_attn_flash: q rows per workgroup

constexpr bool attn_hd_supported(int64_t hd) {
  return hd >= ATTN_HD_MIN && hd <= ATTN_HD_MAX && hd % ATTN_HD_STEP == 0;
}

// The rung rule.
//
// Head dim 64 (pinned, tests/test_attn_plan_cpu.py):
//   seq <= 64 small, seq <= 288 mid, longer flash.
//
// Head dim above 64 (tests/test_attn_hd_plan_cpu.py):
//   seq <= 64 small;
//   193..288 at head dim >= 96 mid;
//   everything else flash.
// Why it differs.  k_attn_mid holds V^T [hd16][296] + P [64][296] bf16 in
// LDS (hd16 = hd rounded up to 16): 75.8 KB at hd 64, two workgroups per
// 160 KiB CU; 85.2 KB at hd 72/80 up to 113.7 KB at 128, one workgroup per
// CU, and it always pays for its full 18 S-fragments (288 columns) per
// 64-row q-tile however short the sequence.  k_attn_flash pays 4 fragments
// per (q-tile, kv-tile) pair.  In fragments per (frame, head): seq 65..128
// mid 36 / flash 16, 129..192 54 / 36, 193..256 72 / 64, 257..288 90 / 100.
// So flash has less to do up to 256 and mid from 257; what was measured
// moves that by head dim.  16 heads, 64 frames, median of 30 launches, legs
// alternating in one process, ms (tools/attn_hd_bench.py, one run per head
// dim, spread between runs not measured; profiles/r05_attn_hd_bench*.log):
//
//   hd   seq   small    mid     flash   torch sdpa + permutes
//   72    50   0.0170  0.0505  0.0177   0.0485
//   72    64   0.0184  0.0510  0.0202   0.0534
//   72    81           0.0807  0.0415   0.0775
//   72   128           0.0883  0.0484   0.0892
//   72   192           0.1259  0.0878   0.2058
//   72   256           0.1671  0.1409   0.2310
//   72   288           0.2014  0.1906   0.2049
//   72   729                   0.9622   1.0647
//   96    64   0.0200  0.0488  0.0209   0.0355
//   96    81           0.0737  0.0437   0.0545
//   96   256           0.1400  0.1418   0.1537
//   96   288           0.1676  0.1979   0.1522
//  128    64   0.0215  0.0566  0.0244   0.0349
//  128    81           0.0840  0.0519   0.0570
//  128   256           0.1641  0.1765   0.1645
//  128   288           0.2038  0.2578   0.1633
//
// small wins wherever it applies.  At hd 72 flash wins the whole 65..288
// band (1.9x at 81, 5 % at 288).  At hd 96 and 128 mid takes 257..288 (18 %
// and 26 % at 288) and 193..256 is a tie at 96 (1.3 %) and mid by 7 % at
// 128; 65..192 is flash's by the fragment count and the seq 81 rows.  Head
// dims 80 and 88 follow 72, 104..120 follow 96/128; none of those was
// measured.  Not built, not measured: a narrower mid (272 columns, 80.6 KB
// at hd 72/80) that would fit two workgroups per CU again.
// Known losses against torch sdpa (not routed around): seq 288 at hd 96
// (mid 0.1676 vs 0.1522 ms, 10 %) and at hd 128 (0.2038 vs 0.1633, 25 %).
constexpr int ATTN_WIDE_MID_HD = 96;    // head dims from here keep a mid band
constexpr int ATTN_WIDE_MID_MIN = 193;  // its first seq: the 4th q-tile

constexpr int attn_rung_for(int seq, int hd) {
  if (seq <= ATTN_SMALL_MAX) return CC_ATTN_SMALL;
  if (seq > ATTN_MID_MAX) return CC_ATTN_FLASH;
  if (hd == ATTN_HD_MIN) return CC_ATTN_MID;
  return hd >= ATTN_WIDE_MID_HD && seq >= ATTN_WIDE_MID_MIN ? CC_ATTN_MID
                                                            : CC_ATTN_FLASH;
}

// Whether `rung` can run a sequence of this length at all (the rule above
// picks among the rungs that can).
constexpr bool attn_rung_covers(int rung, int seq) {
  return rung == CC_ATTN_SMALL ? seq <= ATTN_SMALL_MAX
         : rung == CC_ATTN_MID ? seq <= ATTN_MID_MAX
                               : rung == CC_ATTN_FLASH;
}

// Returns CC_OK and fills *p, or sets the error and returns its code.
// `force_rung` >= 0 replaces the rule's choice (cc_attn_rung, the A/B entry
// of tools/attn_hd_bench.py); it must be a rung that covers seq.
inline int attn_plan(int64_t n_frames, int seq, int heads, int hidden,
                     cc_attn_plan_info* p, int force_rung = -1) {
  if (n_frames <= 0 || seq <= 0 || heads <= 0)
    return set_error(CC_ERR_INVALID,
                     "bad attn args (n_frames %lld, seq %d, heads %d)",
                     (long long)n_frames, seq, heads);
  if (hidden <= 0 || hidden % heads != 0 || !attn_hd_supported(hidden / heads))
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_attn needs a head dim that is a multiple of %d in "
                     "[%d, %d] (hidden %d, heads %d)",
                     ATTN_HD_STEP, ATTN_HD_MIN, ATTN_HD_MAX, hidden, heads);
  if (force_rung > CC_ATTN_FLASH ||
      (force_rung >= 0 && !attn_rung_covers(force_rung, seq)))
    return set_error(CC_ERR_UNSUPPORTED, "attn rung %d does not cover seq %d",
                     force_rung, seq);
  // small and mid: one workgroup per (frame, head); flash: one per
  // (frame, head, 64-row q-tile)
  const int rung =
      force_rung >= 0 ? force_rung : attn_rung_for(seq, hidden / heads);
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
