// Launch plan of cc_attn_cross (few-query cross-attention, cc_attncross.hip):
// which head geometry it takes, how a clip's keys are cut into splits and how
// much workspace the partials need.  Host-only, no HIP types, so the rule can
// be evaluated (tests/test_attn_cross_plan_cpu.py) without a device.  The
// launcher executes exactly what this returns.
//
// Measured on one MI355X (tools/attn_cross_bench.py: n = 8 clips, 32 queries,
// 12 heads of 64; whole hotpath.attn_cross calls, combine kernel and workspace
// allocation included; HIP events, legs alternating in one process, median of
// 30 after 5 warm-up, in microseconds; DESIGN.md §29 has both runs):
//
//     nk     splits 1      2      4      8   | torch sdpa + permutes
//   2056       34.8     29.8   30.0   34.2   |   79.5
//   4616       58.0     41.7   39.8   41.9   |  145.7
//   8200       91.0     58.6   53.5   54.5   |  237.4
//
// and 6 splits (576 workgroups, more than the device holds at once) 32.5,
// 44.3 and 57.6: slower than both 4 and 8 at the two longer shapes.  The rule
// below yields 4 at all three (384 workgroups): the best leg at 4616 and 8200,
// 0.2 us (under the legs' p10..p90 spread) behind 2 splits at 2056.  The
// kernel loses to sdpa at no measured shape.
#pragma once

#include <cstdint>

#include "cc_common.hpp"

namespace cc {

constexpr int XATTN_HD = 64;      // the one head dim: four 16-wide k-steps
constexpr int XATTN_NQ_MAX = 32;  // one 32-row MFMA tile of queries
constexpr int XATTN_CHUNK = 32;   // keys per MFMA tile
constexpr int XATTN_BLOCK = 256;  // 4 waves, chunks dealt round-robin
// The plan's own choice of splits is the largest power of two that keeps the
// grid within XATTN_RESIDENT_WGS, the workgroups an MI355X holds at once (256
// compute units x 2: the kernel's 180 VGPRs allow two waves a SIMD), so the
// grid runs as one round with no tail; see the table above.  It gives a split
// no fewer than XATTN_MIN_CHUNKS chunks, two rounds of its four waves: a
// split that is not the only one writes an f32 partial (m, l, O[32][64]), as
// many bytes as two chunks of K and V it reads.
constexpr int XATTN_RESIDENT_WGS = 512;
constexpr int XATTN_MIN_CHUNKS = 8;

constexpr bool attn_cross_supported(int heads, int H) {
  return heads >= 1 && H == heads * XATTN_HD;
}

// f32 elements of one (clip, head, split) partial: m[32], l[32], O[32][64]
constexpr int64_t XATTN_PARTIAL_FLOATS =
    2 * XATTN_NQ_MAX + (int64_t)XATTN_NQ_MAX * XATTN_HD;

// Returns CC_OK and fills *p, or sets the error and returns its code.
// `splits` 0 asks for the plan's choice; an explicit value is clamped to the
// chunk count and then to the splits that `chunks_per_split` leaves non-empty.
inline int attn_cross_plan(int64_t n, int nq, int nk, int heads, int H,
                           int splits, cc_attn_cross_plan_info* p) {
  if (n <= 0 || nq <= 0 || nk <= 0 || splits < 0)
    return set_error(CC_ERR_INVALID,
                     "bad attn_cross args (n %lld, nq %d, nk %d, splits %d)",
                     (long long)n, nq, nk, splits);
  if (!attn_cross_supported(heads, H))
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_attn_cross needs head dim %d (heads %d, H %d)",
                     XATTN_HD, heads, H);
  if (nq > XATTN_NQ_MAX)
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_attn_cross takes at most %d queries a clip (%d)",
                     XATTN_NQ_MAX, nq);
  const int chunks = (int)(((int64_t)nk + XATTN_CHUNK - 1) / XATTN_CHUNK);
  if (splits == 0) {
    const int64_t units = n * heads;
    int want = 1;
    while (2 * want * units <= XATTN_RESIDENT_WGS) want *= 2;
    const int most = chunks / XATTN_MIN_CHUNKS > 0 ? chunks / XATTN_MIN_CHUNKS : 1;
    splits = want < most ? want : most;
  }
  if (splits > chunks) splits = chunks;
  const int per = (chunks + splits - 1) / splits;
  splits = (chunks + per - 1) / per;  // no empty split
  if (n * heads > 0x7fffffffLL / splits)
    return set_error(CC_ERR_INVALID,
                     "attn_cross grid too large (n %lld x %d heads x %d)",
                     (long long)n, heads, splits);
  p->splits = splits;
  p->chunk = XATTN_CHUNK;
  p->chunks_per_split = per;
  p->grid = (int32_t)(n * heads * splits);
  p->block = XATTN_BLOCK;
  p->workspace_floats =
      splits == 1 ? 0 : n * heads * splits * XATTN_PARTIAL_FLOATS;
  return CC_OK;
}

}  // namespace cc
