// GEMM launch plan: the single statement of which body a cc_gemm_bf16*
// call runs and how it is launched.  Host-only, no HIP types, so the rule
// can be evaluated (and is pinned, tests/test_gemm_plan_cpu.py) without a
// device.  cc_gemm.hip's launcher executes exactly what this returns.
#pragma once

#include <cstdint>
#include <cstdlib>

#include "cc_common.hpp"

namespace cc {

constexpr int GEMM_BK = 64;     // K-tile of both bodies
constexpr int GEMM_T128 = 128;  // k_gemm_bf16 block tile (square)
constexpr int GEMM_T256 = 256;  // k_gemm_bf16_t256 block tile (square)
constexpr int GEMM_FLEET = 256; // persistent fleet: one 256² WG per CU

// A/B knobs, read from the environment once per process (tools/
// t256_graph_repro.py, tools/persist_ab.py).  The defaults are production.
struct GemmKnobs {
  int tile = -1;    // CC_GEMM_TILE: 0 / 1 force the 128² / 256² body
  int persist = 1;  // CC_GEMM_PERSIST: 0 = one 256² tile per WG
  // CC_GEMM_FUSE_STATS: 0 = cc_gemm_bf16_res_stats runs the plain residual
  // GEMM and the stand-alone stats kernel on the 256² body too
  int fuse_stats = 1;
};

inline const GemmKnobs& gemm_env_knobs() {
  static const GemmKnobs k = [] {
    GemmKnobs v;
    if (const char* e = getenv("CC_GEMM_TILE")) v.tile = atoi(e);
    if (const char* e = getenv("CC_GEMM_PERSIST")) v.persist = atoi(e);
    if (const char* e = getenv("CC_GEMM_FUSE_STATS")) v.fuse_stats = atoi(e);
    return v;
  }();
  return k;
}

// lda / ldr are the row strides (elements) of A and of the residual; ldr
// is ignored without a residual.  Returns CC_OK and fills *p, or sets the
// error and returns its code.
inline int gemm_plan(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldr,
                     bool has_bias, int act, bool has_residual,
                     const GemmKnobs& knobs, cc_gemm_plan_info* p) {
  if (M <= 0 || N <= 0 || K <= 0)
    return set_error(CC_ERR_INVALID, "bad gemm args");
  if (K % GEMM_BK != 0)
    return set_error(CC_ERR_UNSUPPORTED,
                     "cc_gemm_bf16 requires K %% 64 == 0 (got %lld)",
                     (long long)K);
  if (!has_residual) ldr = N;
  if (lda < K || ldr < N)
    return set_error(CC_ERR_INVALID,
                     "gemm row stride below row length (lda %lld < K "
                     "%lld or ldr %lld < N %lld)",
                     (long long)lda, (long long)K, (long long)ldr,
                     (long long)N);
  if (lda % 8 != 0)
    return set_error(CC_ERR_INVALID,
                     "gemm lda %lld breaks the 16-byte alignment of the "
                     "direct-to-LDS loads (needs lda %% 8 == 0)",
                     (long long)lda);
  // A launch with lda != K or ldr != N is "strided" and always runs the
  // 128² body, the only one that carries the strides (the persistent 256²
  // loop stays dense: it is the hot kernel and the strided launches are
  // the small M = frames ones).
  const bool strided = lda != K || ldr != N;
  const int nbx = (int)((N + GEMM_T128 - 1) / GEMM_T128);
  const int nby = (int)((M + GEMM_T128 - 1) / GEMM_T128);
  const int nwg = nbx * nby;
  const int nbx2 = (int)((N + GEMM_T256 - 1) / GEMM_T256);
  const int nby2 = (int)((M + GEMM_T256 - 1) / GEMM_T256);
  const int nwg2 = nbx2 * nby2;
  // The 256² K-loop needs an even number of K-tiles, at least 4; M <= 128
  // is a single row of 128² tiles.
  const bool t256_ok =
      (K % 128 == 0) && (K >= 256) && M > GEMM_T256 / 2;
  // 256² 8-phase body for the shapes its halved A/B re-read traffic pays
  // on: K >= 1536 or N >= 1536 (profiles/r01_v10_b64.log), and, since it
  // became persistent, every shape whose 256-tile grid fills the fleet —
  // that includes N = 768 && K = 768 at large M (out64 720 -> 796 TF,
  // profiles/r02_gemm_persist.log).  What stays on the 128² body are the
  // shapes whose 256-tile grid would underfill the fleet (e.g. the tiny
  // visual-projection GEMM).
  // Exception for the K-trigger at M = frames (the CLS-only last layer's
  // fc2, N 768 / K 3072 at M 4704): 57 256-tiles leave most of the fleet
  // idle where the 128 body has 222 tiles — measured 67.1 vs 53.1 us per
  // launch, and 84.8 vs 67.6 us at the L/14 shape (76 vs 296 tiles),
  // profiles/r03_gemm_small_m_ab.log.  Kept narrow: only when the
  // 256-grid fills under half the fleet while the 128-grid fills at
  // least half.  The N-trigger stays: fc1 at the same M (228 / 304
  // 256-tiles) measured faster on the 256 body (29.7 vs 41.2 us).
  const bool underfill =
      N < 1536 && nwg2 < GEMM_FLEET / 2 && nwg >= GEMM_FLEET / 2;
  const bool t256 =
      !strided && t256_ok &&
      (knobs.tile >= 0
           ? knobs.tile != 0
           : ((K >= 1536 && !underfill) || N >= 1536 || nwg2 >= GEMM_FLEET));
  if (!t256) {
    p->body = GEMM_T128;
    p->tiles_x = nbx;
    p->tiles_y = nby;
    p->grid = nwg;
    p->block = 256;
    // XCD remap only for outputs that spill L3 (measured negative on the
    // L2-resident ViT shapes, profiles/r01_opt3)
    p->xcd_remap = ((M * N) > (48LL << 20)) ? 1 : 0;
    p->epi_staged = 0;  // the 128² body has only the scalar epilogue
    return CC_OK;
  }
  p->body = GEMM_T256;
  p->tiles_x = nbx2;
  p->tiles_y = nby2;
  // persistent fleet: 1 WG/CU, each walking tiles bid, bid + grid, ...
  p->grid = knobs.persist && nwg2 > GEMM_FLEET ? GEMM_FLEET : nwg2;
  p->block = 512;
  // stride + XCD remap order pays on skinny-N grids (row-band L2
  // sharing: qkv/fc1/fc2/patch +9-13%); on wide grids plain stride
  // wins (square8k 1295 vs 944 — profiles/r02_gemm_persist.log)
  p->xcd_remap = nbx2 <= 16 ? 1 : 0;
  // bf16 epilogue: LDS-staged coalesced when the launch fuses bias/act/
  // residual (A/B: tower 582 -> 812 TF, bench 3184 -> 4188 clips/s,
  // profiles/r02_epi_ab.log), scalar for bare C=A*B^T launches where the
  // 4-pass staging is pure overhead (bare fc1 928 scalar vs 825 staged,
  // profiles/r02_gemm_v20.log).  f32 outputs always store scalar.
  // (act: 0 none, 1 quick-gelu, 2 tanh-gelu, 3 erf-gelu.)
  p->epi_staged = (has_bias || has_residual || (act >= 1 && act <= 3)) ? 1 : 0;
  return CC_OK;
}

}  // namespace cc
