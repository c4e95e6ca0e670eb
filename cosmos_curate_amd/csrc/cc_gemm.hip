// bf16 MFMA GEMM for the ViT forward — hand-written for gfx950 (CDNA4).
//
// Replaces the cuBLAS GEMMs under CLIPModel.get_image_features
// (/root/reference/cosmos_curate/models/clip.py:71): patch-embed-as-GEMM,
// QKV / attention-out projections, MLP fc1/fc2, visual projection
// (SURVEY.md §2b row 8).
//
// C[M,N] = act(A[M,K] x B[N,K]^T + bias[N]) [+ residual[M,N]];
// A,B bf16 row-major, f32 accumulate on v_mfma_f32_16x16x32_bf16, output
// f32 or bf16.  The fused epilogue (quick-gelu, residual add) removes the
// bandwidth-bound elementwise kernels between GEMMs (one 206 MB round
// trip per MLP layer at the bench shape).
//
// Two kernel bodies; which one a call runs, its grid and its epilogue are
// decided by cc::gemm_plan (cc_gemm_plan.hpp) and nowhere else.
//
// Shared by both (cdna_hip_programming.md §5, step-3 ladder + measured
// fixes):
//   - BK=64 K-tiles, global->LDS via __builtin_amdgcn_global_load_lds
//     width 16, double-buffered.
//   - LDS image XOR-swizzled: the 16-byte slot for (row, k16) lives at
//     k16 ^ (row & 7).  glds demands a lane-linear LDS destination, so the
//     swizzle is applied to the per-lane GLOBAL source address (guide §5
//     "pre-swizzling the per-lane global address"); fragment ds_read_b128
//     applies the same XOR.  Measured motivation: linear layout put 4
//     same-bank rows in each 16-lane read group (SQ_LDS_BANK_CONFLICT =
//     0.75x extra LDS cycles, profiles/r01_pmc).
//   - XCD-aware bijective block remap (L2 affinity, guide §5.4): block b
//     of nwg runs on XCD b%8, so adjacent output tiles share an XCD's L2.
//   - M/N edges by clamped global loads + predicated stores; K % 64 == 0
//     required (all ViT shapes comply).
//
// k_gemm_bf16 (128² body): 128x128 block tile, 256 threads = 4 waves
// (2x2), each wave a 64x64 sub-tile = 4x4 MFMA fragments of 16x16; one
// barrier + vmcnt(0) per K-tile; one tile per workgroup; scalar epilogue.
// The only body that takes row strides for A and the residual.  Runs the
// small and the strided launches.
//
// k_gemm_bf16_t256 (256² body): 256x256 block tile, 512 threads = 8 waves
// (2x4), each wave 128x64; 8-phase schedule with counted vmcnt waits, a
// persistent fleet of workgroups walking the tile list, and an LDS-staged
// coalesced bf16 epilogue for fused launches.  Dense operands, K % 128 ==
// 0 and K >= 256 only.  Runs every large ViT GEMM (details at the kernel).

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_gemm_plan.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BM = cc::GEMM_T128, BN = cc::GEMM_T128, BK = cc::GEMM_BK;
constexpr int WM = 64, WN = 64;  // per-wave sub-tile (2x2 wave grid)
constexpr int FRAG = 16;         // mfma 16x16x32
constexpr int MFR = WM / FRAG;   // 4
constexpr int NFR = WN / FRAG;   // 4

__device__ __forceinline__ unsigned short f32_to_bf16_rne(float v) {
  union {
    float f;
    unsigned int u;
  } cv{v};
  unsigned int lsb = (cv.u >> 16) & 1;
  return (unsigned short)((cv.u + 0x7fffu + lsb) >> 16);
}

// fused activations (quick-gelu / SigLIP tanh-gelu / InternVideo2 erf-gelu;
// see epilogue notes)
template <int ACT>
__device__ __forceinline__ float cc_act(float v) {
  if constexpr (ACT == 1)
    return v * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * v));
  if constexpr (ACT == 2) {  // tanh-gelu (SigLIP gelu_pytorch_tanh)
    // tanh(z) = 1 - 2/(e^{2z}+1): __expf+rcp beats libm tanhf
    // (~80 us/launch at the SigLIP fc1 shape, r01_siglip_prof)
    float z = 0.7978845608028654f * (v + 0.044715f * v * v * v);
    float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * z) + 1.0f);
    return 0.5f * v * (1.0f + t);
  }
  if constexpr (ACT == 3)  // exact (erf) gelu: torch gelu(approximate="none")
    return 0.5f * v * (1.0f + erff(v * 0.70710678f));
  return v;
}

// XCD-aware bijective remap of a linear block id (guide §5.4): block b
// ran on XCD b%8; give XCD x the contiguous tile range so its L2 sees
// adjacent tiles.  q = nwg/8, r = nwg%8.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  int q = nwg >> 3, r = nwg & 7;
  int xcd = orig & 7, lid = orig >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lid;
}

// one wave stages CHUNKS x 8 rows of a [rows x BK] bf16 tile into LDS via
// glds (1 KB per chunk), with the k16 ^ (row&7) source swizzle.  lds_base
// = this wave's slice.  The 128² body stages 32-row slices (4 chunks), the
// 256² body 16-row slices of a 128-row half-tile (2 chunks).
template <int CHUNKS>
__device__ __forceinline__ void stage_rows(const __bf16* __restrict__ src,
                                           long ld, long row0, long row_limit,
                                           long k0, __bf16* lds_base,
                                           int lane) {
  const int lrow8 = lane >> 3;            // local row within each 8-row chunk
  const int slot = lane & 7;              // LDS 16B slot this lane fills
  const int gk16 = slot ^ lrow8;          // swizzle: global k16 feeding slot
#pragma unroll
  for (int j = 0; j < CHUNKS; j++) {
    long grow = row0 + j * 8 + lrow8;
    grow = grow < 0 ? 0 : (grow >= row_limit ? row_limit - 1 : grow);
    const __bf16* gptr = src + grow * ld + k0 + (long)gk16 * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)gptr,
        (__attribute__((address_space(3))) unsigned int*)(lds_base + j * 8 * BK),
        16, 0, 0);
  }
}

// fragment read honoring the swizzle: elements (row, kk+8*(lane>>4)..+8)
__device__ __forceinline__ bf16x8 frag_read(const __bf16* tile, int row,
                                            int k16) {
  int slot = k16 ^ (row & 7);
  return *(const bf16x8*)(tile + (long)row * BK + slot * 8);
}

// lda / ldr: row strides (elements) of A and of the residual — K and N
// for dense operands; larger when the rows are a strided subset of a
// bigger tensor (the CLS rows of [frames*seq, hidden]).  B and C are
// always dense.
//
// LN_IN (both bodies): A is the raw input of a LayerNorm
// whose affine part is folded into B, and the epilogue finishes the
// normalisation per row before the activation:
//   act(rstd_m * (acc - mean_m * colsum[n]) + bias[n])
// with murstd[m] = (mean, rstd) of A's row m and bias = W beta + b.
template <int ACT, bool HAS_BIAS, bool HAS_RES, bool LN_IN>  // ACT 1 = quick-gelu
__global__ __launch_bounds__(256, 2) void k_gemm_bf16(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    void* __restrict__ C, const float* __restrict__ bias,
    const __bf16* __restrict__ residual, long M, long N, long K, long lda,
    long ldr, int c_is_bf16, int nbx, int nwg, int do_remap,
    const float* __restrict__ colsum, const float2* __restrict__ murstd) {
  __shared__ __bf16 lds[2 * (BM + BN) * BK];  // one __shared__ object (G16 4a)
#define AS(b) (lds + (b) * (BM * BK))
#define BS(b) (lds + 2 * (BM * BK) + (b) * (BN * BK))

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int waveM = wid >> 1, waveN = wid & 1;

  int orig = blockIdx.x;
  if (do_remap) orig = xcd_remap(orig, nwg);
  const long bm = (long)(orig / nbx) * BM;
  const long bn = (long)(orig % nbx) * BN;

  const long arow0 = bm + 32 * wid;
  const long brow0 = bn + 32 * wid;

  f32x4 acc[MFR][NFR] = {};

  const long KT = K / BK;
  stage_rows<4>(A, lda, arow0, M, 0, AS(0) + 32 * wid * BK, lane);
  stage_rows<4>(B, K, brow0, N, 0, BS(0) + 32 * wid * BK, lane);

  const int arow_frag = waveM * WM + (lane & 15);
  const int brow_frag = waveN * WN + (lane & 15);
  int buf = 0;
  for (long kt = 0; kt < KT; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const __bf16* At = AS(buf);
    const __bf16* Bt = BS(buf);
    // Register-double-buffered fragments (graduated v9, profiles/
    // r01_gemm_v9.log): read BOTH k-groups up front (16 ds_read_b128 into
    // 64 live VGPRs) and issue the glds m0 chain under their latency, so
    // the phase runs ONE wait + 32 back-to-back MFMAs.  The previous
    // per-group form made hipcc reuse 24 staging VGPRs = 4 full
    // lgkmcnt(0) drains per phase (+12-18% measured from this change).
    bf16x8 afrag[2][MFR], bfrag[2][NFR];
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int k16 = (g << 2) + (lane >> 4);
#pragma unroll
      for (int m = 0; m < MFR; m++)
        afrag[g][m] = frag_read(At, arow_frag + m * FRAG, k16);
#pragma unroll
      for (int n = 0; n < NFR; n++)
        bfrag[g][n] = frag_read(Bt, brow_frag + n * FRAG, k16);
    }
    if (kt + 1 < KT) {
      const long k0 = (kt + 1) * BK;
      stage_rows<4>(A, lda, arow0, M, k0, AS(buf ^ 1) + 32 * wid * BK, lane);
      stage_rows<4>(B, K, brow0, N, k0, BS(buf ^ 1) + 32 * wid * BK, lane);
    }
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
      for (int m = 0; m < MFR; m++)
#pragma unroll
        for (int n = 0; n < NFR; n++)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[g][m], bfrag[g][n], acc[m][n], 0, 0, 0);
    buf ^= 1;
  }

  // epilogue: C/D map for 16x16x32: col = lane&15, row = (lane>>4)*4 + reg.
  // Interior tiles take the unguarded path: per-element bounds branches
  // around the residual/bias loads force hipcc into one dependent
  // load+vmcnt(0) per element (guide §5 trap (c); 458 vs 632 TF measured).
  const long crow_base = bm + waveM * WM + 4 * (lane >> 4);
  const long ccol_base = bn + waveN * WN + (lane & 15);
  const bool interior = (bm + BM <= M) && (bn + BN <= N);
  if (interior) {
#pragma unroll
    for (int m = 0; m < MFR; m++) {
      float2 mr[4] = {};  // LN_IN: (mean, rstd) of this fragment's 4 rows
      if constexpr (LN_IN) {
#pragma unroll
        for (int r = 0; r < 4; r++) mr[r] = murstd[crow_base + m * FRAG + r];
      }
#pragma unroll
      for (int n = 0; n < NFR; n++) {
        const long col = ccol_base + n * FRAG;
        float bval = 0.0f;
        if constexpr (HAS_BIAS) bval = bias[col];
        if constexpr (LN_IN) {
          const float sval = colsum[col];
#pragma unroll
          for (int r = 0; r < 4; r++)
            acc[m][n][r] = mr[r].y * (acc[m][n][r] - mr[r].x * sval);
        }
        // batch the residual loads (independent, one wait) before the
        // store sequence — an interleaved load/store chain serializes
        float rv[4];
        if constexpr (HAS_RES) {
#pragma unroll
          for (int r = 0; r < 4; r++)
            rv[r] = (float)residual[(crow_base + m * FRAG + r) * ldr + col];
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const long row = crow_base + m * FRAG + r;
          float v = cc_act<ACT>(acc[m][n][r] + bval);
          if constexpr (HAS_RES) v += rv[r];
          if (c_is_bf16)
            ((unsigned short*)C)[row * N + col] = f32_to_bf16_rne(v);
          else
            ((float*)C)[row * N + col] = v;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int m = 0; m < MFR; m++) {
#pragma unroll
    for (int n = 0; n < NFR; n++) {
      const long col = ccol_base + n * FRAG;
      if (col >= N) continue;
      float bval = 0.0f;
      if constexpr (HAS_BIAS) bval = bias[col];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long row = crow_base + m * FRAG + r;
        if (row >= M) continue;
        if constexpr (LN_IN) {
          const float2 mr = murstd[row];
          acc[m][n][r] = mr.y * (acc[m][n][r] - mr.x * colsum[col]);
        }
        float v = cc_act<ACT>(acc[m][n][r] + bval);
        if constexpr (HAS_RES) v += (float)residual[row * ldr + col];
        if (c_is_bf16)
          ((unsigned short*)C)[row * N + col] = f32_to_bf16_rne(v);
        else
          ((float*)C)[row * N + col] = v;
      }
    }
  }
#undef AS
#undef BS
}

// ---- 256x256 8-phase template kernel (guide "The 256² 8-phase
// template", schedule derived + race-screened through tools/gemm_v10
// ... v22; round-2 ladder in DESIGN.md §9a) ----
// 512 threads = 8 waves (2M x 4N), per-wave 128x64 = 8x4 frags; LDS
// 128 KiB; PERSISTENT fleet (grid = min(nwg, 256)); raw s_barrier
// phases; COUNTED vmcnt(4) publish before the last barrier of each K-tile
// (B(t+2) spans each boundary in flight); T19 scheduler weave of next-phase ds_reads into
// the MFMA clusters; template-selected epilogue (LDS-staged coalesced
// for fused bias/act/residual, scalar otherwise; EPI_STAGED is always
// ACT != 0 || HAS_BIAS || HAS_RES).  Which shapes it serves is
// cc::gemm_plan's rule (the ViT GEMM mix; batch-64 per-shape TF in
// profiles/r02_gemm_v21.log + the epilogue-on numbers in
// profiles/r02_epi_ab2.log).
constexpr int BM2 = cc::GEMM_T256, BN2 = cc::GEMM_T256;
constexpr int WM2 = 128, WN2 = 64;
constexpr int MFR2 = WM2 / FRAG;  // 8
constexpr int NFR2 = WN2 / FRAG;  // 4

//
// LN_IN: the folded-LayerNorm epilogue (see k_gemm_bf16).  The tile's 256
// (mean, rstd) pairs are a 2 KB LDS table behind the 128 KiB of operand
// buffers, staged like the operands: one 4-byte-wide glds per wave (its
// 32 rows), issued with the tile's prologue, landed by the rep-top
// wait and published by the rep-top barrier; the epilogue reads it.
// No VGPR carries it (a register-held pair was spilled around the
// epilogue and its vmcnt(0) exposed one load latency per tile).  TWO
// tables, alternating per tile: tile r+1's glds is issued before tile r's
// epilogue reads table r.  Table (r+1)&1 was last read in epilogue r-1,
// which every wave left before any wave passed rep-top barrier r, and the
// glds is issued after that.
//
// STATS: the epilogue also writes the LayerNorm statistics of the C rows
// it stores, stats[row][col/64] = (sum, sum of squares) over the wave's
// 64 columns of that row, taken in f32 from the rounded bf16 values.  In
// the staged read-back 8 adjacent lanes hold one row's 64 columns, so it
// is 3 DPP adds per value, no LDS, no barrier.  Needs N % 64 == 0.
// LN_IN and STATS launches are bf16-out and always staged.
//
// Column tables: the tile's 256 bias values, and under
// LN_IN its 256 column sums, are staged the same way, 2 KB per tile: wave w
// fills floats [64 w, 64 w + 64) with one 4-byte-wide glds, waves 0-3 the
// bias of the tile's columns, waves 4-7 the column sums (the bias again
// without LN_IN, so every wave issues the same number of loads and the
// hand-counted waits of the epilogue hold for all of them).  The column is
// clamped like the A rows; the store is what is predicated.  A plain
// VGPR-destination load here would make hipcc drain the whole prologue
// burst with vmcnt(0) (it waits that way for any ordinary load issued
// beside LDS-DMA).  TWO tables, alternating per tile, for the reason the
// (mean, rstd) tables alternate: tile r+1's glds is issued before tile r's
// epilogue reads table r.  Table (r+1)&1 was last read in epilogue r-1,
// which every wave left before any wave passed rep-top barrier r, and the
// glds is issued after that.
constexpr int LN_TAB = BM2 * 4;  // one table: 256 float2 = 2 KB, in bf16 elements
constexpr int COL_TAB = BN2 * 4;  // bias[256] + colsum[256] floats = 2 KB

// 16 B from global memory, invisible to hipcc's wait bookkeeping: the
// caller waits with a hand-counted vmcnt (res_wait below) before the first
// use
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
// (base must be wave-uniform: it is the scalar half of the address)
__device__ __forceinline__ void load16_uncounted(u32x4& dst, const void* base,
                                                 unsigned byte_off) {
  // s_nop 4: the base may come straight from a v_readfirstlane, and hipcc
  // pads no hazard for an instruction inside an asm string
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2"
               : "=v"(dst)
               : "v"(byte_off), "s"(base)
               : "memory");
}
// The wait for a pass's 4 loads: vmcnt(CNT_NEXT) when the next tile's
// prologue is in the queue, vmcnt(CNT_LAST) when it is not, then ONE
// statement that takes the four destinations "+v", so that no use of them
// is scheduled above it.  The wait statements themselves name no register:
// with the registers tied to two alternative statements hipcc copied them
// into each statement's own operands ahead of the wait, reading them before
// the data had landed.  Any copy it makes for the one statement below sits
// behind the wait.
template <int CNT_NEXT, int CNT_LAST>
__device__ __forceinline__ void res_wait(bool has_next, u32x4 (&r)[4]) {
  static_assert(CNT_NEXT >= CNT_LAST && CNT_LAST >= 0 && CNT_NEXT < 64,
                "vmcnt is a 6-bit field");
  if (has_next)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CNT_NEXT) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CNT_LAST) : "memory");
  asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3])::"memory");
}

// v + (the same value in the lane DPP control CTRL names)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                            CTRL, 0xf, 0xf, false);
  return v + __builtin_bit_cast(float, o);
}
// sum over each aligned group of 8 lanes (every lane gets the total):
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
__device__ __forceinline__ float sum8(float v) {
  return dpp_add<0x141>(dpp_add<0x4e>(dpp_add<0xb1>(v)));
}

template <int ACT, bool HAS_BIAS, bool HAS_RES, bool EPI_STAGED, bool LN_IN,
          bool STATS>
__global__ __launch_bounds__(512, 1) void k_gemm_bf16_t256(
    const __bf16* __restrict__ A, const __bf16* __restrict__ B,
    void* __restrict__ C, const float* __restrict__ bias,
    const __bf16* __restrict__ residual, long M, long N, long K,
    int c_is_bf16, int nbx, int nwg, int order_mode,
    const float* __restrict__ colsum, const float2* __restrict__ murstd,
    float2* __restrict__ stats) {
  static_assert(!STATS || HAS_RES, "the stats epilogue is the residual one");
  // Round-2 structure: PERSISTENT multi-tile (grid = min(nwg, 256), one
  // WG per CU) around the round-1 8-phase glds schedule.  Each WG walks
  // tiles bid, bid+grid, ... and issues the NEXT tile's 12-glds
  // prologue BEFORE the epilogue stores, so prologue HBM latency hides
  // under the C writeback instead of stalling a fresh WG (it does only
  // because nothing in the staged epilogue makes hipcc wait vmcnt(0)
  // after it: see the epilogue).  Measured
  // +18-27% at every batch-64 ViT shape and +13% at square8k
  // (profiles/r02_gemm_persist.log: fc1 711->874, fc2 795->968, patch
  // 814->964, qkv 724->887 TF within one box).  order_mode: 0 = plain
  // stride; 1 = stride + bijective XCD remap (skinny-N grids, L2 row
  // sharing).  Sync structure per K-tile is UNCHANGED from the
  // race-screened v11 (vmcnt(0) publish at ph3, leading barriers).
  static_assert(!LN_IN || HAS_BIAS, "the folded norm always carries a bias");
  // a launch with a bias stages the column tables, whichever epilogue its
  // output type then takes
  constexpr bool COLTAB = HAS_BIAS;
  // 128 KiB (+ the two 2 KB (mean, rstd) tables under LN_IN, + the two
  // 2 KB column tables with a bias: 136 KiB at the most)
  __shared__ __bf16 lds[2 * (BM2 + BN2) * BK + (LN_IN ? 2 * LN_TAB : 0) +
                        (COLTAB ? 2 * COL_TAB : 0)];
// column table b; this wave stages floats [64 wid, 64 wid + 64) of it
#define COLTAB_AT(b)                                                        \
  ((float*)(lds + 2 * (BM2 + BN2) * BK + (LN_IN ? 2 * LN_TAB : 0) +         \
            (b) * COL_TAB))
#define STAGE_COL2(b)                                                       \
  do {                                                                      \
    if constexpr (COLTAB) {                                                 \
      const long c = bn + (wid & 3) * 64 + lane;                            \
      const float* g = ((LN_IN && wid >= 4) ? colsum : bias) +              \
                       (c < N ? c : N - 1);                                 \
      __builtin_amdgcn_global_load_lds(                                     \
          (const __attribute__((address_space(1))) unsigned int*)g,         \
          (__attribute__((address_space(3))) unsigned int*)(COLTAB_AT(b) +  \
                                                            wid * 64),      \
          4, 0, 0);                                                         \
    }                                                                       \
  } while (0)
// table b; this wave stages dwords [64 wid, 64 wid + 64) of it: dword d is
// component d & 1 of tile row d >> 1, the row clamped like the A rows
#define LNTAB(b) ((float*)(lds + 2 * (BM2 + BN2) * BK + (b) * LN_TAB))
#define STAGE_LN2(b)                                                        \
  do {                                                                      \
    if constexpr (LN_IN) {                                                  \
      const long r = bm + (tid >> 1);                                       \
      const float* g = (const float*)(murstd + (r < M ? r : M - 1)) +       \
                       (tid & 1);                                           \
      __builtin_amdgcn_global_load_lds(                                     \
          (const __attribute__((address_space(1))) unsigned int*)g,         \
          (__attribute__((address_space(3))) unsigned int*)(LNTAB(b) +      \
                                                            wid * 64),      \
          4, 0, 0);                                                         \
    }                                                                       \
  } while (0)
#define A2T(b) (lds + (b) * (BM2 * BK))
#define B2T(b) (lds + 2 * (BM2 * BK) + (b) * (BN2 * BK))
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int waveM = wid >> 2, waveN = wid & 3;
  const long KT = K / BK;  // the plan guarantees even, >= 4
  const long srow = wid * 16;
  const int arow_base = waveM * WM2 + (lane & 15);
  const int brow_base = waveN * WN2 + (lane & 15);
  bf16x8 bfragT[NFR2][2];  // held for the whole K-tile
  bf16x8 afrag[2][2];      // one quadrant: 2 M-frags x 2 k-steps

// one wave stages its 16-row slice of a 128-row half-tile: 2 glds.
#define STAGE_A2(t, h)                                                      \
  stage_rows<2>(A, K, bm + (h) * 128 + srow, M, (t) * BK,                   \
                A2T((t) & 1) + ((h) * 128 + srow) * BK, lane)
#define STAGE_B2(t, h)                                                      \
  stage_rows<2>(B, K, bn + (h) * 128 + srow, N, (t) * BK,                   \
                B2T((t) & 1) + ((h) * 128 + srow) * BK, lane)

  const int tiles = (nwg + (int)gridDim.x - 1) / (int)gridDim.x;
  long bm, bn;
  {
    int orig = (int)blockIdx.x;
    if (order_mode == 1) orig = xcd_remap(orig, nwg);
    bm = (long)(orig / nbx) * BM2;
    bn = (long)(orig % nbx) * BN2;
  }
  // first prologue: A(0) h0,h1, B(0) h0,h1, B(1) h0,h1 (12 glds); later
  // tiles' prologues issue under the previous epilogue.
  STAGE_LN2(0);
  STAGE_COL2(0);
  STAGE_A2(0, 0);
  STAGE_A2(0, 1);
  STAGE_B2(0, 0);
  STAGE_B2(0, 1);
  STAGE_B2(1, 0);
  STAGE_B2(1, 1);

  // glds of one prologue per wave, and stores of one staged epilogue per
  // wave: 4 passes x 4 chunks, each one C store (+ one stats store).  Both
  // are the same for every wave and every tile (the stores are issued
  // unconditionally and range-checked by the hardware), which is what lets
  // the waits below be counted.
  constexpr int PRO_LOADS = 12 + (LN_IN ? 1 : 0) + (COLTAB ? 1 : 0);
  constexpr int PASS_STORES = STATS ? 8 : 4;
  const bool staged = (c_is_bf16 && EPI_STAGED) || LN_IN || STATS;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first prologue

  for (int rep = 0; rep < tiles; rep++) {
    if ((int)blockIdx.x + rep * (int)gridDim.x >= nwg) break;
    f32x4 acc[MFR2][NFR2] = {};
    // rep-top wait: land this tile's prologue, then publish it with the
    // barrier.  After a staged epilogue the queue is, youngest first,
    // [C/stats stores of the 4 passes : 4 PASS_STORES, prologue :
    // PRO_LOADS, <older>], so vmcnt(4 PASS_STORES) retires the prologue and
    // leaves the stores in flight: their acknowledgement is not waited for
    // here.  They retire at the first K-tile's counted waits, which they
    // are older than.  Nothing needs them sooner: a store's data is read
    // from its registers when it issues; the staging slice (A-buf1) was
    // read back by ds_read, and that data waited for, before the store it
    // fed; and the next tile writes only A-buf0 and the B-bufs until
    // STAGE_A2(1, .) in its first K-tile, which sits behind this barrier
    // and the epilogue's last ds_read.  The scalar epilogue's store count
    // is the compiler's business, so it drains; the first tile has no
    // stores ahead of it and drained before the loop.
    if (rep > 0) {
      if (staged)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * PASS_STORES) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

#define PHASE_MFMA2(q)                                                      \
  do {                                                                      \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                      \
    /* T19 dictation (round 2, +1-3%/shape, profiles/r02_gemm_v21.log):  */ \
    /* weave the next phase's ds_reads and the glds issues between the   */ \
    /* 16 MFMAs so their latency hides under the cluster (the source-    */ \
    /* level version of this, v12, regressed; the compile-time directive */ \
    /* does it without perturbing issue order elsewhere).  setprio       */ \
    /* dropped: it fenced the scheduler out of exactly this interleave.  */ \
    /* pattern 3 of the sweep (profiles/r02_t19_sweep.log): lead with   */ \
    /* 2 MFMAs, then weave [dsr, 2 MFMA, vmem] x6 — best at every ViT   */ \
    /* shape (patch 1041, qkv 916, fc1 914, fc2 1056 TF vs 875-1009     */ \
    /* for the coarser patterns).                                       */ \
    __builtin_amdgcn_sched_group_barrier(0x8 /*MFMA*/, 2, 0);               \
    _Pragma("unroll") for (int gi = 0; gi < 6; gi++) {                      \
      __builtin_amdgcn_sched_group_barrier(0x100 /*DS_READ*/, 1, 0);        \
      __builtin_amdgcn_sched_group_barrier(0x8 /*MFMA*/, 2, 0);             \
      __builtin_amdgcn_sched_group_barrier(0x10 /*VMEM*/, 1, 0);            \
    }                                                                       \
    _Pragma("unroll") for (int g = 0; g < 2; g++) {                         \
      _Pragma("unroll") for (int m = 0; m < 2; m++) {                       \
        _Pragma("unroll") for (int n = 0; n < NFR2; n++) {                  \
          acc[2 * (q) + m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(    \
              afrag[m][g], bfragT[n][g], acc[2 * (q) + m][n], 0, 0, 0);     \
        }                                                                   \
      }                                                                     \
    }                                                                       \
  } while (0)
  /* NOTE: no trailing barrier per phase (v11, profiles/r01_v11_ab.log,
     +5-8%): the B-buffer write-after-read hazard needs only 2-phase
     separation, which the per-phase leading barrier provides — wave W
     drains its reads (lgkm0) before it reaches the NEXT phase's
     barrier, and any other wave's conflicting glds issues only after
     passing that barrier, two phases later.  Race-screened +
     determinism-checked at 774-3156-block grids. */

#define READ_A2(At, q)                                                      \
  _Pragma("unroll") for (int g = 0; g < 2; g++) {                           \
    const int k16 = (g << 2) + (lane >> 4);                                 \
    _Pragma("unroll") for (int m = 0; m < 2; m++) afrag[m][g] =             \
        frag_read(At, arow_base + (q) * 32 + m * FRAG, k16);                \
  }

#define READ_B2(Bt)                                                         \
  _Pragma("unroll") for (int g = 0; g < 2; g++) {                           \
    const int k16 = (g << 2) + (lane >> 4);                                 \
    _Pragma("unroll") for (int n = 0; n < NFR2; n++) bfragT[n][g] =         \
        frag_read(Bt, brow_base + n * FRAG, k16);                           \
  }

// one K-tile = 4 phases; stages the next A halves in ph1-2 and the
// tile-after-next B halves in ph3-4 (issue order proves vmcnt(4)):
#define KTILE2(t)                                                           \
  do {                                                                      \
    const __bf16* At = A2T((t) & 1);                                        \
    const __bf16* Bt = B2T((t) & 1);                                        \
    /* no-op since the publish below moved back before the barrier (the */ \
    /* queue holds only B(t+1):4 here, or nothing at tile 0 of a rep);  */ \
    /* kept as the compiler fence the measured schedule was built with. */ \
    /* At tile 0 of a later rep the queue holds the previous epilogue's */ \
    /* stores instead, which nothing here depends on: the count lets    */ \
    /* them all stand, so they retire at the publish below              */ \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + 4 * PASS_STORES)           \
                 : "memory");                                               \
    READ_B2(Bt);                                                            \
    READ_A2(At, 0);                                                         \
    if ((t) + 1 < KT) STAGE_A2((t) + 1, 0);                                 \
    __builtin_amdgcn_s_barrier();                                           \
    PHASE_MFMA2(0);                                                         \
    READ_A2(At, 1);                                                         \
    if ((t) + 1 < KT) STAGE_A2((t) + 1, 1);                                 \
    __builtin_amdgcn_s_barrier();                                           \
    PHASE_MFMA2(1);                                                         \
    READ_A2(At, 2);                                                         \
    __builtin_amdgcn_s_barrier();                                           \
    PHASE_MFMA2(2);                                                         \
    READ_A2(At, 3);                                                         \
    /* COUNTED publish (round 2, replaces the per-tile vmcnt(0) drain):  */ \
    /* the next tile's LDS reads need A(t+1) [ph1-2, 4 loads/wave] and   */ \
    /* B(t+1) [issued one tile earlier, strictly older] landed.  After   */ \
    /* issuing B(t+2)'s 4 loads, the per-wave VMEM queue newest-first is */ \
    /* [B(t+2):4, A(t+1):4, <older>]; vmcnt(4) retires everything except */ \
    /* B(t+2), which keeps spanning the tile boundary.  r01's            */ \
    /* "nondeterministic counted wait" (profiles/r01_t256_det2.log) sat  */ \
    /* BEFORE the B(t+2) issues with exactly 4 loads outstanding — a     */ \
    /* no-op wait, not out-of-order retirement; this placement fixes the */ \
    /* count.  Verified: 6-run multi-shape determinism screen + full GPU */ \
    /* parity suite (profiles/r02_gemm_v19.log).  Measured: fc1 864->905,*/ \
    /* fc2 950->1023, patch 940->1004 TF within one box.                 */ \
    if ((t) + 2 < KT) {                                                     \
      STAGE_B2((t) + 2, 0);                                                 \
      STAGE_B2((t) + 2, 1);                                                 \
      /* The wait sits HERE, before the barrier.  For a while it sat at  */ \
      /* the next tile's top (one more MFMA cluster of latency cover):   */ \
      /* that retires only the waiting wave's own loads, and the reads   */ \
      /* right after it take rows other waves staged, with no barrier    */ \
      /* after THEIR wait - a late load was read stale.  Dormant until   */ \
      /* the folded-LN route changed the memory traffic around the GEMMs */ \
      /* (1-7 of 224 bench rows off by ~1e-4 in 6 of 6 runs; 0 of 6 with */ \
      /* the wait here, profiles/r04_lnfold_det.txt).  Rule: counted     */ \
      /* wait, then a barrier, then the first read*/ \
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                      \
    } else {                                                                \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* tail drain */     \
    }                                                                       \
    __builtin_amdgcn_s_barrier();                                           \
    PHASE_MFMA2(3);                                                         \
  } while (0)

    for (long it = 0; it < KT / 2; ++it) {
      KTILE2(2 * it);
      KTILE2(2 * it + 1);
    }

    const long ebm = bm, ebn = bn;
    // barrier before the epilogue: the bf16 epilogue below stages C
    // through A-buf1, whose rows 96-127/224-255 other waves were still
    // reading in the last phase; the next tile's prologue (further
    // below) overwrites A-buf0/B-bufs with the same hazard.
    __builtin_amdgcn_s_barrier();
    // From here to the end of the tile every lane-dependent value is
    // derived again from an opaque copy of the thread id.  Derived from
    // `tid` itself, the address parts the epilogue and the next prologue
    // need (and the K-loop does not) are hoisted out of the rep loop, held
    // across the K-loop, spilled there, and reloaded here: a scratch
    // reload is a VGPR-destination load, so each one costs a vmcnt(0) in
    // the middle of the prefetch.
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));
    {  // NOLINT: shadows on purpose
    const int tid = tid_e, lane = tid_e & 63, wid = tid_e >> 6;
    const int waveM = wid >> 2, waveN = wid & 3;
    const long srow = wid * 16;
    const bool has_next = rep + 1 < tiles &&
                          (int)blockIdx.x + (rep + 1) * (int)gridDim.x < nwg;
    // Residual of the staged epilogue: pass p (32 tile rows of this wave)
    // adds 4 chunks of 16 B per lane, resq[p][0..3].  The loads are
    // branch-free (row and column clamped like stage_rows clamps: an
    // out-of-range lane loads a value that is never stored) and hidden
    // from hipcc in asm, which would otherwise wait vmcnt(0) for each one
    // beside the LDS-DMA in flight, draining the prologue below and taking
    // one HBM round trip per chunk, 16 per tile.  Passes 0-2 are issued
    // HERE, ahead of the prologue: the counter retires in issue order, so
    // whatever is issued after the prologue burst waits for all of it.
    // afrag and bfragT are dead, which is the 48 VGPRs the 12 loads take.
    // Pass 3 is issued after pass 0's write phase has freed a quarter of
    // the accumulators.
    //
    // Addressing of the read-back (loads and stores alike): chunk i of
    // pass p is 8 columns of tile row waveM 128 + 32 p + 8 i + lane / 8.
    // Everything is a 32-bit element offset from the tile's first row
    // (at most 256 N), on a wave-uniform 64-bit base, so no 64-bit lane
    // value is live across the K-loop.  row_off is made opaque here: the
    // 16 row offsets derived from it do not depend on the tile, and hoisted
    // out of the rep loop they are spilled, each reload a vmcnt(0).
    const int n32 = (int)N;
    const int tile_rows = (int)((M - ebm) < BM2 ? (M - ebm) : BM2);
    int row_off = (waveM * WM2 + (lane >> 3)) * n32;
    asm volatile("" : "+v"(row_off));
    const int col_abs = (int)ebn + waveN * WN2 + (lane & 7) * 8;
    u32x4 resq[4][4];
    auto issue_res = [&](int p) {
      if constexpr (HAS_RES) {
        const __bf16* rbase = residual + ebm * N;  // wave-uniform
        const int last_row = (tile_rows - 1) * n32;
        const int col = col_abs < n32 ? col_abs : n32 - 8;  // N % 8 == 0
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int ro = row_off + (p * 32 + i * 8) * n32;
          load16_uncounted(resq[p][i], rbase,
                           ((ro < last_row ? ro : last_row) + col) * 2);
        }
      }
    };
    // advance + issue the next tile's prologue BEFORE the epilogue's
    // write phase, so its HBM latency hides under the C writeback.  Each
    // epilogue calls it itself: the staged one after its first residual
    // loads, whose registers then live in that branch alone (live across
    // the join of a common call they were spilled straight after the
    // loads were issued, before the data had landed).
    auto next_prologue = [&] {
      if (has_next) {
        int orig = (int)blockIdx.x + (rep + 1) * (int)gridDim.x;
        if (order_mode == 1) orig = xcd_remap(orig, nwg);
        bm = (long)(orig / nbx) * BM2;
        bn = (long)(orig % nbx) * BN2;
        STAGE_LN2((rep + 1) & 1);
        STAGE_COL2((rep + 1) & 1);
        STAGE_A2(0, 0);
        STAGE_A2(0, 1);
        STAGE_B2(0, 0);
        STAGE_B2(0, 1);
        STAGE_B2(1, 0);
        STAGE_B2(1, 1);
      }
    };

    // ---- epilogue ----
    // bf16 output (all tower-internal GEMMs): LDS-staged + coalesced.
    // The fragment C/D map scatters 2-byte lanes (col = lane&15, row =
    // 4*(lane>>4)+r): storing it directly costs one 2 B store per
    // element and the same pattern for the fused residual loads — the
    // dominant cost at the thin ViT shapes once the K-loop is fed
    // (attn_out 429 vs ~790 TF bare, profiles/r02_persist_ab.log).
    // Instead: 4 passes of 2 M-fragments stage bf16(act(acc+bias))
    // through this wave's free 4 KB slice of A-buf1 (last read before
    // the barrier above; the next prologue writes only A-buf0/B-bufs),
    // then read back row-contiguous 16 B chunks, fuse the residual add
    // in f32, and store full b128s (8 lanes cover 128 contiguous
    // bytes of a C row).  Residual numerics: the pre-residual value is
    // rounded to bf16 once before the f32 add — one extra rounding vs
    // the scalar path, inside the embedding-cosine contract.
    const long crow_base = ebm + waveM * WM2 + 4 * (lane >> 4);
    const long ccol_base = ebn + waveN * WN2 + (lane & 15);
    if (staged) {
      issue_res(0);
      issue_res(1);
      issue_res(2);
      next_prologue();
      __bf16* slice = A2T(1) + wid * 2048;  // 4 KB per wave
      // bias and column sum depend only on the n-fragment: 4 values per
      // lane each, read from this tile's column table (landed by the
      // rep-top wait, published by the rep-top barrier)
      float bhoist[NFR2] = {};
      float shoist[NFR2] = {};  // LN_IN: column sums of the folded weight
      if constexpr (COLTAB) {
        const float* ct = COLTAB_AT(rep & 1) + waveN * WN2 + (lane & 15);
#pragma unroll
        for (int n = 0; n < NFR2; n++) {
          bhoist[n] = ct[n * FRAG];
          if constexpr (LN_IN) shoist[n] = ct[BN2 + n * FRAG];
        }
      }
      // Stores: one descriptor per tile for C (and one for the stats),
      // base = the tile's first row, num_records = the bytes of the rows
      // of this tile that exist.  A lane's byte offset is (tile row, column),
      // so a row >= M lies beyond num_records and the hardware drops the
      // store; a column >= N, or a stats lane that is not its group's
      // leader, is sent there by a select.  Every wave therefore issues the
      // same 4 (8) stores per pass whatever the tile, no branch around any
      // of them, and the offsets stay far below 4 GB however large C is.
      // Built from wave-uniform values only.
      constexpr unsigned OOB = 0x80000000u;
      const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
          (__bf16*)C + ebm * N, 0, tile_rows * n32 * 2, 0x00020000);
      __amdgpu_buffer_rsrc_t s_rsrc = c_rsrc;
      if constexpr (STATS)
        s_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            stats + ebm * (N >> 6), 0, tile_rows * (n32 >> 6) * 8, 0x00020000);
      // Hand-counted waits of the residual passes.  Issue order per wave:
      //   R0 R1 R2 (4 loads each) | prologue (PRO, or nothing after the
      //   last tile) | pass 0 write phase | R3 | wait R0, St0 | wait R1,
      //   St1 | wait R2, St2 | wait R3, St3       (St = PASS_STORES)
#define RES_WAIT(p, cnt)                                                    \
  res_wait<(cnt) + PRO_LOADS, (cnt)>(has_next, resq[p])
#pragma unroll
      for (int p = 0; p < 4; p++) {
#pragma unroll
        for (int mm = 0; mm < 2; mm++) {
          const int m = 2 * p + mm;
          float2 mr[4] = {};  // LN_IN: (mean, rstd) of this lane's 4 rows
          if constexpr (LN_IN) {
            // read as float, not float2: hipcc puts a vmcnt(0) in front
            // of an LDS read that its type-based alias analysis cannot
            // tell from the LDS-DMA in flight (the prologue's), and it can
            // tell a float from the DMA's dwords but not a HIP vector type
            const float* t = LNTAB(rep & 1) +
                             2 * (waveM * WM2 + m * FRAG + 4 * (lane >> 4));
#pragma unroll
            for (int r = 0; r < 4; r++)
              mr[r] = make_float2(t[2 * r], t[2 * r + 1]);
          }
#pragma unroll
          for (int n = 0; n < NFR2; n++) {
            const float bval = bhoist[n];
            const int lrow_b = mm * 16 + 4 * (lane >> 4);
            const int lcol = n * FRAG + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
              if constexpr (LN_IN)
                acc[m][n][r] = mr[r].y * (acc[m][n][r] - mr[r].x * shoist[n]);
              float v = cc_act<ACT>(acc[m][n][r] + bval);
              *(unsigned short*)(slice + (lrow_b + r) * 64 + lcol) =
                  f32_to_bf16_rne(v);
            }
          }
        }
        if constexpr (HAS_RES) {
          if (p == 0) {
            issue_res(3);
            // youngest first: [R3:4, PRO, R2:4, R1:4, R0]
            RES_WAIT(0, 12);
          } else if (p == 1) {
            // [St0, R3:4, PRO, R2:4, R1]
            RES_WAIT(1, PASS_STORES + 8);
          } else if (p == 2) {
            // [St1, St0, R3:4, PRO, R2]
            RES_WAIT(2, 2 * PASS_STORES + 4);
          } else {
            // [St2, St1, St0, R3]; the prologue is older than R3 and
            // retires with it
            res_wait<3 * PASS_STORES, 3 * PASS_STORES>(has_next, resq[3]);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int elem = i * 512 + lane * 8;
          const int ro = row_off + (p * 32 + i * 8) * n32;  // tile row x N
          const bool col_ok = col_abs < n32;  // N % 8 == 0 always
          const unsigned c_off = col_ok ? (unsigned)(ro + col_abs) * 2 : OOB;
          bf16x8 v8 = *(const bf16x8*)(slice + elem);
          float s = 0.0f, ss = 0.0f;
          if constexpr (HAS_RES) {
            const bf16x8 r8 = __builtin_bit_cast(bf16x8, resq[p][i]);
#pragma unroll
            for (int e = 0; e < 8; e++) {
              v8[e] = (__bf16)((float)v8[e] + (float)r8[e]);
              if constexpr (STATS) {
                const float f = (float)v8[e];
                s += f;
                ss += f * f;
              }
            }
          }
          __builtin_amdgcn_raw_buffer_store_b128(
              __builtin_bit_cast(u32x4, v8), c_rsrc, (int)c_off, 0, 0);
          if constexpr (STATS) {
            // the 8 lanes of a row hold its 64 columns (N % 64 == 0, so
            // they share the side of the N edge); lanes whose row or
            // column is out of range sum values that are never stored
            s = sum8(s);
            ss = sum8(ss);
            const unsigned s_off =
                (col_ok && (lane & 7) == 0)
                    ? (unsigned)((ro + col_abs) >> 6) * 8
                    : OOB;
            u32x2 st;
            st[0] = __builtin_bit_cast(unsigned, s);
            st[1] = __builtin_bit_cast(unsigned, ss);
            __builtin_amdgcn_raw_buffer_store_b64(st, s_rsrc, (int)s_off, 0, 0);
          }
        }
      }
#undef RES_WAIT
    } else {
      // scalar store path (f32 outputs always; bf16 when epi_staged=0).
      // bias hoisted exactly like the staged path: 4 loads per lane
      // instead of one dependent load per fragment (the old
      // per-element-load serialization, guide trap (c)).
      next_prologue();
      const bool interior = (ebm + BM2 <= M) && (ebn + BN2 <= N);
      float bhoist2[NFR2] = {};
      if constexpr (HAS_BIAS) {
        // from the column table as well (a column >= N reads a clamped
        // value that is never stored)
        const float* ct = COLTAB_AT(rep & 1) + waveN * WN2 + (lane & 15);
#pragma unroll
        for (int n = 0; n < NFR2; n++) bhoist2[n] = ct[n * FRAG];
      }
#pragma unroll
      for (int m = 0; m < MFR2; m++) {
#pragma unroll
        for (int n = 0; n < NFR2; n++) {
          const long col = ccol_base + n * FRAG;
          if (!interior && col >= N) continue;
          const float bval = bhoist2[n];
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const long row = crow_base + m * FRAG + r;
            if (!interior && row >= M) continue;
            float v = cc_act<ACT>(acc[m][n][r] + bval);
            if constexpr (HAS_RES) v += (float)residual[row * N + col];
            if (c_is_bf16)
              ((unsigned short*)C)[row * N + col] = f32_to_bf16_rne(v);
            else
              ((float*)C)[row * N + col] = v;
          }
        }
      }
    }
    }  // lane-dependent values of the epilogue
  }
#undef LNTAB
#undef STAGE_LN2
#undef COLTAB_AT
#undef STAGE_COL2
#undef A2T
#undef B2T
#undef STAGE_A2
#undef STAGE_B2
#undef PHASE_MFMA2
#undef READ_A2
#undef READ_B2
#undef KTILE2
}

struct GemmArgs {
  const __bf16 *A, *B;
  void* C;
  const float* bias;
  const __bf16* residual;
  long M, N, K, lda, ldr;
  int c_is_bf16;
  hipStream_t stream;
  // folded-LayerNorm launches only (LN_IN / STATS)
  const float* colsum = nullptr;
  const float2* murstd = nullptr;
  float2* stats = nullptr;
};

// One launch per (ACT, HAS_BIAS, HAS_RES, LN_IN, STATS); the plan picks
// the body.  The 256² epilogue is a TEMPLATE parameter fixed by the same
// five, not a runtime branch: carrying both epilogues in one instantiation
// spilled VGPRs in the rep loop and cost ~10% bare
// (profiles/r02_t19_sweep.log, prod column vs the single-epilogue tool
// kernels).  The 128² body has no STATS form: cc_gemm_bf16_res_stats
// follows it with the stand-alone stats kernel.
template <int ACT, bool HB, bool HR, bool LN = false, bool ST = false>
void gemm_run(const cc_gemm_plan_info& p, const GemmArgs& g) {
  const int nwg = p.tiles_x * p.tiles_y;
  if (p.body == cc::GEMM_T256)
    hipLaunchKernelGGL(
        (k_gemm_bf16_t256<ACT, HB, HR, ACT != 0 || HB || HR, LN, ST>),
        dim3(p.grid), dim3(p.block), 0, g.stream, g.A, g.B, g.C, g.bias,
        g.residual, g.M, g.N, g.K, g.c_is_bf16, p.tiles_x, nwg, p.xcd_remap,
        g.colsum, g.murstd, g.stats);
  else
    hipLaunchKernelGGL((k_gemm_bf16<ACT, HB, HR, LN>), dim3(p.grid),
                       dim3(p.block), 0, g.stream, g.A, g.B, g.C, g.bias,
                       g.residual, g.M, g.N, g.K, g.lda, g.ldr, g.c_is_bf16,
                       p.tiles_x, nwg, p.xcd_remap, g.colsum, g.murstd);
}

using GemmRunFn = void (*)(const cc_gemm_plan_info&, const GemmArgs&);
// a null entry is a combination that is not instantiated: erf-gelu (act 3)
// exists with a bias and no residual only, what an fc1 needs
constexpr GemmRunFn kGemmRun[4][2][2] = {  // [act][has_bias][has_residual]
    {{gemm_run<0, false, false>, gemm_run<0, false, true>},
     {gemm_run<0, true, false>, gemm_run<0, true, true>}},
    {{gemm_run<1, false, false>, gemm_run<1, false, true>},
     {gemm_run<1, true, false>, gemm_run<1, true, true>}},
    {{gemm_run<2, false, false>, gemm_run<2, false, true>},
     {gemm_run<2, true, false>, gemm_run<2, true, true>}},
    {{nullptr, nullptr}, {gemm_run<3, true, false>, nullptr}}};
// folded-norm consumers: bias (= W beta + b) always, no residual
constexpr GemmRunFn kGemmRunLn[4] = {  // [act]
    gemm_run<0, true, false, true>, gemm_run<1, true, false, true>,
    gemm_run<2, true, false, true>, gemm_run<3, true, false, true>};

// act: 0 none, 1 quick-gelu, 2 tanh-gelu (SigLIP), 3 erf-gelu
// (InternVideo2); no other value is taken
int check_act(int act) {
  if (act < 0 || act > 3)
    return cc::set_error(CC_ERR_INVALID,
                         "gemm act must be 0 (none), 1 (quick-gelu), 2 "
                         "(tanh-gelu) or 3 (erf-gelu), got %d", act);
  return CC_OK;
}

int gemm_launch(const void* A, int64_t lda, const void* B, void* C, int64_t M,
                int64_t N, int64_t K, const float* bias, int c_dtype, int act,
                const void* residual, int64_t ldr, uint64_t stream) {
  if (!A || !B || !C) return cc::set_error(CC_ERR_INVALID, "bad gemm args");
  if (int rc = check_act(act)) return rc;
  const GemmRunFn run = kGemmRun[act][bias != nullptr][residual != nullptr];
  if (!run)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "gemm act %d is instantiated with a bias and "
                         "without a residual only", act);
  cc_gemm_plan_info plan;
  if (int rc = cc::gemm_plan(M, N, K, lda, ldr, bias != nullptr, act,
                             residual != nullptr, cc::gemm_env_knobs(), &plan))
    return rc;
  const GemmArgs args{(const __bf16*)A, (const __bf16*)B, C, bias,
                      (const __bf16*)residual, (long)M, (long)N, (long)K,
                      (long)lda, (long)ldr, c_dtype == 1 ? 1 : 0,
                      (hipStream_t)stream};
  return cc::timed_launch("gemm_bf16", stream, [&] { run(plan, args); });
}

// cc_gemm_bf16_ln / cc_gemm_bf16_rms: the finalize kernel of the norm,
// then the LN_IN GEMM on the (mean, rstd) pairs it wrote
int gemm_norm_in(bool rms, const void* A, int64_t row_step, const void* stats,
                 void* murstd, const void* Wfold, const float* colsum,
                 const float* cbias, void* C, int64_t M, int64_t N, int64_t K,
                 int act, float eps, uint64_t stream) {
  if (!A || !stats || !murstd || !Wfold || !colsum || !cbias || !C ||
      row_step <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad gemm_ln args");
  if (int rc = check_act(act)) return rc;
  if (!cc::ln_h_supported(K))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "gemm_ln: no LayerNorm statistics at K %lld",
                         (long long)K);
  cc_gemm_plan_info plan;
  if (int rc = cc::gemm_plan(M, N, K, row_step * K, N, true, act, false,
                             cc::gemm_env_knobs(), &plan))
    return rc;
  if (int rc = rms ? cc_rms_finalize(stats, M, K, row_step, eps, murstd, stream)
                   : cc_ln_finalize(stats, M, K, row_step, eps, murstd, stream))
    return rc;
  GemmArgs args{(const __bf16*)A, (const __bf16*)Wfold, C, cbias, nullptr,
                (long)M, (long)N, (long)K, (long)(row_step * K), (long)N, 1,
                (hipStream_t)stream};
  args.colsum = colsum;
  args.murstd = (const float2*)murstd;
  return cc::timed_launch("gemm_bf16", stream, [&] {
    kGemmRunLn[act](plan, args);
  });
}
}  // namespace

extern "C" int cc_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t lda,
                            int64_t ldr, int has_bias, int act,
                            int has_residual, cc_gemm_plan_info* out) {
  if (!out) return cc::set_error(CC_ERR_INVALID, "cc_gemm_plan: null out");
  return cc::gemm_plan(M, N, K, lda, ldr, has_bias != 0, act,
                       has_residual != 0, cc::GemmKnobs{}, out);
}

extern "C" int cc_gemm_bf16_ex(const void* A, const void* B, void* C,
                               int64_t M, int64_t N, int64_t K,
                               const float* bias, int c_dtype, int act,
                               const void* residual, uint64_t stream) {
  return gemm_launch(A, K, B, C, M, N, K, bias, c_dtype, act, residual, N,
                     stream);
}

extern "C" int cc_gemm_bf16_strided(const void* A, int64_t lda, const void* B,
                                    void* C, int64_t M, int64_t N, int64_t K,
                                    const float* bias, int c_dtype, int act,
                                    const void* residual, int64_t ldr,
                                    uint64_t stream) {
  return gemm_launch(A, lda, B, C, M, N, K, bias, c_dtype, act, residual, ldr,
                     stream);
}

extern "C" int cc_gemm_bf16(const void* A, const void* B, void* C, int64_t M,
                            int64_t N, int64_t K, const float* bias,
                            int c_dtype, uint64_t stream) {
  return cc_gemm_bf16_ex(A, B, C, M, N, K, bias, c_dtype, 0, nullptr, stream);
}

extern "C" int cc_gemm_bf16_res_stats(const void* A, const void* B, void* C,
                                      int64_t M, int64_t N, int64_t K,
                                      const float* bias, const void* residual,
                                      void* stats, uint64_t stream) {
  if (!A || !B || !C || !bias || !residual || !stats)
    return cc::set_error(CC_ERR_INVALID, "bad gemm_res_stats args");
  if (!cc::ln_h_supported(N))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "gemm_res_stats: no LayerNorm statistics at N %lld",
                         (long long)N);
  cc_gemm_plan_info plan;
  if (int rc = cc::gemm_plan(M, N, K, K, N, true, 0, true,
                             cc::gemm_env_knobs(), &plan))
    return rc;
  GemmArgs args{(const __bf16*)A, (const __bf16*)B, C, bias,
                (const __bf16*)residual, (long)M, (long)N, (long)K, (long)K,
                (long)N, 1, (hipStream_t)stream};
  if (plan.body == cc::GEMM_T256 && cc::gemm_env_knobs().fuse_stats) {
    args.stats = (float2*)stats;
    return cc::timed_launch("gemm_bf16", stream, [&] {
      gemm_run<0, true, true, false, true>(plan, args);
    });
  }
  if (int rc = cc::timed_launch("gemm_bf16", stream, [&] {
        gemm_run<0, true, true>(plan, args);
      }))
    return rc;
  return cc_ln_stats_bf16(C, M, N, stats, stream);
}

extern "C" int cc_gemm_bf16_ln(const void* A, int64_t row_step,
                               const void* stats, void* murstd,
                               const void* Wfold, const float* colsum,
                               const float* cbias, void* C, int64_t M,
                               int64_t N, int64_t K, int act, float eps,
                               uint64_t stream) {
  return gemm_norm_in(false, A, row_step, stats, murstd, Wfold, colsum, cbias,
                      C, M, N, K, act, eps, stream);
}

extern "C" int cc_gemm_bf16_rms(const void* A, int64_t row_step,
                                const void* stats, void* murstd,
                                const void* Wfold, const float* colsum,
                                const float* cbias, void* C, int64_t M,
                                int64_t N, int64_t K, int act, float eps,
                                uint64_t stream) {
  return gemm_norm_in(true, A, row_step, stats, murstd, Wfold, colsum, cbias,
                      C, M, N, K, act, eps, stream);
}
