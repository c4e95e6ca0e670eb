// Fused multi-head attention for the ViT encoders — three ladder rungs
// by sequence length, all reading Q/K/V straight out of the fused-QKV
// GEMM output ([n*seq, 3*H] rows tokens) and writing O contiguous
// [n*seq, H] (the out-projection GEMM's input layout), replacing
// torch-rocm sdpa (~94 TF/s) + the qkv permute copies.  Which rung a
// sequence length runs, and its grid, is decided by cc::attn_plan
// (cc_attn_plan.hpp) and nowhere else; cc_attn executes that plan:
//   k_attn_small  (ViT-B/32's 50): everything LDS-resident, 2 WG/CU —
//                 see its note on the direct-global variant that
//                 measured slower here;
//   k_attn_mid    (ViT-L/14's 257, SigLIP-L16-256's 256): Q/K fragments
//                 direct from global (16B-contiguous rows), LDS only
//                 V^T + P -> 2 WG/CU at head dim 64, 1 above;
//   k_attn_flash  (SigLIP-384-class; above head dim 64 also most of
//                 65..288, e.g. SigLIP-so400m-224's 256 at head dim 72):
//                 K/V streamed in 64-row tiles with online softmax, O
//                 rescaled flash-style.
// Plus k_attn_cls (any seq, head dim 64): one query row per (frame, head)
// for the last layer of a CLS-pooled tower — separate q, strided K/V,
// O [n, H].
//
// Head dim: each rung is a template on HD, instantiated for every
// multiple of 8 in [64, 128] (so400m 72, ViT-H 80, ViT-g 88, bigG 104,
// ...).  The MFMA shapes pad it: QK^T runs ceil(HD/32) 16x16x32 k-steps,
// PV ceil(HD/16) column fragments.  Nothing past column HD of a head is
// ever read or written; the three rungs are sequences of the shared steps
// below, and the argument is made there, once: every global read goes
// through load_chunk, every global write through store_o, and stage_vt
// ties the two together.  At HD = 64 every pad predicate folds away.
//
// Numerics (all rungs): f32 accumulation and softmax (matches sdpa's
// f32 softmax on bf16 inputs); probabilities round to bf16 before PV,
// covered by sdpa-parity tests at seq 50/100/257/288/576/700/1024 and
// the end-to-end cosine tests.

#include <hip/hip_runtime.h>

#include "cc_attn_plan.hpp"
#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
// The shared steps take their LDS tiles as LDS pointers.  Through a generic
// pointer parameter the tile offsets no longer fold into the ds
// instructions, and k_attn_mid has no registers to spare for them (it
// spilled: +16 B of scratch per lane at head dim 64, 64 B at 128).
typedef __attribute__((address_space(3))) __bf16 lds_bf16;
typedef __attribute__((address_space(3))) bf16x8 lds_bf16x8;

constexpr int SMAX = cc::ATTN_SMALL_MAX;  // padded sequence tile
constexpr int LD = 72;     // LDS row stride (pad 8 elements vs 64 banks)

// What the MFMA shapes make of a head dim.
template <int HD>
struct HeadDim {
  static_assert(cc::attn_hd_supported(HD), "head dim outside the ladder");
  static constexpr int HDK = (HD + 31) / 32 * 32;  // QK^T k extent (k-steps of 32)
  static constexpr int NF = (HD + 15) / 16;        // PV column fragments
  static constexpr int HDV = NF * 16;              // V^T rows held in LDS
  // staging passes: a pass covers 64 head columns, thread t -> row t>>2,
  // columns 64*pass + 16*(t&3) .. +15
  static constexpr int NPASS = (HD + 63) / 64;
};

// ---- the steps the rungs share ----
// A wave owns 16 rows of a 64-row tile.  In the 16x16 MFMA accumulator
// fragments x[n][reg] is (row 4*(lane>>4) + reg, column 16*n + (lane&15))
// of those 16 rows; the operand fragments are (row lane&15, 8 elements at
// 8*(lane>>4) of each k-step of 32).

// The 8 elements at head column d of a Q, K or V row inside the sequence
// (`head_row` points at the head's column 0): loaded if the chunk is inside
// the head, else a zero register — never a load, because what lies past
// column HD is the next head, the next Q/K/V section, the next row or past
// the buffer.  d is a multiple of 8, so with HD % 8 == 0 a chunk lies
// wholly inside or wholly outside [0, HD).  Zero pad chunks on both MFMA
// operands add exactly 0 to every score.  Head offsets are multiples of 16
// bytes for every such HD and the launcher checks the bases, which keeps
// the 16-byte load legal.  Callers test the row once, around all its
// chunks: one test per chunk split small's staging loads into six blocks.
template <int HD>
__device__ __forceinline__ bf16x8 load_chunk(const __bf16* head_row, int d) {
  bf16x8 v = {};
  if (d < HD) v = *(const bf16x8*)(head_row + d);
  return v;
}

// Head columns [d0, d0+16) of one V row (two chunks) into column `col` of
// the transposed image Vt[HDV][LDV].
template <int LDV>
__device__ __forceinline__ void store_vt(lds_bf16* Vt, int d0, int col,
                                         bf16x8 v0, bf16x8 v1) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    Vt[(d0 + e) * LDV + col] = v0[e];
    Vt[(d0 + 8 + e) * LDV + col] = v1[e];
  }
}

// One V row into column `col` of Vt: thread t takes head columns 64*pass +
// 16*(t&3) .. +15 (its row is t>>2, the caller's business).  d0 % 16 == 0,
// so both chunks lie on one side of HDV.  Rows [HD, HDV) of V^T and dead
// rows (not loaded) are written as zeros: row d of V^T feeds only output
// column d, and store_o drops columns >= HD.
template <int HD, int LDV>
__device__ __forceinline__ void stage_vt(lds_bf16* Vt, const __bf16* v_row,
                                         bool live, int col, int tid) {
#pragma unroll
  for (int ps = 0; ps < HeadDim<HD>::NPASS; ps++) {
    const int d0 = 64 * ps + 16 * (tid & 3);
    if (d0 >= HeadDim<HD>::HDV) continue;
    bf16x8 v0 = {}, v1 = {};
    if (live) {
      v0 = load_chunk<HD>(v_row, d0);
      v1 = load_chunk<HD>(v_row, d0 + 8);
    }
    store_vt<LDV>(Vt, d0, col, v0, v1);
  }
}

// S = Q K^T for one wave: query row `qrow`, NFR fragments of key rows from
// k0, both read directly from global (`qkv + head0` is the head's column 0
// of the frame's row 0) and clamped to seq-1 — those are masked in the
// softmax.
template <int HD, int NFR>
__device__ __forceinline__ void qk_global(f32x4 (&acc)[NFR],
                                          const __bf16* qkv, long head0,
                                          int hidden, int qrow, int k0, int seq,
                                          int lane) {
  qrow = qrow < seq ? qrow : seq - 1;
  const int k0e = 8 * (lane >> 4);
#pragma unroll
  for (int kk = 0; kk < HeadDim<HD>::HDK; kk += 32) {
    const bf16x8 qf = load_chunk<HD>(
        qkv + head0 + (long)qrow * 3 * hidden, kk + k0e);
#pragma unroll
    for (int n = 0; n < NFR; n++) {
      int krow = k0 + n * 16 + (lane & 15);
      krow = krow < seq ? krow : seq - 1;
      const bf16x8 kf = load_chunk<HD>(
          qkv + head0 + (long)krow * 3 * hidden + hidden, kk + k0e);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, acc[n], 0, 0, 0);
    }
  }
}

// Row `reg` of NFR score fragments whose column 0 is key `col0 - (lane&15)`:
// scores scaled, then masked at seq, folded into the running max `mx`; acc
// becomes exp(score - mx), 0 where masked; returns the row's sum.
template <int NFR>
__device__ __forceinline__ float row_exp_sum(f32x4 (&acc)[NFR], int reg,
                                             float scale, int col0, int seq,
                                             float& mx) {
#pragma unroll
  for (int nn = 0; nn < NFR; nn++) {
    float s = acc[nn][reg] * scale;
    if (nn * 16 + col0 >= seq) s = -1e30f;
    acc[nn][reg] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  float sum = 0.0f;
#pragma unroll
  for (int nn = 0; nn < NFR; nn++) {
    float e = __expf(acc[nn][reg] - mx);
    if (nn * 16 + col0 >= seq) e = 0.0f;
    acc[nn][reg] = e;
    sum += e;
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off);
  return sum;
}

// Whole-row softmax (the resident rungs): acc becomes the probabilities.
template <int NFR>
__device__ __forceinline__ void softmax_rows(f32x4 (&acc)[NFR], float scale,
                                             int seq, int lane) {
#pragma unroll
  for (int reg = 0; reg < 4; reg++) {
    float mx = -1e30f;
    const float inv = 1.0f / row_exp_sum(acc, reg, scale, lane & 15, seq, mx);
#pragma unroll
    for (int nn = 0; nn < NFR; nn++) acc[nn][reg] = acc[nn][reg] * inv;
  }
}

// Probabilities round to bf16 here, into the wave's rows of P[64][LDP].
template <int NFR, int LDP>
__device__ __forceinline__ void store_p(lds_bf16* P, const f32x4 (&p)[NFR],
                                        int row0, int lane) {
#pragma unroll
  for (int nn = 0; nn < NFR; nn++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++)
      P[(row0 + reg) * LDP + nn * 16 + (lane & 15)] = (__bf16)p[nn][reg];
}

// o += P V for the wave's rows over keys [0, KEXT): P[64][LDP] x Vt[HDV][LDP].
template <int HD, int KEXT, int LDP>
__device__ __forceinline__ void pv_mfma(f32x4 (&o)[HeadDim<HD>::NF],
                                        const lds_bf16* P, const lds_bf16* Vt,
                                        int wid, int lane) {
  const int j0 = 8 * (lane >> 4);
#pragma unroll
  for (int kk = 0; kk < KEXT; kk += 32) {
    const bf16x8 pf =
        *(const lds_bf16x8*)(P + (16 * wid + (lane & 15)) * LDP + kk + j0);
#pragma unroll
    for (int n = 0; n < HeadDim<HD>::NF; n++) {
      const bf16x8 vf =
          *(const lds_bf16x8*)(Vt + (n * 16 + (lane & 15)) * LDP + kk + j0);
      o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o[n], 0, 0, 0);
    }
  }
}

// This lane's four O rows, from row `row0` of the frame, divided by l[reg]
// if DIV.  Rows >= seq and columns >= HD of the last fragment are not
// stored: those columns are the next head's output or past the row end.
template <int HD, bool DIV>
__device__ __forceinline__ void store_o(__bf16* out, long frame, int head,
                                        int hidden, int seq, int row0, int lane,
                                        const f32x4 (&o)[HeadDim<HD>::NF],
                                        const float* l) {
  const int dcol = lane & 15;
#pragma unroll
  for (int nn = 0; nn < HeadDim<HD>::NF; nn++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int row = row0 + reg;
      if (row < seq && (nn * 16 + 16 <= HD || nn * 16 + dcol < HD)) {
        float v = o[nn][reg];
        if constexpr (DIV) v = v / l[reg];
        out[(frame * seq + row) * (long)hidden + head * HD + nn * 16 + dcol] =
            (__bf16)v;
      }
    }
}

// NOTE: the direct-global Q/K variant (4 WG/CU) was tried here too and
// measured SLOWER (89 -> 126 us/launch, profiles/r01_rocprof_b32_afterfusions.txt)
// — at seq=50 the whole K tile L1/LDS-fits and re-reading it from L2
// per wave costs more than the staging saves (guide rule 7); the
// LDS-resident form below stays.  k_attn_mid (seq 257) keeps the
// direct-global form where it measured FASTER (L/14 step 80.3 -> 75.1 ms).
template <int HD>
__global__ __launch_bounds__(256, 2) void k_attn_small(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ out, long n_frames,
    int seq, int heads, int hidden, float scale) {
  using G = HeadDim<HD>;
  constexpr int LDQ = G::HDK + 8;  // Q / K row stride (72 at HD 64)
  // one workgroup per (frame, head)
  const long fh = blockIdx.x;
  const long frame = fh / heads;
  const int head = fh % heads;
  if (frame >= n_frames) return;

  // Q, K [SMAX][LDQ] (columns [HD, HDK) zero), Vt [HDV][LD], P [SMAX][LD]
  __shared__ __bf16 lds[2 * SMAX * LDQ + (G::HDV + SMAX) * LD];
  __bf16* Q = lds;
  __bf16* K = lds + SMAX * LDQ;
  lds_bf16* Vt = (lds_bf16*)lds + 2 * SMAX * LDQ;
  lds_bf16* P = Vt + G::HDV * LD;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;  // 4 waves; wave w owns S rows [16w, 16w+16)
  const int rb = 16 * wid + 4 * (lane >> 4);  // first accumulator row

  // ---- stage Q, K and V^T: thread t -> row t>>2, 16 head columns per
  // pass, as stage_vt (d0 % 16 == 0, so both chunks lie on one side of HDK
  // and of HDV <= HDK).  A pass issues its six loads together, ahead of
  // its LDS stores: taken one by one behind them they cost 18 % at seq 50.
  {
    const int row = tid >> 2;
    const bool live = row < seq;
    const __bf16* src =
        qkv + ((frame * seq + row) * 3) * (long)hidden + (long)head * HD;
#pragma unroll
    for (int ps = 0; ps < G::NPASS; ps++) {
      const int d0 = 64 * ps + 16 * (tid & 3);
      if (d0 >= G::HDK) continue;
      bf16x8 q[2] = {}, k[2] = {}, v[2] = {};
      if (live) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
          q[c] = load_chunk<HD>(src, d0 + 8 * c);
          k[c] = load_chunk<HD>(src + hidden, d0 + 8 * c);
          v[c] = load_chunk<HD>(src + 2 * hidden, d0 + 8 * c);
        }
      }
#pragma unroll
      for (int c = 0; c < 2; c++) {
        *(bf16x8*)(Q + row * LDQ + d0 + 8 * c) = q[c];
        *(bf16x8*)(K + row * LDQ + d0 + 8 * c) = k[c];
      }
      if (d0 < G::HDV) store_vt<LD>(Vt, d0, row, v[0], v[1]);
    }
  }
  __syncthreads();

  // ---- S = Q K^T, rows [16w,16w+16), cols 0..63 ----
  f32x4 acc[SMAX / 16] = {};
  {
    const int qrow = 16 * wid + (lane & 15);
    const int k0e = 8 * (lane >> 4);
#pragma unroll
    for (int kk = 0; kk < G::HDK; kk += 32) {
      bf16x8 qf = *(const bf16x8*)(Q + qrow * LDQ + kk + k0e);
#pragma unroll
      for (int n = 0; n < SMAX / 16; n++) {
        bf16x8 kf = *(const bf16x8*)(K + (n * 16 + (lane & 15)) * LDQ + kk + k0e);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, acc[n], 0, 0, 0);
      }
    }
  }
  softmax_rows(acc, scale, seq, lane);
  store_p<SMAX / 16, LD>(P, acc, rb, lane);
  __syncthreads();

  f32x4 oacc[G::NF] = {};
  pv_mfma<HD, SMAX, LD>(oacc, P, Vt, wid, lane);
  store_o<HD, false>(out, frame, head, hidden, seq, rb, lane, oacc, nullptr);
}


// ---- mid-sequence variant: ViT-L/14's seq=257 ----
// One workgroup per (frame, head), Q in 64-row tiles.  Q and K
// fragments are 16-byte contiguous in the fused-QKV layout, so they
// load STRAIGHT from global/L2 (no LDS staging) — only V^T (transposed
// image for the PV matmul) and P live in LDS: 74 KB -> 2 WG/CU, which
// doubles the waves/SIMD vs the LDS-everything form (measured 621 us
// -> see profiles/r01_attn_mid2; the LDS-everything form capped at
// ~204 TF with 1 wave/SIMD).  Above head dim 64 the V^T image grows
// past half the CU's LDS and one workgroup per CU runs; the plan then
// keeps this rung only where it still measured faster than flash
// (cc_attn_plan.hpp has the numbers).
constexpr int SMID = cc::ATTN_MID_MAX;  // padded sequence (18 x 16-col frags)
constexpr int LDM = SMID + 8;   // LDS s-stride for Vt / P rows

template <int HD>
__global__ __launch_bounds__(256, 2) void k_attn_mid(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ out, long n_frames,
    int seq, int heads, int hidden, float scale) {
  using G = HeadDim<HD>;
  const long fh = blockIdx.x;
  const long frame = fh / heads;
  const int head = fh % heads;
  if (frame >= n_frames) return;

  __shared__ __bf16 lds[(G::HDV + 64) * LDM];
  lds_bf16* Vt = (lds_bf16*)lds;     // [HDV][LDM] rows d, cols s
  lds_bf16* P = Vt + G::HDV * LDM;   // [64][LDM] rows q, cols s

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int rb = 16 * wid + 4 * (lane >> 4);  // first accumulator row
  const long qkv_base = (frame * (long)seq * 3) * hidden + (long)head * HD;

  // ---- V^T: all SMID rows, 64 per step, thread t -> row t>>2
#pragma unroll
  for (int j = 0; j < SMID / 64 + 1; j++) {
    const int r = j * 64 + (tid >> 2);
    if (r >= SMID) break;
    stage_vt<HD, LDM>(Vt, qkv + qkv_base + (long)r * 3 * hidden + 2 * hidden,
                      r < seq, r, tid);
  }

  const int n_qtiles = (seq + 63) / 64;
  for (int qt = 0; qt < n_qtiles; qt++) {
    const int q0 = qt * 64;
    __syncthreads();  // Vt ready (first iter); P free (later iters)

    f32x4 acc[SMID / 16];
#pragma unroll
    for (int n = 0; n < SMID / 16; n++) acc[n] = f32x4{};
    qk_global<HD>(acc, qkv, qkv_base, hidden, q0 + 16 * wid + (lane & 15), 0,
                  seq, lane);
    softmax_rows(acc, scale, seq, lane);
    store_p<SMID / 16, LDM>(P, acc, rb, lane);
    __syncthreads();

    f32x4 oacc[G::NF] = {};
    pv_mfma<HD, SMID, LDM>(oacc, P, Vt, wid, lane);
    store_o<HD, false>(out, frame, head, hidden, seq, q0 + rb, lane, oacc,
                       nullptr);
  }
}


// ---- flash variant (past the mid rung): K/V streamed in 64-row tiles
// with online softmax ----
// One workgroup per (frame, head, q-tile of 64 rows); Q and K fragments
// load straight from global (16B-contiguous in the fused-QKV layout,
// same trick as k_attn_mid); per KV-tile, V^T and the probability tile
// stage through a small LDS image (~19 KB at head dim 64, ~28 KB at 128
// -> high occupancy).  f32
// running max/sum per row, O accumulators rescaled flash-style,
// probabilities rounded to bf16 before PV (same numerics contract as
// the resident kernels).
constexpr int FKV = 64;        // kv tile rows
constexpr int LDF = FKV + 8;   // LDS s-stride

template <int HD>
__global__ __launch_bounds__(256, 2) void k_attn_flash(
    const __bf16* __restrict__ qkv, __bf16* __restrict__ out, long n_frames,
    int seq, int heads, int hidden, float scale) {
  using G = HeadDim<HD>;
  const int n_qtiles = (seq + 63) / 64;
  const long fhq = blockIdx.x;
  const int qt = (int)(fhq % n_qtiles);
  const long fh = fhq / n_qtiles;
  const long frame = fh / heads;
  const int head = fh % heads;
  if (frame >= n_frames) return;

  __shared__ __bf16 lds[(G::HDV + 64) * LDF];
  lds_bf16* Vt = (lds_bf16*)lds;     // [HDV d][LDF s]
  lds_bf16* P = Vt + G::HDV * LDF;   // [64 q][LDF s]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int rb = 16 * wid + 4 * (lane >> 4);  // first accumulator row
  const long qkv_base = (frame * (long)seq * 3) * hidden + (long)head * HD;
  const int q0 = qt * 64;

  // per-lane row state (rows 4*(lane>>4) + reg of this wave's 16)
  float m_run[4], l_run[4];
  f32x4 oacc[G::NF] = {};
#pragma unroll
  for (int r = 0; r < 4; r++) {
    m_run[r] = -1e30f;
    l_run[r] = 0.0f;
  }

  const int n_kv = (seq + FKV - 1) / FKV;
  for (int kt = 0; kt < n_kv; kt++) {
    const int k0 = kt * FKV;
    __syncthreads();  // P/Vt free from the previous tile
    // ---- V^T tile: thread t -> row k0 + (t>>2)
    {
      const int r = k0 + (tid >> 2);
      stage_vt<HD, LDF>(Vt, qkv + qkv_base + (long)r * 3 * hidden + 2 * hidden,
                        r < seq, tid >> 2, tid);
    }

    f32x4 acc[FKV / 16] = {};
    qk_global<HD>(acc, qkv, qkv_base, hidden, q0 + 16 * wid + (lane & 15), k0,
                  seq, lane);

    // ---- online softmax update (per row); acc: unnormalized probabilities
    float alpha[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      float mx = m_run[reg];
      const float sum =
          row_exp_sum(acc, reg, scale, k0 + (lane & 15), seq, mx);
      alpha[reg] = __expf(m_run[reg] - mx);
      l_run[reg] = l_run[reg] * alpha[reg] + sum;
      m_run[reg] = mx;
    }
    store_p<FKV / 16, LDF>(P, acc, rb, lane);
    __syncthreads();

    // ---- O = alpha * O + P V
    f32x4 pv[G::NF] = {};
    pv_mfma<HD, FKV, LDF>(pv, P, Vt, wid, lane);
#pragma unroll
    for (int n = 0; n < G::NF; n++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++)
        oacc[n][reg] = oacc[n][reg] * alpha[reg] + pv[n][reg];
  }

  store_o<HD, true>(out, frame, head, hidden, seq, q0 + rb, lane, oacc, l_run);
}

// ---- CLS-query variant: one query row per (frame, head) ----
// The last encoder layer of a CLS-pooled tower needs attention only for
// token 0 of each frame (post-LN and the projection read nothing else),
// but every token still serves as a key and a value.  With one query row
// MFMA buys nothing; the kernel is a bandwidth pass over K and V, read
// in place from the K/V GEMM output through a common row stride.
//
// One wave per (frame, head), four waves per workgroup, no LDS and no
// barriers.  Keys stream in 64-row chunks; lane (jg = lane>>3, dg =
// lane&7) owns keys j = 8*jj + jg (jj = 0..7) and the 8 dims
// [8*dg, 8*dg+8): every load instruction fetches eight full 128-byte
// K (or V) rows, 16 bytes per lane.  q.K partial dots reduce across the
// 8 dg lanes; the score of key 8*jj+jg then already sits in the lanes
// that multiply it into V, so P.V needs no exchange.  Online softmax
// across chunks exactly as k_attn_flash (f32 running max/sum,
// unnormalized probabilities rounded to bf16 before PV, O / l at the
// end); the cross-lane reductions run in a fixed order, no atomics ->
// bit-identical from run to run.
constexpr int CLS_HD = cc::ATTN_CLS_HD;

__global__ __launch_bounds__(256) void k_attn_cls(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k,
    const __bf16* __restrict__ v, long ldkv, __bf16* __restrict__ out,
    long n_frames, int seq, int heads, int hidden, float scale) {
  const int lane = threadIdx.x & 63;
  const long fh = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (fh >= n_frames * heads) return;  // whole wave; no barriers below
  const long frame = fh / heads;
  const int head = (int)(fh % heads);
  const int jg = lane >> 3;
  const int dg = lane & 7;

  float qf[8];
  {
    const bf16x8 q8 =
        *(const bf16x8*)(q + frame * (long)hidden + head * CLS_HD + dg * 8);
#pragma unroll
    for (int e = 0; e < 8; e++) qf[e] = (float)q8[e] * scale;
  }
  const long kv_base = frame * (long)seq * ldkv + (long)head * CLS_HD + dg * 8;

  float m_run = -1e30f, l_run = 0.0f;
  float oacc[8] = {};
  for (int k0 = 0; k0 < seq; k0 += 64) {
    // all 16 row loads of the chunk up front (V does not wait for the
    // softmax); rows past seq clamp to seq-1 and are masked below
    bf16x8 kr[8], vr[8];
#pragma unroll
    for (int jj = 0; jj < 8; jj++) {
      int j = k0 + jj * 8 + jg;
      j = j < seq ? j : seq - 1;
      kr[jj] = *(const bf16x8*)(k + kv_base + (long)j * ldkv);
      vr[jj] = *(const bf16x8*)(v + kv_base + (long)j * ldkv);
    }
    float s[8];
    float mx = m_run;
#pragma unroll
    for (int jj = 0; jj < 8; jj++) {
      float d = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; e++) d += qf[e] * (float)kr[jj][e];
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      if (k0 + jj * 8 + jg >= seq) d = -1e30f;
      s[jj] = d;
      mx = fmaxf(mx, d);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float alpha = __expf(m_run - mx);
    float sum = 0.0f;
    float pv[8] = {};
#pragma unroll
    for (int jj = 0; jj < 8; jj++) {
      const bool live = k0 + jj * 8 + jg < seq;
      const float e = live ? __expf(s[jj] - mx) : 0.0f;
      sum += e;
      const float p = (float)(__bf16)e;  // bf16 probabilities before PV
#pragma unroll
      for (int d = 0; d < 8; d++)
        pv[d] += live ? p * (float)vr[jj][d] : 0.0f;
    }
    sum += __shfl_xor(sum, 8);
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    l_run = l_run * alpha + sum;
    m_run = mx;
#pragma unroll
    for (int d = 0; d < 8; d++) oacc[d] = oacc[d] * alpha + pv[d];
  }
  // fold the 8 key groups (fixed order), normalize, one 16-byte store
  // per dim group
#pragma unroll
  for (int d = 0; d < 8; d++) {
    float o = oacc[d];
    o += __shfl_xor(o, 8);
    o += __shfl_xor(o, 16);
    o += __shfl_xor(o, 32);
    oacc[d] = o;
  }
  if (jg == 0) {
    const float inv = 1.0f / l_run;
    bf16x8 o8;
#pragma unroll
    for (int d = 0; d < 8; d++) o8[d] = (__bf16)(oacc[d] * inv);
    *(bf16x8*)(out + frame * (long)hidden + head * CLS_HD + dg * 8) = o8;
  }
}

}  // namespace

extern "C" int cc_attn_cls(const void* q, const void* k, const void* v,
                           int64_t ldkv, void* out, int64_t n_frames, int seq,
                           int heads, int hidden, float scale,
                           uint64_t stream) {
  if (!q || !k || !v || !out || n_frames <= 0 || seq <= 0 || heads <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad attn_cls args");
  if (hidden != heads * CLS_HD)
    return cc::set_error(CC_ERR_UNSUPPORTED, "cc_attn_cls needs hd == 64");
  // 16-byte row loads: stride and bases must keep every row 16B-aligned
  if (ldkv < hidden || ldkv % 8 != 0 || ((uintptr_t)q & 15) ||
      ((uintptr_t)k & 15) || ((uintptr_t)v & 15) || ((uintptr_t)out & 15))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_cls needs ldkv >= hidden, ldkv %% 8 == 0 "
                         "and 16-byte aligned q/k/v/out");
  const int64_t nwave = n_frames * heads;
  if ((nwave + 3) / 4 > 0x7fffffffLL)
    return cc::set_error(CC_ERR_INVALID, "attn_cls grid too large");
  dim3 block(256), grid((unsigned)((nwave + 3) / 4));
  return cc::timed_launch("attn_cls", stream, [&] {
    hipLaunchKernelGGL(k_attn_cls, grid, block, 0, (hipStream_t)stream,
                       (const __bf16*)q, (const __bf16*)k, (const __bf16*)v,
                       (long)ldkv, (__bf16*)out, (long)n_frames, seq, heads,
                       hidden, scale);
  });
}

namespace {

using AttnKernel = void (*)(const __bf16*, __bf16*, long, int, int, int,
                            float);
// timing names, indexed by cc_attn_plan_info.rung
constexpr const char* kAttnLabels[3] = {"attn_small", "attn_mid",
                                        "attn_flash"};
// the head dims cc::attn_hd_supported accepts, in order
#define CC_ATTN_HDS(X) X(64) X(72) X(80) X(88) X(96) X(104) X(112) X(120) X(128)
// [(hd - ATTN_HD_MIN) / ATTN_HD_STEP][rung]
constexpr AttnKernel kAttnKernels[][3] = {
#define ROW(H) {k_attn_small<H>, k_attn_mid<H>, k_attn_flash<H>},
    CC_ATTN_HDS(ROW)
#undef ROW
};
static_assert(sizeof(kAttnKernels) / sizeof(kAttnKernels[0]) ==
                  (cc::ATTN_HD_MAX - cc::ATTN_HD_MIN) / cc::ATTN_HD_STEP + 1,
              "one kernel row per supported head dim");

// The one launcher: runs what cc::attn_plan says.  `only` >= 0 (the rung
// entries) additionally requires the plan to land on that rung; `force`
// >= 0 (cc_attn_rung) makes the plan take that rung.
int attn_launch(int only, int force, const void* qkv, void* out,
                int64_t n_frames, int seq, int heads, int hidden, float scale,
                uint64_t stream) {
  if (!qkv || !out) return cc::set_error(CC_ERR_INVALID, "bad attn args");
  // 16-byte row loads: rows and head offsets are 16B multiples at
  // hd % 8 == 0, bases must be too
  if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn needs 16-byte aligned qkv/out");
  cc_attn_plan_info plan;
  if (int rc = cc::attn_plan(n_frames, seq, heads, hidden, &plan, force))
    return rc;
  if (only >= 0 && only != plan.rung)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "cc_%s does not cover seq %d, which runs %s (cc_attn "
                         "picks the rung)",
                         kAttnLabels[only], seq, kAttnLabels[plan.rung]);
  const AttnKernel kernel =
      kAttnKernels[(hidden / heads - cc::ATTN_HD_MIN) / cc::ATTN_HD_STEP]
                  [plan.rung];
  return cc::timed_launch(kAttnLabels[plan.rung], stream, [&] {
    hipLaunchKernelGGL(kernel, dim3(plan.grid), dim3(plan.block), 0,
                       (hipStream_t)stream, (const __bf16*)qkv, (__bf16*)out,
                       (long)n_frames, seq, heads, hidden, scale);
  });
}

}  // namespace

extern "C" int cc_attn_plan(int64_t n_frames, int seq, int heads, int hidden,
                            cc_attn_plan_info* out) {
  if (!out) return cc::set_error(CC_ERR_INVALID, "cc_attn_plan: null out");
  return cc::attn_plan(n_frames, seq, heads, hidden, out);
}

extern "C" int cc_attn(const void* qkv, void* out, int64_t n_frames, int seq,
                       int heads, int hidden, float scale, uint64_t stream) {
  return attn_launch(-1, -1, qkv, out, n_frames, seq, heads, hidden, scale,
                     stream);
}

extern "C" int cc_attn_small(const void* qkv, void* out, int64_t n_frames,
                             int seq, int heads, int hidden, float scale,
                             uint64_t stream) {
  return attn_launch(CC_ATTN_SMALL, -1, qkv, out, n_frames, seq, heads, hidden,
                     scale, stream);
}

extern "C" int cc_attn_mid(const void* qkv, void* out, int64_t n_frames,
                           int seq, int heads, int hidden, float scale,
                           uint64_t stream) {
  return attn_launch(CC_ATTN_MID, -1, qkv, out, n_frames, seq, heads, hidden,
                     scale, stream);
}

extern "C" int cc_attn_flash(const void* qkv, void* out, int64_t n_frames,
                             int seq, int heads, int hidden, float scale,
                             uint64_t stream) {
  return attn_launch(CC_ATTN_FLASH, -1, qkv, out, n_frames, seq, heads, hidden,
                     scale, stream);
}

extern "C" int cc_attn_rung(int rung, const void* qkv, void* out,
                            int64_t n_frames, int seq, int heads, int hidden,
                            float scale, uint64_t stream) {
  if (rung < CC_ATTN_SMALL || rung > CC_ATTN_FLASH)
    return cc::set_error(CC_ERR_INVALID, "cc_attn_rung: no rung %d", rung);
  return attn_launch(-1, rung, qkv, out, n_frames, seq, heads, hidden, scale,
                     stream);
}
