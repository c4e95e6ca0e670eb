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
// ever read or written — those addresses are the next head, the next
// Q/K/V section, the next row or past the buffer:
//   - a fragment chunk is 8 elements at a multiple of 8, so with
//     HD % 8 == 0 it lies wholly inside or wholly outside [0, HD); an
//     outside chunk is a zero register (both operands, so the pad
//     contributes exactly 0 to every score), never a load;
//   - V^T rows >= HD are written as zeros; they feed only output columns
//     >= HD, which are never stored.
// Head offsets are multiples of 16 bytes for every such HD, which keeps
// the bf16x8 loads legal.  At HD = 64 every pad predicate folds away.
//
// Numerics (all rungs): f32 accumulation and softmax (matches sdpa's
// f32 softmax on bf16 inputs); probabilities round to bf16 before PV,
// covered by sdpa-parity tests at seq 50/100/257/288/576/700/1024 and
// the end-to-end cosine tests.

#include <hip/hip_runtime.h>

#include <vector>

#include "cc_attn_plan.hpp"
#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

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
  __bf16* Vt = lds + 2 * SMAX * LDQ;
  __bf16* P = Vt + G::HDV * LD;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;  // 4 waves; wave w owns S rows [16w, 16w+16)

  // ---- load Q/K/V tiles: thread t handles row t>>2, cols (t&3)*16.. ----
  {
    const int row = tid >> 2;
    const int d0 = (tid & 3) * 16;
    const long base = ((frame * seq + row) * 3) * (long)hidden + (long)head * HD;
    bf16x8 z = {};
    bf16x8 q0 = z, q1 = z, k0 = z, k1 = z, v0 = z, v1 = z;
    if (row < seq) {
      q0 = *(const bf16x8*)(qkv + base + d0);
      q1 = *(const bf16x8*)(qkv + base + d0 + 8);
      k0 = *(const bf16x8*)(qkv + base + hidden + d0);
      k1 = *(const bf16x8*)(qkv + base + hidden + d0 + 8);
      v0 = *(const bf16x8*)(qkv + base + 2 * hidden + d0);
      v1 = *(const bf16x8*)(qkv + base + 2 * hidden + d0 + 8);
    }
    *(bf16x8*)(Q + row * LDQ + d0) = q0;
    *(bf16x8*)(Q + row * LDQ + d0 + 8) = q1;
    *(bf16x8*)(K + row * LDQ + d0) = k0;
    *(bf16x8*)(K + row * LDQ + d0 + 8) = k1;
    // V transposed: Vt[d][row] = V[row][d]
#pragma unroll
    for (int e = 0; e < 8; e++) {
      Vt[(d0 + e) * LD + row] = v0[e];
      Vt[(d0 + 8 + e) * LD + row] = v1[e];
    }
  }
  // ---- head dims above 64: columns 64 + (t&3)*16.. of the same row.  A
  // chunk inside the head is loaded, one outside stays zero; d0 % 16 == 0,
  // so both chunks lie on one side of HDK (Q/K extent) and of HDV (Vt
  // rows) ----
  if constexpr (HD > 64) {
    const int row = tid >> 2;
    const int d0 = 64 + (tid & 3) * 16;
    const long base = ((frame * seq + row) * 3) * (long)hidden + (long)head * HD;
    bf16x8 z = {};
    bf16x8 q0 = z, q1 = z, k0 = z, k1 = z, v0 = z, v1 = z;
    if (row < seq && d0 < HD) {
      q0 = *(const bf16x8*)(qkv + base + d0);
      k0 = *(const bf16x8*)(qkv + base + hidden + d0);
      v0 = *(const bf16x8*)(qkv + base + 2 * hidden + d0);
    }
    if (row < seq && d0 + 8 < HD) {
      q1 = *(const bf16x8*)(qkv + base + d0 + 8);
      k1 = *(const bf16x8*)(qkv + base + hidden + d0 + 8);
      v1 = *(const bf16x8*)(qkv + base + 2 * hidden + d0 + 8);
    }
    if (d0 < G::HDK) {
      *(bf16x8*)(Q + row * LDQ + d0) = q0;
      *(bf16x8*)(Q + row * LDQ + d0 + 8) = q1;
      *(bf16x8*)(K + row * LDQ + d0) = k0;
      *(bf16x8*)(K + row * LDQ + d0 + 8) = k1;
    }
    if (d0 < G::HDV) {
#pragma unroll
      for (int e = 0; e < 8; e++) {
        Vt[(d0 + e) * LD + row] = v0[e];
        Vt[(d0 + 8 + e) * LD + row] = v1[e];
      }
    }
  }
  __syncthreads();

  // ---- S = Q K^T * scale, rows [16w,16w+16), cols 0..63 ----
  f32x4 acc[4] = {};
  {
    const int qrow = 16 * wid + (lane & 15);
    const int k0e = 8 * (lane >> 4);
#pragma unroll
    for (int kk = 0; kk < G::HDK; kk += 32) {
      bf16x8 qf = *(const bf16x8*)(Q + qrow * LDQ + kk + k0e);
#pragma unroll
      for (int n = 0; n < 4; n++) {
        bf16x8 kf = *(const bf16x8*)(K + (n * 16 + (lane & 15)) * LDQ + kk + k0e);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, acc[n], 0, 0, 0);
      }
    }
  }

  // ---- masked, scaled softmax over cols (per row) ----
  // acc value (row = 16w + (lane>>4)*4 + reg, col = n*16 + lane&15)
  float pr[4][4];  // probabilities, same layout
  {
    const int colr = lane & 15;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      float mx = -1e30f;
      float sv[4];
#pragma unroll
      for (int nn = 0; nn < 4; nn++) {
        float s = acc[nn][reg] * scale;
        if (nn * 16 + colr >= seq) s = -1e30f;
        sv[nn] = s;
        mx = fmaxf(mx, s);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        mx = fmaxf(mx, __shfl_xor(mx, off));
      float sum = 0.0f;
#pragma unroll
      for (int nn = 0; nn < 4; nn++) {
        float e = __expf(sv[nn] - mx);
        if (nn * 16 + colr >= seq) e = 0.0f;
        sv[nn] = e;
        sum += e;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int nn = 0; nn < 4; nn++) pr[nn][reg] = sv[nn] * inv;
    }
  }
  // write P (bf16) to LDS for the PV matmul
  {
    const int colr = lane & 15;
    const int rbase = 16 * wid + 4 * (lane >> 4);
#pragma unroll
    for (int nn = 0; nn < 4; nn++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++)
        P[(rbase + reg) * LD + nn * 16 + colr] = (__bf16)pr[nn][reg];
  }
  __syncthreads();

  // ---- O = P Vt^T : rows [16w,16w+16) of O, cols d = 0..HDV-1 ----
  f32x4 oacc[G::NF] = {};
  {
    const int prow = 16 * wid + (lane & 15);
    const int j0 = 8 * (lane >> 4);
#pragma unroll
    for (int kk = 0; kk < SMAX; kk += 32) {
      bf16x8 pf = *(const bf16x8*)(P + prow * LD + kk + j0);
#pragma unroll
      for (int n = 0; n < G::NF; n++) {
        bf16x8 vf = *(const bf16x8*)(Vt + (n * 16 + (lane & 15)) * LD + kk + j0);
        oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, oacc[n], 0, 0, 0);
      }
    }
  }
  // ---- store O: (row = 16w + (lane>>4)*4 + reg, d = n*16 + lane&15);
  // columns >= HD of the last fragment belong to the next head ----
  {
    const int dcol = lane & 15;
    const int rbase = 16 * wid + 4 * (lane >> 4);
#pragma unroll
    for (int nn = 0; nn < G::NF; nn++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int row = rbase + reg;
        if (row < seq && (nn * 16 + 16 <= HD || nn * 16 + dcol < HD))
          out[(frame * seq + row) * (long)hidden + head * HD + nn * 16 + dcol] =
              (__bf16)oacc[nn][reg];
      }
  }
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
  __bf16* Vt = lds;                  // [HDV][LDM] rows d, cols s
  __bf16* P = lds + G::HDV * LDM;    // [64][LDM] rows q, cols s

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const long qkv_base = (frame * (long)seq * 3) * hidden + (long)head * HD;

  // ---- V^T load: 64 rows per pass, thread t -> row t>>2, d (t&3)*16
  {
    const int row = tid >> 2;
    const int d0 = (tid & 3) * 16;
#pragma unroll
    for (int j = 0; j < SMID / 64 + 1; j++) {
      const int r = j * 64 + row;
      if (r >= SMID) break;
      bf16x8 z = {};
      bf16x8 v0 = z, v1 = z;
      if (r < seq) {
        const long base = qkv_base + (long)r * 3 * hidden + 2 * hidden;
        v0 = *(const bf16x8*)(qkv + base + d0);
        v1 = *(const bf16x8*)(qkv + base + d0 + 8);
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        Vt[(d0 + e) * LDM + r] = v0[e];
        Vt[(d0 + 8 + e) * LDM + r] = v1[e];
      }
    }
  }
  // ---- head dims above 64: d 64 + (t&3)*16.. of the same rows; chunks
  // past HD are zero rows of V^T, rows past HDV are not held
  if constexpr (HD > 64) {
    const int row = tid >> 2;
    const int d0 = 64 + (tid & 3) * 16;
    if (d0 < G::HDV) {
#pragma unroll
      for (int j = 0; j < SMID / 64 + 1; j++) {
        const int r = j * 64 + row;
        if (r >= SMID) break;
        bf16x8 z = {};
        bf16x8 v0 = z, v1 = z;
        if (r < seq) {
          const long base = qkv_base + (long)r * 3 * hidden + 2 * hidden;
          if (d0 < HD) v0 = *(const bf16x8*)(qkv + base + d0);
          if (d0 + 8 < HD) v1 = *(const bf16x8*)(qkv + base + d0 + 8);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
          Vt[(d0 + e) * LDM + r] = v0[e];
          Vt[(d0 + 8 + e) * LDM + r] = v1[e];
        }
      }
    }
  }

  const int n_qtiles = (seq + 63) / 64;
  for (int qt = 0; qt < n_qtiles; qt++) {
    const int q0 = qt * 64;
    __syncthreads();  // Vt ready (first iter); P free (later iters)

    // ---- S = Q K^T: wave rows [16*wid, +16), 18 col frags; Q/K frags
    // read directly from global (16B contiguous), rows clamped to seq-1
    // (masked in softmax anyway); chunks past HD are zero, not loaded.
    f32x4 acc[SMID / 16];
#pragma unroll
    for (int n = 0; n < SMID / 16; n++) acc[n] = f32x4{};
    {
      int qrow = q0 + 16 * wid + (lane & 15);
      qrow = qrow < seq ? qrow : seq - 1;
      const int k0e = 8 * (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < G::HDK; kk += 32) {
        const bool in = kk + 32 <= HD || kk + k0e < HD;
        bf16x8 qf = {};
        if (in)
          qf = *(const bf16x8*)(qkv + qkv_base + (long)qrow * 3 * hidden + kk +
                                k0e);
#pragma unroll
        for (int n = 0; n < SMID / 16; n++) {
          int krow = n * 16 + (lane & 15);
          krow = krow < seq ? krow : seq - 1;
          bf16x8 kf = {};
          if (in)
            kf = *(const bf16x8*)(qkv + qkv_base + (long)krow * 3 * hidden +
                                  hidden + kk + k0e);
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, acc[n], 0, 0, 0);
        }
      }
    }

    // ---- softmax per row (cols masked at seq)
    {
      const int colr = lane & 15;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        float mx = -1e30f;
        float sv[SMID / 16];
#pragma unroll
        for (int nn = 0; nn < SMID / 16; nn++) {
          float sc = acc[nn][reg] * scale;
          if (nn * 16 + colr >= seq) sc = -1e30f;
          sv[nn] = sc;
          mx = fmaxf(mx, sc);
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          mx = fmaxf(mx, __shfl_xor(mx, off));
        float sum = 0.0f;
#pragma unroll
        for (int nn = 0; nn < SMID / 16; nn++) {
          float e = __expf(sv[nn] - mx);
          if (nn * 16 + colr >= seq) e = 0.0f;
          sv[nn] = e;
          sum += e;
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int nn = 0; nn < SMID / 16; nn++) acc[nn][reg] = sv[nn] * inv;
      }
    }
    // ---- P to LDS (bf16)
    {
      const int colr = lane & 15;
      const int rbase = 16 * wid + 4 * (lane >> 4);
#pragma unroll
      for (int nn = 0; nn < SMID / 16; nn++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
          P[(rbase + reg) * LDM + nn * 16 + colr] = (__bf16)acc[nn][reg];
    }
    __syncthreads();

    // ---- O = P V : rows [16*wid,+16), d cols 0..HDV-1
    f32x4 oacc[G::NF] = {};
    {
      const int prow = 16 * wid + (lane & 15);
      const int j0 = 8 * (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < SMID; kk += 32) {
        bf16x8 pf = *(const bf16x8*)(P + prow * LDM + kk + j0);
#pragma unroll
        for (int n = 0; n < G::NF; n++) {
          bf16x8 vf =
              *(const bf16x8*)(Vt + (n * 16 + (lane & 15)) * LDM + kk + j0);
          oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, oacc[n], 0, 0, 0);
        }
      }
    }
    {
      const int dcol = lane & 15;
      const int rbase = 16 * wid + 4 * (lane >> 4);
#pragma unroll
      for (int nn = 0; nn < G::NF; nn++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int row = q0 + rbase + reg;
          if (row < seq && (nn * 16 + 16 <= HD || nn * 16 + dcol < HD))
            out[(frame * seq + row) * (long)hidden + head * HD + nn * 16 +
                dcol] = (__bf16)oacc[nn][reg];
        }
    }
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
  __bf16* Vt = lds;                  // [HDV d][LDF s]
  __bf16* P = lds + G::HDV * LDF;    // [64 q][LDF s]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const long qkv_base = (frame * (long)seq * 3) * hidden + (long)head * HD;
  const int q0 = qt * 64;

  // per-lane row state (rows rbase..rbase+3 of this wave's 16)
  const int rbase_l = 4 * (lane >> 4);
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
    // ---- V^T tile into LDS (thread t -> row t>>2, d (t&3)*16, +64 per
    // head-dim pass; chunks past HD are zero rows of V^T)
    __syncthreads();  // P/Vt free from the previous tile
#pragma unroll
    for (int ps = 0; ps < G::NPASS; ps++) {
      const int row = tid >> 2;
      const int d0 = (tid & 3) * 16 + 64 * ps;
      if (d0 >= G::HDV) continue;
      const bool in0 = d0 < HD, in1 = d0 + 8 < HD;
      bf16x8 z = {};
      bf16x8 v0 = z, v1 = z;
      if (k0 + row < seq) {
        const long base = qkv_base + (long)(k0 + row) * 3 * hidden + 2 * hidden;
        if (in0) v0 = *(const bf16x8*)(qkv + base + d0);
        if (in1) v1 = *(const bf16x8*)(qkv + base + d0 + 8);
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        Vt[(d0 + e) * LDF + row] = v0[e];
        Vt[(d0 + 8 + e) * LDF + row] = v1[e];
      }
    }

    // ---- S tile = Q K^T (wave rows, 4 col frags), direct global Q/K;
    // chunks past HD are zero, not loaded
    f32x4 acc[4] = {};
    {
      int qrow = q0 + 16 * wid + (lane & 15);
      qrow = qrow < seq ? qrow : seq - 1;
      const int k0e = 8 * (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < G::HDK; kk += 32) {
        const bool in = kk + 32 <= HD || kk + k0e < HD;
        bf16x8 qf = {};
        if (in)
          qf = *(const bf16x8*)(qkv + qkv_base + (long)qrow * 3 * hidden + kk +
                                k0e);
#pragma unroll
        for (int n = 0; n < 4; n++) {
          int krow = k0 + n * 16 + (lane & 15);
          krow = krow < seq ? krow : seq - 1;
          bf16x8 kf = {};
          if (in)
            kf = *(const bf16x8*)(qkv + qkv_base + (long)krow * 3 * hidden +
                                  hidden + kk + k0e);
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, acc[n], 0, 0, 0);
        }
      }
    }

    // ---- online softmax update (per row)
    float alpha[4];
    {
      const int colr = lane & 15;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        float mx = m_run[reg];
        float sv[4];
#pragma unroll
        for (int nn = 0; nn < 4; nn++) {
          float sc = acc[nn][reg] * scale;
          if (k0 + nn * 16 + colr >= seq) sc = -1e30f;
          sv[nn] = sc;
          mx = fmaxf(mx, sc);
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          mx = fmaxf(mx, __shfl_xor(mx, off));
        alpha[reg] = __expf(m_run[reg] - mx);
        float sum = 0.0f;
#pragma unroll
        for (int nn = 0; nn < 4; nn++) {
          float e = __expf(sv[nn] - mx);
          if (k0 + nn * 16 + colr >= seq) e = 0.0f;
          sv[nn] = e;
          sum += e;
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off);
        l_run[reg] = l_run[reg] * alpha[reg] + sum;
        m_run[reg] = mx;
#pragma unroll
        for (int nn = 0; nn < 4; nn++) acc[nn][reg] = sv[nn];
      }
    }
    // ---- P tile to LDS (unnormalized probabilities, bf16)
    {
      const int colr = lane & 15;
      const int rb = 16 * wid + rbase_l;
#pragma unroll
      for (int nn = 0; nn < 4; nn++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
          P[(rb + reg) * LDF + nn * 16 + colr] = (__bf16)acc[nn][reg];
    }
    __syncthreads();

    // ---- O = alpha * O + P V
    f32x4 pv[G::NF] = {};
    {
      const int prow = 16 * wid + (lane & 15);
      const int j0 = 8 * (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < FKV; kk += 32) {
        bf16x8 pf = *(const bf16x8*)(P + prow * LDF + kk + j0);
#pragma unroll
        for (int n = 0; n < G::NF; n++) {
          bf16x8 vf =
              *(const bf16x8*)(Vt + (n * 16 + (lane & 15)) * LDF + kk + j0);
          pv[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, pv[n], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int n = 0; n < G::NF; n++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++)
        oacc[n][reg] = oacc[n][reg] * alpha[reg] + pv[n][reg];
  }

  // ---- store O / l (columns >= HD of the last fragment: next head's)
  {
    const int dcol = lane & 15;
    const int rb = 16 * wid + rbase_l;
#pragma unroll
    for (int nn = 0; nn < G::NF; nn++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int row = q0 + rb + reg;
        if (row < seq && (nn * 16 + 16 <= HD || nn * 16 + dcol < HD))
          out[(frame * seq + row) * (long)hidden + head * HD + nn * 16 + dcol] =
              (__bf16)(oacc[nn][reg] / l_run[reg]);
      }
  }
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
