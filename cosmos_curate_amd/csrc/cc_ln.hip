// Fused bf16 LayerNorm — row-wise (x - mean)/sqrt(var + eps) * w + b.
//
// Replaces torch-rocm's vectorized_layer_norm in the ViT forward.  Since
// LN1/LN2 are folded into the GEMMs that consume them it
// runs 2 calls/step at the bench shape (LN2 at M = frames and the post-LN
// on the CLS rows); with the fold off, 25 at ~5.9 TB/s.  Stats in
// f32 (torch layer_norm opmath semantics), bf16 in/out, f32 affine
// params.  One wave per row: H/64 elements per lane, two shfl_xor
// reduction trees (sum, sumsq), bf16x4 (8 B) loads/stores (guide §5
// rule 2: scalar/narrow bf16 access leaves >2x bandwidth on the table;
// measured 4.7 TB/s at bf16x2).
// H is one of the instantiated multiples of 256 (768/1024/3072/4096 all
// comply), 128, or 1152 (SigLIP-so400m): 1152 = 4.5 x 256, so the last of
// its five 256-column steps covers 128 columns and runs on lanes 0..31 —
// the idle half loads and stores nothing and adds zeros to the sums.
// 1408 (InternVideo2-1B) = 5.5 x 256 is the same case.
//
// RMSNorm (InternVideo2): cc_rmsnorm_bf16 is the same wave-per-row pass
// without the mean, y = bf16(x * rsqrt(sum x^2 / H + eps)) * w, and
// cc_qk_rmsnorm_bf16 runs it in place on the q and k sections of a QKV
// GEMM output, one wave per (row, section).
//
// Also here: the row statistics of the folded LayerNorm.
// cc_ln_stats_bf16 reads x once and writes f32 partial sums (sum, sum of
// squares) per 64-column block, [M, H/64, 2] — the layout the residual
// GEMM's epilogue also fills (cc_gemm.hip); cc_ln_finalize adds a row's
// partials in index order and writes (mean, rstd) [M, 2] for the
// consuming GEMM's epilogue.  No atomics, fixed order: bit-identical from
// run to run.
//
// And cc_embed_assemble_ln — the ViT embedding assembly
// ([CLS; patch tokens] + position embedding, then pre-LN) fused into
// one pass.  Replaces a torch cat + f32 add + bf16 cast + layer_norm
// chain (4 kernel launches, ~300 us/step at the bench shape) with one
// bandwidth-bound kernel (reference models/clip.py uses HF
// CLIPVisionEmbeddings: cat + pos_embed add, then pre_layrnorm).

#include <hip/hip_runtime.h>

#include <vector>

#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Whether lane `lane` holds columns in the 256-column step that starts at
// 64-column block c of a row of CHUNK blocks.  Constant true wherever the
// step is whole (always, when CHUNK % 4 == 0).
template <int CHUNK>
__device__ __forceinline__ bool step_live(int c, int lane) {
  return c + 4 <= CHUNK || 4 * lane < (CHUNK - c) * 64;
}

// CHUNK = H / 64, the 64-column blocks of a row; a lane holds 4 elements
// of each 256-column step (CHUNK % 4 != 0: see step_live)
template <int CHUNK>
__global__ void k_layernorm_bf16(const __bf16* __restrict__ x,
                                 const float* __restrict__ w,
                                 const float* __restrict__ b,
                                 __bf16* __restrict__ y, long M, int H,
                                 float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;          // 4 waves per block
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= M) return;
  const __bf16* xr = x + row * H;
  __bf16* yr = y + row * H;

  float vals[(CHUNK + 3) / 4 * 4];
  float s = 0.0f, ss = 0.0f;
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    // coalesced: lane i reads elements (c*64 + 4i .. +3)
    bf16x4 p = {};
    if (step_live<CHUNK>(c, lane)) p = *(const bf16x4*)(xr + c * 64 + 4 * lane);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      vals[c + j] = (float)p[j];
      s += vals[c + j];
      ss += vals[c + j] * vals[c + j];
    }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  const float inv_n = 1.0f / (float)H;
  const float mean = s * inv_n;
  const float var = ss * inv_n - mean * mean;
  const float rstd = rsqrtf(var + eps);
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    if (!step_live<CHUNK>(c, lane)) continue;
    const int i0 = c * 64 + 4 * lane;
    f32x4 wv = *(const f32x4*)(w + i0);
    f32x4 bv = *(const f32x4*)(b + i0);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; j++)
      o[j] = (__bf16)((vals[c + j] - mean) * rstd * wv[j] + bv[j]);
    *(bf16x4*)(yr + i0) = o;
  }
}

// One row of RMSNorm, y = bf16(x * rstd) * w with rstd = rsqrt(sum x^2 / H
// + eps): the normalised value is rounded to bf16 BEFORE the weight
// multiply (the order of the InternVideo2 module: normalise in f32, cast to
// the input type, multiply by the weight).  xr == yr is allowed: a lane
// stores only the columns it loaded, after the last load of the row.
template <int CHUNK>
__device__ __forceinline__ void rms_row(const __bf16* xr,
                                        const float* __restrict__ w,
                                        __bf16* yr, int H, float eps,
                                        int lane) {
  float vals[(CHUNK + 3) / 4 * 4];
  float ss = 0.0f;
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    bf16x4 p = {};
    if (step_live<CHUNK>(c, lane)) p = *(const bf16x4*)(xr + c * 64 + 4 * lane);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      vals[c + j] = (float)p[j];
      ss += vals[c + j] * vals[c + j];
    }
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss * (1.0f / (float)H) + eps);
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    if (!step_live<CHUNK>(c, lane)) continue;
    const int i0 = c * 64 + 4 * lane;
    f32x4 wv = *(const f32x4*)(w + i0);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; j++)
      o[j] = (__bf16)((float)(__bf16)(vals[c + j] * rstd) * wv[j]);
    *(bf16x4*)(yr + i0) = o;
  }
}

template <int CHUNK>
__global__ void k_rmsnorm_bf16(const __bf16* __restrict__ x,
                               const float* __restrict__ w,
                               __bf16* __restrict__ y, long M, int H,
                               float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;          // 4 waves per block
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= M) return;
  rms_row<CHUNK>(x + row * H, w, y + row * H, H, eps, lane);
}

// QK-norm in place on qkv [M, ld]: wave u normalises section u & 1 (0: q,
// columns [0, H) with wq; 1: k, columns [H, 2H) with wk) of row u >> 1.
// Columns from 2H on are never addressed.
template <int CHUNK>
__global__ void k_qk_rmsnorm_bf16(__bf16* qkv, const float* __restrict__ wq,
                                  const float* __restrict__ wk, long M, int H,
                                  long ld, float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long unit = (long)blockIdx.x * 4 + wave;
  if (unit >= 2 * M) return;
  const int sec = (int)(unit & 1);
  __bf16* xr = qkv + (unit >> 1) * ld + (long)sec * H;
  rms_row<CHUNK>(xr, sec ? wk : wq, xr, H, eps, lane);
}

// out[row] = LN( src(row) + pos[t] ) where row = f*tokens + t,
// src = cls (t==0) or tok[f*(tokens-1) + t - 1]; add in f32 like the
// torch chain it replaces (h.float() + pos -> bf16 -> layer_norm).
template <int CHUNK>
__global__ void k_embed_assemble_ln(const __bf16* __restrict__ tok,
                                    const float* __restrict__ cls,
                                    const float* __restrict__ pos,
                                    const float* __restrict__ w,
                                    const float* __restrict__ b,
                                    __bf16* __restrict__ y, long nrows,
                                    int tokens, int H, float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= nrows) return;
  const long f = row / tokens;
  const int t = (int)(row - f * tokens);
  const __bf16* tr = (t == 0) ? nullptr : tok + (f * (tokens - 1) + t - 1) * H;
  const float* pr = pos + (long)t * H;
  __bf16* yr = y + row * H;

  float vals[CHUNK];
  float s = 0.0f, ss = 0.0f;
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    const int i0 = c * 64 + 4 * lane;
    f32x4 pv = *(const f32x4*)(pr + i0);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      // cls follows the torch path: f32 param cast to bf16 first
      float base = tr ? (float)tr[i0 + j] : (float)(__bf16)cls[i0 + j];
      // match torch: (f32 add) rounded to bf16, stats on the bf16 value
      float v = (float)(__bf16)(base + pv[j]);
      vals[c + j] = v;
      s += v;
      ss += v * v;
    }
  }
  s = wave_sum(s);
  ss = wave_sum(ss);
  const float inv_n = 1.0f / (float)H;
  const float mean = s * inv_n;
  const float var = ss * inv_n - mean * mean;
  const float rstd = rsqrtf(var + eps);
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    const int i0 = c * 64 + 4 * lane;
    f32x4 wv = *(const f32x4*)(w + i0);
    f32x4 bv = *(const f32x4*)(b + i0);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; j++)
      o[j] = (__bf16)((vals[c + j] - mean) * rstd * wv[j] + bv[j]);
    *(bf16x4*)(yr + i0) = o;
  }
}

// narrow rows (H=128: 2 elements/lane) keep the bf16x2 form
__global__ void k_layernorm_bf16_h128(const __bf16* __restrict__ x,
                                      const float* __restrict__ w,
                                      const float* __restrict__ b,
                                      __bf16* __restrict__ y, long M,
                                      float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= M) return;
  const __bf16* xr = x + row * 128;
  __bf16* yr = y + row * 128;
  bf16x2 p = *(const bf16x2*)(xr + 2 * lane);
  float v0 = (float)p.x, v1 = (float)p.y;
  float s = wave_sum(v0 + v1);
  float ss = wave_sum(v0 * v0 + v1 * v1);
  const float mean = s / 128.0f;
  const float var = ss / 128.0f - mean * mean;
  const float rstd = rsqrtf(var + eps);
  const int i0 = 2 * lane;
  bf16x2 o;
  o.x = (__bf16)((v0 - mean) * rstd * w[i0] + b[i0]);
  o.y = (__bf16)((v1 - mean) * rstd * w[i0 + 1] + b[i0 + 1]);
  *(bf16x2*)(yr + i0) = o;
}

// sum over each aligned group of 2^k lanes, every lane gets the total
template <int GROUP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = GROUP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// stats[row][blk] = (sum, sum of squares) of x[row][64*blk .. 64*blk+63];
// one wave per row, read-only on x.  Lane i of step c holds columns
// c*64 + 4i .. +3, so 16 adjacent lanes hold one 64-column block; in a
// partial last step (step_live) the idle lanes take part in the shuffles
// with zeros and write nothing.
template <int CHUNK>
__global__ void k_ln_stats_bf16(const __bf16* __restrict__ x,
                                float2* __restrict__ stats, long M, int H) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= M) return;
  const __bf16* xr = x + row * H;
  float2* sr = stats + row * CHUNK;
#pragma unroll
  for (int c = 0; c < CHUNK; c += 4) {
    const bool live = step_live<CHUNK>(c, lane);
    bf16x4 p = {};
    if (live) p = *(const bf16x4*)(xr + c * 64 + 4 * lane);
    float s = 0.0f, ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float v = (float)p[j];
      s += v;
      ss += v * v;
    }
    s = group_sum<16>(s);
    ss = group_sum<16>(ss);
    if (live && (lane & 15) == 0) sr[c + (lane >> 4)] = make_float2(s, ss);
  }
}

// H = 128: 2 elements per lane, 32 lanes per 64-column block
__global__ void k_ln_stats_bf16_h128(const __bf16* __restrict__ x,
                                     float2* __restrict__ stats, long M) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= M) return;
  bf16x2 p = *(const bf16x2*)(x + row * 128 + 2 * lane);
  const float v0 = (float)p.x, v1 = (float)p.y;
  const float s = group_sum<32>(v0 + v1);
  const float ss = group_sum<32>(v0 * v0 + v1 * v1);
  if ((lane & 31) == 0) stats[row * 2 + (lane >> 5)] = make_float2(s, ss);
}

// murstd[r] = (mean, rstd) of stats row r * row_step: 8 lanes per row,
// lane j adds partials j, j+8, ... in that order, then a 3-step tree.
// Same form as k_layernorm_bf16: var = sumsq/H - mean^2, rsqrtf(var+eps).
__global__ void k_ln_finalize(const float2* __restrict__ stats,
                              float2* __restrict__ murstd, long M, int P,
                              long row_step, float inv_n, float eps) {
  const long row = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int j = threadIdx.x & 7;
  float s = 0.0f, ss = 0.0f;
  if (row < M) {
    const float2* sr = stats + row * row_step * P;
    for (int p = j; p < P; p += 8) {
      const float2 v = sr[p];
      s += v.x;
      ss += v.y;
    }
  }
  s = group_sum<8>(s);
  ss = group_sum<8>(ss);
  if (row < M && j == 0) {
    const float mean = s * inv_n;
    const float var = ss * inv_n - mean * mean;
    murstd[row] = make_float2(mean, rsqrtf(var + eps));
  }
}

// The RMSNorm form of k_ln_finalize: murstd[r] = (0, rsqrt(sumsq/H + eps)),
// the pair with which the LN_IN epilogue rstd * (acc - mean * s) + c is
// RMSNorm.  Same lanes, same order of additions; the sums are not read.
__global__ void k_rms_finalize(const float2* __restrict__ stats,
                               float2* __restrict__ murstd, long M, int P,
                               long row_step, float inv_n, float eps) {
  const long row = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int j = threadIdx.x & 7;
  float ss = 0.0f;
  if (row < M) {
    const float2* sr = stats + row * row_step * P;
    for (int p = j; p < P; p += 8) ss += sr[p].y;
  }
  ss = group_sum<8>(ss);
  if (row < M && j == 0)
    murstd[row] = make_float2(0.0f, rsqrtf(ss * inv_n + eps));
}

// the CHUNK (= H / 64) values the templates are instantiated for; the
// entry points reject every other H before they launch, so the switches
// below need no default.  CC_LN_CHUNKS256: whole 256-column steps, all
// three templates; CC_LN_CHUNKS adds 18 (H = 1152) and 22 (H = 1408) for
// k_layernorm_bf16, k_ln_stats_bf16 and the RMSNorm kernels, which handle
// the partial last step (the RMSNorm kernels take H = 128 as CHUNK 2 the
// same way: one step, lanes 0..31).
#define CC_LN_CHUNKS256(X) X(4) X(8) X(12) X(16) X(32) X(48) X(64)
#define CC_LN_CHUNKS(X) CC_LN_CHUNKS256(X) X(18) X(22)

#define OR_EQ(C) || H == 64 * C
bool has_chunk(int64_t H) { return false CC_LN_CHUNKS(OR_EQ); }
bool has_chunk256(int64_t H) { return false CC_LN_CHUNKS256(OR_EQ); }
#undef OR_EQ

}  // namespace

bool cc::ln_h_supported(int64_t H) { return H == 128 || has_chunk(H); }

extern "C" int cc_ln_stats_bf16(const void* x, int64_t M, int64_t H,
                                void* stats, uint64_t stream) {
  if (!x || !stats || M <= 0 || H <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad ln_stats args");
  if (!cc::ln_h_supported(H))
    return cc::set_error(CC_ERR_UNSUPPORTED, "unsupported H %lld", (long long)H);
  dim3 block(256), grid((M + 3) / 4);
  return cc::timed_launch("ln_stats", stream, [&] {
    switch (H / 64) {
      case 2:
        hipLaunchKernelGGL(k_ln_stats_bf16_h128, grid, block, 0,
                           (hipStream_t)stream, (const __bf16*)x,
                           (float2*)stats, (long)M);
        break;
#define CASE(C)                                                            \
  case C:                                                                  \
    hipLaunchKernelGGL(k_ln_stats_bf16<C>, grid, block, 0,                 \
                       (hipStream_t)stream, (const __bf16*)x,              \
                       (float2*)stats, (long)M, (int)H);                   \
    break;
        CC_LN_CHUNKS(CASE)
#undef CASE
    }
  });
}

extern "C" int cc_ln_finalize(const void* stats, int64_t M, int64_t H,
                              int64_t row_step, float eps, void* murstd,
                              uint64_t stream) {
  if (!stats || !murstd || M <= 0 || H <= 0 || row_step <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad ln_finalize args");
  if (!cc::ln_h_supported(H))
    return cc::set_error(CC_ERR_UNSUPPORTED, "unsupported H %lld", (long long)H);
  dim3 block(256), grid((M + 31) / 32);  // 8 lanes per row
  return cc::timed_launch("ln_finalize", stream, [&] {
    hipLaunchKernelGGL(k_ln_finalize, grid, block, 0, (hipStream_t)stream,
                       (const float2*)stats, (float2*)murstd, (long)M,
                       (int)(H / 64), (long)row_step, 1.0f / (float)H, eps);
  });
}

extern "C" int cc_rms_finalize(const void* stats, int64_t M, int64_t H,
                               int64_t row_step, float eps, void* murstd,
                               uint64_t stream) {
  if (!stats || !murstd || M <= 0 || H <= 0 || row_step <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad rms_finalize args");
  if (!cc::ln_h_supported(H))
    return cc::set_error(CC_ERR_UNSUPPORTED, "unsupported H %lld", (long long)H);
  dim3 block(256), grid((M + 31) / 32);  // 8 lanes per row
  return cc::timed_launch("ln_finalize", stream, [&] {
    hipLaunchKernelGGL(k_rms_finalize, grid, block, 0, (hipStream_t)stream,
                       (const float2*)stats, (float2*)murstd, (long)M,
                       (int)(H / 64), (long)row_step, 1.0f / (float)H, eps);
  });
}

extern "C" int cc_rmsnorm_bf16(const void* x, const void* w, void* y,
                               int64_t M, int64_t H, float eps,
                               uint64_t stream) {
  if (!x || !w || !y || M <= 0 || H <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad rmsnorm args");
  if (!cc::ln_h_supported(H))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "rmsnorm: H must be a width cc_layernorm_bf16 "
                         "takes (got %lld)",
                         (long long)H);
  dim3 block(256), grid((M + 3) / 4);
  return cc::timed_launch("rmsnorm_bf16", stream, [&] {
    switch (H / 64) {
#define CASE(C)                                                            \
  case C:                                                                  \
    hipLaunchKernelGGL(k_rmsnorm_bf16<C>, grid, block, 0,                  \
                       (hipStream_t)stream, (const __bf16*)x,              \
                       (const float*)w, (__bf16*)y, (long)M, (int)H, eps); \
    break;
      CASE(2)
      CC_LN_CHUNKS(CASE)
#undef CASE
    }
  });
}

extern "C" int cc_qk_rmsnorm_bf16(void* qkv, int64_t M, int64_t H, int64_t ld,
                                  const void* wq, const void* wk, float eps,
                                  uint64_t stream) {
  if (!qkv || !wq || !wk || M <= 0 || H <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad qk_rmsnorm args");
  if (ld < 2 * H || ld % 4 != 0)
    return cc::set_error(CC_ERR_INVALID,
                         "qk_rmsnorm: ld %lld must hold the q and k sections "
                         "(>= 2H = %lld) and keep rows 8-byte aligned "
                         "(ld %% 4 == 0)",
                         (long long)ld, (long long)(2 * H));
  if (!cc::ln_h_supported(H))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "qk_rmsnorm: H must be a width cc_layernorm_bf16 "
                         "takes (got %lld)",
                         (long long)H);
  dim3 block(256), grid((2 * M + 3) / 4);  // one wave per (row, section)
  return cc::timed_launch("qk_rmsnorm", stream, [&] {
    switch (H / 64) {
#define CASE(C)                                                            \
  case C:                                                                  \
    hipLaunchKernelGGL(k_qk_rmsnorm_bf16<C>, grid, block, 0,               \
                       (hipStream_t)stream, (__bf16*)qkv, (const float*)wq, \
                       (const float*)wk, (long)M, (int)H, (long)ld, eps);  \
    break;
      CASE(2)
      CC_LN_CHUNKS(CASE)
#undef CASE
    }
  });
}

extern "C" int cc_layernorm_bf16(const void* x, const void* w, const void* b,
                                 void* y, int64_t M, int64_t H, float eps,
                                 uint64_t stream) {
  if (!x || !w || !b || !y || M <= 0 || H <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad layernorm args");
  if (!cc::ln_h_supported(H))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "H must be 128, 1152, 1408 or an instantiated "
                         "k*256, <=4096 (got %lld)",
                         (long long)H);
  dim3 block(256), grid((M + 3) / 4);
  return cc::timed_launch("layernorm_bf16", stream, [&] {
    switch (H / 64) {
      case 2:
        hipLaunchKernelGGL(k_layernorm_bf16_h128, grid, block, 0,
                           (hipStream_t)stream, (const __bf16*)x,
                           (const float*)w, (const float*)b, (__bf16*)y,
                           (long)M, eps);
        break;
#define CASE(C)                                                            \
  case C:                                                                  \
    hipLaunchKernelGGL(k_layernorm_bf16<C>, grid, block, 0,                \
                       (hipStream_t)stream, (const __bf16*)x,              \
                       (const float*)w, (const float*)b, (__bf16*)y,       \
                       (long)M, (int)H, eps);                              \
    break;
        CC_LN_CHUNKS(CASE)
#undef CASE
    }
  });
}

extern "C" int cc_embed_assemble_ln(const void* tok, const void* cls,
                                    const void* pos, const void* w,
                                    const void* b, void* y, int64_t n_frames,
                                    int64_t tokens, int64_t H, float eps,
                                    uint64_t stream) {
  if (!tok || !cls || !pos || !w || !b || !y || n_frames <= 0 || tokens <= 1 ||
      H <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad embed_assemble args");
  if (H % 256 != 0 || H > 64 * 64)
    return cc::set_error(CC_ERR_UNSUPPORTED, "H must be k*256, <=4096 (got %lld)",
                         (long long)H);
  if (!has_chunk256(H))
    return cc::set_error(CC_ERR_UNSUPPORTED, "unsupported H %lld", (long long)H);
  const long nrows = (long)n_frames * tokens;
  dim3 block(256), grid((nrows + 3) / 4);
  return cc::timed_launch("embed_assemble_ln", stream, [&] {
    switch (H / 64) {
#define CASE(C)                                                            \
  case C:                                                                  \
    hipLaunchKernelGGL(k_embed_assemble_ln<C>, grid, block, 0,             \
                       (hipStream_t)stream, (const __bf16*)tok,            \
                       (const float*)cls, (const float*)pos,               \
                       (const float*)w, (const float*)b, (__bf16*)y,       \
                       nrows, (int)tokens, (int)H, eps);                   \
    break;
      CC_LN_CHUNKS256(CASE)
#undef CASE
    }
  });
}
