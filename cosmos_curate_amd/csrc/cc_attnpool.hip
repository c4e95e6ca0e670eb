// One-query attention pooling for gfx950: the pooling heads of
// SigLIP (MAP probe) and InternVideo2 (clip_projector), where one query per
// (frame, head) attends over every token.
//
// With one query the K projection collapses into U [16 heads, H] and the V
// projection moves behind the pooling (cc_hotpath.h), so what is left per
// frame is two skinny contractions over the raw bf16 tokens X [seq, H],
//   S = U X^T   [16, seq]      and      Z = P^T X   [16, H],
// with the 16 heads on one MFMA dimension, both fed from ONE read of X.
//
// k_attn_pool<H>: a workgroup of 8 waves owns one (frame, split of the
// tokens).  Wave w owns columns [w*H/8, (w+1)*H/8) for both contractions:
// KS = H/128 k-steps of the 16x16x16 bf16 MFMA.  Its slice of U, hi and lo
// term of the two-term bf16 split, stays in registers for the whole kernel
// (4*KS VGPRs, 44 at H 1408).  Per chunk of 32 tokens:
//   1. the chunk's rows, prefetched into registers (16-byte loads) while the
//      chunk before was computed, go to LDS X[32][H+8] (90.6 KB at 1408);
//   2. every wave: partial scores [16 heads][32 tokens] over its columns, hi
//      and lo pass into the same accumulators, B fragments = 8-byte row reads
//      of X; the 8 partials meet in LDS (16 KB);
//   3. thread (head, token) — all 512, one each, so no wave waits for a
//      serial softmax — sums the partials in wave order, applies rstd_t and
//      -mu_t*rstd_t*usum_h, masks tokens >= seq, and updates the running
//      max m and sums l and sum c with 32-lane butterflies; w = e*rstd goes
//      to LDS as bf16 P^T, l and sum c = sum e*rstd*mu are summed in f32
//      from the unrounded values;
//   4. every wave rescales its Z accumulators by exp(m_old - m_new) and adds
//      P^T X over the chunk.  The B fragment of that MFMA holds 4 tokens of
//      one column per lane, a transposed read of the row-major chunk.  Which
//      column a lane's accumulator stands for is free, so a lane reads 4
//      (or 2, or 1) ADJACENT columns of each of its 4 token rows in one
//      8-byte (4-, 2-byte) LDS read and deals them to 4 (2, 1) fragments:
//      fragment q of a group holds columns {4c + q}.  Which token a k index
//      stands for is free as well: lane group g takes tokens 8g + 4s + j
//      (k-step s, element j), which puts the four groups' rows 8 apart and,
//      with the row pad of 8 elements, their reads on disjoint banks.
// One split: (Z - sum c) / l goes straight to zhat.  More: (m, l, sum c, Z)
// go to the workspace and k_attn_pool_combine adds them in split order.  No
// atomics anywhere, so two runs agree bit for bit.
//
// Numerics: scores, softmax, l, sum c and Z accumulate in f32; U enters as
// hi + lo (relative error 2^-17); the one rounded operand is w in bf16.

#include <hip/hip_runtime.h>

#include <cmath>

#include "cc_attnpool_plan.hpp"
#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int CH = cc::POOL_CHUNK;
constexpr int NW = cc::POOL_BLOCK / 64;  // waves
constexpr int HM = cc::POOL_HEADS_MAX;
constexpr int LDP = 40;  // P^T row stride: 32 tokens + 8, rows stay 16-byte aligned
static_assert(CH == 32 && NW == 8 && HM == 16, "the lane maps below assume these");

__device__ __forceinline__ f32x4 mfma16(s16x4 a, s16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// What H makes of the wave's column slice: KS fragments of 16 columns, dealt
// in groups of 4, then 2, then 1 for the transposed reads of step 4.
template <int H>
struct PoolDim {
  static_assert(cc::attn_pool_supported(1, H), "width outside the plan");
  static constexpr int KS = H / cc::POOL_H_STEP;
  static constexpr int WCOLS = KS * 16;  // columns per wave
  static constexpr int LDX = H + 8;      // X row stride in LDS (elements)
  static constexpr int N4 = KS / 4, N2 = KS % 4 / 2, N1 = KS % 2;
  static constexpr int X_BYTES = CH * LDX * 2;
  static constexpr int SP_BYTES = NW * HM * CH * 4;
  static constexpr int P_BYTES = HM * LDP * 2;
  static constexpr int LDS_BYTES = X_BYTES + SP_BYTES + P_BYTES + HM * 4;
  // column, inside the wave's slice, of lane column c of fragment f
  __device__ static constexpr int col(int f, int c) {
    return f < 4 * N4            ? 16 * (f & ~3) + 4 * c + (f & 3)
           : f < 4 * N4 + 2 * N2 ? 16 * (4 * N4) + 2 * c + (f - 4 * N4)
                                 : 16 * f + c;
  }
};

// Step 4 for G fragments from f0: Z[f0 + q] += P^T X over the chunk, for the
// columns {slice column 16*f0 + G*c + q}.  a[s] = P^T fragment of k-step s.
template <int G, int KS>
__device__ __forceinline__ void pv_group(f32x4 (&z)[KS], int f0,
                                         const short* xcol, int ldx,
                                         const s16x4 (&a)[2], int g) {
  typedef __attribute__((ext_vector_type(G))) short vec;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    short r[4][G];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const short* p = xcol + (8 * g + 4 * s + j) * ldx;
      if constexpr (G == 1) {
        r[j][0] = *p;
      } else {
        const vec v = *(const vec*)p;
#pragma unroll
        for (int q = 0; q < G; q++) r[j][q] = v[q];
      }
    }
#pragma unroll
    for (int q = 0; q < G; q++) {
      const s16x4 b = {r[0][q], r[1][q], r[2][q], r[3][q]};
      z[f0 + q] = mfma16(a[s], b, z[f0 + q]);
    }
  }
}

template <int H>
__global__ __launch_bounds__(cc::POOL_BLOCK) void k_attn_pool(
    const short* __restrict__ x, long ldx, const float* __restrict__ murstd,
    const short* __restrict__ u_hi, const short* __restrict__ u_lo,
    long u_stride, const float* __restrict__ usum, float* __restrict__ zhat,
    float* __restrict__ ws, int seq, int heads, int splits, int per) {
  using D = PoolDim<H>;
  constexpr int KS = D::KS, LDX = D::LDX, RC = H / 8;  // RC: 16-byte chunks a row
  __shared__ __attribute__((aligned(16))) unsigned char lds[D::LDS_BYTES];
  short* X = (short*)lds;
  float* SP = (float*)(lds + D::X_BYTES);
  short* P = (short*)(lds + D::X_BYTES + D::SP_BYTES);
  float* AL = (float*)(lds + D::X_BYTES + D::SP_BYTES + D::P_BYTES);

  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int c16 = lane & 15, g = lane >> 4;
  const long frame = blockIdx.x / splits;
  const int split = blockIdx.x % splits;
  const int chunks = (seq + CH - 1) / CH;
  const int c0 = split * per;
  const int c1 = c0 + per < chunks ? c0 + per : chunks;
  const int wb = wid * D::WCOLS;  // the wave's first column

  // the wave's slice of U: A fragments (row = head c16, 4 columns at 4g)
  s16x4 uh[KS], ul[KS];
  {
    const long ub = frame * u_stride + (long)c16 * H + wb + 4 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      uh[ks] = *(const s16x4*)(u_hi + ub + 16 * ks);
      ul[ks] = *(const s16x4*)(u_lo + ub + 16 * ks);
    }
  }
  // softmax role: thread (head sh, chunk token st)
  const int sh = tid >> 5, st = tid & 31;
  const float us = usum[(u_stride ? frame * HM : 0) + sh];
  float m_run = -INFINITY, l_run = 0.0f, c_run = 0.0f;

  f32x4 z[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) z[ks] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // a chunk's rows in flight: thread t holds 16-byte pieces t + 512*i
  u32x4 pre[KS];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < KS; i++) {
      const int q = tid + cc::POOL_BLOCK * i;
      const int tok = chunk * CH + q / RC;
      pre[i] = u32x4{0u, 0u, 0u, 0u};  // rows from seq on are zeros, never loads
      if (tok < seq)
        pre[i] = *(const u32x4*)(x + (frame * seq + tok) * ldx + (q % RC) * 8);
    }
  };
  if (c0 < c1) fetch(c0);

  for (int chunk = c0; chunk < c1; chunk++) {
    // 1. the prefetched rows into LDS, the next chunk's into flight
#pragma unroll
    for (int i = 0; i < KS; i++) {
      const int q = tid + cc::POOL_BLOCK * i;
      *(u32x4*)(X + (q / RC) * LDX + (q % RC) * 8) = pre[i];
    }
    __syncthreads();
    if (chunk + 1 < c1) fetch(chunk + 1);

    // 2. partial scores over the wave's columns
    {
      f32x4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;
      const short* xr = X + c16 * LDX + wb + 4 * g;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const s16x4 b0 = *(const s16x4*)(xr + 16 * ks);
        const s16x4 b1 = *(const s16x4*)(xr + 16 * LDX + 16 * ks);
        s0 = mfma16(uh[ks], b0, s0);
        s1 = mfma16(uh[ks], b1, s1);
        s0 = mfma16(ul[ks], b0, s0);
        s1 = mfma16(ul[ks], b1, s1);
      }
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        SP[(wid * HM + 4 * g + reg) * CH + c16] = s0[reg];
        SP[(wid * HM + 4 * g + reg) * CH + 16 + c16] = s1[reg];
      }
    }
    __syncthreads();

    // 3. online softmax, one (head, token) per thread
    {
      const int tok = chunk * CH + st;
      const bool live = tok < seq;
      float dot = 0.0f;
#pragma unroll
      for (int w = 0; w < NW; w++) dot += SP[(w * HM + sh) * CH + st];
      float mu = 0.0f, rs = 1.0f;
      if (live && murstd) {
        const float2 v = *(const float2*)(murstd + 2 * (frame * seq + tok));
        mu = v.x;
        rs = v.y;
      }
      const float s = live ? rs * (dot - mu * us) : -INFINITY;
      float mx = s;
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float m_new = fmaxf(m_run, mx);  // finite: the chunk's token 0 is live
      const float e = live ? __expf(s - m_new) : 0.0f;
      const float al = m_run == -INFINITY ? 0.0f : __expf(m_run - m_new);
      const float wgt = e * rs;
      float se = e, sc = wgt * mu;
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) {
        se += __shfl_xor(se, off);
        sc += __shfl_xor(sc, off);
      }
      l_run = l_run * al + se;
      c_run = c_run * al + sc;
      m_run = m_new;
      P[sh * LDP + st] = __builtin_bit_cast(short, (__bf16)wgt);
      if (st == 0) AL[sh] = al;
    }
    __syncthreads();

    // 4. rescale, then Z += P^T X
    {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const float al = AL[4 * g + reg];
#pragma unroll
        for (int ks = 0; ks < KS; ks++) z[ks][reg] *= al;
      }
      // P^T fragment: head c16, tokens 8g .. 8g+7 = k-steps 0 and 1
      const s16x8 pa = *(const s16x8*)(P + c16 * LDP + 8 * g);
      const s16x4 a[2] = {{pa[0], pa[1], pa[2], pa[3]}, {pa[4], pa[5], pa[6], pa[7]}};
#pragma unroll
      for (int i = 0; i < D::N4; i++)
        pv_group<4, KS>(z, 4 * i, X + wb + 64 * i + 4 * c16, LDX, a, g);
      if constexpr (D::N2 == 1)
        pv_group<2, KS>(z, 4 * D::N4, X + wb + 64 * D::N4 + 2 * c16, LDX, a, g);
      if constexpr (D::N1 == 1)
        pv_group<1, KS>(z, KS - 1, X + wb + 16 * (KS - 1) + c16, LDX, a, g);
    }
    __syncthreads();  // X, SP, P and AL are rewritten by the next chunk
  }

  // the heads' (m, l, sum c) to every wave, through the idle SP
  if (st == 0) {
    SP[sh] = m_run;
    SP[HM + sh] = l_run;
    SP[2 * HM + sh] = c_run;
  }
  __syncthreads();
  if (splits == 1) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int head = 4 * g + reg;
      if (head >= heads) continue;
      const float inv = 1.0f / SP[HM + head], cs = SP[2 * HM + head];
      float* o = zhat + (frame * heads + head) * H + wb;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) o[D::col(ks, c16)] = (z[ks][reg] - cs) * inv;
    }
  } else {
    float* part = ws + (long)blockIdx.x * cc::attn_pool_partial_floats(H);
    if (tid < 3 * HM) part[tid] = SP[tid];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      float* o = part + 3 * HM + (4 * g + reg) * H + wb;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) o[D::col(ks, c16)] = z[ks][reg];
    }
  }
}

// The splits of one (frame, head), added in split order: block = frame*heads
// + head, thread = column.  An empty split carries m = -inf and weighs 0.
__global__ __launch_bounds__(256) void k_attn_pool_combine(
    const float* __restrict__ ws, float* __restrict__ zhat, int heads, int H,
    int splits) {
  __shared__ float wgt[cc::POOL_SPLITS_MAX];
  const long frame = blockIdx.x / heads;
  const int head = blockIdx.x % heads;
  const long pf = cc::attn_pool_partial_floats(H);
  const float* base = ws + frame * splits * pf;
  float m = -INFINITY;
  for (int i = 0; i < splits; i++) m = fmaxf(m, base[i * pf + head]);
  float l = 0.0f, c = 0.0f;
  for (int i = 0; i < splits; i++) {
    const float mi = base[i * pf + head];
    const float w = mi == -INFINITY ? 0.0f : __expf(mi - m);
    l += w * base[i * pf + HM + head];
    c += w * base[i * pf + 2 * HM + head];
    if (threadIdx.x == 0) wgt[i] = w;
  }
  __syncthreads();
  const float inv = 1.0f / l;
  for (int col = threadIdx.x; col < H; col += 256) {
    float zsum = 0.0f;
    for (int i = 0; i < splits; i++)
      zsum += wgt[i] * base[i * pf + 3 * HM + (long)head * H + col];
    zhat[(frame * heads + head) * H + col] = (zsum - c) * inv;
  }
}

using PoolKernel = void (*)(const short*, long, const float*, const short*,
                            const short*, long, const float*, float*, float*,
                            int, int, int, int);
// one instantiation per supported width, [H / POOL_H_STEP - 1]
constexpr PoolKernel kPoolKernels[] = {
    k_attn_pool<128>,  k_attn_pool<256>,  k_attn_pool<384>,  k_attn_pool<512>,
    k_attn_pool<640>,  k_attn_pool<768>,  k_attn_pool<896>,  k_attn_pool<1024>,
    k_attn_pool<1152>, k_attn_pool<1280>, k_attn_pool<1408>};
static_assert(sizeof(kPoolKernels) / sizeof(kPoolKernels[0]) ==
                  cc::POOL_H_MAX / cc::POOL_H_STEP,
              "one kernel per supported width");

}  // namespace

extern "C" int cc_attn_pool_supported(int heads, int H) {
  return cc::attn_pool_supported(heads, H) ? 1 : 0;
}

extern "C" int cc_attn_pool_plan(int64_t n, int seq, int heads, int H,
                                 int splits, cc_attn_pool_plan_info* out) {
  if (!out) return cc::set_error(CC_ERR_INVALID, "cc_attn_pool_plan: null out");
  return cc::attn_pool_plan(n, seq, heads, H, splits, out);
}

extern "C" int cc_attn_pool(const void* x, int64_t ldx, const float* murstd,
                            const void* u_hi, const void* u_lo,
                            int64_t u_stride, const float* usum, float* zhat,
                            int64_t n, int seq, int heads, int H, int splits,
                            float* workspace, int64_t workspace_floats,
                            uint64_t stream) {
  cc_attn_pool_plan_info plan;
  if (int rc = cc::attn_pool_plan(n, seq, heads, H, splits, &plan)) return rc;
  if (!x || !u_hi || !u_lo || !usum || !zhat)
    return cc::set_error(CC_ERR_INVALID, "cc_attn_pool: null pointer");
  // 16-byte token loads, 8-byte U and murstd loads
  if (((uintptr_t)x & 15) || ((uintptr_t)u_hi & 15) || ((uintptr_t)u_lo & 15) ||
      ((uintptr_t)zhat & 15) || ((uintptr_t)murstd & 7) || ((uintptr_t)usum & 3))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_pool needs 16-byte aligned x/u_hi/u_lo/zhat "
                         "and an 8-byte aligned murstd");
  if (ldx < H || ldx % 8 != 0 ||
      (u_stride != 0 && (u_stride < (int64_t)HM * H || u_stride % 8 != 0)))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_pool needs ldx >= H, ldx %% 8 == 0 and "
                         "u_stride 0 or >= 16*H, u_stride %% 8 == 0 (ldx %lld, "
                         "u_stride %lld)",
                         (long long)ldx, (long long)u_stride);
  if (plan.splits > 1 && (!workspace || ((uintptr_t)workspace & 15) ||
                          workspace_floats < plan.workspace_floats))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_pool: %d splits need a 16-byte aligned "
                         "workspace of %lld floats (got %lld)",
                         plan.splits, (long long)plan.workspace_floats,
                         (long long)workspace_floats);
  if (plan.splits > 1 && n * heads > 0x7fffffffLL)
    return cc::set_error(CC_ERR_INVALID, "attn_pool combine grid too large");
  const PoolKernel kernel = kPoolKernels[H / cc::POOL_H_STEP - 1];
  int rc = cc::timed_launch("attn_pool", stream, [&] {
    hipLaunchKernelGGL(kernel, dim3(plan.grid), dim3(plan.block), 0,
                       (hipStream_t)stream, (const short*)x, (long)ldx, murstd,
                       (const short*)u_hi, (const short*)u_lo, (long)u_stride,
                       usum, zhat, workspace, seq, heads, plan.splits,
                       plan.chunks_per_split);
  });
  if (rc != CC_OK || plan.splits == 1) return rc;
  return cc::timed_launch("attn_pool_combine", stream, [&] {
    hipLaunchKernelGGL(k_attn_pool_combine, dim3((unsigned)(n * heads)),
                       dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, zhat, heads, H, plan.splits);
  });
}
