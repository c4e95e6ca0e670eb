// Few-query cross-attention for gfx950: the Q-Former of the
// Cosmos-Embed1 tower, where nq <= 32 learned queries per clip attend over
// every token of every frame (nk in the thousands), head dim 64.
//
// With 32 query rows there is exactly one 32-row MFMA tile per (clip, head),
// so the parallelism comes from the keys: the grid is n * heads * splits, a
// workgroup owns a contiguous range of 32-key chunks, and its four waves take
// those chunks round-robin, each with its own running (m, l, O) in registers.
// No barrier inside the loop: a wave shares nothing with the others until
// the merge.
//
// The S^T formulation.  Both products run transposed on
// v_mfma_f32_32x32x16_bf16:
//   S^T [32 keys, 32 queries] = K Q^T     A = K chunk,  B = Q^T, 4 k-steps
//   O^T [64 hd,   32 queries] += V^T P^T  A = V^T,      B = P^T, 2 k-steps,
//                                         two 32-row tiles of hd
// In the 32x32 accumulator lane l holds column l&31 and rows 8i + 4(l>>5) + j
// (register 4i + j).  With the queries on the columns
//   - a lane owns ONE query: its running max, sum and rescale factor are
//     scalars of that lane, the softmax over a chunk's 32 keys is 16 values
//     in registers plus one exchange with lane l^32, and O^T is rescaled
//     without any cross-lane traffic;
//   - P^T leaves the accumulator already in B-operand layout: which key a k
//     index stands for is free as long as both operands agree, so k-step s
//     of lane half h is keys {8(2s + e/4) + 4h + e%4}, registers 8s .. 8s+7
//     rounded to bf16 in place.  P never touches LDS.
// The alternative, O = P V with the queries on the rows, keeps P in
// A-operand layout just as well but spreads a query's 64 outputs over 32
// lanes: every chunk then needs 16 cross-lane reads of the rescale factor.
//
// Where the operands come from:
//   - Q: lane (query l&31, half h) loads its 64 contiguous bytes (head
//     columns 32h .. 32h+31, k-step ks = columns 32h + 8ks ..) once; rows from
//     nq on are zero registers.
//   - K: the same map with the chunk's key l&31 in place of the query, four
//     16-byte loads global -> registers.  Each K row is read once per
//     workgroup, so LDS would only add a round trip.
//   - V needs keys along the MFMA k dimension, eight keys of one head column
//     per lane, and its rows hold head columns: the one operand that goes
//     through LDS, a 4.5 KB row-major image per wave (row stride 72).  Which
//     head column an accumulator row stands for is free, so lane (c, h) reads
//     the ADJACENT columns 2c, 2c+1 of each of its eight keys in one 4-byte
//     read and deals them to the two tiles: row c of tile t is column 2c + t.
//     A lane's 4 rows 8i + 4h + j of both tiles are then 8 adjacent head
//     columns, one 16-byte store at the end.
// K and V of the wave's next chunk are in flight (registers) while the
// current one is computed.  Keys from nk on are never loaded: their K and V
// registers are zeros and their scores are masked to -inf before the max.
//
// At the end the waves meet in LDS (35 KB, over the V images): thread
// (query, 8 head columns) adds the four (m, l, O) in wave order.  One split:
// O / l goes out as bf16.  More: (m, l, O) f32 go to the workspace and
// k_attn_cross_combine adds them in split order.  No atomics anywhere, so two
// runs agree bit for bit.
//
// Numerics: the contract of the online-softmax kernels of cc_attn.hip.
// Scores, max and exp in f32; the unnormalised P rounded to bf16 before PV,
// the sum taken before rounding; PV in f32; bf16 out.
//
// Budget per lane: O^T 32 + S^T 16 + Q 16 + K 16 + V 16 accumulator and
// operand registers; the compiler reports 180 VGPRs (accumulators included),
// no scratch: two waves a SIMD, two workgroups a compute unit.  LDS 35,840
// bytes a workgroup.

#include <hip/hip_runtime.h>

#include <cmath>

#include "cc_attncross_plan.hpp"
#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int HD = cc::XATTN_HD;
constexpr int NQ = cc::XATTN_NQ_MAX;
constexpr int CH = cc::XATTN_CHUNK;
constexpr int NW = cc::XATTN_BLOCK / 64;  // waves
constexpr int LDV = HD + 8;               // V image row stride (elements)
constexpr int V_BYTES = CH * LDV * 2;     // one wave's V image
constexpr int LDO = HD + 4;               // merge image row stride (floats)
constexpr int PART = 2 * NQ + NQ * LDO;   // one wave's (m, l, O) in LDS
constexpr int LDS_BYTES = NW * PART * 4;
static_assert(HD == 64 && NQ == 32 && CH == 32 && NW == 4,
              "the lane maps below assume these");
static_assert(NW * V_BYTES <= LDS_BYTES, "the V images lie under the merge");

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// LDS written by some lanes of a wave and read by others of the same wave:
// DS operations of one wave execute in order, so no s_barrier is needed; the
// fences keep the compiler from moving the accesses across and wait for the
// outstanding ones.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The (m, l, O[8 columns]) of `count` partials `stride` floats apart, each laid
// out [m 32][l 32][O 32 x ldo], added in order for query qn, columns 8g ..
template <typename Ptr>
__device__ __forceinline__ void merge_partials(Ptr base, long stride, int ldo,
                                               int count, int qn, int g,
                                               float& m, float& l,
                                               float (&o)[8]) {
  m = -INFINITY;
  for (int i = 0; i < count; i++) m = fmaxf(m, base[i * stride + qn]);
  l = 0.0f;
#pragma unroll
  for (int e = 0; e < 8; e++) o[e] = 0.0f;
  for (int i = 0; i < count; i++) {
    Ptr p = base + i * stride;
    const float mi = p[qn];
    // a wave that had no chunk carries m = -inf and weighs nothing
    const float w = mi == -INFINITY ? 0.0f : __expf(mi - m);
    l += w * p[NQ + qn];
    const f32x4 a = *(const f32x4*)(p + 2 * NQ + qn * ldo + 8 * g);
    const f32x4 b = *(const f32x4*)(p + 2 * NQ + qn * ldo + 8 * g + 4);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      o[e] += w * a[e];
      o[4 + e] += w * b[e];
    }
  }
}

__device__ __forceinline__ void store_out(__bf16* dst, const float (&o)[8],
                                          float l) {
  const float inv = 1.0f / l;
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; e++) r[e] = (__bf16)(o[e] * inv);
  *(bf16x8*)dst = r;
}

__global__ __launch_bounds__(cc::XATTN_BLOCK) void k_attn_cross(
    const __bf16* __restrict__ q, long ldq, const __bf16* __restrict__ kv,
    long ldkv, __bf16* __restrict__ out, float* __restrict__ ws, int nq, int nk,
    int heads, int hidden, float scale, int splits, int per) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int split = blockIdx.x % splits;
  const long ch = blockIdx.x / splits;
  const int head = (int)(ch % heads);
  const long clip = ch / heads;
  const int chunks = (nk + CH - 1) / CH;
  const int c0 = split * per;
  const int c1 = c0 + per < chunks ? c0 + per : chunks;

  // Q^T fragments: query c, head columns 32h + 8ks ..
  bf16x8 qf[4] = {};
  if (c < nq) {
    const __bf16* qr = q + (clip * nq + c) * ldq + head * HD + 32 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) qf[ks] = *(const bf16x8*)(qr + 8 * ks);
  }
  const __bf16* kbase = kv + clip * nk * ldkv + head * HD;
  const __bf16* vbase = kbase + hidden;

  // a chunk in flight: K fragments (key c, the lane's 32 columns) and the
  // wave's share of the V rows, 16-byte piece lane + 64t = (row, 8 columns)
  bf16x8 kf[4];
  u32x4 vf[4];
  auto fetch = [&](int chunk) {
    const int key = chunk * CH + c;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) kf[ks] = bf16x8{};
    if (key < nk) {
      const __bf16* kr = kbase + (long)key * ldkv + 32 * h;
#pragma unroll
      for (int ks = 0; ks < 4; ks++) kf[ks] = *(const bf16x8*)(kr + 8 * ks);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int p = lane + 64 * t;
      const int vkey = chunk * CH + (p >> 3);
      vf[t] = u32x4{0u, 0u, 0u, 0u};  // rows from nk on are zeros, never loads
      if (vkey < nk)
        vf[t] = *(const u32x4*)(vbase + (long)vkey * ldkv + (p & 7) * 8);
    }
  };

  unsigned short* V = (unsigned short*)(lds + wid * V_BYTES);
  float m_run = -INFINITY, l_run = 0.0f;
  f32x16 o0 = {}, o1 = {};

  int chunk = c0 + wid;
  if (chunk < c1) fetch(chunk);
  for (; chunk < c1; chunk += NW) {
    // the V rows into the wave's image
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int p = lane + 64 * t;
      *(u32x4*)(V + (p >> 3) * LDV + (p & 7) * 8) = vf[t];
    }
    // S^T = K Q^T
    f32x16 s = {};
#pragma unroll
    for (int ks = 0; ks < 4; ks++) s = mfma32(kf[ks], qf[ks], s);
    const int key0 = chunk * CH + 4 * h;
    if (chunk + NW < c1) fetch(chunk + NW);

    // online softmax of query c over this lane's 16 keys and lane^32's
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int key = key0 + 8 * (r >> 2) + (r & 3);
      s[r] = key < nk ? s[r] * scale : -INFINITY;
      mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);  // finite: the chunk's key 0 is live
    const float al = m_run == -INFINITY ? 0.0f : __expf(m_run - m_new);
    float sum = 0.0f;
    bf16x8 pf[2];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float e = __expf(s[r] - m_new);  // 0 for a masked key
      sum += e;
      pf[r >> 3][r & 7] = (__bf16)e;
    }
    l_run = l_run * al + sum;  // this half's keys; the halves meet at the end
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      o0[r] *= al;
      o1[r] *= al;
    }

    // O^T += V^T P^T
    wave_lds_sync();
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      unsigned d[8];
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int row = 8 * (2 * ks + (e >> 2)) + 4 * h + (e & 3);
        d[e] = *(const unsigned*)(V + row * LDV + 2 * c);
      }
      u32x4 lo, hi;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        lo[e] = (d[2 * e] & 0xffffu) | (d[2 * e + 1] << 16);
        hi[e] = (d[2 * e] >> 16) | (d[2 * e + 1] & 0xffff0000u);
      }
      o0 = mfma32(__builtin_bit_cast(bf16x8, lo), pf[ks], o0);
      o1 = mfma32(__builtin_bit_cast(bf16x8, hi), pf[ks], o1);
    }
    wave_lds_sync();  // the next chunk's rows overwrite the image
  }

  // the waves' (m, l, O) into LDS, over the V images
  l_run += __shfl_xor(l_run, 32);
  __syncthreads();
  float* MW = (float*)lds;
  {
    float* mine = MW + wid * PART;
    if (h == 0) {
      mine[c] = m_run;
      mine[NQ + c] = l_run;
    }
    // rows 8i + 4h + j of the two tiles = head columns 16i + 8h + 2j + tile
#pragma unroll
    for (int i = 0; i < 4; i++) {
      float* dst = mine + 2 * NQ + c * LDO + 16 * i + 8 * h;
      *(f32x4*)dst = f32x4{o0[4 * i], o1[4 * i], o0[4 * i + 1], o1[4 * i + 1]};
      *(f32x4*)(dst + 4) =
          f32x4{o0[4 * i + 2], o1[4 * i + 2], o0[4 * i + 3], o1[4 * i + 3]};
    }
  }
  __syncthreads();

  // thread (query qn, columns 8g ..): the four waves in wave order.  Wave 0
  // always had a chunk, so m is finite and l positive.
  const int qn = tid & 31, g = tid >> 5;
  float m, l, o[8];
  merge_partials((const float*)MW, (long)PART, LDO, NW, qn, g, m, l, o);
  if (splits == 1) {
    if (qn < nq)
      store_out(out + (clip * nq + qn) * hidden + head * HD + 8 * g, o, l);
  } else {
    float* part = ws + (long)blockIdx.x * cc::XATTN_PARTIAL_FLOATS;
    if (g == 0) {
      part[qn] = m;
      part[NQ + qn] = l;
    }
    float* dst = part + 2 * NQ + qn * HD + 8 * g;
    *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
    *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
  }
}

// The splits of one (clip, head), added in split order: block = clip*heads +
// head, thread = (query, 8 head columns).  No split is empty.
__global__ __launch_bounds__(cc::XATTN_BLOCK) void k_attn_cross_combine(
    const float* __restrict__ ws, __bf16* __restrict__ out, int nq, int heads,
    int hidden, int splits) {
  const long clip = blockIdx.x / heads;
  const int head = blockIdx.x % heads;
  const int qn = threadIdx.x & 31, g = threadIdx.x >> 5;
  if (qn >= nq) return;
  const float* base = ws + (long)blockIdx.x * splits * cc::XATTN_PARTIAL_FLOATS;
  float m, l, o[8];
  merge_partials(base, (long)cc::XATTN_PARTIAL_FLOATS, HD, splits, qn, g, m, l,
                 o);
  store_out(out + (clip * nq + qn) * hidden + head * HD + 8 * g, o, l);
}

}  // namespace

extern "C" int cc_attn_cross_supported(int heads, int hidden) {
  return cc::attn_cross_supported(heads, hidden) ? 1 : 0;
}

extern "C" int cc_attn_cross_plan(int64_t n, int nq, int nk, int heads,
                                  int hidden, int splits,
                                  cc_attn_cross_plan_info* out) {
  if (!out) return cc::set_error(CC_ERR_INVALID, "cc_attn_cross_plan: null out");
  return cc::attn_cross_plan(n, nq, nk, heads, hidden, splits, out);
}

extern "C" int cc_attn_cross(const void* q, int64_t ldq, const void* kv,
                             int64_t ldkv, void* out, int64_t n, int nq, int nk,
                             int heads, int hidden, float scale, int splits,
                             float* workspace, int64_t workspace_floats,
                             uint64_t stream) {
  cc_attn_cross_plan_info plan;
  if (int rc = cc::attn_cross_plan(n, nq, nk, heads, hidden, splits, &plan))
    return rc;
  if (!q || !kv || !out)
    return cc::set_error(CC_ERR_INVALID, "cc_attn_cross: null pointer");
  // 16-byte row pieces of q, K, V and out
  if (((uintptr_t)q & 15) || ((uintptr_t)kv & 15) || ((uintptr_t)out & 15))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_cross needs 16-byte aligned q/kv/out");
  if (ldq < hidden || ldq % 8 != 0 || ldkv < 2 * (int64_t)hidden || ldkv % 8 != 0)
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_cross needs ldq >= H, ldkv >= 2H, both "
                         "multiples of 8 (ldq %lld, ldkv %lld, H %d)",
                         (long long)ldq, (long long)ldkv, hidden);
  if (plan.splits > 1 && (!workspace || ((uintptr_t)workspace & 15) ||
                          workspace_floats < plan.workspace_floats))
    return cc::set_error(CC_ERR_INVALID,
                         "cc_attn_cross: %d splits need a 16-byte aligned "
                         "workspace of %lld floats (got %lld)",
                         plan.splits, (long long)plan.workspace_floats,
                         (long long)workspace_floats);
  int rc = cc::timed_launch("attn_cross", stream, [&] {
    hipLaunchKernelGGL(k_attn_cross, dim3(plan.grid), dim3(plan.block), 0,
                       (hipStream_t)stream, (const __bf16*)q, (long)ldq,
                       (const __bf16*)kv, (long)ldkv, (__bf16*)out, workspace,
                       nq, nk, heads, hidden, scale, plan.splits,
                       plan.chunks_per_split);
  });
  if (rc != CC_OK || plan.splits == 1) return rc;
  return cc::timed_launch("attn_cross_combine", stream, [&] {
    hipLaunchKernelGGL(k_attn_cross_combine, dim3((unsigned)(n * heads)),
                       dim3(cc::XATTN_BLOCK), 0, (hipStream_t)stream,
                       (const float*)workspace, (__bf16*)out, nq, heads, hidden,
                       plan.splits);
  });
}
