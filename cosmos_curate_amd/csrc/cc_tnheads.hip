// The heads of TransNetV2 (DESIGN.md "TransNetV2 native heads"): everything
// after the conv trunk of csrc/cc_conv.hip, for all windows of a forward in
// one pass.  Five kernels:
//
//   hist512_u8      u8 frames -> L2-normalised 512-bin RGB histograms
//   framesim_embed  the three pooled stack outputs -> spatial means ->
//                   projection -> L2-normalised 128-wide embedding
//   simband_fc      the 101-wide band of a window's T x T similarity matrix
//                   (never the matrix) -> Linear(101, 128) -> relu
//   fc1_relu        Linear(256 + 4608, 1024) + relu on the 16x16x32 bf16
//                   MFMA with hi/lo split operands (f32-grade accuracy)
//   cls_sigmoid     Linear(1024, 1) + sigmoid
//
// Every sum is f32 in an order fixed by the shape of one window alone: no
// float atomics, no split-K, no tile choice that looks at the batch, and a
// workgroup never spans two windows.  Results are bit-identical from run to
// run and for any number of windows.  The histogram's counts are integers
// (LDS atomics, order-free, exact).
//
// Built with -ffp-contract=off: the histogram promises bit-equality with its
// numpy restatement, and the chains below say fmaf where they mean it.

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kLookup = 101;  // lookup window of both similarity heads
constexpr int kHalf = 50;
constexpr int kSimOut = 128;  // outputs of their Linear(101, 128)
constexpr int kEmbed = 128;   // width of the frame-similarity embedding
constexpr int kMaxMeans = 512;

// sum over the 64 lanes in a fixed butterfly; every lane gets the same bits
// (each step adds the same two numbers on both sides, and + commutes)
__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---- 1. colour histogram ---------------------------------------------------
// One workgroup per frame.  bin = (r>>5)<<6 | (g>>5)<<3 | (b>>5); integer
// counts c; out = float(c) / max(sqrtf(float(sum c^2)), 1e-12).  pixels <=
// 4096 keeps sum c^2 <= 2^24, exact in f32 (and in int).
__global__ __launch_bounds__(256) void k_hist512(
    const uint8_t* __restrict__ frames, float* __restrict__ out, int pixels) {
  __shared__ int cnt[512];
  __shared__ int part[4];
  const int tid = threadIdx.x;
  cnt[tid] = 0;
  cnt[tid + 256] = 0;
  __syncthreads();
  const uint8_t* f = frames + (long)blockIdx.x * pixels * 3;
  for (int p = tid; p < pixels; p += 256) {
    const int r = f[3 * p], g = f[3 * p + 1], b = f[3 * p + 2];
    atomicAdd(&cnt[((r >> 5) << 6) | ((g >> 5) << 3) | (b >> 5)], 1);
  }
  __syncthreads();
  const int c0 = cnt[tid], c1 = cnt[tid + 256];
  int sq = c0 * c0 + c1 * c1;  // integers: any order gives the same sum
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, 64);
  if ((tid & 63) == 0) part[tid >> 6] = sq;
  __syncthreads();
  const int total = part[0] + part[1] + part[2] + part[3];
  const float norm = fmaxf(sqrtf((float)total), 1e-12f);
  float* o = out + (long)blockIdx.x * 512;
  o[tid] = (float)c0 / norm;
  o[tid + 256] = (float)c1 / norm;
}

// ---- 2. frame-similarity embedding ------------------------------------------
// One workgroup per frame.  means[c] of each map: f32 sum over the pixels in
// ascending order, then / hw; the maps' means concatenated in map order.  A
// thread owns 8 channels of one map (one 16-byte load per pixel) and keeps 12
// pixels' loads in flight; the order of each channel's sum is still pixel 0,
// 1, 2, ...  e[o] = bias[o] + chain_k fmaf(means[k], wt[k][o]) (k ascending,
// the bias added last); out = e / max(sqrtf(sum e^2), 1e-12), sum e^2 as a
// fixed tree.
struct EmbedMaps {
  const __bf16* x[3];
  int hw[3];
  int c[3];
  int n;
};

constexpr int kMeanBatch = 12;

__global__ __launch_bounds__(256) void k_framesim_embed(
    EmbedMaps maps, const float* __restrict__ wt, const float* __restrict__ bias,
    float* __restrict__ out, int K) {
  __shared__ float means[kMaxMeans];
  __shared__ float part[2];
  const int tid = threadIdx.x;
  const long frame = blockIdx.x;
  const int c8 = tid * 8;  // K <= 512: at most 64 threads own channels
  if (c8 < K) {
    int i = 0, base = 0;
#pragma unroll
    for (int q = 0; q < 2; q++)
      if (i == q && q + 1 < maps.n && c8 - base >= maps.c[q]) {
        base += maps.c[q];
        i = q + 1;
      }
    const int C = i == 0 ? maps.c[0] : i == 1 ? maps.c[1] : maps.c[2];
    const int hw = i == 0 ? maps.hw[0] : i == 1 ? maps.hw[1] : maps.hw[2];
    const __bf16* x = (i == 0 ? maps.x[0] : i == 1 ? maps.x[1] : maps.x[2]) +
                      frame * hw * C + (c8 - base);
    float sum[8] = {};
    int p = 0;
#pragma unroll 1
    for (; p + kMeanBatch <= hw; p += kMeanBatch) {
      bf16x8 v[kMeanBatch];
#pragma unroll
      for (int q = 0; q < kMeanBatch; q++) v[q] = *(const bf16x8*)(x + (long)(p + q) * C);
#pragma unroll
      for (int q = 0; q < kMeanBatch; q++)
#pragma unroll
        for (int e = 0; e < 8; e++) sum[e] += (float)v[q][e];
    }
#pragma unroll 1
    for (; p < hw; p++) {
      const bf16x8 v = *(const bf16x8*)(x + (long)p * C);
#pragma unroll
      for (int e = 0; e < 8; e++) sum[e] += (float)v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) means[c8 + e] = sum[e] / (float)hw;
  }
  __syncthreads();
  float e = 0.0f;
  if (tid < kEmbed) {
    const float* w = wt + tid;
#pragma unroll 1
    for (int k = 0; k < K; k += 8) {  // K % 8 == 0
      float w8[8];
#pragma unroll
      for (int q = 0; q < 8; q++) w8[q] = w[(long)(k + q) * kEmbed];
#pragma unroll
      for (int q = 0; q < 8; q++) e = fmaf(means[k + q], w8[q], e);
    }
    e += bias[tid];
    const float sq = wave_sum(e * e);
    if ((tid & 63) == 0) part[tid >> 6] = sq;
  }
  __syncthreads();
  if (tid < kEmbed) {
    const float norm = fmaxf(sqrtf(part[0] + part[1]), 1e-12f);
    out[frame * kEmbed + tid] = e / norm;
  }
}

// ---- 3. similarity band + Linear(101, 128) + relu ---------------------------
// A workgroup takes kSimFrames consecutive frames of ONE window (their partner
// rows overlap, so they hit in L1).  Per frame g, wave v computes the band
// entries j = v, v+4, ..., kSimBatch of them at a time with their rows' loads
// in flight together: s[g][j] = <x[b,t0+g], x[b,t0+g+j-50]>, each lane an
// ascending fmaf chain over its D/64 elements, then the butterfly.  A partner
// outside [0,T) gives 0: its load is clamped into the window and the product
// dropped, so the loop has no branch.  Then y[o] = relu(fc_b[o] + chain_j
// fmaf(fc_wt[j][o], s[j])), j ascending, with fc_wt [101][128] staged in LDS:
// one thread per (frame, output).
constexpr int kSimFrames = 2;
constexpr int kSimBatch = 5;
constexpr int kSimW4 = kLookup * kSimOut / 4;  // fc_wt in 16-byte pieces

template <int D>
__global__ __launch_bounds__(256) void k_simband_fc(
    const float* __restrict__ x, const float* __restrict__ fc_wt,
    const float* __restrict__ fc_b, float* __restrict__ out, int T,
    int groups_per_window, int ldo, int col) {
  constexpr int V = D / 64;  // floats per lane: 2 or 8
  __shared__ f32x4 wl4[kSimW4];
  __shared__ float s[kSimFrames][kLookup + 3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x / groups_per_window;
  const int t0 = (int)(blockIdx.x % groups_per_window) * kSimFrames;
  const int ng = min(kSimFrames, T - t0);
  const float* xw = x + b * T * D + lane * V;  // this window's rows, this lane's part

#pragma unroll
  for (int it = 0; it < (kSimW4 + 255) / 256; it++) {
    const int i = tid + 256 * it;
    if (i < kSimW4) wl4[i] = ((const f32x4*)fc_wt)[i];
  }

#pragma unroll 1
  for (int g = 0; g < ng; g++) {
    const int t = t0 + g;
    float own[V];
#pragma unroll
    for (int i = 0; i < V; i += 2)
      *(float2*)(own + i) = *(const float2*)(xw + (long)t * D + i);
#pragma unroll 1
    for (int j0 = wave; j0 < kLookup; j0 += 4 * kSimBatch) {
      float pr[kSimBatch][V];
#pragma unroll
      for (int q = 0; q < kSimBatch; q++) {
        const int u = min(max(t + j0 + 4 * q - kHalf, 0), T - 1);
#pragma unroll
        for (int i = 0; i < V; i += 2)
          *(float2*)(pr[q] + i) = *(const float2*)(xw + (long)u * D + i);
      }
#pragma unroll
      for (int q = 0; q < kSimBatch; q++) {
        const int j = j0 + 4 * q, u = t + j - kHalf;
        float d = 0.0f;
#pragma unroll
        for (int i = 0; i < V; i++) d = fmaf(own[i], pr[q][i], d);
        d = wave_sum(d);
        if (lane == 0 && j < kLookup) s[g][j] = (unsigned)u < (unsigned)T ? d : 0.0f;
      }
    }
  }
  __syncthreads();

  const int g = tid >> 7, o = tid & (kSimOut - 1);
  if (g < ng) {
    const float* wl = (const float*)wl4;
    float a = 0.0f;
#pragma unroll 4
    for (int j = 0; j < kLookup; j++) a = fmaf(wl[j * kSimOut + o], s[g][j], a);
    out[(b * T + t0 + g) * ldo + col + o] = fmaxf(a + fc_b[o], 0.0f);
  }
}

// ---- 4. fc1 + relu, split bf16 ----------------------------------------------
// y[m][n] = relu(bias[n] + sum_k a[m][k] * w[n][k]) with a = [hd | feat] and
// w = w_hi + w_lo, on the 16x16x32 bf16 MFMA into ONE f32 accumulator, in this
// order: feat.w_hi, feat.w_lo, hd_hi.w_hi, hd_hi.w_lo, hd_lo.w_hi (each over
// its k ascending); hd_hi = bf16(hd), hd_lo = bf16(hd - float(hd_hi)) formed
// in registers.  As in cc_conv.hip the weights are the A operand (rows =
// outputs n) and the frames the B operand (columns = m), fragments are read
// straight from global memory (8 contiguous k per lane) and a lane ends with
// four consecutive n of one m: one 16-byte store.  No LDS, no barriers.
//
// A wave owns 32 frames x 32 outputs (2x2 fragments); the four waves of a
// workgroup are four consecutive output tiles of one frame tile, so they
// share the activation lines.  Workgroups are numbered output-group fastest:
// with N = 1024 there are 8 output groups, so each of the 8 XCDs sees one
// group's weights only (2.5 MB of hi+lo, resident in its L2) whatever M is.
// One 100-frame window is 4 x 32 = 128 wave tiles.
constexpr int kFcM = 32, kFcN = 32;

__device__ inline bf16x8 split_hi(const f32x4 a, const f32x4 b) {
  bf16x8 h;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    h[i] = (__bf16)a[i];
    h[4 + i] = (__bf16)b[i];
  }
  return h;
}

__device__ inline bf16x8 split_lo(const f32x4 a, const f32x4 b, const bf16x8 h) {
  bf16x8 l;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    l[i] = (__bf16)(a[i] - (float)h[i]);
    l[4 + i] = (__bf16)(b[i] - (float)h[4 + i]);
  }
  return l;
}

// U k-steps of 32: all their fragments loaded, then their MFMAs in k order,
// so the loads of a block are in flight together
template <int U, typename Frag>
__device__ inline void mma_steps(f32x4 (&acc)[2][2], Frag frag,
                                 const __bf16* w0, const __bf16* w1, int k) {
  bf16x8 af[U][2], wf[U][2];
#pragma unroll
  for (int u = 0; u < U; u++) {
    af[u][0] = frag(0, k + 32 * u);
    af[u][1] = frag(1, k + 32 * u);
    wf[u][0] = *(const bf16x8*)(w0 + k + 32 * u);
    wf[u][1] = *(const bf16x8*)(w1 + k + 32 * u);
  }
  __builtin_amdgcn_sched_barrier(0);  // keep every load ahead of the first MFMA
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int f = 0; f < 2; f++)
        acc[c][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf[u][c], af[u][f], acc[c][f], 0, 0, 0);
}

// acc += frag . w over k = 0 .. K-1 ascending (K % 32 == 0)
template <typename Frag>
__device__ inline void mma_pass(f32x4 (&acc)[2][2], Frag frag, const __bf16* w0,
                                const __bf16* w1, int K) {
  int k = 0;
#pragma unroll 1
  for (; k + 256 <= K; k += 256) mma_steps<8>(acc, frag, w0, w1, k);
#pragma unroll 1
  for (; k < K; k += 32) mma_steps<1>(acc, frag, w0, w1, k);
}

__global__ __launch_bounds__(256) void k_fc1_relu(
    const float* __restrict__ hd, const __bf16* __restrict__ feat,
    const __bf16* __restrict__ w_hi, const __bf16* __restrict__ w_lo,
    const float* __restrict__ bias, float* __restrict__ y, long M, int KH,
    int KF, int N, int n_groups) {
  const int lane = threadIdx.x & 63;
  const int n0 = ((int)(blockIdx.x % n_groups) * 4 + (threadIdx.x >> 6)) * kFcN;
  if (n0 >= N) return;
  const long m0 = (long)(blockIdx.x / n_groups) * kFcM;
  const int nfr = min(2, (N - n0) / 16);  // wave-uniform
  const int kq = 8 * (lane >> 4);
  const long K = (long)KH + KF;

  // a column past M's end reads row M-1 (in bounds) and is never stored:
  // columns do not mix, and the loops stay free of branches
  long m[2], mr[2];
  bool live[2];
#pragma unroll
  for (int f = 0; f < 2; f++) {
    m[f] = m0 + 16 * f + (lane & 15);
    live[f] = m[f] < M;
    mr[f] = live[f] ? m[f] : M - 1;
  }
  // the second output fragment of a wave past N's end re-reads the first's
  // rows (in bounds) and is never stored
  long wrow[2];
  wrow[0] = (long)(n0 + (lane & 15)) * K;
  wrow[1] = (long)(n0 + (nfr > 1 ? 16 : 0) + (lane & 15)) * K;

  f32x4 acc[2][2] = {};
  const __bf16* fa[2] = {feat + mr[0] * KF + kq, feat + mr[1] * KF + kq};
  const float* ha[2] = {hd + mr[0] * KH + kq, hd + mr[1] * KH + kq};
  const __bf16* wh[2] = {w_hi + wrow[0] + kq, w_hi + wrow[1] + kq};
  const __bf16* wl[2] = {w_lo + wrow[0] + kq, w_lo + wrow[1] + kq};

  const auto feat_frag = [&](int f, int k) { return *(const bf16x8*)(fa[f] + k); };
  const auto hd_hi_frag = [&](int f, int k) {
    return split_hi(*(const f32x4*)(ha[f] + k), *(const f32x4*)(ha[f] + k + 4));
  };
  const auto hd_lo_frag = [&](int f, int k) {
    const f32x4 v0 = *(const f32x4*)(ha[f] + k), v1 = *(const f32x4*)(ha[f] + k + 4);
    return split_lo(v0, v1, split_hi(v0, v1));
  };

  mma_pass(acc, feat_frag, wh[0] + KH, wh[1] + KH, KF);
  mma_pass(acc, feat_frag, wl[0] + KH, wl[1] + KH, KF);
  mma_pass(acc, hd_hi_frag, wh[0], wh[1], KH);
  mma_pass(acc, hd_hi_frag, wl[0], wl[1], KH);
  mma_pass(acc, hd_lo_frag, wh[0], wh[1], KH);

  // acc[c][f][r] is (output n0 + 16c + 4*(lane>>4) + r, frame m[f])
#pragma unroll
  for (int c = 0; c < 2; c++) {
    if (c >= nfr) continue;
    const int n = n0 + 16 * c + 4 * (lane >> 4);
    const f32x4 bv = *(const f32x4*)(bias + n);
#pragma unroll
    for (int f = 0; f < 2; f++) {
      if (!live[f]) continue;
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; r++) o[r] = fmaxf(acc[c][f][r] + bv[r], 0.0f);
      *(f32x4*)(y + m[f] * N + n) = o;
    }
  }
}

// ---- 5. classifier + sigmoid -------------------------------------------------
// One wave per row: lane l chains fmaf over n = l, l+64, ... ascending, the
// butterfly, + b, 1 / (1 + expf(-z)).
__global__ __launch_bounds__(256) void k_cls_sigmoid(
    const float* __restrict__ y, const float* __restrict__ w, float b,
    float* __restrict__ p, long M, int N) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* row = y + m * N;
  float a = 0.0f;
  for (int n = lane; n < N; n += 64) a = fmaf(w[n], row[n], a);
  const float z = wave_sum(a) + b;
  if (lane == 0) p[m] = 1.0f / (1.0f + expf(-z));
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// one workgroup per `per` units; false when they do not fit one launch
bool grid_for(long units, int per, dim3* grid) {
  const long g = (units + per - 1) / per;
  if (g > 0x7fffffffL) return false;
  *grid = dim3((unsigned)g);
  return true;
}

}  // namespace

extern "C" int cc_tn_hist512_u8(const void* frames_u8, void* out,
                                int64_t frames, int pixels, uint64_t stream) {
  if (!frames_u8 || !out || frames <= 0 || pixels <= 0)
    return cc::set_error(CC_ERR_INVALID, "tn_hist512: null pointer or "
                         "non-positive size");
  if (misaligned(out, 16))
    return cc::set_error(CC_ERR_INVALID,
                         "tn_hist512: out must be 16-byte aligned");
  if (pixels > 4096)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_hist512: at most 4096 pixels per frame keep the "
                         "sum of squared counts exact in f32 (got %d)", pixels);
  dim3 block(256), grid;
  if (!grid_for(frames, 1, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_hist512: more than 2^31-1 workgroups");
  return cc::timed_launch("tn_hist512", stream, [&] {
    hipLaunchKernelGGL(k_hist512, grid, block, 0, (hipStream_t)stream,
                       (const uint8_t*)frames_u8, (float*)out, pixels);
  });
}

extern "C" int cc_tn_framesim_embed(const void* x0, const void* x1,
                                    const void* x2, int hw0, int hw1, int hw2,
                                    int c0, int c1, int c2, int n_maps,
                                    const float* proj_wt, const float* proj_b,
                                    void* out, int64_t frames, int out_dim,
                                    uint64_t stream) {
  if (n_maps < 1 || n_maps > 3)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_framesim_embed: one to three maps (got %d)", n_maps);
  EmbedMaps maps = {};
  maps.n = n_maps;
  const void* xs[3] = {x0, x1, x2};
  const int hws[3] = {hw0, hw1, hw2}, cs[3] = {c0, c1, c2};
  long K = 0;
  for (int i = 0; i < n_maps; i++) {
    if (!xs[i] || hws[i] <= 0 || cs[i] <= 0)
      return cc::set_error(CC_ERR_INVALID, "tn_framesim_embed: null pointer or "
                           "non-positive size");
    if (misaligned(xs[i], 16))
      return cc::set_error(CC_ERR_INVALID,
                           "tn_framesim_embed: maps must be 16-byte aligned");
    maps.x[i] = (const __bf16*)xs[i];
    maps.hw[i] = hws[i];
    maps.c[i] = cs[i];
    K += cs[i];
  }
  if (!proj_wt || !proj_b || !out || frames <= 0)
    return cc::set_error(CC_ERR_INVALID, "tn_framesim_embed: null pointer or "
                         "non-positive size");
  if (misaligned(proj_wt, 16) || misaligned(proj_b, 16) || misaligned(out, 16))
    return cc::set_error(CC_ERR_INVALID, "tn_framesim_embed: proj_wt, proj_b "
                         "and out must be 16-byte aligned");
  if (K > kMaxMeans)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_framesim_embed: at most %d channels over the maps "
                         "(got %ld)", kMaxMeans, K);
  for (int i = 0; i < n_maps; i++)
    if (cs[i] % 8 != 0)
      return cc::set_error(CC_ERR_UNSUPPORTED,
                           "tn_framesim_embed: channels must be a multiple of 8 "
                           "(got %d)", cs[i]);
  if (out_dim != kEmbed)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_framesim_embed: output width must be %d (got %d)",
                         kEmbed, out_dim);
  for (int i = 0; i < n_maps; i++)
    if (frames > INT64_MAX / 2 / hws[i] / cs[i])
      return cc::set_error(CC_ERR_UNSUPPORTED,
                           "tn_framesim_embed: tensor too large");
  dim3 block(256), grid;
  if (!grid_for(frames, 1, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_framesim_embed: more than 2^31-1 workgroups");
  return cc::timed_launch("tn_framesim_embed", stream, [&] {
    hipLaunchKernelGGL(k_framesim_embed, grid, block, 0, (hipStream_t)stream,
                       maps, proj_wt, proj_b, (float*)out, (int)K);
  });
}

extern "C" int cc_tn_simband_fc(const float* x, const float* fc_wt,
                                const float* fc_b, void* out, int64_t B, int T,
                                int D, int ldo, int col, uint64_t stream) {
  if (!x || !fc_wt || !fc_b || !out || B <= 0 || T <= 0)
    return cc::set_error(CC_ERR_INVALID, "tn_simband_fc: null pointer or "
                         "non-positive size");
  if (misaligned(x, 16) || misaligned(fc_wt, 16) || misaligned(fc_b, 16) ||
      misaligned(out, 16))
    return cc::set_error(CC_ERR_INVALID, "tn_simband_fc: x, fc_wt, fc_b and "
                         "out must be 16-byte aligned");
  if (col < 0 || ldo <= 0 || (int64_t)col + kSimOut > ldo)
    return cc::set_error(CC_ERR_INVALID, "tn_simband_fc: columns [%d, %d) do "
                         "not fit a row of %d", col, col + kSimOut, ldo);
  if (D != 128 && D != 512)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_simband_fc: D must be 128 or 512 (got %d)", D);
  if (B > INT64_MAX / 8 / T / (D > ldo ? D : ldo))
    return cc::set_error(CC_ERR_UNSUPPORTED, "tn_simband_fc: tensor too large");
  const int gpw = (T + kSimFrames - 1) / kSimFrames;
  dim3 block(256), grid;
  if (!grid_for((long)B * gpw, 1, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_simband_fc: more than 2^31-1 workgroups");
  return cc::timed_launch("tn_simband_fc", stream, [&] {
    if (D == 128)
      hipLaunchKernelGGL(k_simband_fc<128>, grid, block, 0, (hipStream_t)stream,
                         x, fc_wt, fc_b, (float*)out, T, gpw, ldo, col);
    else
      hipLaunchKernelGGL(k_simband_fc<512>, grid, block, 0, (hipStream_t)stream,
                         x, fc_wt, fc_b, (float*)out, T, gpw, ldo, col);
  });
}

extern "C" int cc_tn_fc1_relu(const float* hd, const void* feat,
                              const void* w_hi, const void* w_lo,
                              const float* bias, void* y, int64_t M, int KH,
                              int KF, int N, uint64_t stream) {
  if (!hd || !feat || !w_hi || !w_lo || !bias || !y || M <= 0 || KH <= 0 ||
      KF <= 0 || N <= 0)
    return cc::set_error(CC_ERR_INVALID, "tn_fc1_relu: null pointer or "
                         "non-positive size");
  if (misaligned(hd, 16) || misaligned(feat, 16) || misaligned(w_hi, 16) ||
      misaligned(w_lo, 16) || misaligned(bias, 16) || misaligned(y, 16))
    return cc::set_error(CC_ERR_INVALID, "tn_fc1_relu: hd, feat, w_hi, w_lo, "
                         "bias and y must be 16-byte aligned");
  if (KH % 32 != 0 || KF % 32 != 0 || N % 16 != 0)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_fc1_relu: KH and KF must be multiples of 32 and N "
                         "of 16 (got %d, %d, %d)", KH, KF, N);
  const int64_t widest = (int64_t)KH + KF > N ? (int64_t)KH + KF : N;
  if (M > INT64_MAX / 8 / widest || (int64_t)N * ((int64_t)KH + KF) > INT64_MAX / 8)
    return cc::set_error(CC_ERR_UNSUPPORTED, "tn_fc1_relu: tensor too large");
  const int n_groups = (N + 4 * kFcN - 1) / (4 * kFcN);
  dim3 block(256), grid;
  if (!grid_for((M + kFcM - 1) / kFcM * n_groups, 1, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_fc1_relu: more than 2^31-1 workgroups");
  return cc::timed_launch("tn_fc1_relu", stream, [&] {
    hipLaunchKernelGGL(k_fc1_relu, grid, block, 0, (hipStream_t)stream, hd,
                       (const __bf16*)feat, (const __bf16*)w_hi,
                       (const __bf16*)w_lo, bias, (float*)y, (long)M, KH, KF, N,
                       n_groups);
  });
}

extern "C" int cc_tn_cls_sigmoid(const float* y, const float* w, float b,
                                 void* p, int64_t M, int N, uint64_t stream) {
  if (!y || !w || !p || M <= 0 || N <= 0)
    return cc::set_error(CC_ERR_INVALID, "tn_cls_sigmoid: null pointer or "
                         "non-positive size");
  if (misaligned(y, 16) || misaligned(w, 16) || misaligned(p, 4))
    return cc::set_error(CC_ERR_INVALID, "tn_cls_sigmoid: y and w must be "
                         "16-byte aligned, p 4-byte");
  if (M > INT64_MAX / 8 / N)
    return cc::set_error(CC_ERR_UNSUPPORTED, "tn_cls_sigmoid: tensor too large");
  dim3 block(256), grid;
  if (!grid_for(M, 4, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tn_cls_sigmoid: more than 2^31-1 workgroups");
  return cc::timed_launch("tn_cls_sigmoid", stream, [&] {
    hipLaunchKernelGGL(k_cls_sigmoid, grid, block, 0, (hipStream_t)stream, y, w,
                       b, (float*)p, (long)M, N);
  });
}
