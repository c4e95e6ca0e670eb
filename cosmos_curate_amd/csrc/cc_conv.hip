// bf16 (2+1)D convolutions of the TransNetV2 trunk (DESIGN.md "TransNetV2
// native trunk"): the 3x3 spatial conv, the 3-tap dilated temporal conv and
// the 2x2 average pool, on channels-last activations [frames, H, W, C].
//
// Both convs are implicit GEMMs on __builtin_amdgcn_mfma_f32_16x16x32_bf16
// with the operands read straight from global memory: in channels-last, the
// 8 contiguous channels of one pixel are one lane's operand fragment, so a
// shifted pixel (spatial tap) or a shifted frame (temporal tap) is just
// another address, and a tap outside the frame or the window is a zero
// register, never a load.  The weights are the A operand (rows = output
// channels) and the pixels the B operand (columns = pixels), which leaves
// each lane four CONSECUTIVE output channels of one pixel: one 8-byte store.
// M is the flattened (frame, pixel) index, so 72-pixel frames still fill
// 64-pixel tiles.  f32 accumulation in a fixed order, no atomics: results
// are bit-identical from run to run and independent of the batch.
//
// A wave owns 64 pixels x up to 64 output channels (4x4 fragments); a
// workgroup is four independent waves with consecutive tile numbers, so the
// waves that share pixels (conv3x3: the channel tiles of one pixel tile;
// tconv3: the four dilation branches) hit each other's lines in L1/L2.  No
// LDS and no barriers: every operand byte is reused 4x from registers, the
// rest comes from the caches (the weights of a layer are at most 2.4 MB).
//
// The 3-channel first layer (1 % of the FLOPs, K = 27) is a plain FMA
// kernel: its K is no multiple of 32 and padding it to one would spend
// more MFMA work on zeros than the layer has.

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kWaveM = 64;  // pixels per wave tile
constexpr int kWaveN = 64;  // output channels per wave tile (at most)

// acc[c][f][r] is (output channel 16c + 4*(lane>>4) + r, pixel 16f +
// (lane&15)) of the wave tile; operand fragments are (row or column lane&15,
// 8 elements at 8*(lane>>4) of each k-step of 32).

// y[n,h,w,co] = sum_{dy,dx,ci} x[n,h+dy,w+dx,ci] * w[co,dy,dx,ci], zero
// padding 1.  Wave tile `tile` = (pixel tile tile / n_tiles, channel tile
// tile % n_tiles).
template <int CIN>
__global__ __launch_bounds__(256) void k_conv3x3_bf16(
    const __bf16* __restrict__ x, const __bf16* __restrict__ w,
    __bf16* __restrict__ y, long M, int H, int W, int Cout, int n_tiles,
    long total_tiles) {
  const int lane = threadIdx.x & 63;
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= total_tiles) return;
  const int co0 = (int)(tile % n_tiles) * kWaveN;
  const long m0 = tile / n_tiles * kWaveM;
  const int nfr = min(4, (Cout - co0) / 16);  // wave-uniform
  const int kq = 8 * (lane >> 4);
  const int HW = H * W;

  long m[4];
  int ph[4], pw[4];
  bool live[4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    m[f] = m0 + 16 * f + (lane & 15);
    live[f] = m[f] < M;
    const int p = (int)(m[f] % HW);
    ph[f] = p / W;
    pw[f] = p - ph[f] * W;
  }

  f32x4 acc[4][4] = {};
  for (int tap = 0; tap < 9; tap++) {
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const __bf16* px[4];
    bool ok[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      ok[f] = live[f] && (unsigned)(ph[f] + dy) < (unsigned)H &&
              (unsigned)(pw[f] + dx) < (unsigned)W;
      // inside the frame, so the shifted pixel is pixel m + dy*W + dx
      px[f] = x + (m[f] + dy * W + dx) * CIN + kq;
    }
    const __bf16* wt = w + ((long)(co0 + (lane & 15)) * 9 + tap) * CIN + kq;
#pragma unroll 2
    for (int kk = 0; kk < CIN; kk += 32) {
      bf16x8 pf[4];
#pragma unroll
      for (int f = 0; f < 4; f++) {
        pf[f] = bf16x8{};
        if (ok[f]) pf[f] = *(const bf16x8*)(px[f] + kk);
      }
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if (c < nfr) {
          const bf16x8 wf = *(const bf16x8*)(wt + (long)c * 16 * 9 * CIN + kk);
#pragma unroll
          for (int f = 0; f < 4; f++)
            acc[c][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf, pf[f], acc[c][f], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int f = 0; f < 4; f++) {
    if (!live[f]) continue;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (c < nfr) {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = (__bf16)acc[c][f][r];
        *(bf16x4*)(y + m[f] * Cout + co0 + 16 * c + 4 * (lane >> 4)) = o;
      }
    }
  }
}

// Branch b (dilation 2^b) of the temporal conv: reads channels [b*2F,
// (b+1)*2F) of x [B,T,HW,8F] at frames t-2^b, t, t+2^b of the same window,
// writes channels [b*F, (b+1)*F) of y [B,T,HW,4F] as relu(acc + bias)
// (+ shortcut).  Wave tile `tile` = (pixel tile tile >> 2, branch tile & 3).
template <int F>
__global__ __launch_bounds__(256) void k_tconv3_bf16(
    const __bf16* __restrict__ x, const __bf16* __restrict__ w,
    const float* __restrict__ bias, const __bf16* __restrict__ shortcut,
    __bf16* __restrict__ y, long M, int T, int HW, long total_tiles) {
  constexpr int NFR = F / 16;
  constexpr int C2 = 2 * F, CI = 8 * F, CO = 4 * F;
  const int lane = threadIdx.x & 63;
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= total_tiles) return;
  const int br = (int)(tile & 3);
  const long m0 = (tile >> 2) * kWaveM;
  const int d = 1 << br;
  const int kq = 8 * (lane >> 4);

  long m[4];
  int t[4];
  bool live[4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    m[f] = m0 + 16 * f + (lane & 15);
    live[f] = m[f] < M;
    t[f] = (int)(m[f] / HW % T);
  }

  f32x4 acc[NFR][4] = {};
#pragma unroll
  for (int tap = 0; tap < 3; tap++) {
    const int off = (tap - 1) * d;
    const __bf16* px[4];
    bool ok[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      // zero padding at the window's own ends: never the neighbour window
      ok[f] = live[f] && (unsigned)(t[f] + off) < (unsigned)T;
      px[f] = x + (m[f] + (long)off * HW) * CI + br * C2 + kq;
    }
    const __bf16* wt = w + ((long)(br * F + (lane & 15)) * 3 + tap) * C2 + kq;
#pragma unroll
    for (int kk = 0; kk < C2; kk += 32) {
      bf16x8 pf[4];
#pragma unroll
      for (int f = 0; f < 4; f++) {
        pf[f] = bf16x8{};
        if (ok[f]) pf[f] = *(const bf16x8*)(px[f] + kk);
      }
#pragma unroll
      for (int c = 0; c < NFR; c++) {
        const bf16x8 wf = *(const bf16x8*)(wt + c * 16 * 3 * C2 + kk);
#pragma unroll
        for (int f = 0; f < 4; f++)
          acc[c][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wf, pf[f], acc[c][f], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int c = 0; c < NFR; c++) {
    const int co = br * F + 16 * c + 4 * (lane >> 4);
    const f32x4 bv = *(const f32x4*)(bias + co);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!live[f]) continue;
      bf16x4 sc = {};
      if (shortcut) sc = *(const bf16x4*)(shortcut + m[f] * CO + co);
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; r++)
        o[r] = (__bf16)(fmaxf(acc[c][f][r] + bv[r], 0.0f) + (float)sc[r]);
      *(bf16x4*)(y + m[f] * CO + co) = o;
    }
  }
}

// First layer: x u8 [frames,H,W,3], value bf16(x/255) (f32 division, one
// rounding), w bf16 [Cout][3][3][3]; one thread per (pixel, 8 output
// channels), f32 FMA over the 27 taps in (dy, dx, ci) order.
__global__ __launch_bounds__(256) void k_conv3x3_u8(
    const uint8_t* __restrict__ x, const __bf16* __restrict__ w,
    __bf16* __restrict__ y, long M, int H, int W, int Cout) {
  const int groups = Cout / 8;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= M * groups) return;
  const long m = id / groups;
  const int co0 = (int)(id % groups) * 8;
  const int p = (int)(m % ((long)H * W));
  const int h = p / W, c = p - h * W;

  float xv[27];
#pragma unroll
  for (int tap = 0; tap < 9; tap++) {
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const bool ok = (unsigned)(h + dy) < (unsigned)H &&
                    (unsigned)(c + dx) < (unsigned)W;
    const uint8_t* q = x + (m + dy * W + dx) * 3;
#pragma unroll
    for (int ci = 0; ci < 3; ci++)
      xv[tap * 3 + ci] =
          ok ? (float)(__bf16)((float)q[ci] / 255.0f) : 0.0f;
  }
  // the 8 channels' weights are 216 contiguous bf16 (432 bytes, a multiple
  // of 16): 27 vector loads, element j = channel j / 27, tap j % 27
  bf16x8 wv[27];
  const bf16x8* wp = (const bf16x8*)(w + (long)co0 * 27);
#pragma unroll
  for (int i = 0; i < 27; i++) wv[i] = wp[i];
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < 27; k++) {
      const int e = j * 27 + k;
      a = fmaf(xv[k], (float)wv[e / 8][e % 8], a);
    }
    o[j] = (__bf16)a;
  }
  *(bf16x8*)(y + m * Cout + co0) = o;
}

// AvgPool3d((1,2,2)): [frames,H,W,C] -> [frames,H/2,W/2,C], odd sizes
// floored; f32 sum of the four, times 0.25, one rounding.  One thread per
// (output pixel, 8 channels).
__global__ __launch_bounds__(256) void k_avgpool2x2_bf16(
    const __bf16* __restrict__ x, __bf16* __restrict__ y, long total, int H,
    int W, int C) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int groups = C / 8, Ho = H / 2, Wo = W / 2;
  const int g = (int)(id % groups);
  long r = id / groups;
  const int wo = (int)(r % Wo);
  r /= Wo;
  const int ho = (int)(r % Ho);
  const long n = r / Ho;
  const __bf16* p = x + ((n * H + 2 * ho) * W + 2 * wo) * C + g * 8;
  const bf16x8 a = *(const bf16x8*)p, b = *(const bf16x8*)(p + C),
               c = *(const bf16x8*)(p + (long)W * C),
               d = *(const bf16x8*)(p + (long)W * C + C);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; j++)
    o[j] = (__bf16)((((float)a[j] + (float)b[j]) + ((float)c[j] + (float)d[j])) *
                    0.25f);
  *(bf16x8*)(y + id * 8) = o;
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// 256-thread workgroups for `units` units of work, `per` per workgroup;
// false when they do not fit one launch
bool grid_for(long units, int per, dim3* grid) {
  const long g = (units + per - 1) / per;
  if (g > 0x7fffffffL) return false;
  *grid = dim3((unsigned)g);
  return true;
}

}  // namespace

extern "C" int cc_conv3x3_bf16(const void* x, const void* w, void* y,
                               int64_t frames, int H, int W, int Cin, int Cout,
                               uint64_t stream) {
  if (!x || !w || !y || frames <= 0 || H <= 0 || W <= 0)
    return cc::set_error(CC_ERR_INVALID, "conv3x3: null pointer or "
                         "non-positive size");
  if (misaligned(x, 16) || misaligned(w, 16) || misaligned(y, 16))
    return cc::set_error(CC_ERR_INVALID,
                         "conv3x3: x, w and y must be 16-byte aligned");
  if (Cin != 64 && Cin != 128 && Cin != 256)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "conv3x3: Cin must be 64, 128 or 256 (got %d)", Cin);
  if (Cout <= 0 || Cout % 16 != 0 || Cout > 512)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "conv3x3: Cout must be a multiple of 16 up to 512 "
                         "(got %d)", Cout);
  if ((int64_t)H * W > 0x7fffffff || frames > INT64_MAX / 512 / ((int64_t)H * W))
    return cc::set_error(CC_ERR_UNSUPPORTED, "conv3x3: tensor too large");
  const long M = (long)frames * H * W;
  const int n_tiles = (Cout + kWaveN - 1) / kWaveN;
  const long total = (M + kWaveM - 1) / kWaveM * n_tiles;
  dim3 block(256), grid;
  if (!grid_for(total, 4, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "conv3x3: more than 2^31-1 workgroups");
  return cc::timed_launch("conv3x3", stream, [&] {
    switch (Cin) {
#define CASE(C)                                                              \
  case C:                                                                    \
    hipLaunchKernelGGL(k_conv3x3_bf16<C>, grid, block, 0,                    \
                       (hipStream_t)stream, (const __bf16*)x,                \
                       (const __bf16*)w, (__bf16*)y, M, H, W, Cout, n_tiles, \
                       total);                                               \
    break;
      CASE(64)
      CASE(128)
      CASE(256)
#undef CASE
    }
  });
}

extern "C" int cc_conv3x3_u8(const void* x, const void* w, void* y,
                             int64_t frames, int H, int W, int Cout,
                             uint64_t stream) {
  if (!x || !w || !y || frames <= 0 || H <= 0 || W <= 0)
    return cc::set_error(CC_ERR_INVALID, "conv3x3_u8: null pointer or "
                         "non-positive size");
  if (misaligned(w, 16) || misaligned(y, 16))
    return cc::set_error(CC_ERR_INVALID,
                         "conv3x3_u8: w and y must be 16-byte aligned");
  if (Cout <= 0 || Cout % 16 != 0 || Cout > 512)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "conv3x3_u8: Cout must be a multiple of 16 up to 512 "
                         "(got %d)", Cout);
  if ((int64_t)H * W > 0x7fffffff || frames > INT64_MAX / 512 / ((int64_t)H * W))
    return cc::set_error(CC_ERR_UNSUPPORTED, "conv3x3_u8: tensor too large");
  const long M = (long)frames * H * W;
  dim3 block(256), grid;
  if (!grid_for(M * (Cout / 8), 256, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "conv3x3_u8: more than 2^31-1 workgroups");
  return cc::timed_launch("conv3x3", stream, [&] {
    hipLaunchKernelGGL(k_conv3x3_u8, grid, block, 0, (hipStream_t)stream,
                       (const uint8_t*)x, (const __bf16*)w, (__bf16*)y, M, H, W,
                       Cout);
  });
}

extern "C" int cc_tconv3_bf16(const void* x, const void* w, const float* bias,
                              const void* shortcut, void* y, int64_t B, int T,
                              int HW, int F, uint64_t stream) {
  if (!x || !w || !bias || !y || B <= 0 || T <= 0 || HW <= 0)
    return cc::set_error(CC_ERR_INVALID, "tconv3: null pointer or "
                         "non-positive size");
  if (misaligned(x, 16) || misaligned(w, 16) || misaligned(bias, 16) ||
      misaligned(y, 16) || misaligned(shortcut, 16))
    return cc::set_error(CC_ERR_INVALID, "tconv3: x, w, bias, shortcut and y "
                         "must be 16-byte aligned");
  if (F != 16 && F != 32 && F != 64)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tconv3: F must be 16, 32 or 64 (got %d)", F);
  if (B > INT64_MAX / 512 / T / HW)
    return cc::set_error(CC_ERR_UNSUPPORTED, "tconv3: tensor too large");
  const long M = (long)B * T * HW;
  const long total = (M + kWaveM - 1) / kWaveM * 4;
  dim3 block(256), grid;
  if (!grid_for(total, 4, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "tconv3: more than 2^31-1 workgroups");
  return cc::timed_launch("tconv3", stream, [&] {
    switch (F) {
#define CASE(FF)                                                             \
  case FF:                                                                   \
    hipLaunchKernelGGL(k_tconv3_bf16<FF>, grid, block, 0,                    \
                       (hipStream_t)stream, (const __bf16*)x,                \
                       (const __bf16*)w, bias, (const __bf16*)shortcut,      \
                       (__bf16*)y, M, T, HW, total);                         \
    break;
      CASE(16)
      CASE(32)
      CASE(64)
#undef CASE
    }
  });
}

extern "C" int cc_avgpool2x2_bf16(const void* x, void* y, int64_t frames, int H,
                                  int W, int C, uint64_t stream) {
  if (!x || !y || frames <= 0 || H < 2 || W < 2 || C <= 0)
    return cc::set_error(CC_ERR_INVALID, "avgpool2x2: null pointer, "
                         "non-positive size or H, W below 2");
  if (misaligned(x, 16) || misaligned(y, 16))
    return cc::set_error(CC_ERR_INVALID,
                         "avgpool2x2: x and y must be 16-byte aligned");
  if (C % 8 != 0)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "avgpool2x2: C must be a multiple of 8 (got %d)", C);
  if (frames > INT64_MAX / 2 / C / H / W)
    return cc::set_error(CC_ERR_UNSUPPORTED, "avgpool2x2: tensor too large");
  const long total = (long)frames * (H / 2) * (W / 2) * (C / 8);
  dim3 block(256), grid;
  if (!grid_for(total, 256, &grid))
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "avgpool2x2: more than 2^31-1 workgroups");
  return cc::timed_launch("avgpool", stream, [&] {
    hipLaunchKernelGGL(k_avgpool2x2_bf16, grid, block, 0, (hipStream_t)stream,
                       (const __bf16*)x, (__bf16*)y, total, H, W, C);
  });
}
