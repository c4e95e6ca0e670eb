// Fused pixel kernels of the hot path — hand-written HIP for gfx950.
//
// Replaces:
//   cvcuda.cvtcolor_into(YUV2RGB_NV12)   nvcodec_utils.py:178
//   cvcuda.resize_into(LINEAR)           nvcodec_utils.py:189-194
//   cvcuda.reformat_into (NCHW/NHWC)     nvcodec_utils.py:267
//   cv2.resize INTER_CUBIC               decoder_utils.py:666-670
//   torchvision normalize chain          models/clip.py:48-62
//
// All kernels are HBM-bandwidth-bound byte work (~3.3 MB
// algorithmic traffic per 1080p frame vs ~8 TB/s HBM3E): the design goal is
// coalesced wave64 access + enough workgroups to fill 256 CUs, not MFMA.
//
// NUMERICS CONTRACT: bit-exact vs oracle/color.py.  Both sides evaluate the
// same f32 expressions in the same order with round-half-up
// (floorf(x+0.5f)); this translation unit is compiled with
// -ffp-contract=off so hipcc cannot fuse mul+add into FMA and change
// rounding vs numpy.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <type_traits>
#include <vector>

#include "cc_common.hpp"
#include "cc_timing.hpp"

#define CC_CHECK_HIP(expr)                                                   \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess)                                                    \
      return cc::set_error(CC_ERR_HIP, "%s failed: %s", #expr,               \
                           hipGetErrorString(_e));                           \
  } while (0)

namespace {

__device__ __forceinline__ unsigned char round_u8(float x) {
  float r = floorf(x + 0.5f);
  r = fminf(fmaxf(r, 0.0f), 255.0f);
  return (unsigned char)r;
}

// pixel-center source coordinate (oracle/color.py:_src_grid)
__device__ __forceinline__ float src_coord(int d, int dst_n, int src_n) {
  float scale = (float)src_n / (float)dst_n;
  return ((float)d + 0.5f) * scale - 0.5f;
}

// The one bilinear definition every bilinear kernel shares; the f32
// association order below is what keeps them bit-exact vs oracle/color.py:
//   y0 = clip(floor(s), 0, n-1); y1 = min(y0+1, n-1); w = clip(s-y0, 0, 1)
// with the clamp of y0 done in float.
struct BilinearTaps {
  int y0, y1, x0, x1;
  float wy, wx;
};

__device__ __forceinline__ BilinearTaps bilinear_taps(int dy, int dx, int dh,
                                                      int dw, int sh, int sw) {
  float syf = src_coord(dy, dh, sh);
  float sxf = src_coord(dx, dw, sw);
  BilinearTaps t;
  t.y0 = (int)fminf(fmaxf(floorf(syf), 0.0f), (float)(sh - 1));
  t.x0 = (int)fminf(fmaxf(floorf(sxf), 0.0f), (float)(sw - 1));
  t.y1 = min(t.y0 + 1, sh - 1);
  t.x1 = min(t.x0 + 1, sw - 1);
  t.wy = fminf(fmaxf(syf - (float)t.y0, 0.0f), 1.0f);
  t.wx = fminf(fmaxf(sxf - (float)t.x0, 0.0f), 1.0f);
  return t;
}

__device__ __forceinline__ unsigned char bilinear_blend_u8(
    float v00, float v01, float v10, float v11, float wx, float wy) {
  float top = v00 * (1.0f - wx) + v01 * wx;
  float bot = v10 * (1.0f - wx) + v11 * wx;
  return round_u8(top * (1.0f - wy) + bot * wy);
}

// ---------------- 8/10/12-bit 4:2:0 semi-planar -> RGB ----------------
// NV12 (u8 samples) and P016 (u16 samples, MSB-aligned) with a selectable
// matrix and range.  Per sample, in f32 and in this order (the contract
// tests/yuv_ref.py restates):
//   s = sample >> (16 - depth)            (depth 8: s = sample)
//   x = float(s) * 2^-(depth-8)           (exact)
//   yf = x_Y - yoff, u = x_U - 128, v = x_V - 128
//   fy = CY*yf; R = fy + CVR*v; G = fy + CVG*v + CUG*u; B = fy + CUB*u
//   round_u8 each.
struct YuvCoef {
  float yoff, cy, cvr, cvg, cug, cub;
};

// entries of each table of the cc_hdr_tables_build image (f32 then u8)
constexpr int kHdrTableEntries = 4096;
static_assert(kHdrTableEntries * 5 == CC_HDR_TABLE_BYTES, "table image size");

// [matrix 0=BT.601 1=BT.709 2=BT.2020-NCL][0 = limited range, 1..3 = full
// range at depth 8/10/12].  Limited: yoff 16, CY 255/219, chroma scale
// sc 255/224; full: yoff 0, CY = sc = 255*2^(d-8)/(2^d-1);
// CVR 2(1-Kr)sc, CVG -2Kr(1-Kr)/Kg*sc, CUG -2Kb(1-Kb)/Kg*sc, CUB 2(1-Kb)sc.
// Every row is the double-precision formula rounded to f32, EXCEPT BT.601
// limited: its five literals are the ones oracle/color.py uses, this row is
// the only place they live here, and every 8-bit NV12 result is pinned to
// them.  Its CVR/CVG sit one ulp off the formula and must not move.
constexpr YuvCoef kYuvCoef[3][4] = {
    {{16.0f, 1.1643835f, 1.5960267f, -0.8129676f, -0.3917623f, 2.0172321f},
     {0.0f, 1.0f, 1.40199995f, -0.714136302f, -0.344136298f, 1.77199996f},
     {0.0f, 0.997067451f, 1.39788854f, -0.712042034f, -0.343127102f,
      1.7668035f},
     {0.0f, 0.996336997f, 1.39686441f, -0.711520374f, -0.342875719f,
      1.76550913f}},
    {{16.0f, 1.16438353f, 1.79274106f, -0.532909334f, -0.21324861f,
      2.11240172f},
     {0.0f, 1.0f, 1.57480001f, -0.46812427f, -0.187324271f, 1.8556f},
     {0.0f, 0.997067451f, 1.57018185f, -0.466751486f, -0.186774939f,
      1.85015833f},
     {0.0f, 0.996336997f, 1.56903148f, -0.466409534f, -0.186638102f,
      1.84880292f}},
    {{16.0f, 1.16438353f, 1.6786741f, -0.650424302f, -0.187326103f,
      2.14177227f},
     {0.0f, 1.0f, 1.47459996f, -0.571353137f, -0.164553121f, 1.88139999f},
     {0.0f, 0.997067451f, 1.47027564f, -0.569677591f, -0.164070562f,
      1.87588274f},
     {0.0f, 0.996336997f, 1.46919858f, -0.56926024f, -0.163950369f,
      1.87450838f}},
};

// what a kernel needs to convert one sample triple, as run-time values;
// yuv420sp_launch is the one place that fills it in
struct YuvParams {
  int shift;
  float scale;
  YuvCoef k;
};

// (8, bt601, limited) as compile-time constants under YuvParams' member
// names: the shift and the scale fold away and the coefficients become
// immediates.  Only the fused resize kernel is instantiated with it — the
// first kernel of bench.py's step, measurably slower with run-time values
// (DESIGN.md §4a).
struct YuvBt601Limited8 {
  static constexpr int shift = 0;
  static constexpr float scale = 1.0f;
  static constexpr YuvCoef k = kYuvCoef[0][0];
};

// YuvParams plus what the PQ (SMPTE ST 2084) -> SDR chain reads: the two
// tables of cc_hdr_tables_build on the device and 1/(peak/white)^2.  The
// scalar and the fused-resize kernel read the tables through the cache;
// the 8-pixels-per-lane kernel copies the image to LDS first (DESIGN.md §4b
// has the A/B).
struct YuvHdrParams : YuvParams {
  const float* tin;           // [4096] code/16 -> linear light / white
  const unsigned char* tout;  // [4096] 4095*c^(1/4) -> 255*c^(1/2.4)
  float inv_w2;
};

__device__ __forceinline__ float hdr_eotf(float c8, const float* tin) {
  float i = fminf(fmaxf(floorf(c8 * 16.0f + 0.5f), 0.0f), 4080.0f);
  return tin[(int)i];
}

__device__ __forceinline__ unsigned char hdr_oetf(float c,
                                                  const unsigned char* tout) {
  float y = sqrtf(sqrtf(c));  // c in [0, 1], so the index is in [0, 4095]
  return tout[(int)floorf(y * 4095.0f + 0.5f)];
}

// What becomes of the three f32 R'G'B' values on the 8-bit scale for PQ
// content, where the SDR types round them to u8: tone-mapped to SDR first.
// Every step is f32 in this order (the contract tests/hdr_ref.py restates);
// the only transcendental steps are the two tables, so the result does not
// depend on a device pow:
//   L  = tin[clamp(floor(c8*16 + 0.5), 0, 4080)]      inverse PQ / white
//   BT.2020 -> BT.709 (BT.2087), row = (m0*R + m1*G) + m2*B, max(., 0)
//   m  = max(max(r, g), b); s = (1 + m*inv_w2) / (1 + m)   extended Reinhard
//   c  = min(c*s, 1)
//   out = tout[floor(sqrt(sqrt(c))*4095 + 0.5)]        inverse BT.1886
// The division and the square roots must be correctly rounded.
__device__ __forceinline__ uchar3 hdr_finish(float r8, float g8, float b8,
                                             const YuvHdrParams& p) {
  const float lr = hdr_eotf(r8, p.tin);
  const float lg = hdr_eotf(g8, p.tin);
  const float lb = hdr_eotf(b8, p.tin);
  const float r = fmaxf((1.6605f * lr + -0.5876f * lg) + -0.0728f * lb, 0.0f);
  const float g = fmaxf((-0.1246f * lr + 1.1329f * lg) + -0.0083f * lb, 0.0f);
  const float b = fmaxf((-0.0182f * lr + -0.1006f * lg) + 1.1187f * lb, 0.0f);
  const float m = fmaxf(fmaxf(r, g), b);
  const float s = (1.0f + m * p.inv_w2) / (1.0f + m);
  return {hdr_oetf(fminf(r * s, 1.0f), p.tout),
          hdr_oetf(fminf(g * s, 1.0f), p.tout),
          hdr_oetf(fminf(b * s, 1.0f), p.tout)};
}

// P = YuvParams, YuvBt601Limited8 or YuvHdrParams: one matrix definition
// for all three.  The finish step is round_u8 per channel, written inside
// the braces as it always was (handing the three sums to a function first
// reorders the SDR kernels' instructions), or hdr_finish.
template <typename P>
__device__ __forceinline__ uchar3 yuv_to_rgb_u8(unsigned sy, unsigned su,
                                                unsigned sv, const P& p) {
  float yf = (float)(sy >> p.shift) * p.scale - p.k.yoff;
  float u = (float)(su >> p.shift) * p.scale - 128.0f;
  float v = (float)(sv >> p.shift) * p.scale - 128.0f;
  float fy = p.k.cy * yf;
  if constexpr (std::is_same_v<P, YuvHdrParams>)
    return hdr_finish(fy + p.k.cvr * v, fy + p.k.cvg * v + p.k.cug * u,
                      fy + p.k.cub * u, p);
  else
    return {round_u8(fy + p.k.cvr * v),
            round_u8(fy + p.k.cvg * v + p.k.cug * u),
            round_u8(fy + p.k.cub * u)};
}

// one pixel (full-res coords); T = sample type, pitch in bytes
template <typename T, typename P>
__device__ __forceinline__ uchar3 yuv420sp_px(
    const unsigned char* __restrict__ y, const unsigned char* __restrict__ uv,
    size_t pitch, int yy, int xx, const P& p) {
  const T* yr = (const T*)(y + (size_t)yy * pitch);
  // the chroma pair through one pointer with constant offsets 0 and 1, so
  // the compiler merges the two loads into one (8 loads per fused-resize
  // thread where it would otherwise issue 12: +22 % time)
  const T* c = (const T*)(uv + (size_t)(yy >> 1) * pitch) + (size_t)(xx & ~1);
  return yuv_to_rgb_u8(yr[xx], c[0], c[1], p);
}

// Scalar path: one thread per pixel over columns [x_start, w) of every
// row — the w % 8 row tails, or whole frames (x_start = 0) whose planes
// are not 16-byte aligned.
template <typename T, typename P>
__global__ void k_yuv420sp_to_rgb_px(const unsigned char* __restrict__ y,
                                     const unsigned char* __restrict__ uv,
                                     int n, int h, int w, int x_start,
                                     size_t pitch, P p,
                                     unsigned char* __restrict__ out) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cw = w - x_start;
  long total = (long)n * h * cw;
  if (idx >= total) return;
  int xx = x_start + (int)(idx % cw);
  long t = idx / cw;
  int yy = t % h;
  int f = t / h;
  uchar3 rgb = yuv420sp_px<T>(y + (size_t)f * pitch * h,
                              uv + (size_t)f * pitch * (h / 2), pitch, yy, xx,
                              p);
  unsigned char* o = out + (((size_t)f * h + yy) * w + xx) * 3;
  o[0] = rgb.x;
  o[1] = rgb.y;
  o[2] = rgb.z;
}

struct __attribute__((packed)) rgb8_run {
  unsigned int d[6];
};

// Vector path: one lane per run of 8 pixels of one row.  One load of 8 Y
// samples and one of the 4 chroma pairs they share (16 B each at 16 bit,
// 8 B at 8 bit; planes and pitch 16-byte aligned, checked by the
// launcher), 24 contiguous output bytes stored as dwords.  Bandwidth-
// bound: 3 B/px in at 16 bit, 3 B/px out.  Sample and byte positions are
// compile-time constants after unrolling, so nothing is indexed at run
// time and nothing spills.  With YuvHdrParams each workgroup first copies
// the table image (20 KB, 16-byte aligned, tin then tout) to LDS: its 2048
// pixels make 12288 table reads, and with unrelated neighbours those cost
// a fifth of the kernel's time through the cache and nothing from LDS
// (DESIGN.md §4b).  8 workgroups of 20 KB fit a CU, so occupancy stays 8.
template <typename T, typename P>
__global__ void k_yuv420sp_to_rgb_v8(const unsigned char* __restrict__ y,
                                     const unsigned char* __restrict__ uv,
                                     int n, int h, int w, size_t pitch, P p,
                                     unsigned char* __restrict__ out) {
  constexpr int BITS = 8 * (int)sizeof(T);
  constexpr int PER = 32 / BITS;  // samples per dword
  constexpr unsigned MASK = (1u << BITS) - 1u;
  if constexpr (std::is_same_v<P, YuvHdrParams>) {
    __shared__ uint4 tables[CC_HDR_TABLE_BYTES / 16];
    const uint4* image = (const uint4*)p.tin;
    for (int i = threadIdx.x; i < CC_HDR_TABLE_BYTES / 16; i += blockDim.x)
      tables[i] = image[i];
    __syncthreads();  // before the early return below: every thread arrives
    p.tin = (const float*)tables;
    p.tout = (const unsigned char*)(tables + kHdrTableEntries / 4);
  }
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int runs = w / 8;
  long total = (long)n * h * runs;
  if (idx >= total) return;
  int x0 = (int)(idx % runs) * 8;
  long t = idx / runs;
  int yy = t % h;
  int f = t / h;
  const unsigned char* yp =
      y + (size_t)f * pitch * h + (size_t)yy * pitch + (size_t)x0 * sizeof(T);
  const unsigned char* uvp = uv + (size_t)f * pitch * (h / 2) +
                             (size_t)(yy >> 1) * pitch +
                             (size_t)x0 * sizeof(T);
  unsigned int yw[4], cw[4];
  if constexpr (sizeof(T) == 2) {
    *(uint4*)yw = *(const uint4*)yp;
    *(uint4*)cw = *(const uint4*)uvp;
  } else {
    *(uint2*)yw = *(const uint2*)yp;
    *(uint2*)cw = *(const uint2*)uvp;
  }
  unsigned int o[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int ju = j & ~1, jv = ju + 1;
    uchar3 rgb = yuv_to_rgb_u8((yw[j / PER] >> (BITS * (j % PER))) & MASK,
                               (cw[ju / PER] >> (BITS * (ju % PER))) & MASK,
                               (cw[jv / PER] >> (BITS * (jv % PER))) & MASK,
                               p);
    o[(3 * j) >> 2] |= (unsigned)rgb.x << (8 * ((3 * j) & 3));
    o[(3 * j + 1) >> 2] |= (unsigned)rgb.y << (8 * ((3 * j + 1) & 3));
    o[(3 * j + 2) >> 2] |= (unsigned)rgb.z << (8 * ((3 * j + 2) & 3));
  }
  unsigned char* op = out + (((size_t)f * h + yy) * w + x0) * 3;
  if (((size_t)op & 7) == 0) {
    // dense NHWC rows with w % 4 == 0 off an aligned base: always here
    uint2* o8 = (uint2*)op;
    o8[0] = make_uint2(o[0], o[1]);
    o8[1] = make_uint2(o[2], o[3]);
    o8[2] = make_uint2(o[4], o[5]);
  } else {
    // unaligned dword stores (e.g. w = 66, odd rows)
    *(rgb8_run*)op = rgb8_run{{o[0], o[1], o[2], o[3], o[4], o[5]}};
  }
}

// Fused convert + bilinear resize.  Equivalent to cvtcolor_into (u8 RGB
// materialized) followed by resize_into(LINEAR): each tap is converted and
// rounded to u8 before the f32 bilinear blend — bit-identical to
// k_yuv420sp_to_rgb_* followed by k_resize_bilinear_u8, without writing
// the intermediate full-resolution RGB to HBM.
template <typename T, typename P>
__global__ void k_yuv420sp_to_rgb_resize(
    const unsigned char* __restrict__ y, const unsigned char* __restrict__ uv,
    int n, int sh, int sw, size_t pitch, P p,
    unsigned char* __restrict__ out, int dh, int dw) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)n * dh * dw;
  if (idx >= total) return;
  int dx = idx % dw;
  long t = idx / dw;
  int dy = t % dh;
  int f = t / dh;
  const unsigned char* yp = y + (size_t)f * pitch * sh;
  const unsigned char* uvp = uv + (size_t)f * pitch * (sh / 2);

  const BilinearTaps b = bilinear_taps(dy, dx, dh, dw, sh, sw);
  uchar3 p00 = yuv420sp_px<T>(yp, uvp, pitch, b.y0, b.x0, p);
  uchar3 p01 = yuv420sp_px<T>(yp, uvp, pitch, b.y0, b.x1, p);
  uchar3 p10 = yuv420sp_px<T>(yp, uvp, pitch, b.y1, b.x0, p);
  uchar3 p11 = yuv420sp_px<T>(yp, uvp, pitch, b.y1, b.x1, p);

  unsigned char* o = out + ((size_t)idx) * 3;
  o[0] = bilinear_blend_u8(p00.x, p01.x, p10.x, p11.x, b.wx, b.wy);
  o[1] = bilinear_blend_u8(p00.y, p01.y, p10.y, p11.y, b.wx, b.wy);
  o[2] = bilinear_blend_u8(p00.z, p01.z, p10.z, p11.z, b.wx, b.wy);
}

// ---------------- u8 NHWC bilinear resize ----------------
__global__ void k_resize_bilinear_u8(const unsigned char* __restrict__ in,
                                     int n, int sh, int sw,
                                     unsigned char* __restrict__ out, int dh,
                                     int dw) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)n * dh * dw;
  if (idx >= total) return;
  int dx = idx % dw;
  long t = idx / dw;
  int dy = t % dh;
  int f = t / dh;
  const unsigned char* src = in + (size_t)f * sh * sw * 3;

  const BilinearTaps b = bilinear_taps(dy, dx, dh, dw, sh, sw);
  unsigned char* o = out + ((size_t)idx) * 3;
#pragma unroll
  for (int c = 0; c < 3; c++)
    o[c] = bilinear_blend_u8(src[((size_t)b.y0 * sw + b.x0) * 3 + c],
                             src[((size_t)b.y0 * sw + b.x1) * 3 + c],
                             src[((size_t)b.y1 * sw + b.x0) * 3 + c],
                             src[((size_t)b.y1 * sw + b.x1) * 3 + c], b.wx,
                             b.wy);
}

// ---------------- u8 NHWC bicubic resize (A=-0.75) ----------------
__device__ __forceinline__ void cubic_w(float tfrac, float w[4]) {
  const float A = -0.75f;
  float x0 = tfrac + 1.0f, x1 = tfrac, x2 = 1.0f - tfrac, x3 = 2.0f - tfrac;
  w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__global__ void k_resize_bicubic_u8(const unsigned char* __restrict__ in,
                                    int n, int sh, int sw,
                                    unsigned char* __restrict__ out, int dh,
                                    int dw) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)n * dh * dw;
  if (idx >= total) return;
  int dx = idx % dw;
  long t = idx / dw;
  int dy = t % dh;
  int f = t / dh;
  const unsigned char* src = in + (size_t)f * sh * sw * 3;

  float syf = src_coord(dy, dh, sh);
  float sxf = src_coord(dx, dw, sw);
  float fy = floorf(syf), fx = floorf(sxf);
  int iy = (int)fy, ix = (int)fx;
  float wy[4], wx[4];
  cubic_w(syf - fy, wy);
  cubic_w(sxf - fx, wx);
  int rows[4], cols[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    rows[k] = min(max(iy - 1 + k, 0), sh - 1);
    cols[k] = min(max(ix - 1 + k, 0), sw - 1);
  }
  unsigned char* o = out + ((size_t)idx) * 3;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    // horizontal then vertical, left-to-right adds (matches oracle order)
    float v = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const unsigned char* row = src + (size_t)rows[r] * sw * 3;
      float hsum = ((float)row[cols[0] * 3 + c] * wx[0] +
                    (float)row[cols[1] * 3 + c] * wx[1]) +
                   (float)row[cols[2] * 3 + c] * wx[2];
      hsum = hsum + (float)row[cols[3] * 3 + c] * wx[3];
      if (r == 0)
        v = hsum * wy[0];
      else if (r == 1)
        v = v + hsum * wy[1];
      else if (r == 2)
        v = v + hsum * wy[2];
      else
        v = v + hsum * wy[3];
    }
    o[c] = round_u8(v);
  }
}

// ---------------- u8 NHWC antialiased separable resize (+ crop) ----------------
// Resize(antialias=True) + CenterCrop of torchvision, computing only the
// cropped region.  The filter lives in the two per-axis tables of
// cc_resize_aa_table_build (int32 first[len], int32 count[len],
// f32 w[len][taps]); the kernel is the same for every filter.  Per output
// pixel and channel, in f32, multiply then add (this file is built with
// -ffp-contract=off), bit-exact vs tests/resize_aa_ref.py:
//   hrow[y] = sum_k wx[ox][k] * float(src[y][firstx[ox] + k])   k ascending from 0.0f
//   v       = sum_k wy[oy][k] * hrow[firsty[oy] + k]            k ascending from 0.0f
//   out     = u8(rintf(min(max(v, 0), 255)))
// rintf is round-half-to-even, which is torch.round in torchvision's
// _cast_squeeze_out; deliberately NOT this file's round_u8 (half up).
//
// One workgroup per (frame, band of kAaBR output rows, block of kAaBC output
// columns).  hrow[y] depends only on (y, ox, c), so it is computed once per
// source row and shared by the band's output rows through LDS.  The band's
// source rows are walked in ascending chunks of as many rows as the LDS
// holds; each chunk is (0) copied to LDS in 16-byte pieces, (1)
// reduced horizontally into f32 hrow values in LDS, (2) added into the
// per-thread vertical accumulators.  Chunks ascend, so every accumulator
// still sees its terms k ascending: a band that needs several chunks gives
// the bits of one that needs one, and there is no tap count past which
// another kernel would be needed.  No atomics, no scratch.
//
// The tables are device memory the launcher cannot read, so the kernel does
// not trust them: first and count are clamped to the source and to `taps`
// where they are read, and a block whose columns span more source pixels
// than the LDS holds shortens the spans.  A table that
// cc_resize_aa_table_build wrote is never changed by either.
constexpr int kAaBC = 32;          // output columns per workgroup
constexpr int kAaBR = 8;           // output rows per workgroup
constexpr int kAaThreads = kAaBC * kAaBR;
// with s_fx / s_cx 40 KiB per workgroup: 4 workgroups per CU (160 KiB LDS)
constexpr int kAaLdsBytes = 40960 - 2 * kAaBC * 4;
constexpr int kAaRowPad = 63;      // most a staged row takes past its span
// 16 bytes at a 4-byte-aligned address
struct __attribute__((packed, aligned(4))) aa_quad {
  unsigned d[4];
};
static_assert(CC_RESIZE_AA_MAX_TAPS % 2 == 1, "taps are odd");
// weights + one staged row of 4096 source pixels + its hrow always fit
static_assert((kAaBC + kAaBR) * CC_RESIZE_AA_MAX_TAPS * 4 + 4096 * 3 +
                  kAaRowPad + kAaBC * 12 <= kAaLdsBytes, "LDS budget");

__global__ __launch_bounds__(kAaThreads) void k_resize_aa_u8(
    const unsigned char* __restrict__ in, int n, int sh, int sw,
    unsigned char* __restrict__ out, int oh, int ow,
    const int32_t* __restrict__ ty, int taps_y,
    const int32_t* __restrict__ tx, int taps_x, int blocks_x, int bands) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kAaLdsBytes];
  __shared__ int s_fx[kAaBC], s_cx[kAaBC];
  const int tid = threadIdx.x;
  const int oxl = tid % kAaBC, oyl = tid / kAaBC;
  const int bx = blockIdx.x % blocks_x;
  const int band = (blockIdx.x / blocks_x) % bands;
  const int f = blockIdx.x / (blocks_x * bands);
  const int ox0 = bx * kAaBC, oy0 = band * kAaBR;
  const int ox = ox0 + oxl, oy = oy0 + oyl;
  const float* __restrict__ wx_g = (const float*)(tx + 2 * (size_t)ow);
  const float* __restrict__ wy_g = (const float*)(ty + 2 * (size_t)oh);

  // this block's columns, clamped to the source row
  if (tid < kAaBC) {
    int fx = 0, cx = 0;
    if (ox < ow) {
      fx = min(max(tx[ox], 0), sw);
      cx = min(max(tx[ow + ox], 0), min(taps_x, sw - fx));
    }
    s_fx[tid] = fx;
    s_cx[tid] = cx;
  }
  // this thread's output row, clamped to the source, and the band's rows
  int fy = 0, cy = 0;
  int y_lo = sh, y_hi = 0;
  for (int r = 0; r < kAaBR; r++) {
    const int o = oy0 + r;
    if (o >= oh) break;
    const int a = min(max(ty[o], 0), sh);
    const int c = min(max(ty[oh + o], 0), min(taps_y, sh - a));
    if (r == oyl) {
      fy = a;
      cy = c;
    }
    if (c > 0) {
      y_lo = min(y_lo, a);
      y_hi = max(y_hi, a + c);
    }
  }
  __syncthreads();
  int x_lo = sw, x_hi = 0;
  for (int i = 0; i < kAaBC; i++)
    if (s_cx[i] > 0) {
      x_lo = min(x_lo, s_fx[i]);
      x_hi = max(x_hi, s_fx[i] + s_cx[i]);
    }
  if (x_hi < x_lo) x_lo = x_hi = 0;

  // LDS: wx[kAaBC][taps_x], wy[kAaBR][taps_y], hrow[rc][3][kAaBC] f32, then
  // rc staged source rows of `stride` bytes
  float* wxs = (float*)lds;
  float* wys = wxs + kAaBC * taps_x;
  float* hrow = wys + kAaBR * taps_y;
  const int rest = kAaLdsBytes - (kAaBC * taps_x + kAaBR * taps_y) * 4;
  const int cap_px = (rest - kAaBC * 12 - kAaRowPad) / 3;
  if (x_hi - x_lo > cap_px) {  // never with a table of the builder's
    x_hi = x_lo + cap_px;
    __syncthreads();  // uniform branch: everyone has read s_fx / s_cx
    if (tid < kAaBC) {
      const int fx = min(s_fx[tid], x_hi);
      s_fx[tid] = fx;
      s_cx[tid] = min(s_cx[tid], x_hi - fx);
    }
  }
  const int span = (x_hi - x_lo) * 3;                  // bytes per row
  const int stride = ((span + 15) & ~15) + 48;         // multiple of 16
  const int rc = rest / (stride + kAaBC * 12);         // >= 1
  unsigned char* srcs = (unsigned char*)(hrow + (size_t)rc * 3 * kAaBC);
  // 16-byte pieces that cover a row at any alignment; 16*nq <= span + 18
  const int nq = (span + 18) / 16;

  for (int i = tid; i < kAaBC * taps_x; i += kAaThreads) {
    const int c = ox0 + i / taps_x;
    wxs[i] = c < ow ? wx_g[(size_t)c * taps_x + i % taps_x] : 0.0f;
  }
  for (int i = tid; i < kAaBR * taps_y; i += kAaThreads) {
    const int r = oy0 + i / taps_y;
    wys[i] = r < oh ? wy_g[(size_t)r * taps_y + i % taps_y] : 0.0f;
  }

  const size_t frame_bytes = (size_t)sh * sw * 3;
  const unsigned char* in_end = in + (size_t)n * frame_bytes;
  const unsigned char* frame = in + (size_t)f * frame_bytes;
  float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;

  for (int r0 = y_lo; r0 < y_hi; r0 += rc) {
    const int rows = min(rc, y_hi - r0);
    __syncthreads();  // the last chunk's readers are done; s_fx, wxs written
    // (0) rows [r0, r0+rows), bytes [x_lo*3, x_hi*3) -> LDS.  A row starts
    // at any byte address; it is read as the 16-byte pieces, from the dword
    // boundary at or below it, that cover it (up to 18 bytes past its span:
    // the neighbouring pixels, rows or frames) and lands in LDS at the same
    // offset mod 4.
    for (int i = tid; i < rows * nq; i += kAaThreads) {
      const int row = i / nq, q = i - row * nq;
      const unsigned char* a = frame + ((size_t)(r0 + row) * sw + x_lo) * 3;
      const unsigned char* p = a - ((size_t)a & 3) + 16 * q;
      uint4 v;
      if (p >= in && p + 16 <= in_end) {
        const aa_quad g = *(const aa_quad*)p;
        v = make_uint4(g.d[0], g.d[1], g.d[2], g.d[3]);
      } else {  // the piece straddles the buffer's first or last byte
        unsigned d[4] = {0, 0, 0, 0};
        for (int b = 0; b < 16; b++)
          if (p + b >= in && p + b < in_end)
            d[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
        v = make_uint4(d[0], d[1], d[2], d[3]);
      }
      *(uint4*)(srcs + (size_t)row * stride + 16 * q) = v;
    }
    __syncthreads();
    // (1) one thread per (row, column): the three channels' horizontal
    // sums, four taps (12 bytes = 3 dwords) per step.  Taps past count
    // take weight 0; the bytes under them are whatever the LDS holds,
    // always finite as u8, and v + 0*x leaves v's value.
    for (int i = tid; i < rows * kAaBC; i += kAaThreads) {
      const int col = i % kAaBC, row = i / kAaBC;
      const int fx = s_fx[col], cx = s_cx[col];
      const unsigned char* a = frame + ((size_t)(r0 + row) * sw + x_lo) * 3;
      // cx > 0 puts fx in [x_lo, x_hi); a column with no taps reads nothing
      const int b = cx > 0 ? (fx - x_lo) * 3 + (int)((size_t)a & 3) : 0;
      const unsigned* p = (const unsigned*)(srcs + (size_t)row * stride) + (b >> 2);
      const unsigned s = b & 3;
      const float* w = wxs + col * taps_x;
      float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
      unsigned d0 = p[0];
      for (int k = 0; k < cx; k += 4) {
        const unsigned d1 = p[1], d2 = p[2], d3 = p[3];
        const unsigned e0 = __builtin_amdgcn_alignbyte(d1, d0, s);
        const unsigned e1 = __builtin_amdgcn_alignbyte(d2, d1, s);
        const unsigned e2 = __builtin_amdgcn_alignbyte(d3, d2, s);
        const float w0 = w[k];
        const float w1 = k + 1 < cx ? w[k + 1] : 0.0f;
        const float w2 = k + 2 < cx ? w[k + 2] : 0.0f;
        const float w3 = k + 3 < cx ? w[k + 3] : 0.0f;
        h0 = h0 + w0 * (float)(e0 & 0xffu);
        h1 = h1 + w0 * (float)((e0 >> 8) & 0xffu);
        h2 = h2 + w0 * (float)((e0 >> 16) & 0xffu);
        h0 = h0 + w1 * (float)(e0 >> 24);
        h1 = h1 + w1 * (float)(e1 & 0xffu);
        h2 = h2 + w1 * (float)((e1 >> 8) & 0xffu);
        h0 = h0 + w2 * (float)((e1 >> 16) & 0xffu);
        h1 = h1 + w2 * (float)(e1 >> 24);
        h2 = h2 + w2 * (float)(e2 & 0xffu);
        h0 = h0 + w3 * (float)((e2 >> 8) & 0xffu);
        h1 = h1 + w3 * (float)((e2 >> 16) & 0xffu);
        h2 = h2 + w3 * (float)(e2 >> 24);
        d0 = d3;
        p += 3;
      }
      float* hr = hrow + (size_t)row * 3 * kAaBC + col;
      hr[0] = h0;
      hr[kAaBC] = h1;
      hr[2 * kAaBC] = h2;
    }
    __syncthreads();
    // (2) this thread's output pixel: the taps whose rows are in the chunk
    const int k_lo = max(r0 - fy, 0), k_hi = min(cy, r0 + rows - fy);
    for (int k = k_lo; k < k_hi; k++) {
      const float w = wys[oyl * taps_y + k];
      const float* hr = hrow + (size_t)(fy + k - r0) * 3 * kAaBC + oxl;
      acc0 = acc0 + w * hr[0];
      acc1 = acc1 + w * hr[kAaBC];
      acc2 = acc2 + w * hr[2 * kAaBC];
    }
  }
  if (ox < ow && oy < oh) {
    unsigned char* o = out + (((size_t)f * oh + oy) * ow + ox) * 3;
    o[0] = (unsigned char)rintf(fminf(fmaxf(acc0, 0.0f), 255.0f));
    o[1] = (unsigned char)rintf(fminf(fmaxf(acc1, 0.0f), 255.0f));
    o[2] = (unsigned char)rintf(fminf(fmaxf(acc2, 0.0f), 255.0f));
  }
}

// ---------------- CLIP preprocess: u8 NHWC -> f32/bf16 NCHW ----------------
__global__ void k_clip_preprocess_f32(const unsigned char* __restrict__ in,
                                      int n, int h, int w, float m0, float m1,
                                      float m2, float s0, float s1, float s2,
                                      float* __restrict__ out) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long hw = (long)h * w;
  long total = (long)n * hw;  // one thread per pixel, 3 channels
  if (idx >= total) return;
  long p = idx % hw;
  int f = idx / hw;
  const unsigned char* px = in + ((size_t)f * hw + p) * 3;
  float* ob = out + (size_t)f * 3 * hw + p;
  float mean[3] = {m0, m1, m2}, stdev[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float x = (float)px[c] / 255.0f;
    ob[(size_t)c * hw] = (x - mean[c]) / stdev[c];
  }
}

__device__ __forceinline__ unsigned short pp_bf16(float x, float mean,
                                                  float stdev) {
  float v = (x - mean) / stdev;  // division kept: bit-exact vs oracle
  // round-to-nearest-even bf16 (torch .to(bfloat16) semantics)
  union {
    float f;
    unsigned int u;
  } cv{v};
  unsigned int lsb = (cv.u >> 16) & 1;
  unsigned int r = cv.u + 0x7fffu + lsb;
  return (unsigned short)(r >> 16);
}

typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;

// 4 pixels per thread: 3 dword reads of the interleaved u8 RGB, one
// 8-byte store per plane (coalesced both ways); scalar tail for
// hw % 4 != 0 pixels.
__global__ void k_clip_preprocess_bf16(const unsigned char* __restrict__ in,
                                       int n, int h, int w, float m0, float m1,
                                       float m2, float s0, float s1, float s2,
                                       unsigned short* __restrict__ out) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // quad index
  long hw = (long)h * w;
  long total_q = ((long)n * hw + 3) / 4;
  if (idx >= total_q) return;
  const float mean[3] = {m0, m1, m2};
  const float stdev[3] = {s0, s1, s2};
  long pix0 = idx * 4;
  long p = pix0 % hw;
  int f = pix0 / hw;
  unsigned char bytes[12];
  if (p + 4 <= hw && ((long)n * hw - pix0) >= 4) {
    const unsigned int* src = (const unsigned int*)(in + ((size_t)f * hw + p) * 3);
    unsigned int d0 = src[0], d1 = src[1], d2 = src[2];
    *(unsigned int*)(bytes + 0) = d0;
    *(unsigned int*)(bytes + 4) = d1;
    *(unsigned int*)(bytes + 8) = d2;
    unsigned short* ob = out + (size_t)f * 3 * hw + p;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      u16x4 o;
#pragma unroll
      for (int j = 0; j < 4; j++)
        o[j] = pp_bf16((float)bytes[3 * j + c] / 255.0f, mean[c], stdev[c]);
      *(u16x4*)(ob + (size_t)c * hw) = o;
    }
  } else {
    // tail quad may cross a frame/row boundary: per-pixel path
    long total = (long)n * hw;
    for (long px = pix0; px < pix0 + 4 && px < total; px++) {
      long pp = px % hw;
      int ff = px / hw;
      const unsigned char* sp = in + ((size_t)ff * hw + pp) * 3;
      unsigned short* ob = out + (size_t)ff * 3 * hw + pp;
#pragma unroll
      for (int c = 0; c < 3; c++)
        ob[(size_t)c * hw] = pp_bf16((float)sp[c] / 255.0f, mean[c], stdev[c]);
    }
  }
}


// normalize + patch-extraction fused: u8 NHWC frames -> the ViT patch
// GEMM's A layout [n*g*g, kpad] bf16, col = c*P*P + ky*P + kx (the
// conv-weight flatten order), cols >= 3*P*P zero-padded.  Replaces the
// torch reshape/permute/pad chain after cc_clip_preprocess (a full
// 2x206 MB round trip per bench step).
__global__ void k_clip_preprocess_patches(
    const unsigned char* __restrict__ in, int n, int h, int w, int patch,
    int kpad, float m0, float m1, float m2, float s0, float s1, float s2,
    unsigned short* __restrict__ out) {
  const int g = w / patch;
  const int pp2 = patch * patch;
  const long rows = (long)n * (h / patch) * g;
  // quad of consecutive cols
  long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long quads_per_row = kpad / 4;
  const long row = q / quads_per_row;
  if (row >= rows) return;
  const int col0 = (int)(q - row * quads_per_row) * 4;
  const float mean[3] = {m0, m1, m2};
  const float stdev[3] = {s0, s1, s2};
  const long f = row / ((h / patch) * g);
  const int pr = (int)(row - f * (h / patch) * g);
  const int ph = pr / g, pw = pr % g;
  u16x4 o = {0, 0, 0, 0};
  const bool quad_fast = (patch % 4 == 0) && (col0 + 4 <= 3 * pp2);
  if (quad_fast) {
    const int c = col0 / pp2;
    const int r = col0 - c * pp2;
    const int ky = r / patch, kx = r % patch;  // kx % 4 == 0 when P%4==0
    const long y = (long)ph * patch + ky;
    const long x = (long)pw * patch + kx;
    const unsigned char* px = in + (((size_t)f * h + y) * w + x) * 3;
#pragma unroll
    for (int j = 0; j < 4; j++)
      o[j] = pp_bf16((float)px[3 * j + c] / 255.0f, mean[c], stdev[c]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int col = col0 + j;
      if (col >= 3 * pp2) break;  // zero pad
      const int c = col / pp2;
      const int r = col - c * pp2;
      const int ky = r / patch, kx = r % patch;
      const long y = (long)ph * patch + ky;
      const long x = (long)pw * patch + kx;
      o[j] = pp_bf16((float)in[(((size_t)f * h + y) * w + x) * 3 + c] / 255.0f,
                     mean[c], stdev[c]);
    }
  }
  *(u16x4*)(out + row * kpad + col0) = o;
}

// 16-col-per-thread variant for patch % 16 == 0 and 16B-aligned rows
// ((3*w) % 16 == 0, e.g. 224/256-px frames): the source span for 16
// consecutive kernel columns of one channel is 48 contiguous bytes at a
// 16-byte-aligned address, so the 16 scalar u8 loads collapse into
// three uint4 loads and the 4 u16x4 stores into two u16x8 stores —
// ~4x fewer VMEM instructions per output for this issue-bound kernel.
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

__global__ void k_clip_preprocess_patches16(
    const unsigned char* __restrict__ in, int n, int h, int w, int patch,
    int kpad, float m0, float m1, float m2, float s0, float s1, float s2,
    unsigned short* __restrict__ out) {
  const int g = w / patch;
  const int pp2 = patch * patch;
  const long rows = (long)n * (h / patch) * g;
  long q = (long)blockIdx.x * blockDim.x + threadIdx.x;  // 16-col groups
  const long grp_per_row = kpad / 16;
  const long row = q / grp_per_row;
  if (row >= rows) return;
  const int col0 = (int)(q - row * grp_per_row) * 16;
  const float mean[3] = {m0, m1, m2};
  const float stdev[3] = {s0, s1, s2};
  const long f = row / ((h / patch) * g);
  const int pr = (int)(row - f * (h / patch) * g);
  const int ph = pr / g, pw = pr % g;
  const int c = col0 / pp2;          // pp2 % 16 == 0: group in one channel
  const int r = col0 - c * pp2;
  const int ky = r / patch, kx = r % patch;  // kx % 16 == 0
  const long y = (long)ph * patch + ky;
  const long x = (long)pw * patch + kx;
  const unsigned char* px = in + (((size_t)f * h + y) * w + x) * 3;
  // 48 B = 16 pixels' worth of the interleaved RGB row, 16B-aligned.
  // Extraction uses CONSTANT word/byte indices per unrolled channel
  // branch (a runtime-indexed local byte array would spill the whole
  // block to scratch — measured 1860 vs 1119 us before this form).
  unsigned int wv[12];
  *(uint4*)(wv) = *(const uint4*)(px);
  *(uint4*)(wv + 4) = *(const uint4*)(px + 16);
  *(uint4*)(wv + 8) = *(const uint4*)(px + 32);
  u16x8 o0, o1;
#define CC_PPJ(c_)                                                          \
  _Pragma("unroll") for (int j = 0; j < 16; j++) {                          \
    const int idx = 3 * j + (c_);                                           \
    const unsigned int byte = (wv[idx >> 2] >> (8 * (idx & 3))) & 0xffu;    \
    const unsigned short val =                                              \
        pp_bf16((float)byte / 255.0f, mean[c_], stdev[c_]);                 \
    if (j < 8) o0[j] = val;                                                 \
    else o1[j - 8] = val;                                                   \
  }
  if (c == 0) {
    CC_PPJ(0)
  } else if (c == 1) {
    CC_PPJ(1)
  } else {
    CC_PPJ(2)
  }
#undef CC_PPJ
  *(u16x8*)(out + row * kpad + col0) = o0;
  *(u16x8*)(out + row * kpad + col0 + 8) = o1;
}

// ---------------- gather + duplicate broadcast ----------------
__global__ void k_gather_frames_u8(const unsigned char* __restrict__ frames,
                                   size_t frame_bytes,
                                   const int32_t* __restrict__ out_src,
                                   int total_out,
                                   unsigned char* __restrict__ out) {
  // out_src[j] = source frame index for output j (prefix-expanded on host)
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)total_out * frame_bytes;
  if (idx >= total) return;
  long b = idx % (long)frame_bytes;
  int j = idx / (long)frame_bytes;
  out[idx] = frames[(size_t)out_src[j] * frame_bytes + b];
}

// ---------------- YUV launcher ----------------
// argument checks of every YUV entry point (all before any launch)
int yuv420sp_check(const void* y, const void* uv, const void* out, int n,
                   int h, int w, size_t pitch, int bit_depth, int matrix,
                   int full_range) {
  if (!y || !uv || !out)
    return cc::set_error(CC_ERR_INVALID, "yuv420sp: null pointer");
  if (n <= 0 || h <= 0 || w <= 0)
    return cc::set_error(CC_ERR_INVALID, "yuv420sp: non-positive size n=%d "
                         "h=%d w=%d", n, h, w);
  if ((h & 1) || (w & 1))
    return cc::set_error(CC_ERR_INVALID,
                         "yuv420sp: 4:2:0 needs even dims (got %dx%d)", w, h);
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12)
    return cc::set_error(CC_ERR_INVALID,
                         "yuv420sp: bit_depth must be 8, 10 or 12 (got %d)",
                         bit_depth);
  if (matrix < 0 || matrix > 2)
    return cc::set_error(CC_ERR_INVALID, "yuv420sp: matrix must be 0 (bt601), "
                         "1 (bt709) or 2 (bt2020) (got %d)", matrix);
  if (full_range != 0 && full_range != 1)
    return cc::set_error(CC_ERR_INVALID,
                         "yuv420sp: full_range must be 0 or 1 (got %d)",
                         full_range);
  const size_t bps = bit_depth == 8 ? 1 : 2;
  if (pitch < (size_t)w * bps)
    return cc::set_error(CC_ERR_INVALID, "yuv420sp: pitch %zu < row bytes %zu",
                         pitch, (size_t)w * bps);
  if (bps == 2 && ((pitch | (size_t)y | (size_t)uv) & 1))
    return cc::set_error(CC_ERR_INVALID, "yuv420sp: 16-bit planes need an "
                         "even pitch and 2-byte-aligned pointers");
  return CC_OK;
}

// The launches of one checked call for sample type T: the fused kernel
// when `resize`, else the vector body and/or the scalar kernel.
template <typename T, typename P>
int yuv420sp_run(const char* name, const unsigned char* y,
                 const unsigned char* uv, int n, int h, int w, size_t pitch,
                 const P& p, bool bt601_limited, unsigned char* out,
                 bool resize, int out_h, int out_w, uint64_t stream) {
  const hipStream_t s = (hipStream_t)stream;
  const dim3 block(256);
  auto blocks = [](long threads) {
    return dim3((unsigned)((threads + 255) / 256));
  };
  if (resize)
    return cc::timed_launch(name, stream, [&] {
      const dim3 grid = blocks((long)n * out_h * out_w);
      if constexpr (sizeof(T) == 1 && std::is_same_v<P, YuvParams>) {
        if (bt601_limited) {
          hipLaunchKernelGGL((k_yuv420sp_to_rgb_resize<T, YuvBt601Limited8>),
                             grid, block, 0, s, y, uv, n, h, w, pitch,
                             YuvBt601Limited8{}, out, out_h, out_w);
          return;
        }
      }
      hipLaunchKernelGGL((k_yuv420sp_to_rgb_resize<T, P>), grid, block, 0,
                         s, y, uv, n, h, w, pitch, p, out, out_h, out_w);
    });
  // 16-byte-aligned planes and pitch: 8-pixel runs go through the vector
  // kernel and only the w % 8 row tails through the scalar one
  const bool aligned = (((size_t)y | (size_t)uv | pitch) & 15) == 0;
  const int x_vec = aligned ? (w / 8) * 8 : 0;
  if (x_vec > 0) {
    int rc = cc::timed_launch(name, stream, [&] {
      hipLaunchKernelGGL((k_yuv420sp_to_rgb_v8<T, P>),
                         blocks((long)n * h * (w / 8)), block, 0, s, y, uv, n,
                         h, w, pitch, p, out);
    });
    if (rc != CC_OK) return rc;
  }
  if (x_vec < w)
    return cc::timed_launch(name, stream, [&] {
      hipLaunchKernelGGL((k_yuv420sp_to_rgb_px<T, P>),
                         blocks((long)n * h * (w - x_vec)), block, 0, s, y, uv,
                         n, h, w, x_vec, pitch, p, out);
    });
  return CC_OK;
}

// the tone-mapping arguments of the cc_yuv420sp_hdr_* entries
struct HdrArgs {
  const void* tables;  // device copy of the cc_hdr_tables_build image
  float inv_w2;
};

// The one launcher behind cc_yuv420sp_to_rgb*, cc_nv12_to_rgb* (which pass
// (8, 0, 0)) and cc_yuv420sp_hdr_to_rgb* (which pass `hdr`): checks, the
// conversion parameters, and the choice of instantiation.  `name` is the
// caller's timing name.
int yuv420sp_launch(const char* name, const void* y, const void* uv, int n,
                    int h, int w, size_t pitch, int bit_depth, int matrix,
                    int full_range, void* out, bool resize, int out_h,
                    int out_w, uint64_t stream,
                    const HdrArgs* hdr = nullptr) {
  int rc = yuv420sp_check(y, uv, out, n, h, w, pitch, bit_depth, matrix,
                          full_range);
  if (rc != CC_OK) return rc;
  if (resize && (out_h <= 0 || out_w <= 0))
    return cc::set_error(CC_ERR_INVALID,
                         "yuv420sp: non-positive output size %dx%d", out_w,
                         out_h);
  if (hdr && (!hdr->tables || ((size_t)hdr->tables & 15)))
    return cc::set_error(CC_ERR_INVALID, "yuv420sp_hdr: tables must be a "
                         "non-null, 16-byte-aligned device pointer");
  if (hdr && !(hdr->inv_w2 >= 0.0f && hdr->inv_w2 <= FLT_MAX))
    return cc::set_error(CC_ERR_INVALID, "yuv420sp_hdr: inv_w2 must be finite "
                         "and non-negative (got %g)", (double)hdr->inv_w2);
  const YuvParams p{bit_depth == 8 ? 0 : 16 - bit_depth,
                    1.0f / (float)(1 << (bit_depth - 8)),
                    kYuvCoef[matrix][full_range ? 1 + (bit_depth - 8) / 2 : 0]};
  const unsigned char* yb = (const unsigned char*)y;
  const unsigned char* uvb = (const unsigned char*)uv;
  if (hdr) {
    const YuvHdrParams hp{
        p, (const float*)hdr->tables,
        (const unsigned char*)hdr->tables + kHdrTableEntries * sizeof(float),
        hdr->inv_w2};
    auto run = bit_depth == 8 ? yuv420sp_run<uint8_t, YuvHdrParams>
                              : yuv420sp_run<uint16_t, YuvHdrParams>;
    return run(name, yb, uvb, n, h, w, pitch, hp, false, (unsigned char*)out,
               resize, out_h, out_w, stream);
  }
  auto run = bit_depth == 8 ? yuv420sp_run<uint8_t, YuvParams>
                            : yuv420sp_run<uint16_t, YuvParams>;
  return run(name, yb, uvb, n, h, w, pitch, p, matrix == 0 && !full_range,
             (unsigned char*)out, resize, out_h, out_w, stream);
}

}  // namespace

extern "C" {

int cc_hip_available(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return cc::set_error(CC_ERR_HIP, "no HIP device (%s)",
                         e == hipSuccess ? "count=0" : hipGetErrorString(e));
  return CC_OK;
}

int cc_malloc(void** dptr, size_t bytes) {
  CC_CHECK_HIP(hipMalloc(dptr, bytes));
  return CC_OK;
}
int cc_free(void* dptr) {
  CC_CHECK_HIP(hipFree(dptr));
  return CC_OK;
}
int cc_memcpy_h2d(void* dst, const void* src, size_t bytes, uint64_t stream) {
  CC_CHECK_HIP(hipMemcpyHtoDAsync((hipDeviceptr_t)dst, const_cast<void*>(src),
                                  bytes, (hipStream_t)stream));
  return CC_OK;
}
int cc_memcpy_d2h(void* dst, const void* src, size_t bytes, uint64_t stream) {
  CC_CHECK_HIP(hipMemcpyDtoHAsync(dst, (hipDeviceptr_t)const_cast<void*>(src),
                                  bytes, (hipStream_t)stream));
  return CC_OK;
}
int cc_stream_sync(uint64_t stream) {
  CC_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  return CC_OK;
}

int cc_timing_enable(int enable) {
  cc::timing().enabled = enable != 0;
  return CC_OK;
}
int cc_timing_reset(void) {
  cc::timed_drain();  // release any pending events
  auto& ts = cc::timing();
  std::lock_guard<std::mutex> lk(ts.mu);
  ts.entries.clear();
  return CC_OK;
}
int cc_timing_report(const char* kernel, double* total_ms, int64_t* count) {
  cc::timed_drain();
  auto& ts = cc::timing();
  std::lock_guard<std::mutex> lk(ts.mu);
  auto it = ts.entries.find(kernel);
  if (it == ts.entries.end()) {
    if (total_ms) *total_ms = 0;
    if (count) *count = 0;
    return CC_OK;
  }
  if (total_ms) *total_ms = it->second.total_ms;
  if (count) *count = it->second.count;
  return CC_OK;
}

int cc_nv12_to_rgb(const void* y, const void* uv, int n, int h, int w,
                   size_t pitch, void* out_rgb, uint64_t stream) {
  return yuv420sp_launch("nv12_to_rgb", y, uv, n, h, w, pitch, 8, 0, 0,
                         out_rgb, false, 0, 0, stream);
}

int cc_nv12_to_rgb_resize(const void* y, const void* uv, int n, int src_h,
                          int src_w, size_t pitch, void* out_rgb, int out_h,
                          int out_w, uint64_t stream) {
  return yuv420sp_launch("nv12_to_rgb_resize", y, uv, n, src_h, src_w, pitch,
                         8, 0, 0, out_rgb, true, out_h, out_w, stream);
}

int cc_yuv420sp_to_rgb(const void* y, const void* uv, int n, int h, int w,
                       size_t pitch_bytes, int bit_depth, int matrix,
                       int full_range, void* out_rgb, uint64_t stream) {
  return yuv420sp_launch("yuv420sp_to_rgb", y, uv, n, h, w, pitch_bytes,
                         bit_depth, matrix, full_range, out_rgb, false, 0, 0,
                         stream);
}

int cc_yuv420sp_to_rgb_resize(const void* y, const void* uv, int n, int src_h,
                              int src_w, size_t pitch_bytes, int bit_depth,
                              int matrix, int full_range, void* out_rgb,
                              int out_h, int out_w, uint64_t stream) {
  return yuv420sp_launch("yuv420sp_to_rgb_resize", y, uv, n, src_h, src_w,
                         pitch_bytes, bit_depth, matrix, full_range, out_rgb,
                         true, out_h, out_w, stream);
}

int cc_hdr_tables_build(int transfer, float reference_white_nits,
                        void* host_out) {
  if (!host_out) return cc::set_error(CC_ERR_INVALID, "hdr tables: null out");
  if (transfer != CC_HDR_TRANSFER_PQ)
    return cc::set_error(CC_ERR_UNSUPPORTED, "hdr tables: transfer %d is not "
                         "built (1 = PQ is)", transfer);
  if (!(reference_white_nits > 0.0f && reference_white_nits <= FLT_MAX))
    return cc::set_error(CC_ERR_INVALID, "hdr tables: reference white must be "
                         "positive and finite (got %g)",
                         (double)reference_white_nits);
  // SMPTE ST 2084 EOTF, in double; each entry rounded once
  const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0;
  const double c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0,
               c3 = 2392.0 / 4096.0 * 32.0;
  float* tin = (float*)host_out;
  for (int i = 0; i < kHdrTableEntries; i++) {
    double nits = 0.0;
    if (i <= 4080) {
      const double e = pow(i / 4080.0, 1.0 / m2);
      nits = 10000.0 * pow(fmax(e - c1, 0.0) / (c2 - c3 * e), 1.0 / m1);
    }
    tin[i] = (float)(nits / (double)reference_white_nits);
  }
  unsigned char* tout = (unsigned char*)(tin + kHdrTableEntries);
  for (int j = 0; j < kHdrTableEntries; j++)
    tout[j] =
        (unsigned char)floor(255.0 * pow(j / 4095.0, 4.0 / 2.4) + 0.5);
  return CC_OK;
}

int cc_yuv420sp_hdr_to_rgb(const void* y, const void* uv, int n, int h, int w,
                           size_t pitch_bytes, int bit_depth, int matrix,
                           int full_range, const void* tables_dev,
                           float inv_w2, void* out_rgb, uint64_t stream) {
  const HdrArgs hdr{tables_dev, inv_w2};
  return yuv420sp_launch("yuv420sp_hdr_to_rgb", y, uv, n, h, w, pitch_bytes,
                         bit_depth, matrix, full_range, out_rgb, false, 0, 0,
                         stream, &hdr);
}

int cc_yuv420sp_hdr_to_rgb_resize(const void* y, const void* uv, int n,
                                  int src_h, int src_w, size_t pitch_bytes,
                                  int bit_depth, int matrix, int full_range,
                                  const void* tables_dev, float inv_w2,
                                  void* out_rgb, int out_h, int out_w,
                                  uint64_t stream) {
  const HdrArgs hdr{tables_dev, inv_w2};
  return yuv420sp_launch("yuv420sp_hdr_to_rgb_resize", y, uv, n, src_h, src_w,
                         pitch_bytes, bit_depth, matrix, full_range, out_rgb,
                         true, out_h, out_w, stream, &hdr);
}

int cc_resize_bilinear_u8(const void* in, int n, int src_h, int src_w,
                          void* out, int dst_h, int dst_w, uint64_t stream) {
  if (!in || !out || n <= 0) return cc::set_error(CC_ERR_INVALID, "bad args");
  long total = (long)n * dst_h * dst_w;
  dim3 block(256), grid((total + 255) / 256);
  return cc::timed_launch("resize_bilinear_u8", stream, [&] {
    hipLaunchKernelGGL(k_resize_bilinear_u8, grid, block, 0,
                       (hipStream_t)stream, (const unsigned char*)in, n, src_h,
                       src_w, (unsigned char*)out, dst_h, dst_w);
  });
}

int cc_resize_bicubic_u8(const void* in, int n, int src_h, int src_w, void* out,
                         int dst_h, int dst_w, uint64_t stream) {
  if (!in || !out || n <= 0) return cc::set_error(CC_ERR_INVALID, "bad args");
  long total = (long)n * dst_h * dst_w;
  dim3 block(256), grid((total + 255) / 256);
  return cc::timed_launch("resize_bicubic_u8", stream, [&] {
    hipLaunchKernelGGL(k_resize_bicubic_u8, grid, block, 0,
                       (hipStream_t)stream, (const unsigned char*)in, n, src_h,
                       src_w, (unsigned char*)out, dst_h, dst_w);
  });
}

int cc_resize_aa_table_build(int filter, int in_size, int out_size,
                             int crop_off, int crop_len, void* host_out,
                             size_t host_out_bytes, int* taps_out) {
  if (filter != CC_RESIZE_AA_BILINEAR && filter != CC_RESIZE_AA_BICUBIC)
    return cc::set_error(CC_ERR_INVALID, "resize_aa table: filter must be 0 "
                         "(bilinear) or 1 (bicubic) (got %d)", filter);
  if (in_size <= 0 || out_size <= 0)
    return cc::set_error(CC_ERR_INVALID, "resize_aa table: non-positive size "
                         "%d -> %d", in_size, out_size);
  if (crop_off < 0 || crop_len <= 0 || crop_len > out_size - crop_off)
    return cc::set_error(CC_ERR_INVALID, "resize_aa table: crop [%d, %d+%d) "
                         "outside [0, %d]", crop_off, crop_off, crop_len,
                         out_size);
  // torch's _compute_indices_min_size_weights_aa, align_corners=False, in
  // double; each weight rounded to f32 once
  const double interp = filter == CC_RESIZE_AA_BICUBIC ? 4.0 : 2.0;
  const double scale = (double)in_size / (double)out_size;
  const double support = scale >= 1.0 ? interp / 2.0 * scale : interp / 2.0;
  const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
  const double taps_d = 2.0 * ceil(support) + 1.0;
  if (taps_d > (double)(1 << 24))
    return cc::set_error(CC_ERR_INVALID, "resize_aa table: %d -> %d needs "
                         "%.0f taps", in_size, out_size, taps_d);
  const int taps = (int)taps_d;
  const size_t bytes = (size_t)crop_len * (2 + (size_t)taps) * 4;
  if (bytes > (size_t)INT32_MAX)
    return cc::set_error(CC_ERR_INVALID, "resize_aa table: %zu bytes", bytes);
  if (taps_out) *taps_out = taps;
  if (!host_out) return (int)bytes;
  if (host_out_bytes < bytes)
    return cc::set_error(CC_ERR_INVALID, "resize_aa table: buffer of %zu "
                         "bytes, %zu needed", host_out_bytes, bytes);
  int32_t* first = (int32_t*)host_out;
  int32_t* count = first + crop_len;
  float* w = (float*)(count + crop_len);
  std::vector<double> ws((size_t)taps);
  for (int n = 0; n < crop_len; n++) {
    const double center = scale * ((double)(crop_off + n) + 0.5);
    const int lo = std::max((int)(center - support + 0.5), 0);
    const int cnt = std::min((int)(center + support + 0.5), in_size) - lo;
    double total = 0.0;
    for (int j = 0; j < cnt; j++) {
      const double x = fabs(((double)(j + lo) - center + 0.5) * invscale);
      double v = 0.0;
      if (filter == CC_RESIZE_AA_BILINEAR) {
        if (x < 1.0) v = 1.0 - x;
      } else {
        const double A = -0.5;  // torch's antialias value, not cv2's -0.75
        if (x < 1.0)
          v = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
        else if (x < 2.0)
          v = A * (((x - 5.0) * x + 8.0) * x - 4.0);
      }
      ws[j] = v;
      total += v;
    }
    first[n] = lo;
    count[n] = cnt;
    for (int j = 0; j < taps; j++)
      w[(size_t)n * taps + j] = j < cnt ? (float)(ws[j] / total) : 0.0f;
  }
  return (int)bytes;
}

int cc_resize_aa_u8(const void* in, int n, int src_h, int src_w, void* out,
                    int out_h, int out_w, const void* table_y_dev, int taps_y,
                    const void* table_x_dev, int taps_x, uint64_t stream) {
  if (!in || !out || !table_y_dev || !table_x_dev)
    return cc::set_error(CC_ERR_INVALID, "resize_aa: null pointer");
  if (n <= 0 || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0 ||
      taps_y <= 0 || taps_x <= 0)
    return cc::set_error(CC_ERR_INVALID, "resize_aa: non-positive size n=%d "
                         "src %dx%d out %dx%d taps %d, %d", n, src_w, src_h,
                         out_w, out_h, taps_y, taps_x);
  if ((((size_t)table_y_dev | (size_t)table_x_dev) & 3) != 0)
    return cc::set_error(CC_ERR_INVALID,
                         "resize_aa: tables must be 4-byte aligned");
  if (taps_y > CC_RESIZE_AA_MAX_TAPS || taps_x > CC_RESIZE_AA_MAX_TAPS)
    return cc::set_error(CC_ERR_UNSUPPORTED, "resize_aa: taps %d, %d above "
                         "%d", taps_y, taps_x, CC_RESIZE_AA_MAX_TAPS);
  const long blocks_x = (out_w + kAaBC - 1) / kAaBC;
  const long bands = (out_h + kAaBR - 1) / kAaBR;
  const long groups = blocks_x * bands * (long)n;
  if (groups > (long)INT32_MAX)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "resize_aa: %ld workgroups do not fit one launch",
                         groups);
  return cc::timed_launch("resize_aa_u8", stream, [&] {
    hipLaunchKernelGGL(k_resize_aa_u8, dim3((unsigned)groups),
                       dim3(kAaThreads), 0, (hipStream_t)stream,
                       (const unsigned char*)in, n, src_h, src_w,
                       (unsigned char*)out, out_h, out_w,
                       (const int32_t*)table_y_dev, taps_y,
                       (const int32_t*)table_x_dev, taps_x, (int)blocks_x,
                       (int)bands);
  });
}

int cc_clip_preprocess(const void* in, int n, int h, int w, const float mean[3],
                       const float stdev[3], void* out, int out_dtype,
                       uint64_t stream) {
  if (!in || !out || !mean || !stdev || n <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad args");
  if (out_dtype != 0 && out_dtype != 1)
    return cc::set_error(CC_ERR_INVALID, "out_dtype must be 0(f32)|1(bf16)");
  long total = (long)n * h * w;
  dim3 block(256), grid((total + 255) / 256);
  dim3 gridq(((total + 3) / 4 + 255) / 256);  // bf16: 4 pixels per thread
  return cc::timed_launch("clip_preprocess", stream, [&] {
    if (out_dtype == 0)
      hipLaunchKernelGGL(k_clip_preprocess_f32, grid, block, 0,
                         (hipStream_t)stream, (const unsigned char*)in, n, h,
                         w, mean[0], mean[1], mean[2], stdev[0], stdev[1],
                         stdev[2], (float*)out);
    else
      hipLaunchKernelGGL(k_clip_preprocess_bf16, gridq, block, 0,
                         (hipStream_t)stream, (const unsigned char*)in, n, h,
                         w, mean[0], mean[1], mean[2], stdev[0], stdev[1],
                         stdev[2], (unsigned short*)out);
  });
}

int cc_clip_preprocess_patches(const void* in, int n, int h, int w, int patch,
                               int kpad, const float mean[3],
                               const float stdev[3], void* out,
                               uint64_t stream) {
  if (!in || !out || !mean || !stdev || n <= 0 || patch <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad args");
  if (h % patch != 0 || w % patch != 0 || kpad % 64 != 0 ||
      kpad < 3 * patch * patch)
    return cc::set_error(CC_ERR_UNSUPPORTED,
                         "need h,w %% patch == 0 and kpad %% 64 == 0, >= 3*P*P");
  const long rows = (long)n * (h / patch) * (w / patch);
  const long pp2 = (long)patch * patch;
  // 16 columns per thread where the kernel's alignment conditions hold,
  // 4 everywhere else
  const bool cols16 = patch % 16 == 0 && (3 * w) % 16 == 0 && kpad == 3 * pp2;
  const long threads = rows * (kpad / (cols16 ? 16 : 4));
  dim3 block(256), grid((unsigned)((threads + 255) / 256));
  return cc::timed_launch("clip_preprocess", stream, [&] {
    if (cols16)
      hipLaunchKernelGGL(k_clip_preprocess_patches16, grid, block, 0,
                         (hipStream_t)stream, (const unsigned char*)in, n, h,
                         w, patch, kpad, mean[0], mean[1], mean[2], stdev[0],
                         stdev[1], stdev[2], (unsigned short*)out);
    else
      hipLaunchKernelGGL(k_clip_preprocess_patches, grid, block, 0,
                         (hipStream_t)stream, (const unsigned char*)in, n, h,
                         w, patch, kpad, mean[0], mean[1], mean[2], stdev[0],
                         stdev[1], stdev[2], (unsigned short*)out);
  });
}

int cc_gather_frames_u8(const void* frames, int n_in, size_t frame_bytes,
                        const int32_t* idx, const int32_t* counts, int n_idx,
                        int total_out, void* out, uint64_t stream) {
  if (!frames || !idx || !counts || !out || n_idx <= 0 || total_out <= 0)
    return cc::set_error(CC_ERR_INVALID, "bad args");
  // expand (idx, counts) -> per-output source index on host (tiny),
  // upload, then one flat copy kernel.
  std::vector<int32_t> src(total_out);
  int pos = 0;
  for (int i = 0; i < n_idx; i++) {
    if (idx[i] < 0 || idx[i] >= n_in)
      return cc::set_error(CC_ERR_INVALID, "idx out of range");
    for (int c = 0; c < counts[i] && pos < total_out; c++) src[pos++] = idx[i];
  }
  if (pos != total_out)
    return cc::set_error(CC_ERR_INVALID, "counts sum != total_out");
  int32_t* d_src = nullptr;
  CC_CHECK_HIP(hipMalloc(&d_src, total_out * sizeof(int32_t)));
  CC_CHECK_HIP(hipMemcpyHtoDAsync((hipDeviceptr_t)d_src, src.data(),
                                  total_out * sizeof(int32_t),
                                  (hipStream_t)stream));
  long total = (long)total_out * (long)frame_bytes;
  dim3 block(256), grid((total + 255) / 256);
  int rc = cc::timed_launch("gather_frames_u8", stream, [&] {
    hipLaunchKernelGGL(k_gather_frames_u8, grid, block, 0, (hipStream_t)stream,
                       (const unsigned char*)frames, frame_bytes, d_src,
                       total_out, (unsigned char*)out);
  });
  // free after the kernel: synchronize the stream (gather is not on the
  // steady-state hot loop; clip selection happens once per clip batch)
  hipStreamSynchronize((hipStream_t)stream);
  hipFree(d_src);
  return rc;
}

}  // extern "C"
