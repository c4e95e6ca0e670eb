// The motion filter's score without a flow field.
//
// check_if_small_motion (pipelines/video/filtering/motion/
// motion_filter_stages.py; motion_vector_backend.py:85-313) paints every
// motion vector's block into a dense (frames, H, W, 2) f32 field — a mask, a
// nonzero, broadcast index tensors and an index_put_ per block size — then
// takes a norm, two reductions and an interpolate.  Of that field the score
// needs one sum and 2 oh x 2 ow pixels a frame, so here it never exists:
//
//   k_ms_zero, k_ms_count, k_ms_scan, k_ms_fill   bin rows by 64 x 32 tile
//   k_ms_paint    one workgroup a (frame, tile): owner map in LDS -> one f64
//                 partial sum and the tile's bilinear taps
//   k_ms_blocks   the same two outputs straight from cc_motion_estimate's
//                 int16 block field (no bins, no owner map)
//   k_ms_finish   one workgroup a clip: the two scores
//
// ---- which row owns a pixel -------------------------------------------------
// A row paints only if (w, h) is exactly (8,8), (16,16), (16,8) or (8,16); its
// `pass` is that position.  Its pixels are trunc(clamp(dst + o, 0, N-1)) for o
// in [-b/2, b/2), the add in f32, every offset evaluated on its own as the
// product does (consecutive f32 sums need not truncate to consecutive
// integers), so a block centred outside the frame paints the edge it clamps
// onto.  Where several rows cover a pixel the winner is the row with the
// highest (pass, row index in its frame): what the product's and the
// reference's loop over block sizes yields when index_put_ writes
// sequentially — passes in BLOCK_OPTIONS order, the later row winning inside a
// pass.  It is NOT the order oracle/motion.py paints in across different block
// sizes, which is pure row order; the two agree wherever only same-size
// blocks overlap and wherever nothing overlaps.  The rule is an integer
// maximum, key = (pass + 1) << 28 | row in frame, so the order in which rows
// reach a pixel is irrelevant: bins need no order and LDS atomicMax needs no
// lock.  Key 0 is "nobody": magnitude 0.
//
// ---- binning ----------------------------------------------------------------
// One thread a row: the frame by binary search in frame_offsets, the extent
// from the first and last offset of either axis (f32 add is monotone, so
// every pixel lies between them; 16 pixels at most, so 2 x 2 tiles at most),
// an integer atomic into counts[frame][tile].  One workgroup a frame turns a
// frame's counts into starts (exclusive scan); a frame's bins begin at
// 4 * its first row, so no scan crosses frames and a bin is as deep as the
// rows that land in it.  The fill kernel recomputes the extent and takes its
// slots by counting the counts back down to zero.
//
// ---- paint ------------------------------------------------------------------
// 256 threads.  The owner map is [32][80] keys (10 KB; the 16-word pad puts
// the four 16-pixel rows a wave paints at once into 64 distinct banks).  Each
// wave takes every fourth bin entry and its lanes take the row's w * h
// offsets 64 at a time.  After the barrier thread t resolves pixels
// (t & 63, (t >> 6) + 4 i): key -> row -> motion, scale -> f32 magnitude
// sqrt(dx^2 + dy^2) / (H + W), reloading only when the key changes; sums them
// in f64 in that order; wave shuffle tree, four waves through LDS, one f64
// partial a (frame, tile).  The tile's share of the frame's 2 oh x 2 ow tap
// pixels is looked up in the same owner map.  Pixels of the tile outside the
// frame are never painted (pixels are clamped into the frame) and add 0.  A
// tile with an empty bin skips the map and writes zeros.
//
// Out of bounds: offsets are clamped to [0, n_rows] / [0, n_frames]; a row is
// binned only if it lies inside its frame's range, so a frame's bin entries
// number at most 4 x its rows and a key's row index is below n_rows; pixels
// are clamped in f32 and again as integers (NaN paints pixel 0).

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_motionscore_plan.hpp"
#include "cc_timing.hpp"

namespace {

constexpr int TW = cc::MS_TILE_W, TH = cc::MS_TILE_H;
constexpr int OWN_STRIDE = TW + 16;
constexpr int NT = cc::MS_BLOCK;
constexpr unsigned ROW_MASK = (1u << cc::MS_KEY_ROW_BITS) - 1;
static_assert(TW == 64 && TH == 32 && NT == 256,
              "the resolve pass maps a wave onto a tile row");

__device__ __forceinline__ long clampl(long v, long lo, long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// the pixel offset o of a block centred on d paints, on an axis of n pixels
__device__ __forceinline__ int pix(float d, int o, int n) {
  float v = d + (float)o;
  v = fminf(fmaxf(v, 0.0f), (float)(n - 1));
  const int p = (int)v;
  return p < 0 ? 0 : (p > n - 1 ? n - 1 : p);
}

// position of (w, h) in BLOCK_OPTIONS, -1 if the row paints nothing
__device__ __forceinline__ int block_pass(float bw, float bh) {
  if (bw == 8.0f) return bh == 8.0f ? 0 : (bh == 16.0f ? 3 : -1);
  if (bw == 16.0f) return bh == 16.0f ? 1 : (bh == 8.0f ? 2 : -1);
  return -1;
}

// f32 magnitude of row `r`: |-motion / scale| / (H + W)
__device__ __forceinline__ float row_mag(const float* __restrict__ r, float hw) {
  float s = r[9];
  s = s == 0.0f ? 1.0f : s;
  const float dx = -r[7] / s, dy = -r[8] / s;
  return sqrtf(dx * dx + dy * dy) / hw;
}

// tap i of an axis of n pixels scaled to o: source pixel of output i >> 1,
// the lower one if i is even; oracle/motion.py::_bilinear_resize_f32
__device__ __forceinline__ int tap_coord(int i, int n, int o, float* wgt) {
  const double s = ((i >> 1) + 0.5) * ((double)n / (double)o) - 0.5;
  const long c0 = clampl((long)floor(s), 0, n - 1);
  const long c1 = c0 + 1 < n ? c0 + 1 : n - 1;
  const double f = s - (double)c0;
  if (wgt) *wgt = (float)(f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f));
  return (int)((i & 1) ? c1 : c0);
}

// sum over the workgroup in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double wg_sum(double v, double* red) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- binning ----------------------------------------------------------------

__global__ __launch_bounds__(NT) void k_ms_zero(int* __restrict__ counts, long n) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i < n) counts[i] = 0;
}

// row r -> its frame, its index in the frame and the tiles its extent
// touches; false if it paints nothing or lies outside its frame's range
__device__ __forceinline__ bool row_tiles(const float* __restrict__ rows,
                                          const long long* __restrict__ foff,
                                          long r, long n_rows, int n_frames,
                                          int H, int W, int* f, int* rif,
                                          long* fbase, int* tx0, int* tx1,
                                          int* ty0, int* ty1) {
  const float* row = rows + r * 10;
  const float bw = row[0], bh = row[1];
  if (block_pass(bw, bh) < 0) return false;
  // the last frame whose first row is <= r
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (int)(((long)lo + hi + 1) >> 1);
    if (foff[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const long a = clampl(foff[lo], 0, n_rows), b = clampl(foff[lo + 1], 0, n_rows);
  if (r < a || r >= b || r - a > (long)ROW_MASK) return false;
  *f = lo;
  *rif = (int)(r - a);
  *fbase = a;
  const int w2 = (int)bw / 2, h2 = (int)bh / 2;
  *tx0 = pix(row[4], -w2, W) / TW;
  *tx1 = pix(row[4], w2 - 1, W) / TW;
  *ty0 = pix(row[5], -h2, H) / TH;
  *ty1 = pix(row[5], h2 - 1, H) / TH;
  return true;
}

__global__ __launch_bounds__(NT) void k_ms_count(
    const float* __restrict__ rows, const long long* __restrict__ foff,
    long n_rows, int n_frames, int H, int W, int T, int tiles_x,
    int* __restrict__ counts) {
  const long r = (long)blockIdx.x * NT + threadIdx.x;
  if (r >= n_rows) return;
  int f, rif, tx0, tx1, ty0, ty1;
  long fbase;
  if (!row_tiles(rows, foff, r, n_rows, n_frames, H, W, &f, &rif, &fbase, &tx0,
                 &tx1, &ty0, &ty1))
    return;
  for (int ty = ty0; ty <= ty1; ty++)
    for (int tx = tx0; tx <= tx1; tx++)
      atomicAdd(&counts[(long)f * T + ty * tiles_x + tx], 1);
}

// starts[f][0..T] = exclusive scan of counts[f][0..T)
__global__ __launch_bounds__(cc::MS_SCAN_BLOCK) void k_ms_scan(
    const int* __restrict__ counts, int T, int* __restrict__ starts) {
  __shared__ int sc[cc::MS_SCAN_BLOCK];
  const int tid = threadIdx.x;
  const int* cnt = counts + (long)blockIdx.x * T;
  int* st = starts + (long)blockIdx.x * (T + 1);
  int carry = 0;
  if (tid == 0) st[0] = 0;
  for (int base = 0; base < T; base += cc::MS_SCAN_BLOCK) {
    const int t = base + tid;
    sc[tid] = t < T ? cnt[t] : 0;
    __syncthreads();
    for (int s = 1; s < cc::MS_SCAN_BLOCK; s <<= 1) {
      const int v = tid >= s ? sc[tid - s] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    if (t < T) st[t + 1] = carry + sc[tid];
    carry += sc[cc::MS_SCAN_BLOCK - 1];
    __syncthreads();
  }
}

// counts the counts back down: the value before the decrement, less one, is
// a slot of the bin nobody else gets
__global__ __launch_bounds__(NT) void k_ms_fill(
    const float* __restrict__ rows, const long long* __restrict__ foff,
    long n_rows, int n_frames, int H, int W, int T, int tiles_x,
    int* __restrict__ counts, const int* __restrict__ starts,
    int* __restrict__ bins) {
  const long r = (long)blockIdx.x * NT + threadIdx.x;
  if (r >= n_rows) return;
  int f, rif, tx0, tx1, ty0, ty1;
  long fbase;
  if (!row_tiles(rows, foff, r, n_rows, n_frames, H, W, &f, &rif, &fbase, &tx0,
                 &tx1, &ty0, &ty1))
    return;
  for (int ty = ty0; ty <= ty1; ty++)
    for (int tx = tx0; tx <= tx1; tx++) {
      const int t = ty * tiles_x + tx;
      const int slot = atomicSub(&counts[(long)f * T + t], 1) - 1;
      bins[4 * fbase + starts[(long)f * (T + 1) + t] + slot] = rif;
    }
}

// ---- paint ------------------------------------------------------------------

__global__ __launch_bounds__(NT) void k_ms_paint(
    const float* __restrict__ rows, const long long* __restrict__ foff,
    long n_rows, int H, int W, int T, int tiles_x, int oh, int ow,
    const int* __restrict__ starts, const int* __restrict__ bins,
    double* __restrict__ partial, float* __restrict__ taps) {
  __shared__ unsigned own[TH * OWN_STRIDE];
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int f = blockIdx.x / T, t = blockIdx.x % T;
  const int x0 = (t % tiles_x) * TW, y0 = (t / tiles_x) * TH;
  const long fbase = clampl(foff[f], 0, n_rows);
  const float* frows = rows + fbase * 10;
  const int b0 = starts[(long)f * (T + 1) + t];
  const int cnt = starts[(long)f * (T + 1) + t + 1] - b0;
  const int* bin = bins + 4 * fbase + b0;
  const float hw = (float)(H + W);

  double sum = 0.0;
  if (cnt > 0) {  // uniform over the workgroup
    for (int i = tid; i < TH * OWN_STRIDE; i += NT) own[i] = 0;
    __syncthreads();
    for (int e = wid; e < cnt; e += NT / 64) {
      const int rif = bin[e];
      const float* row = frows + (long)rif * 10;
      const float bwf = row[0], bhf = row[1], dx = row[4], dy = row[5];
      const int bw = (int)bwf, bh = (int)bhf;
      const unsigned key =
          ((unsigned)(block_pass(bwf, bhf) + 1) << cc::MS_KEY_ROW_BITS) |
          (unsigned)rif;
      const int sh = bw == 8 ? 3 : 4;
      for (int i = lane; i < bw * bh; i += 64) {
        const int lx = pix(dx, (i & (bw - 1)) - bw / 2, W) - x0;
        const int ly = pix(dy, (i >> sh) - bh / 2, H) - y0;
        if ((unsigned)lx < (unsigned)TW && (unsigned)ly < (unsigned)TH)
          atomicMax(&own[ly * OWN_STRIDE + lx], key);
      }
    }
    __syncthreads();
    unsigned last = 0;
    float mag = 0.0f;
#pragma unroll
    for (int i = 0; i < TH / (NT / 64); i++) {
      const unsigned key = own[(wid + (NT / 64) * i) * OWN_STRIDE + lane];
      if (key != last) {
        last = key;
        mag = key ? row_mag(frows + (long)(key & ROW_MASK) * 10, hw) : 0.0f;
      }
      sum += (double)mag;
    }
  }
  sum = wg_sum(sum, red);
  if (tid == 0) partial[blockIdx.x] = sum;

  const int ntaps = 4 * oh * ow;
  for (int k = tid; k < ntaps; k += NT) {
    const int lx = tap_coord(k % (2 * ow), W, ow, nullptr) - x0;
    const int ly = tap_coord(k / (2 * ow), H, oh, nullptr) - y0;
    if ((unsigned)lx < (unsigned)TW && (unsigned)ly < (unsigned)TH) {
      const unsigned key = cnt > 0 ? own[ly * OWN_STRIDE + lx] : 0u;
      taps[(long)f * ntaps + k] =
          key ? row_mag(frows + (long)(key & ROW_MASK) * 10, hw) : 0.0f;
    }
  }
}

// ---- estimated blocks -------------------------------------------------------
// 16 x 16 blocks tile the frame, so pixel (y, x) belongs to block (y/16, x/16)
// (the pixels a partial last block clamps onto are its own) and
// |delta| = sqrt(dx^2 + dy^2): blocks_to_mv_rows writes motion = 4 d, scale 4.
// Workgroup (frame, part) sums |d| * area(block & frame) over 1024 blocks;
// part 0 also looks the frame's taps up.

__device__ __forceinline__ float est_mag(const short* __restrict__ field,
                                         long block, float hw) {
  const short2 d = *(const short2*)(field + 2 * block);
  const float dx = -(float)d.x, dy = -(float)d.y;
  return sqrtf(dx * dx + dy * dy) / hw;
}

__global__ __launch_bounds__(NT) void k_ms_blocks(
    const short* __restrict__ field, int H, int W, int P, int oh, int ow,
    double* __restrict__ partial, float* __restrict__ taps) {
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / P, part = blockIdx.x % P;
  const int nbx = (W + 15) / 16, nby = (H + 15) / 16, nb = nbx * nby;
  const short* ff = field + (long)f * nb * 2;
  const float hw = (float)(H + W);
  double sum = 0.0;
#pragma unroll
  for (int q = 0; q < cc::MS_EST_PER_WG / NT; q++) {
    const int b = part * cc::MS_EST_PER_WG + q * NT + tid;
    if (b < nb) {
      const int by = b / nbx, bx = b % nbx;
      const int aw = W - 16 * bx < 16 ? W - 16 * bx : 16;
      const int ah = H - 16 * by < 16 ? H - 16 * by : 16;
      sum += (double)est_mag(ff, b, hw) * (double)(aw * ah);
    }
  }
  sum = wg_sum(sum, red);
  if (tid == 0) partial[blockIdx.x] = sum;
  if (part != 0) return;
  const int ntaps = 4 * oh * ow;
  for (int k = tid; k < ntaps; k += NT) {
    const int x = tap_coord(k % (2 * ow), W, ow, nullptr);
    const int y = tap_coord(k / (2 * ow), H, oh, nullptr);
    taps[(long)f * ntaps + k] = est_mag(ff, (long)(y / 16) * nbx + x / 16, hw);
  }
}

// ---- finish -----------------------------------------------------------------
// One workgroup a clip.  global_mean: thread t adds partials t, t + 256, ... of
// the clip's frames (they are contiguous), then the fixed tree.
// per_patch_min: thread t takes patches t, t + 256, ...; a tap's temporal
// mean is its f64 sum over the frames in frame order / n, rounded to f32; the
// blend is _bilinear_resize_f32's, f32 weights, top and bottom row first.

__global__ __launch_bounds__(NT) void k_ms_finish(
    const double* __restrict__ partial, const float* __restrict__ taps,
    const int* __restrict__ coff, int n_frames, int P, int H, int W, int oh,
    int ow, double* __restrict__ out) {
  __shared__ double red[NT / 64];
  __shared__ float redm[NT / 64];
  const int tid = threadIdx.x;
  const long f0 = clampl(coff[blockIdx.x], 0, n_frames);
  const long f1 = clampl(coff[blockIdx.x + 1], 0, n_frames);
  const long n = f1 - f0;
  if (n <= 0) {  // uniform
    if (tid < 2) out[2 * (long)blockIdx.x + tid] = 0.0;
    return;
  }
  double s = 0.0;
  for (long i = f0 * P + tid; i < f1 * P; i += NT) s += partial[i];
  s = wg_sum(s, red);

  const int ntaps = 4 * oh * ow;
  auto mean = [&](int ty, int tx) {
    const float* p = taps + f0 * ntaps + (long)ty * 2 * ow + tx;
    double a = 0.0;
    for (long f = 0; f < n; f++) a += (double)p[f * ntaps];
    return (float)(a / (double)n);
  };
  float m = INFINITY;
  for (int q = tid; q < oh * ow; q += NT) {
    const int i = q / ow, j = q % ow;
    float wy, wx;
    tap_coord(2 * i, H, oh, &wy);
    tap_coord(2 * j, W, ow, &wx);
    const float top = mean(2 * i, 2 * j) * (1.0f - wx) + mean(2 * i, 2 * j + 1) * wx;
    const float bot =
        mean(2 * i + 1, 2 * j) * (1.0f - wx) + mean(2 * i + 1, 2 * j + 1) * wx;
    const float v = top * (1.0f - wy) + bot * wy;
    m = v < m ? v : m;
  }
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const float o = __shfl_xor(m, sft);
    m = o < m ? o : m;
  }
  if ((tid & 63) == 0) redm[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < NT / 64; k++) m = redm[k] < m ? redm[k] : m;
    out[2 * (long)blockIdx.x] = (double)m;
    out[2 * (long)blockIdx.x + 1] = s / ((double)n * (double)H * (double)W);
  }
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

int launch_finish(const cc_motion_score_plan_info& plan, const double* partial,
                  const float* taps, const void* clip_offsets, int64_t n_frames,
                  int P, int64_t h, int64_t w, int64_t oh, int64_t ow, void* out,
                  uint64_t stream) {
  return cc::timed_launch("motion_score_finish", stream, [&] {
    hipLaunchKernelGGL(k_ms_finish, dim3(plan.finish_grid), dim3(plan.block), 0,
                       (hipStream_t)stream, partial, taps,
                       (const int*)clip_offsets, (int)n_frames, P, (int)h,
                       (int)w, (int)oh, (int)ow, (double*)out);
  });
}

}  // namespace

extern "C" int cc_motion_score_plan(int64_t n_frames, int64_t n_rows,
                                    int64_t n_clips, int64_t h, int64_t w,
                                    int64_t oh, int64_t ow,
                                    cc_motion_score_plan_info* out) {
  if (!out)
    return cc::set_error(CC_ERR_INVALID, "cc_motion_score_plan: null out");
  return cc::motion_score_plan(n_frames, n_rows, n_clips, h, w, oh, ow, out);
}

extern "C" int cc_motion_score_rows(
    const void* rows_f32, const void* frame_offsets_i64,
    const void* clip_offsets_i32, int64_t n_rows, int64_t n_frames,
    int64_t n_clips, int64_t h, int64_t w, int64_t oh, int64_t ow,
    void* out_f64, void* workspace, int64_t workspace_bytes, uint64_t stream) {
  cc_motion_score_plan_info plan;
  int rc = cc::motion_score_plan(n_frames, n_rows, n_clips, h, w, oh, ow, &plan);
  if (rc != CC_OK) return rc;
  if ((n_rows > 0 && !rows_f32) || !frame_offsets_i64 || !clip_offsets_i32 ||
      !out_f64 || !workspace || misaligned(rows_f32, 4) ||
      misaligned(frame_offsets_i64, 8) || misaligned(clip_offsets_i32, 4) ||
      misaligned(out_f64, 8) || misaligned(workspace, 16))
    return cc::set_error(CC_ERR_INVALID,
                         "motion_score_rows: null or misaligned pointer");
  if (workspace_bytes < plan.workspace_bytes)
    return cc::set_error(CC_ERR_INVALID,
                         "motion_score_rows workspace %lld < %lld bytes",
                         (long long)workspace_bytes,
                         (long long)plan.workspace_bytes);
  char* ws = (char*)workspace;
  double* partial = (double*)ws;
  float* taps = (float*)(ws + plan.partial_bytes);
  int* counts = (int*)(ws + plan.partial_bytes + plan.tap_bytes);
  int* starts = (int*)((char*)counts + plan.count_bytes);
  int* bins = (int*)((char*)starts + plan.start_bytes);
  const float* rows = (const float*)rows_f32;
  const long long* foff = (const long long*)frame_offsets_i64;
  const hipStream_t st = (hipStream_t)stream;
  const int T = plan.tiles_per_frame;
  if (n_frames > 0) {
    rc = cc::timed_launch("motion_score_bin", stream, [&] {
      hipLaunchKernelGGL(k_ms_zero, dim3(plan.zero_grid), dim3(plan.block), 0,
                         st, counts, (long)(n_frames * T));
    });
    if (rc != CC_OK) return rc;
    if (n_rows > 0) {
      rc = cc::timed_launch("motion_score_bin", stream, [&] {
        hipLaunchKernelGGL(k_ms_count, dim3(plan.bin_grid), dim3(plan.block), 0,
                           st, rows, foff, (long)n_rows, (int)n_frames, (int)h,
                           (int)w, T, plan.tiles_x, counts);
      });
      if (rc != CC_OK) return rc;
    }
    rc = cc::timed_launch("motion_score_bin", stream, [&] {
      hipLaunchKernelGGL(k_ms_scan, dim3(plan.scan_grid), dim3(plan.scan_block),
                         0, st, (const int*)counts, T, starts);
    });
    if (rc != CC_OK) return rc;
    if (n_rows > 0) {
      rc = cc::timed_launch("motion_score_bin", stream, [&] {
        hipLaunchKernelGGL(k_ms_fill, dim3(plan.bin_grid), dim3(plan.block), 0,
                           st, rows, foff, (long)n_rows, (int)n_frames, (int)h,
                           (int)w, T, plan.tiles_x, counts, (const int*)starts,
                           bins);
      });
      if (rc != CC_OK) return rc;
    }
    rc = cc::timed_launch("motion_score_paint", stream, [&] {
      hipLaunchKernelGGL(k_ms_paint, dim3(plan.paint_grid), dim3(plan.block), 0,
                         st, rows, foff, (long)n_rows, (int)h, (int)w, T,
                         plan.tiles_x, (int)oh, (int)ow, (const int*)starts,
                         (const int*)bins, partial, taps);
    });
    if (rc != CC_OK) return rc;
  }
  return launch_finish(plan, partial, taps, clip_offsets_i32, n_frames, T, h, w,
                       oh, ow, out_f64, stream);
}

extern "C" int cc_motion_score_blocks(
    const void* field_i16, const void* clip_offsets_i32, int64_t n_frames,
    int64_t n_clips, int64_t h, int64_t w, int64_t oh, int64_t ow,
    void* out_f64, void* workspace, int64_t workspace_bytes, uint64_t stream) {
  cc_motion_score_plan_info plan;
  int rc = cc::motion_score_plan(n_frames, 0, n_clips, h, w, oh, ow, &plan);
  if (rc != CC_OK) return rc;
  if ((n_frames > 0 && !field_i16) || !clip_offsets_i32 || !out_f64 ||
      !workspace || misaligned(field_i16, 4) || misaligned(clip_offsets_i32, 4) ||
      misaligned(out_f64, 8) || misaligned(workspace, 16))
    return cc::set_error(CC_ERR_INVALID,
                         "motion_score_blocks: null or misaligned pointer");
  if (workspace_bytes < plan.est_workspace_bytes)
    return cc::set_error(CC_ERR_INVALID,
                         "motion_score_blocks workspace %lld < %lld bytes",
                         (long long)workspace_bytes,
                         (long long)plan.est_workspace_bytes);
  double* partial = (double*)workspace;
  float* taps = (float*)((char*)workspace + plan.est_partial_bytes);
  if (n_frames > 0) {
    rc = cc::timed_launch("motion_score_blocks", stream, [&] {
      hipLaunchKernelGGL(k_ms_blocks, dim3(plan.est_grid), dim3(plan.block), 0,
                         (hipStream_t)stream, (const short*)field_i16, (int)h,
                         (int)w, plan.est_partials, (int)oh, (int)ow, partial,
                         taps);
    });
    if (rc != CC_OK) return rc;
  }
  return launch_finish(plan, partial, taps, clip_offsets_i32, n_frames,
                       plan.est_partials, h, w, oh, ow, out_f64, stream);
}
