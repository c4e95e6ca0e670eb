// Block-matching motion estimation on luma — hand-written HIP for gfx950.
//
// Replaces the motion-vector source of the motion filter:
//   decode_for_motion (codec side data)   motion_vector_backend.py:169-250
// rocDecode exposes no motion vectors, so the per-block displacement field
// is estimated from the NV12/P016 luma the device path already carries.
//
// ARITHMETIC CONTRACT (all integer; bit-exact vs tests/motion_est_ref.py):
//   Y8(s)  = s for 1-byte samples, s >> 8 for 2-byte (P016, MSB-aligned)
//   grid   = ceil(h/16) x ceil(w/16) blocks of 16x16
//   C(y,x) = Y8(cur[min(y,h-1)][min(x,w-1)])
//   R(y,x) = Y8(ref[clamp(y,0,h-1)][clamp(x,0,w-1)])
//   SAD(by,bx,dx,dy) = sum_{j,i<16} |C(16by+j,16bx+i) - R(16by+j+dy,16bx+i+dx)|
//   cost   = SAD + lambda*(|dx|+|dy|),  dx,dy in [-range, range]
//   winner = lexicographic minimum of (cost, dx^2+dy^2, dy, dx)
// The winner is the minimum of a total order, so it does not depend on the
// order candidates are evaluated or reduced in; no atomics anywhere.
//
// One 256-thread workgroup per block.  The (16+2R)^2 reference window and
// the 16x16 current block are staged once into LDS as Y8 bytes with
// clamped loads (<= 6.9 KB at R=32), so the search loop has no bounds
// checks.  Candidates are spread over lanes with dx fastest: neighbouring
// lanes read the same or neighbouring LDS dwords (broadcast / distinct
// banks).  Per candidate row: 5 aligned dword reads, 4 v_alignbyte_b32 to
// shift to the candidate column, 4 v_sad_u8 (4 pixels each) against the
// current block held in 64 registers.

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_timing.hpp"

namespace {

constexpr int kBlk = 16;
constexpr int kMaxRange = 32;
constexpr int kMaxRows = kBlk + 2 * kMaxRange;         // 80 window rows
constexpr int kMaxRowDw = (kMaxRows + 3) / 4 + 1;      // 21 dwords per row

// window row length in dwords: the 16+2R bytes rounded up, plus one dword
// so the 5-dword read of the last candidate column stays inside the row
__host__ __device__ constexpr int row_dwords(int range) {
  return (kBlk + 2 * range + 3) / 4 + 1;
}

// Four Y8 samples of one row at columns clamp(x0..x0+3, 0, w-1), packed
// little-endian.  Runs wholly inside the row at a naturally aligned
// address take one vector load; everything else loads sample by sample, so
// nothing beyond sample alignment is assumed of pointers or pitch.
template <typename T>
__device__ __forceinline__ unsigned load4_y8(const unsigned char* row, int x0,
                                             int w) {
  if (x0 >= 0 && x0 + 3 < w) {
    const T* p = (const T*)row + x0;
    if constexpr (sizeof(T) == 1) {
      if (((size_t)p & 3) == 0) return *(const unsigned*)p;
    } else {
      if (((size_t)p & 7) == 0) {
        uint2 v = *(const uint2*)p;
        return ((v.x >> 8) & 0xffu) | ((v.x >> 24) << 8) |
               (((v.y >> 8) & 0xffu) << 16) | ((v.y >> 24) << 24);
      }
    }
  }
  unsigned out = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int x = min(max(x0 + k, 0), w - 1);
    unsigned s = ((const T*)row)[x];
    if constexpr (sizeof(T) == 2) s >>= 8;
    out |= s << (8 * k);
  }
  return out;
}

template <typename T>
__global__ __launch_bounds__(256) void k_motion_estimate(
    const unsigned char* cur, const unsigned char* ref, int h, int w,
    size_t pitch, size_t frame_stride, int range, int lambda,
    short* __restrict__ mv_out, unsigned* __restrict__ cost_out) {
  __shared__ unsigned s_win[kMaxRows * kMaxRowDw];
  __shared__ unsigned s_cur[kBlk * kBlk / 4];
  __shared__ unsigned long long s_best[4];

  const int tid = threadIdx.x;
  const int bx = blockIdx.x, by = blockIdx.y, f = blockIdx.z;
  const unsigned char* cf = cur + (size_t)f * frame_stride;
  const unsigned char* rf = ref + (size_t)f * frame_stride;
  const int rows = kBlk + 2 * range;
  const int sdw = row_dwords(range);

  // stage the edge-replicated reference window (pad dwords included, so
  // every LDS dword the search reads is initialised) and the current block
  for (int i = tid; i < rows * sdw; i += 256) {
    int r = i / sdw, c = i - r * sdw;
    int y = min(max(by * kBlk - range + r, 0), h - 1);
    s_win[i] = load4_y8<T>(rf + (size_t)y * pitch, bx * kBlk - range + 4 * c, w);
  }
  if (tid < kBlk * kBlk / 4) {
    int y = min(by * kBlk + (tid >> 2), h - 1);
    s_cur[tid] = load4_y8<T>(cf + (size_t)y * pitch, bx * kBlk + 4 * (tid & 3), w);
  }
  __syncthreads();

  unsigned c[kBlk * kBlk / 4];
#pragma unroll
  for (int k = 0; k < kBlk * kBlk / 4; k++) c[k] = s_cur[k];

  // key = cost:38 | dx^2+dy^2:12 | dy+32:7 | dx+32:7 — integer order of
  // the key is the lexicographic order of the contract
  unsigned long long best = ~0ull;
  const int side = 2 * range + 1;
  for (int cand = tid; cand < side * side; cand += 256) {
    const int oy = cand / side, ox = cand - oy * side;
    const unsigned* p = s_win + oy * sdw + (ox >> 2);
    const unsigned sh = ox & 3;
    unsigned sad = 0;
#pragma unroll
    for (int j = 0; j < kBlk; j++) {
      unsigned d[5];
#pragma unroll
      for (int k = 0; k < 5; k++) d[k] = p[j * sdw + k];
#pragma unroll
      for (int k = 0; k < 4; k++)
        sad = __builtin_amdgcn_sad_u8(
            c[4 * j + k], __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh), sad);
    }
    const int dx = ox - range, dy = oy - range;
    const unsigned cost = sad + (unsigned)lambda * (unsigned)(abs(dx) + abs(dy));
    const unsigned long long key =
        ((unsigned long long)cost << 26) |
        ((unsigned long long)(dx * dx + dy * dy) << 14) |
        ((unsigned long long)(dy + kMaxRange) << 7) |
        (unsigned long long)(dx + kMaxRange);
    best = key < best ? key : best;
  }

  // fixed-order reduction: butterfly inside each wave, then 4 waves via LDS
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    unsigned long long o = __shfl_xor(best, off, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < 4; k++) best = s_best[k] < best ? s_best[k] : best;
    const size_t blk = ((size_t)f * gridDim.y + by) * gridDim.x + bx;
    mv_out[2 * blk] = (short)((int)(best & 127) - kMaxRange);
    mv_out[2 * blk + 1] = (short)((int)((best >> 7) & 127) - kMaxRange);
    if (cost_out) cost_out[blk] = (unsigned)(best >> 26);
  }
}

}  // namespace

extern "C" {

int cc_motion_estimate(const void* cur, const void* ref, int n, int h, int w,
                       size_t pitch_bytes, size_t frame_stride_bytes,
                       int bytes_per_sample, int search_range, int lambda,
                       void* mv_out, void* cost_out, uint64_t stream) {
  if (!cur || !ref || !mv_out)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: null pointer");
  if (n <= 0 || h <= 0 || w <= 0)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: non-positive size "
                         "n=%d h=%d w=%d", n, h, w);
  if (search_range < 1 || search_range > kMaxRange)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: search_range must "
                         "be 1..%d (got %d)", kMaxRange, search_range);
  if (lambda < 0 || lambda > 255)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: lambda must be "
                         "0..255 (got %d)", lambda);
  if (bytes_per_sample != 1 && bytes_per_sample != 2)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: bytes_per_sample "
                         "must be 1 or 2 (got %d)", bytes_per_sample);
  const size_t bps = (size_t)bytes_per_sample;
  if (pitch_bytes < (size_t)w * bps)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: pitch %zu < row "
                         "bytes %zu", pitch_bytes, (size_t)w * bps);
  if (frame_stride_bytes < pitch_bytes * (size_t)h)
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: frame stride %zu < "
                         "plane bytes %zu", frame_stride_bytes,
                         pitch_bytes * (size_t)h);
  if (bps == 2 &&
      ((pitch_bytes | frame_stride_bytes | (size_t)cur | (size_t)ref) & 1))
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: 16-bit planes need "
                         "an even pitch, an even frame stride and 2-byte-"
                         "aligned pointers");
  if (((size_t)mv_out & 1) || ((size_t)cost_out & 3))
    return cc::set_error(CC_ERR_INVALID, "motion_estimate: mv_out must be "
                         "2-byte and cost_out 4-byte aligned");
  const long nbx = ((long)w + kBlk - 1) / kBlk, nby = ((long)h + kBlk - 1) / kBlk;
  // grid (nbx, nby, n): y and z are 16-bit, and the runtime caps a launch
  // at 2^32 threads in all
  if (nby > 65535 || n > 65535 || nbx * nby * (long)n * 256 >= (1L << 32))
    return cc::set_error(CC_ERR_UNSUPPORTED, "motion_estimate: %ld x %ld "
                         "blocks x %d pairs does not fit one launch", nbx, nby,
                         n);
  dim3 block(256), grid((unsigned)nbx, (unsigned)nby, (unsigned)n);
  return cc::timed_launch("motion_estimate", stream, [&] {
    if (bps == 1)
      hipLaunchKernelGGL(k_motion_estimate<uint8_t>, grid, block, 0,
                         (hipStream_t)stream, (const unsigned char*)cur,
                         (const unsigned char*)ref, h, w, pitch_bytes,
                         frame_stride_bytes, search_range, lambda,
                         (short*)mv_out, (unsigned*)cost_out);
    else
      hipLaunchKernelGGL(k_motion_estimate<uint16_t>, grid, block, 0,
                         (hipStream_t)stream, (const unsigned char*)cur,
                         (const unsigned char*)ref, h, w, pitch_bytes,
                         frame_stride_bytes, search_range, lambda,
                         (short*)mv_out, (unsigned*)cost_out);
  });
}

}  // extern "C"
