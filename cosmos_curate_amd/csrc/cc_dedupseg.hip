// The pruning scan of semantic dedup over every cluster at once.
//
// cc_pairwise_max_earlier (cc_dedup.hip) scans one cluster whose rows were
// gathered into scan order; semdedup() called it once a cluster, with a
// nonzero, a sort, a gather, a normalise and a count read back around every
// call (SemDedupActor.dedup, pipelines/video/dedup/dedup_actor.py:315-460, is
// the same loop).  Here e stays in its original order, `order` maps scan
// positions to rows, `offsets` cuts the positions into segments, and three
// launches whose grids depend on (m, d, k) alone do all segments:
//
//   k_pairwise_seg_prefix   work items per segment, prefix-summed  (1 workgroup)
//   k_pairwise_seg          persistent grid over the work list
//   k_pairwise_seg_combine  merges the partials of j-tiles cut into chunks
//
// ---- work list --------------------------------------------------------------
// Segment c of L positions has T = ceil(L/128) j-tiles; j-tile t needs the
// i-tiles 0..t and is cut into ceil((t+1)/C) items of at most C i-tiles (C
// from the plan, cc_dedup_plan.hpp).  A segment therefore has
// C q (q+1)/2 + r (q+1) items, q = T / C, r = T % C; the prologue writes the
// prefix of these counts (segments this rank does not own count zero), and a
// workgroup turns item number w into (segment, j-tile, chunk) with a binary
// search over the prefix and a walk over at most PS_MAX_CHUNKS groups of C
// j-tiles.  Nothing is read back and no grid is sized from the offsets: the
// grid is fixed and strides over prefix[k] items.
//
// ---- one item: k_kmeans_assign with the earlier rows as centroids ----------
// 4 waves, 2 (i halves) x 2 (j halves), each a 64 x 64 block as four 32x32
// accumulators of the exact-f32 MFMA v_mfma_f32_32x32x2_f32.  i rows are the
// A operand and j rows the B operand, so an accumulator lane stands for ONE j
// position (column lane&31) and its 16 registers for 16 i positions: the
// running (best, index) is two pairs a lane, kept in registers across all
// i-tiles of the item.  After the last i-tile lanes l and l^32 meet in one
// shuffle, the two i-half waves in 2 KiB of LDS, and thread r writes j
// position r: to maxv/argi if the j-tile is one item, else to slice `chunk` of
// the partials.  Ties go to the smallest i: a lane meets its i positions in
// ascending order and replaces only on >, every merge compares indices on
// equality, and the combine kernel merges chunks in ascending order with the
// same rule.  The strict i < j mask only bites on the diagonal tile (i-tile ==
// j-tile), where it is a compare of tile-local positions; it also hides the
// zero rows staged past the segment's end, which can only lie in the diagonal
// tile above every valid j.
//
// Data movement is the assign kernel's: d in chunks of 32 columns, LDS
// double-buffered, global -> registers (8 float4 a thread, issued before the
// step's 64 MFMAs) -> LDS (after them), one barrier a step, the (i-tile,
// chunk) steps of an item one flat sequence.  Rows are gathered through
// `order`: a thread stages 4 rows of each tile, 8 threads cover a row's 128
// bytes, so the gather costs nothing in coalescing.  The j rows' indices are
// loaded once an item, an i-tile's indices one tile ahead so no row load waits
// on an index load.  Both tiles row-major [128][36] f32; lane l reads one
// float4 (columns kk + 4*(l>>5) .. +3 of row l&31) and spends it on four
// consecutive MFMAs; with a 36-dword stride the 16 lanes a ds_read_b128 serves
// at a time start at sixteen distinct multiples of 4 banks: conflict-free (the
// derivation is in cc_kmeans.hip).  The reduce scratch has its own 2 KiB
// behind the tiles, so the next item may stage while slow threads still write.
//
// Out of bounds: offsets are clamped to [0, m], positions past a segment's end
// and order values outside [0, m) are staged as zeros and never dereferenced,
// and a partial slice index is below the plan's max_chunks because no segment
// is longer than m.

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_dedup_plan.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int TS = cc::PS_TILE;
constexpr int DK = cc::PS_DK;
constexpr int LS = DK + 4;     // LDS row stride in floats
constexpr int TILE = TS * LS;  // floats of one staged tile
static_assert(TS == 128 && DK == 32 && cc::PS_BLOCK == 256,
              "the wave split and the staging slots assume this tile");

// take candidate (v, i) over (bv, bi) if larger, or equal with a smaller index
__device__ __forceinline__ void take_better(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// segment c as (first scan position, length), clamped into [0, m]
__device__ __forceinline__ void seg_range(const int* __restrict__ off, long c,
                                          long m, long& a, long& L) {
  long x = off[c], y = off[c + 1];
  x = x < 0 ? 0 : (x > m ? m : x);
  y = y < 0 ? 0 : (y > m ? m : y);
  a = x;
  L = y > x ? y - x : 0;
}

__device__ __forceinline__ long long seg_items(long L, int C) {
  const long long T = (L + TS - 1) / TS, q = T / C, r = T % C;
  return C * q * (q + 1) / 2 + r * (q + 1);
}

__global__ __launch_bounds__(cc::PS_PREFIX_BLOCK) void k_pairwise_seg_prefix(
    const int* __restrict__ off, long k, long m, int C, int seg_first,
    int seg_step, long long* __restrict__ prefix) {
  __shared__ long long sc[cc::PS_PREFIX_BLOCK];
  const int tid = threadIdx.x;
  long long carry = 0;
  if (tid == 0) prefix[0] = 0;
  for (long base = 0; base < k; base += cc::PS_PREFIX_BLOCK) {
    const long c = base + tid;
    long long n = 0;
    if (c < k && c % seg_step == seg_first) {
      long a, L;
      seg_range(off, c, m, a, L);
      n = seg_items(L, C);
    }
    sc[tid] = n;
    __syncthreads();
    for (int s = 1; s < cc::PS_PREFIX_BLOCK; s <<= 1) {
      const long long v = tid >= s ? sc[tid - s] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    if (c < k) prefix[c + 1] = carry + sc[tid];
    carry += sc[cc::PS_PREFIX_BLOCK - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(cc::PS_BLOCK, 2) void k_pairwise_seg(
    const float* __restrict__ e, long m, int d, const int* __restrict__ order,
    const int* __restrict__ off, int k, const long long* __restrict__ prefix,
    int C, float* __restrict__ maxv, int* __restrict__ argi,
    float* __restrict__ wsv, int* __restrict__ wsi, long slice) {
  // I tile [2][128][36], J tile [2][128][36], reduce scratch [4][128]: 75776 B
  __shared__ __attribute__((aligned(16))) float lds[4 * TILE + 4 * TS];
#define IT(b) (lds + (b) * TILE)
#define JT(b) (lds + (2 + (b)) * TILE)
  float* redv = lds + 4 * TILE;          // [2][128]
  int* redi = (int*)(redv + 2 * TS);     // [2][128]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l31 = lane & 31, h = lane >> 5;
  const int wid = tid >> 6;
  const int waveI = wid >> 1, waveJ = wid & 1;
  const int nchunk = d / DK;
  // staging slots: float4 q of this thread is row (tid>>3) + 32q, columns
  // 4*(tid&7)..+3 of the chunk; 8 threads cover a row's 128 bytes
  const int sr = tid >> 3, sc = (tid & 7) * 4;
  const int aoff = (waveI * 64 + l31) * LS + 4 * h;
  const int boff = (waveJ * 64 + l31) * LS + 4 * h;

  const long long total = prefix[k];
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    // ---- item w -> (segment, j-tile t, chunk): uniform over the workgroup
    int lo = 0, hi = k - 1;
    while (lo < hi) {
      const int mid = (int)(((long)lo + hi) >> 1);
      if (prefix[mid + 1] > w) hi = mid; else lo = mid + 1;
    }
    long a, L;
    seg_range(off, lo, m, a, L);
    long long rem = w - prefix[lo];
    int g = 0;  // group of C j-tiles, each cut into g + 1 chunks
    while (rem >= (long long)C * (g + 1)) {
      rem -= (long long)C * (g + 1);
      ++g;
    }
    const int nch = g + 1;
    const int t = g * C + (int)(rem / nch);
    const int chunk = (int)(rem % nch);
    const int it0 = chunk * C;
    const int it1 = it0 + C - 1 < t ? it0 + C - 1 : t;

    // rows of e behind this thread's 4 staging rows of tile `tile`; -1 = none
    auto load_idx = [&](int tile, int* r) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const long pos = (long)tile * TS + sr + 32 * q;
        r[q] = pos < L ? order[a + pos] : -1;
      }
    };
    int rj[4], ri[4], ri_next[4] = {-1, -1, -1, -1};
    load_idx(t, rj);
    load_idx(it0, ri);

    float4 pi[4], pj[4];
    auto fetch = [&](int ch) {
      const long col = (long)ch * DK + sc;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        pi[q] = (unsigned long)ri[q] < (unsigned long)m
                    ? *(const float4*)(e + (long)ri[q] * d + col)
                    : float4{0, 0, 0, 0};
        pj[q] = (unsigned long)rj[q] < (unsigned long)m
                    ? *(const float4*)(e + (long)rj[q] * d + col)
                    : float4{0, 0, 0, 0};
      }
    };
    auto stash = [&](int b) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        *(float4*)(IT(b) + (sr + 32 * q) * LS + sc) = pi[q];
        *(float4*)(JT(b) + (sr + 32 * q) * LS + sc) = pj[q];
      }
    };

    f32x16 acc[2][2] = {};  // [i sub-block][j sub-block]
    float bestv[2] = {-INFINITY, -INFINITY};
    int besti[2] = {0, 0};

    // buffer 0 was last read before the barrier that ended the previous item
    fetch(0);
    stash(0);
    __syncthreads();
    if (it0 < it1) load_idx(it0 + 1, ri_next);

    int buf = 0;
    for (int it = it0; it <= it1; it++) {
      for (int ch = 0; ch < nchunk; ch++) {
        const bool last_ch = ch + 1 == nchunk;
        const bool more = !(last_ch && it == it1);
        if (more) {
          if (last_ch) {
#pragma unroll
            for (int q = 0; q < 4; q++) ri[q] = ri_next[q];
          }
          fetch(last_ch ? 0 : ch + 1);
          if (last_ch && it + 2 <= it1) load_idx(it + 2, ri_next);
        }
        const float* A = IT(buf) + aoff;
        const float* B = JT(buf) + boff;
#pragma unroll
        for (int kk = 0; kk < DK; kk += 8) {
          const float4 a0 = *(const float4*)(A + kk);
          const float4 a1 = *(const float4*)(A + 32 * LS + kk);
          const float4 b0 = *(const float4*)(B + kk);
          const float4 b1 = *(const float4*)(B + 32 * LS + kk);
          const float av0[4] = {a0.x, a0.y, a0.z, a0.w};
          const float av1[4] = {a1.x, a1.y, a1.z, a1.w};
          const float bv0[4] = {b0.x, b0.y, b0.z, b0.w};
          const float bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int s = 0; s < 4; s++) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv0[s], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], bv1[s], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv0[s], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], bv1[s], acc[1][1], 0, 0, 0);
          }
        }
        // buf^1 was last read before the barrier that ended the previous step
        if (more) stash(buf ^ 1);
        __syncthreads();
        buf ^= 1;
      }
      // C/D map 32x32: column (j) = lane&31, row (i) = (reg&3) + 8*(reg>>2) +
      // 4*(lane>>5): ascending in reg, so > keeps the smallest i a lane sees.
      // Below the diagonal tile every i is earlier than every j.
      const bool diag = it == t;
#pragma unroll
      for (int ci = 0; ci < 2; ci++) {
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int il = waveI * 64 + ci * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
          const int gi = (int)((unsigned)it * TS + il);
#pragma unroll
          for (int cj = 0; cj < 2; cj++) {
            const int jl = waveJ * 64 + cj * 32 + l31;
            const float v = acc[ci][cj][reg];
            if (v > bestv[cj] && (!diag || il < jl)) {
              bestv[cj] = v;
              besti[cj] = gi;
            }
          }
        }
      }
#pragma unroll
      for (int ci = 0; ci < 2; ci++)
#pragma unroll
        for (int cj = 0; cj < 2; cj++) acc[ci][cj] = f32x16{};
    }

    // the two half-waves of a j position, then the two i-half waves
#pragma unroll
    for (int cj = 0; cj < 2; cj++) {
      const float ov = __shfl_xor(bestv[cj], 32);
      const int oi = __shfl_xor(besti[cj], 32);
      take_better(bestv[cj], besti[cj], ov, oi);
      if (h == 0) {
        const int r = waveJ * 64 + cj * 32 + l31;
        redv[waveI * TS + r] = bestv[cj];
        redi[waveI * TS + r] = besti[cj];
      }
    }
    __syncthreads();
    const long gj = (long)t * TS + tid;
    if (tid < TS && gj < L) {
      float bv = redv[tid];
      int bi = redi[tid];
      take_better(bv, bi, redv[TS + tid], redi[TS + tid]);
      const long p = a + gj;
      if (nch == 1) {
        if (gj == 0) {  // legacy: a segment's first row scores 0 against itself
          bv = 0.0f;
          bi = 0;
        }
        maxv[p] = bv;
        argi[p] = bi;
      } else {
        wsv[(long)chunk * slice + p] = bv;
        wsi[(long)chunk * slice + p] = bi;
      }
    }
  }
#undef IT
#undef JT
}

// one thread a scan position: a j-tile that was cut into chunks gets the best
// of its partials, merged in chunk order
__global__ __launch_bounds__(cc::PS_COMBINE_BLOCK) void k_pairwise_seg_combine(
    const int* __restrict__ off, int k, long m, int C, int seg_first,
    int seg_step, const float* __restrict__ wsv, const int* __restrict__ wsi,
    long slice, float* __restrict__ maxv, int* __restrict__ argi) {
  const long p = (long)blockIdx.x * cc::PS_COMBINE_BLOCK + threadIdx.x;
  if (p >= m) return;
  // the segment of position p: the last c with off[c] <= p
  int lo = 0, hi = k + 1;
  while (lo < hi) {
    const int mid = (int)(((long)lo + hi) >> 1);
    if (off[mid] <= p) lo = mid + 1; else hi = mid;
  }
  const int c = lo - 1;
  if (c < 0 || c >= k || c % seg_step != seg_first) return;
  long a, L;
  seg_range(off, c, m, a, L);
  if (p < a || p >= a + L) return;
  const int nch = (int)((p - a) / TS / C) + 1;
  if (nch == 1) return;  // written by its one item
  float bv = wsv[p];
  int bi = wsi[p];
  for (int s = 1; s < nch; s++)
    take_better(bv, bi, wsv[(long)s * slice + p], wsi[(long)s * slice + p]);
  maxv[p] = bv;
  argi[p] = bi;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" int cc_pairwise_seg_plan(int64_t m, int64_t d, int64_t k,
                                    cc_pairwise_seg_plan_info* out) {
  if (!out)
    return cc::set_error(CC_ERR_INVALID, "cc_pairwise_seg_plan: null out");
  return cc::pairwise_seg_plan(m, d, k, out);
}

extern "C" int64_t cc_pairwise_seg_workspace_bytes(int64_t m, int64_t d,
                                                   int64_t k) {
  cc_pairwise_seg_plan_info plan;
  const int rc = cc::pairwise_seg_plan(m, d, k, &plan);
  return rc != CC_OK ? rc : plan.workspace_bytes;
}

extern "C" int cc_pairwise_max_earlier_seg(
    const void* e_f32, int64_t m, int64_t d, const void* order_i32,
    const void* offsets_i32, int64_t k, int64_t seg_first, int64_t seg_step,
    void* maxv_f32, void* argi_i32, void* workspace, int64_t workspace_bytes,
    uint64_t stream) {
  if (!e_f32 || !order_i32 || !offsets_i32 || !maxv_f32 || !argi_i32 ||
      !workspace || misaligned(e_f32) || misaligned(workspace))
    return cc::set_error(CC_ERR_INVALID,
                         "pairwise_seg: null or misaligned pointer");
  cc_pairwise_seg_plan_info plan;
  int rc = cc::pairwise_seg_plan(m, d, k, &plan);
  if (rc != CC_OK) return rc;
  if (seg_step < 1 || seg_step > 0x7fffffffLL || seg_first < 0 ||
      seg_first >= seg_step)
    return cc::set_error(CC_ERR_INVALID,
                         "pairwise_seg: seg_first %lld not in [0, seg_step %lld)",
                         (long long)seg_first, (long long)seg_step);
  if (workspace_bytes < plan.workspace_bytes)
    return cc::set_error(CC_ERR_INVALID,
                         "pairwise_seg workspace %lld < %lld bytes",
                         (long long)workspace_bytes,
                         (long long)plan.workspace_bytes);
  long long* prefix = (long long*)workspace;
  const long slice = (long)((m + 3) / 4 * 4);
  float* wsv = (float*)((char*)workspace + plan.prefix_bytes);
  int* wsi = (int*)(wsv + (long)plan.max_chunks * slice);
  const hipStream_t st = (hipStream_t)stream;
  rc = cc::timed_launch("pairwise_seg_prefix", stream, [&] {
    hipLaunchKernelGGL(k_pairwise_seg_prefix, dim3(1), dim3(plan.prefix_block),
                       0, st, (const int*)offsets_i32, (long)k, (long)m,
                       plan.chunk_tiles, (int)seg_first, (int)seg_step, prefix);
  });
  if (rc != CC_OK) return rc;
  rc = cc::timed_launch("pairwise_seg", stream, [&] {
    hipLaunchKernelGGL(k_pairwise_seg, dim3(plan.grid), dim3(plan.block), 0, st,
                       (const float*)e_f32, (long)m, (int)d,
                       (const int*)order_i32, (const int*)offsets_i32, (int)k,
                       (const long long*)prefix, plan.chunk_tiles,
                       (float*)maxv_f32, (int*)argi_i32, wsv, wsi, slice);
  });
  if (rc != CC_OK || plan.max_chunks == 1) return rc;
  return cc::timed_launch("pairwise_seg_combine", stream, [&] {
    hipLaunchKernelGGL(k_pairwise_seg_combine, dim3(plan.combine_grid),
                       dim3(plan.combine_block), 0, st,
                       (const int*)offsets_i32, (int)k, (long)m,
                       plan.chunk_tiles, (int)seg_first, (int)seg_step,
                       (const float*)wsv, (const int*)wsi, slice,
                       (float*)maxv_f32, (int*)argi_i32);
  });
}
