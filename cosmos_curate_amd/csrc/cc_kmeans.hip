// One spherical k-means step for semantic dedup: assign, then accumulate.
//
// Replaces the per-iteration body of the k-means fit in front of the pruning
// scan (SemDedupActor.kmeans, pipelines/video/dedup/dedup_actor.py:182-313,
// cuML KMeansMG there; torch `e @ cent.T`, argmax, f64 index_add_ here until
// now).  The [k, d] normalise tail and the all-reduce stay in torch.
//
// ---- k_kmeans_assign: labels[i] = argmax_c e_i . cent_c --------------------
// Work split.  One workgroup of 4 waves owns 128 rows of e and marches over
// all ceil(k/128) centroid tiles; the scores live only in accumulators.  The
// waves are 2 (centroid halves) x 2 (row halves); each holds a 64 x 64 block
// as four 32x32 accumulators of the exact-f32 MFMA v_mfma_f32_32x32x2_f32
// (products and sums are f32; the result differs from an fmaf chain only in
// summation order).  Centroids are the A operand and rows of e the B operand,
// so an accumulator lane stands for ONE row of e (column lane&31) and its 16
// registers for 16 centroids: the running (best, index) is two pairs a lane,
// not one per register.  After the last tile lanes l and l^32 (same row) meet
// in one shuffle, the two centroid-half waves in 2 KiB of LDS, and thread r
// writes row r's label.  Ties go to the smallest index: a lane meets its
// centroids in ascending order and replaces only on >, and every merge of
// two candidates compares indices on equality.  Centroids c >= k are skipped
// at the compare (their staged rows are zeros, never read from memory), rows
// i >= m are staged as zeros and not written.
//
// Why this tile.  At (m, d, k) = (1M, 512, 1000) a step is 1.05 TFLOP: 6.8 ms
// at the 155 TF f32-MFMA ceiling.  A workgroup re-reads its 128 x d tile of e
// once per centroid tile, 8 x 2 GB = 16 GB from L2 / Infinity Cache / HBM,
// and all of cent (2 MB, L2-resident) once per row tile: per 32-column step a
// workgroup loads 32 KiB and issues 4 x 64 MFMAs of 64 cycles, i.e. 8 bytes a
// cycle a CU with two workgroups resident, 4.9 TB/s over 256 CUs at 2.4 GHz,
// half of it L2 hits.  So the kernel is MFMA-bound if the loads stay in
// flight, and the tile is chosen for issue rate: 64 x 64 a wave means one
// 16-byte A read and one 16-byte B read feed four MFMAs (below), and 73.7 KB
// of LDS lets two workgroups share a CU, so one's barrier and epilogue hide
// behind the other's MFMAs.  A 256-row tile would halve the centroid traffic
// that already hits L2 and cost the second workgroup.
//
// Data movement.  d is staged in chunks of 32 columns, LDS double-buffered,
// global -> registers (8 float4 a thread, issued before the step's MFMAs) ->
// LDS (after them), one barrier a step.  The (centroid tile, chunk) steps
// form one flat sequence, so the prefetch runs across tile boundaries.
//
// LDS layout.  Both tiles are row-major [128][36] f32: 32 columns and 4 of
// padding.  Which k index an MFMA step pairs is free as long as A and B
// agree, so lane l reads ONE float4, columns kk + 4*(l>>5) .. +3 of row l&31,
// and spends its four components on four consecutive MFMAs (step s pairs
// column kk+s from the lower half-wave with kk+4+s from the upper).  A
// ds_read_b128 is served 16 lanes at a time (8 on a 32-bank LDS); within
// such a group the lanes hold consecutive rows at one column offset, and
// with a row stride of 36 dwords row i starts at bank 36 i mod 64 = 0, 36, 8,
// 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28: sixteen distinct
// multiples of 4, so 16 lanes x 4 dwords cover 64 banks once (mod 32: 4 i,
// eight distinct).  Conflict-free by construction, against cc_dedup.hip's
// 64-dword stride that puts all 32 rows of a fragment on one bank.  Per 8
// columns a wave issues 4 ds_read_b128 and 16 MFMAs.
//
// ---- k_kmeans_accumulate + k_kmeans_combine: sums[c] = sum of c's rows -----
// Input is the stable sort of the labels (order) and the clusters' offsets
// into it; both come from torch (sort, searchsorted) with no host
// synchronisation.  The sorted positions are cut into pieces of 512, one
// workgroup each, whatever the labels are: k = 8 over 1M rows is 1954
// workgroups, and a 100k-row cluster among 1000 is 196 of them.  Thread t
// owns columns 4t..4t+3 (d/4 threads), so one gathered row is one coalesced
// read; rows are walked in order, 8 loads in flight, and added in order into
// four f64 accumulators.  At the end of a run (the cluster changes or the
// piece ends) the accumulator is stored: a run that is a whole cluster goes to
// sums[c]; a run whose cluster began before the piece goes to head[piece], one
// whose cluster goes on after it to tail[piece] (a piece inside one big
// cluster is all head).  k_kmeans_combine, one thread per (cluster, column),
// writes zeros for an empty cluster, leaves a cluster that lay in one piece
// alone, and otherwise adds tail[first piece] + head[following pieces] in
// piece order.  No floating-point atomics and no sum whose order depends on
// scheduling: same arguments, same bits.  Workspace: head and tail,
// 2 * ceil(m/512) * d doubles (cc_kmeans_plan.hpp).
// Offsets that are not a partition of [0, m) cannot take the kernels out of
// bounds: positions stay inside the piece, row indices outside [0, m) and
// clusters outside [0, k) are skipped.

#include <hip/hip_runtime.h>

#include "cc_common.hpp"
#include "cc_kmeans_plan.hpp"
#include "cc_timing.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int TR = cc::KM_TILE_ROWS;
constexpr int TC = cc::KM_TILE_CENTS;
constexpr int DK = cc::KM_DK;
constexpr int LS = DK + 4;       // LDS row stride in floats (see LDS layout)
constexpr int TILE = TR * LS;    // floats of one staged tile
constexpr int PIECE = cc::KM_PIECE;
static_assert(TR == 128 && TC == 128 && DK == 32 && cc::KM_BLOCK == 256,
              "the wave split and the staging slots assume this tile");

// take candidate (v, i) over (bv, bi) if larger, or equal with a smaller index
__device__ __forceinline__ void take_better(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__global__ __launch_bounds__(cc::KM_BLOCK, 2) void k_kmeans_assign(
    const float* __restrict__ e, long m, int d, const float* __restrict__ cent,
    int k, int* __restrict__ labels, float* __restrict__ best_out) {
  // E tile [2][128][36] then C tile [2][128][36]: 73728 B
  __shared__ __attribute__((aligned(16))) float lds[4 * TILE];
#define ET(b) (lds + (b) * TILE)
#define CT(b) (lds + (2 + (b)) * TILE)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l31 = lane & 31, h = lane >> 5;
  const int wid = tid >> 6;
  const int waveC = wid >> 1, waveR = wid & 1;
  const long row0 = (long)blockIdx.x * TR;
  const int nchunk = d / DK;
  const int nct = (k + TC - 1) / TC;

  // staging slots: float4 q of this thread is row (tid>>3) + 32q, columns
  // 4*(tid&7)..+3 of the chunk; 8 threads cover a row's 128 bytes
  const int sr = tid >> 3, sc = (tid & 7) * 4;
  float4 pe[4], pc[4];
  auto fetch = [&](int ct, int ch) {
    const long col = (long)ch * DK + sc;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const long gr = row0 + sr + 32 * q;
      const long gc = (long)ct * TC + sr + 32 * q;
      pe[q] = gr < m ? *(const float4*)(e + gr * d + col) : float4{0, 0, 0, 0};
      pc[q] = gc < k ? *(const float4*)(cent + gc * d + col) : float4{0, 0, 0, 0};
    }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      *(float4*)(ET(b) + (sr + 32 * q) * LS + sc) = pe[q];
      *(float4*)(CT(b) + (sr + 32 * q) * LS + sc) = pc[q];
    }
  };

  f32x16 acc[2][2] = {};  // [centroid sub-block][row sub-block]
  float bestv[2] = {-INFINITY, -INFINITY};
  int besti[2] = {0, 0};

  fetch(0, 0);
  stash(0);
  __syncthreads();

  const int aoff = (waveC * 64 + l31) * LS + 4 * h;
  const int boff = (waveR * 64 + l31) * LS + 4 * h;
  int buf = 0;
  for (int ct = 0; ct < nct; ct++) {
    for (int ch = 0; ch < nchunk; ch++) {
      const bool last_ch = ch + 1 == nchunk;
      const bool more = !(last_ch && ct + 1 == nct);
      if (more) fetch(last_ch ? ct + 1 : ct, last_ch ? 0 : ch + 1);
      const float* A = CT(buf) + aoff;
      const float* B = ET(buf) + boff;
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
    // C/D map 32x32: column (row of e) = lane&31, row (centroid) =
    // (reg&3) + 8*(reg>>2) + 4*(lane>>5): ascending in reg, so > keeps the
    // smallest index a lane sees
#pragma unroll
    for (int ci = 0; ci < 2; ci++) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int c = ct * TC + waveC * 64 + ci * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (c < k) {
#pragma unroll
          for (int rj = 0; rj < 2; rj++) {
            const float v = acc[ci][rj][reg];
            if (v > bestv[rj]) {
              bestv[rj] = v;
              besti[rj] = c;
            }
          }
        }
      }
    }
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
#pragma unroll
      for (int rj = 0; rj < 2; rj++) acc[ci][rj] = f32x16{};
  }

  // the two half-waves of a row, then the two centroid-half waves; the tiles
  // are dead after the loop's last barrier, the scratch lies over them
  float* redv = lds;                // [2][128]
  int* redi = (int*)(lds + 2 * TR);  // [2][128]
#pragma unroll
  for (int rj = 0; rj < 2; rj++) {
    const float ov = __shfl_xor(bestv[rj], 32);
    const int oi = __shfl_xor(besti[rj], 32);
    take_better(bestv[rj], besti[rj], ov, oi);
    if (h == 0) {
      const int r = waveR * 64 + rj * 32 + l31;
      redv[waveC * TR + r] = bestv[rj];
      redi[waveC * TR + r] = besti[rj];
    }
  }
  __syncthreads();
  if (tid < TR && row0 + tid < m) {
    float bv = redv[tid];
    int bi = redi[tid];
    take_better(bv, bi, redv[TR + tid], redi[TR + tid]);
    labels[row0 + tid] = bi;
    if (best_out) best_out[row0 + tid] = bv;
  }
#undef ET
#undef CT
}

__global__ void k_kmeans_accumulate(
    const float* __restrict__ e, long m, int d, const int* __restrict__ order,
    const int* __restrict__ off, int k, double* __restrict__ sums,
    double* __restrict__ ws, int pieces) {
  __shared__ int ord[PIECE];
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const long P0 = (long)p * PIECE;
  const long P1 = P0 + PIECE < m ? P0 + PIECE : m;
  for (int i = tid; i < (int)(P1 - P0); i += blockDim.x) ord[i] = order[P0 + i];
  __syncthreads();
  if (tid >= d / 4) return;
  const float* ecol = e + 4 * tid;

  // the cluster of position P0: the last c with off[c] <= P0
  int lo = 0, hi = k + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= P0) lo = mid + 1; else hi = mid;
  }
  int c = lo > 0 ? lo - 1 : 0;

  long j = P0;
  while (j < P1) {
    while (c < k && off[c + 1] <= j) ++c;  // empty clusters
    if (c >= k) break;                      // positions past off[k]
    const long a = off[c], b = off[c + 1];
    if (a > j) {                            // positions before off[0]
      j = a < P1 ? a : P1;
      continue;
    }
    const long end = b < P1 ? b : P1;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (long i = j; i < end; i += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        v[u] = float4{0, 0, 0, 0};
        if (i + u < end) {
          const int r = ord[i + u - P0];
          if (r >= 0 && r < m) v[u] = *(const float4*)(ecol + (long)r * d);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {  // +0.0 past the end changes nothing
        s0 += (double)v[u].x;
        s1 += (double)v[u].y;
        s2 += (double)v[u].z;
        s3 += (double)v[u].w;
      }
    }
    double* dst = a < P0   ? ws + (long)p * d
                  : b > P1 ? ws + ((long)pieces + p) * d
                           : sums + (long)c * d;
    *(double2*)(dst + 4 * tid) = double2{s0, s1};
    *(double2*)(dst + 4 * tid + 2) = double2{s2, s3};
    j = end;
  }
}

__global__ __launch_bounds__(cc::KM_COMBINE_BLOCK) void k_kmeans_combine(
    const int* __restrict__ off, int k, long m, int d,
    const double* __restrict__ ws, int pieces, double* __restrict__ sums) {
  const int c = blockIdx.x;
  const int col = blockIdx.y * cc::KM_COMBINE_BLOCK + threadIdx.x;
  if (col >= d) return;
  long a = off[c], b = off[c + 1];
  a = a < 0 ? 0 : a;
  b = b > m ? m : b;
  double* out = sums + (long)c * d + col;
  if (b <= a) {
    *out = 0.0;
    return;
  }
  const long p0 = a / PIECE, p1 = (b - 1) / PIECE;
  if (p0 == p1) return;  // a whole cluster inside one piece: already written
  double s = ws[((long)pieces + p0) * d + col];  // tail of the first piece
  for (long p = p0 + 1; p <= p1; p += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++)
      v[u] = p + u <= p1 ? ws[(p + u) * d + col] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; u++) s += v[u];
  }
  *out = s;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" int cc_kmeans_plan(int64_t m, int64_t d, int64_t k,
                              cc_kmeans_plan_info* out) {
  if (!out) return cc::set_error(CC_ERR_INVALID, "cc_kmeans_plan: null out");
  return cc::kmeans_plan(m, d, k, out);
}

extern "C" int64_t cc_kmeans_workspace_bytes(int64_t m, int64_t d, int64_t k) {
  cc_kmeans_plan_info plan;
  const int rc = cc::kmeans_plan(m, d, k, &plan);
  return rc != CC_OK ? rc : plan.workspace_bytes;
}

extern "C" int cc_kmeans_assign(const void* e_f32, int64_t m, int64_t d,
                                const void* cent_f32, int64_t k,
                                void* labels_i32, void* best_f32,
                                uint64_t stream) {
  if (!e_f32 || !cent_f32 || !labels_i32 || misaligned(e_f32) ||
      misaligned(cent_f32))
    return cc::set_error(CC_ERR_INVALID,
                         "kmeans_assign: null or misaligned pointer");
  cc_kmeans_plan_info plan;
  const int rc = cc::kmeans_plan(m, d, k, &plan);
  if (rc != CC_OK) return rc;
  return cc::timed_launch("kmeans_assign", stream, [&] {
    hipLaunchKernelGGL(k_kmeans_assign, dim3(plan.assign_grid),
                       dim3(plan.assign_block), 0, (hipStream_t)stream,
                       (const float*)e_f32, (long)m, (int)d,
                       (const float*)cent_f32, (int)k, (int*)labels_i32,
                       (float*)best_f32);
  });
}

extern "C" int cc_kmeans_accumulate(const void* e_f32, int64_t m, int64_t d,
                                    const void* order_i32,
                                    const void* offsets_i32, int64_t k,
                                    void* sums_f64, void* workspace,
                                    int64_t workspace_bytes, uint64_t stream) {
  if (!e_f32 || !order_i32 || !offsets_i32 || !sums_f64 || !workspace ||
      misaligned(e_f32) || misaligned(sums_f64) || misaligned(workspace))
    return cc::set_error(CC_ERR_INVALID,
                         "kmeans_accumulate: null or misaligned pointer");
  cc_kmeans_plan_info plan;
  int rc = cc::kmeans_plan(m, d, k, &plan);
  if (rc != CC_OK) return rc;
  if (m > cc::KM_ACC_M_MAX)
    return cc::set_error(CC_ERR_INVALID,
                         "kmeans_accumulate takes at most 2^31-1 rows (%lld)",
                         (long long)m);
  if (workspace_bytes < plan.workspace_bytes)
    return cc::set_error(CC_ERR_INVALID,
                         "kmeans_accumulate workspace %lld < %lld bytes",
                         (long long)workspace_bytes,
                         (long long)plan.workspace_bytes);
  rc = cc::timed_launch("kmeans_accumulate", stream, [&] {
    hipLaunchKernelGGL(k_kmeans_accumulate, dim3(plan.pieces),
                       dim3(plan.acc_block), 0, (hipStream_t)stream,
                       (const float*)e_f32, (long)m, (int)d,
                       (const int*)order_i32, (const int*)offsets_i32, (int)k,
                       (double*)sums_f64, (double*)workspace, plan.pieces);
  });
  if (rc != CC_OK) return rc;
  return cc::timed_launch("kmeans_combine", stream, [&] {
    hipLaunchKernelGGL(k_kmeans_combine,
                       dim3((unsigned)k, (unsigned)plan.combine_grid_y),
                       dim3(cc::KM_COMBINE_BLOCK), 0, (hipStream_t)stream,
                       (const int*)offsets_i32, (int)k, (long)m, (int)d,
                       (const double*)workspace, plan.pieces,
                       (double*)sums_f64);
  });
}
