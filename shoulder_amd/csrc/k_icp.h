// k_icp.h -- rigid registration of point sets onto the resident batch (include/shoulder_hip.h sh_register_points): the three kernels
// that, with the unchanged k_cp_walk / k_cp_join between them, make one evaluation of the loop.  The host enqueues max_iter + 1
// evaluations on the context's stream and looks at nothing in between; a humerus that is done sets its flag and is skipped from then
// on by all three (the walk still runs for it, on moved points that no longer change, and finds the same pairs).
//   k_icp_move  (chunk of 256 points, humerus): p' = T p (sh_scalar.h canal_map_point) into "icp.moved"[b][i].
//   k_icp_sum   (block of SH_ICP_BLOCK = 256 points, humerus), 256 lanes.  Each lane forms the terms of its pair (icp_pair_terms; a
//               lane past Q and a rejected pair hold +0.0), then the terms go through LDS SH_ICP_GROUP at a time: 256 slots per term,
//               slot[i] += slot[i + h] for h = 128 .. 1 with a barrier between the levels, slot 0 to "icp.part"[b][block][term].  The
//               tree of a term involves that term alone, so the grouping (8 terms, 16 KB) changes no byte; it saves barriers against
//               term by term and stays far below what holding all 29 terms at once (59 KB) would cost in occupancy.  In a level the
//               lanes of a wave read consecutive doubles: no bank conflicts.  phase 0 sums the INPUT points instead (terms n and
//               sum p), for the pivot's mean.
//   k_icp_step  (humerus), one wave.  Lane t < SH_ICP_TERMS adds term t of the block rows in block order starting at 0.0; lane 0
//               then runs icp_step (report, stop or solve and update "icp.T"), writes the history row and the record, and sets
//               the flag.  phase 0 stores cbar = sum p / Q behind the transform instead.
// The order of every floating-point sum is fixed by the definition: no atomics, nothing depends on B, the grid or the walk's split.
#pragma once
#include "k_closest.h"

namespace sh {

#define SH_ICP_GROUP 8        // terms that share one pass through LDS
#define SH_ICP_TSTRIDE 20     // doubles per humerus in "icp.T": the transform (16), cbar (3), one spare

static_assert(SH_ICP_BLOCK == 256 && SH_ICP_BLOCK == SH_CP_CHUNK, "k_icp_sum: one pair per lane, the walk's chunk is the sum's block");
static_assert(SH_ICP_TERMS % SH_ICP_GROUP == 0, "k_icp_sum: whole groups of terms");
static_assert(sizeof(sh_registration) == 168, "sh_registration is nineteen doubles and four int32");

__global__ void __launch_bounds__(SH_ICP_BLOCK)
k_icp_move(const double* __restrict__ points /* Q x 3, or B x Q x 3 */, int Q, int per_humerus, const double* __restrict__ Tst /* B x SH_ICP_TSTRIDE */,
           const int* __restrict__ flags, double* __restrict__ moved /* B x Q x 3 */) {
  const int b = blockIdx.y;
  if (flags[b] != 0) return;
  const int q = (int)blockIdx.x * SH_ICP_BLOCK + (int)threadIdx.x;
  if (q >= Q) return;
  const double* p = points + 3 * ((per_humerus ? (size_t)b * Q : (size_t)0) + (size_t)q);
  double o[3];
  canal_map_point(Tst + (size_t)b * SH_ICP_TSTRIDE, p[0], p[1], p[2], o);
  double* m = moved + 3 * ((size_t)b * Q + q);
  m[0] = o[0]; m[1] = o[1]; m[2] = o[2];
}

__global__ void __launch_bounds__(SH_ICP_BLOCK)
k_icp_sum(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
          const double* __restrict__ points, const double* __restrict__ moved, const sh_closest* __restrict__ near, int Q, int per_humerus, int phase,
          int metric, double reject, const double* __restrict__ Tst, const int* __restrict__ flags, double* __restrict__ part /* B x blocks x SH_ICP_TERMS */) {
  __shared__ double slot[SH_ICP_GROUP][SH_ICP_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (flags[b] != 0) return;      // (uniform in the workgroup)
  const int q = (int)blockIdx.x * SH_ICP_BLOCK + tid;
  double t[SH_ICP_TERMS];
#pragma unroll
  for (int i = 0; i < SH_ICP_TERMS; ++i) t[i] = 0.0;
  if (q < Q) {
    if (phase == 0) {
      const double* p = points + 3 * ((per_humerus ? (size_t)b * Q : (size_t)0) + (size_t)q);
      t[0] = 1.0; t[2] = p[0]; t[3] = p[1]; t[4] = p[2];
    } else {
      const size_t i = (size_t)b * Q + q;
      const double pm[3] = {moved[3 * i], moved[3 * i + 1], moved[3 * i + 2]};
      const sh_closest nr = near[i];
      double A[3] = {0.0, 0.0, 0.0}, ab[3] = {0.0, 0.0, 0.0}, ac[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};      // (A: cp_face fills it, nothing reads it)
      if (metric == SH_ICP_METRIC_PLANE && nr.status == 0 && nr.face >= 0 && (long long)nr.face < foff[b + 1] - foff[b]) {
        const double* T = Tst + (size_t)b * SH_ICP_TSTRIDE;
        cp_face(verts, faces, voff, foff, b, nr.face, A, ab, ac);
        canal_map_point(T, T[16], T[17], T[18], c);
      }
      icp_pair_terms(metric, pm, nr.point, nr.status, reject, ab, ac, c, t);
    }
  }
  double* row = part + ((size_t)b * gridDim.x + blockIdx.x) * SH_ICP_TERMS;
#pragma unroll
  for (int g = 0; g < SH_ICP_TERMS; g += SH_ICP_GROUP) {
#pragma unroll
    for (int j = 0; j < SH_ICP_GROUP; ++j) slot[j][tid] = t[g + j];
    __syncthreads();
    for (int h = SH_ICP_BLOCK / 2; h >= 1; h >>= 1) {
      if (tid < h) {
#pragma unroll
        for (int j = 0; j < SH_ICP_GROUP; ++j) slot[j][tid] += slot[j][tid + h];
      }
      __syncthreads();
    }
    if (tid < SH_ICP_GROUP) row[g + tid] = slot[tid][0];
    __syncthreads();      // the next group overwrites the slots
  }
}

__global__ void __launch_bounds__(64)
k_icp_step(const double* __restrict__ part, int blocks, int Q, int phase, int metric, int k, int max_iter, double tol, double* __restrict__ Tst,
           int* __restrict__ flags, double* __restrict__ hist /* B x (max_iter + 1) x 2 */, sh_registration* __restrict__ out /* B */) {
  __shared__ double tot[SH_ICP_TERMS];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (flags[b] != 0) return;
  if (tid < SH_ICP_TERMS) {
    double s = 0.0;
    for (int blk = 0; blk < blocks; ++blk) s += part[((size_t)b * blocks + blk) * SH_ICP_TERMS + tid];
    tot[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double* Tb = Tst + (size_t)b * SH_ICP_TSTRIDE;
  if (phase == 0) {
    const double n = (double)Q;
    Tb[16] = tot[2] / n; Tb[17] = tot[3] / n; Tb[18] = tot[4] / n;
    return;
  }
  sh_registration r = out[b];
  double T[16], sums[SH_ICP_TERMS], rec[3] = {r.rms, r.rms_first, r.min_pivot}, h[2];
  int irec[4];
  for (int i = 0; i < 16; ++i) { T[i] = Tb[i]; r.T[i] = T[i]; }
  for (int i = 0; i < SH_ICP_TERMS; ++i) sums[i] = tot[i];
  const double cbar[3] = {Tb[16], Tb[17], Tb[18]};
  const int done = icp_step(metric, k, max_iter, tol, sums, cbar, T, rec, irec, h);
  r.rms = rec[0]; r.rms_first = rec[1]; r.min_pivot = rec[2];
  r.pairs = irec[0]; r.iterations = irec[1]; r.converged = irec[2]; r.status = irec[3];
  out[b] = r;
  double* hr = hist + ((size_t)b * (max_iter + 1) + k) * 2;
  hr[0] = h[0]; hr[1] = h[1];
  if (done) flags[b] = 1;
  else for (int i = 0; i < 16; ++i) Tb[i] = T[i];
}

}  // namespace sh
