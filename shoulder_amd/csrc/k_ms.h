// k_ms.h -- the two kernels that sh_register_multistart (include/shoulder_hip.h) puts around the unchanged chain of sh_register_points,
// one lane per humerus each, so that the host enqueues the K starts and the fine stage without looking at anything in between.
//   k_ms_seed  start k >= 0: T0s[b][k] into "icp.T"[b], the flag cleared, "icp.out"[b] zeroed (what the parent call's copies and
//              clears do).  k < 0, in front of the fine stage: the winner's coarse T from "ms.coarse"; a humerus without a winner gets
//              its flag SET -- the chain skips it -- and its record written here: zeros, T = T0s[b][0], status SH_ERR_GEOMETRY.
//   k_ms_pick  behind start k: "icp.out"[b] into "ms.coarse"[b][k], folded into "ms.best"[b] / "ms.winner"[b] under
//              ms_candidate_wins (sh_arthro.h): the smallest (rms, k) among status 0, pairs >= min_pairs.
#pragma once
#include "k_icp.h"

namespace sh {

__global__ void __launch_bounds__(64)
k_ms_seed(const double* __restrict__ T0s /* B x K x 16 */, int B, int K, int k, const sh_registration* __restrict__ coarse /* B x K */,
          const int* __restrict__ winner, double* __restrict__ Tst /* B x SH_ICP_TSTRIDE */, int* __restrict__ flags, sh_registration* __restrict__ out /* B */) {
  const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (b >= B) return;
  sh_registration r;
  for (int i = 0; i < 16; ++i) r.T[i] = 0.0;
  r.rms = 0.0; r.rms_first = 0.0; r.min_pivot = 0.0; r.pairs = 0; r.iterations = 0; r.converged = 0; r.status = 0;
  const double* src = T0s + 16 * ((size_t)b * K + (k >= 0 ? k : 0));
  int flag = 0;
  if (k < 0) {
    const int w = winner[b];
    if (w >= 0 && w < K) src = coarse[(size_t)b * K + w].T;
    else { flag = 1; r.status = SH_ERR_GEOMETRY_DEV; for (int i = 0; i < 16; ++i) r.T[i] = src[i]; }
  }
  double* Tb = Tst + (size_t)b * SH_ICP_TSTRIDE;
  for (int i = 0; i < 16; ++i) Tb[i] = src[i];
  for (int i = 16; i < SH_ICP_TSTRIDE; ++i) Tb[i] = 0.0;
  flags[b] = flag;
  out[b] = r;
}

__global__ void __launch_bounds__(64)
k_ms_pick(const sh_registration* __restrict__ out /* B */, int B, int K, int k, int min_pairs, sh_registration* __restrict__ coarse /* B x K */,
          double* __restrict__ best /* B */, int* __restrict__ winner /* B */) {
  const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (b >= B) return;
  const sh_registration r = out[b];
  coarse[(size_t)b * K + k] = r;
  const int w = k == 0 ? -1 : winner[b];
  const double br = k == 0 ? 0.0 : best[b];
  if (ms_candidate_wins(r.status, r.pairs, r.rms, min_pairs, w, br)) { best[b] = r.rms; winner[b] = k; }
  else if (k == 0) { best[b] = 0.0; winner[b] = -1; }
}

}  // namespace sh
