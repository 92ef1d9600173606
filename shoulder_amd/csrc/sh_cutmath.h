// sh_cutmath.h -- the device helpers that the slice layer (k_slices.h), the mesh clip (k_clip.h) and batched resection (k_resect.h)
// share.  No kernels here, so any unit may include it.
#pragma once
#include "sh_common.h"

namespace sh {

#define SH_MAXLOOPS 32      // loops per plane in the LDS joins (k_slices.h, k_resect_join.h)
#define SH_CLIP_TOL 1e-8      // trimesh.constants.tol.merge

__device__ inline uint32_t hash_key64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33;
  return (uint32_t)k;
}

// class of a face from its three signs: 0 dropped, 1 kept, 2 quad, 3 triangle, 4 = lies in the plane (decided by its normal)
__device__ inline int clip_class(int s0, int s1, int s2) {
  const int sum = s0 + s1 + s2, asum = abs(s0) + abs(s1) + abs(s2);
  if (asum == 0) return 4;
  if (asum >= 2 && abs(sum) <= 1) return sum < 0 ? 2 : 3;
  return sum == -asum ? 1 : 0;
}

// crossing point of edge j (o[j] -> o[(j+1)%3]) with the plane: slice_faces_plane's  dist = num / denom;  point = dist * d + o
__device__ inline void clip_cross(const double* O /* 3 x 3 */, int j, const double* pl, double* out) {
  const double* o = O + 3 * j; const double* o1 = O + 3 * ((j + 1) % 3);
  const double dx = o1[0] - o[0], dy = o1[1] - o[1], dz = o1[2] - o[2];
  const double num = ((pl[0] - o[0]) * pl[3] + (pl[1] - o[1]) * pl[4]) + (pl[2] - o[2]) * pl[5];
  double den = (dx * pl[3] + dy * pl[4]) + dz * pl[5];
  if (den == 0.0) den = 1e-12;
  const double dist = num / den;
  out[0] = dist * dx + o[0]; out[1] = dist * dy + o[1]; out[2] = dist * dz + o[2];
}

}  // namespace sh
