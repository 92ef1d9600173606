// k_mass.h -- mass properties of the resident batch (include/shoulder_hip.h sh_mass_properties): the surface and volume integrals of
// every humerus in two kernels.
//   k_mass_sum   (block of SH_MASS_BLOCK = 256 faces, humerus), 256 lanes.  Each lane forms the 24 terms of its face (sh_scalar.h
//                mass_face_terms, relative to the pivot: vertex 0 of the humerus; a lane past the last face holds +0.0), then the
//                terms go through LDS SH_MASS_GROUP at a time exactly as in k_icp_sum: 256 slots per term, slot[i] += slot[i + h] for
//                h = 128 .. 1 with a barrier between the levels, slot 0 to "mass.part"[b][block][term].  8 terms, 16 KB.  A
//                workgroup past the blocks of a smaller humerus stores nothing (the host clears "mass.part").
//   k_mass_join  (humerus), one wave.  Lane t < SH_MASS_TERMS adds term t of the humerus' block rows in block order starting at 0.0;
//                lane 0 then runs mass_finish and stores the record.
// The order of every floating-point sum is fixed by the definition: no atomics, nothing depends on B, the grid or the humerus' place.
#pragma once
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_MASS_GROUP 8        // terms that share one pass through LDS

static_assert(SH_MASS_BLOCK == 256, "k_mass_sum: one face per lane of a 256-lane workgroup");
static_assert(SH_MASS_TERMS % SH_MASS_GROUP == 0 && SH_MASS_TERMS <= 64, "k_mass_sum: whole groups of terms; k_mass_join: a lane per term");
static_assert(sizeof(sh_mass) == SH_MASS_DOUBLES * 8 + 16 && offsetof(sh_mass, faces) == SH_MASS_DOUBLES * 8 && offsetof(sh_mass, shell_centroid) == 24 &&
              offsetof(sh_mass, shell_axes) == 120 && offsetof(sh_mass, center_mass) == 192 && offsetof(sh_mass, principal_axes) == 312,
              "sh_mass is the 48 doubles of mass_finish in its order and four int32");

__global__ void __launch_bounds__(SH_MASS_BLOCK)
k_mass_sum(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
           double* __restrict__ part /* B x gridDim.x x SH_MASS_TERMS */) {
  __shared__ double slot[SH_MASS_GROUP][SH_MASS_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b];
  if ((long long)blockIdx.x * SH_MASS_BLOCK >= nf) return;      // (uniform in the workgroup)
  const long long fi = (long long)blockIdx.x * SH_MASS_BLOCK + tid;
  double t[SH_MASS_TERMS];
#pragma unroll
  for (int i = 0; i < SH_MASS_TERMS; ++i) t[i] = 0.0;
  if (fi < nf) {
    const float* vb = verts + 3 * voff[b];
    const int* f = faces + 3 * (foff[b] + fi);
    const float *v0 = vb + 3 * (size_t)f[0], *v1 = vb + 3 * (size_t)f[1], *v2 = vb + 3 * (size_t)f[2];
    const double o[3] = {(double)vb[0], (double)vb[1], (double)vb[2]};
    const double A[3] = {(double)v0[0], (double)v0[1], (double)v0[2]};
    const double B[3] = {(double)v1[0], (double)v1[1], (double)v1[2]};
    const double C[3] = {(double)v2[0], (double)v2[1], (double)v2[2]};
    mass_face_terms(o, A, B, C, t);
  }
  double* row = part + ((size_t)b * gridDim.x + blockIdx.x) * SH_MASS_TERMS;
#pragma unroll
  for (int g = 0; g < SH_MASS_TERMS; g += SH_MASS_GROUP) {
#pragma unroll
    for (int j = 0; j < SH_MASS_GROUP; ++j) slot[j][tid] = t[g + j];
    __syncthreads();
    for (int h = SH_MASS_BLOCK / 2; h >= 1; h >>= 1) {
      if (tid < h) {
#pragma unroll
        for (int j = 0; j < SH_MASS_GROUP; ++j) slot[j][tid] += slot[j][tid + h];
      }
      __syncthreads();
    }
    if (tid < SH_MASS_GROUP) row[g + tid] = slot[tid][0];
    __syncthreads();      // the next group overwrites the slots
  }
}

__global__ void __launch_bounds__(64)
k_mass_join(const float* __restrict__ verts, const long long* __restrict__ voff, const long long* __restrict__ foff, const double* __restrict__ part,
            int blocks /* rows per humerus in part */, sh_mass* __restrict__ out /* B */) {
  __shared__ double tot[SH_MASS_TERMS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b];
  long long nblk = (nf + SH_MASS_BLOCK - 1) / SH_MASS_BLOCK;
  if (nblk > blocks) nblk = blocks;
  if (tid < SH_MASS_TERMS) {
    double s = 0.0;
    for (long long blk = 0; blk < nblk; ++blk) s += part[((size_t)b * blocks + blk) * SH_MASS_TERMS + tid];
    tot[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double T[SH_MASS_TERMS], o[3] = {0.0, 0.0, 0.0}, rec[SH_MASS_DOUBLES];
  int irec[4];
  for (int i = 0; i < SH_MASS_TERMS; ++i) T[i] = tot[i];
  if (voff[b + 1] > voff[b]) {
    const float* vb = verts + 3 * voff[b];
    o[0] = (double)vb[0]; o[1] = (double)vb[1]; o[2] = (double)vb[2];
  }
  mass_finish(T, o, (int)nf, rec, irec);
  double* od = (double*)(out + b);
  for (int i = 0; i < SH_MASS_DOUBLES; ++i) od[i] = rec[i];
  out[b].faces = irec[0]; out[b].degenerate = irec[1]; out[b].status = irec[2]; out[b].vstatus = irec[3];
}

}  // namespace sh
