// k_winding.h -- generalized winding numbers of the resident batch (include/shoulder_hip.h sh_winding_numbers): for every (humerus,
// query point) the sum over ALL faces of the humerus of the signed solid angle sh_scalar.h solid_angle_tri, divided by 4 pi.  No cull and
// no far-field approximation: every face contributes.  Unlike the minimum of k_closest.h a floating-point sum depends on its order, so
// the order is part of the definition and the kernels follow it whatever the launch shape:
//     w = (sum over blocks, in block order from 0 (sum over the faces of the block, in face order from 0, omega_f)) / (4 pi)
// with a block SH_WIND_BLOCK = 2048 consecutive faces (8 tiles of 256).  A lane owns its point's sums alone: no floating-point atomics,
// no floating-point sums across lanes, and a (humerus, point) result depends on that mesh and that point alone.
//   k_wn_walk   (chunk of 256 points, humerus, split s of S) workgroups of 256 lanes.  One query point per lane, in registers.  The
//               workgroup walks the BLOCKS cp_split_range(blocks of the humerus, S, s): whole blocks are the unit of the face split, a
//               split never cuts one.  The lanes load the 256 faces of a tile together (resect_tile_face: the float32 vertices
//               widened) and put the corners A, B, C into LDS, 72 B per face.  Then every lane reads the same LDS address face after
//               face (one address: a broadcast, no bank conflicts) and adds solid_angle_tri to its block sum, which started at 0.  At
//               the end of a block the lane either stores the block sum to "wn.part"[b][q][block] (S > 1) or, when its workgroup owns
//               all blocks (S == 1), adds it to its total, which started at 0 -- the blocks come in order -- and stores the total to
//               "wn.part"[b][q] at the end.  A call with few points wastes lanes: Q = 4 costs what Q = 256 costs.
//   k_wn_join   one thread per (humerus, point): the block sums added in block order from 0 (S > 1; for S == 1 the total is there),
//               then winding_record: w = sum / 4 pi, inside = |w| >= 0.5, or SH_ERR_GEOMETRY_DEV with zeros when the sum is not finite.
// Both paths perform the same additions in the same order (0.0 + x is x for every x a sum that started at 0.0 can be), so S changes no
// byte.  A smaller humerus of a ragged batch has fewer blocks than S: its surplus splits are empty and store nothing.
#pragma once
#include "k_resect.h"

namespace sh {

#define SH_WN_TILE SH_RS_TILE
#define SH_WN_CHUNK 256      // points per workgroup: one per lane
#define SH_WN_BLOCK_TILES (SH_WIND_BLOCK / SH_WN_TILE)

static_assert(sizeof(sh_winding) == 16, "sh_winding is a double and two int32");
static_assert(SH_WN_TILE == SH_WN_CHUNK, "k_wn_walk: a lane stages one face and owns one point");
static_assert(SH_WIND_BLOCK % SH_WN_TILE == 0, "a block is a whole number of tiles");

__global__ void __launch_bounds__(SH_WN_CHUNK)
k_wn_walk(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
          const double* __restrict__ points /* Q x 3, or B x Q x 3 */, int Q, int per_humerus, int S, int stride /* of "wn.part" per point: 1 when S == 1 */,
          double* __restrict__ part /* B x Q x stride */) {
  __shared__ __attribute__((aligned(16))) double s_tri[SH_WN_TILE][9];      // A, B, C
  const int b = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
  const int q = (int)blockIdx.x * SH_WN_CHUNK + tid;
  const bool has = q < Q;      // (a lane without a point still stages its face; it walks point 0 of the chunk's humerus and stores nothing)
  const double* pg = points + 3 * ((per_humerus ? (size_t)b * Q : (size_t)0) + (size_t)(has ? q : 0));
  const double p[3] = {pg[0], pg[1], pg[2]};
  const long long nf = foff[b + 1] - foff[b];
  const int blocks = (int)((nf + SH_WIND_BLOCK - 1) / SH_WIND_BLOCK);
  const int tiles = (int)((nf + SH_WN_TILE - 1) / SH_WN_TILE);
  int k0, k1;
  cp_split_range(blocks, S, s, &k0, &k1);
  double* out = part + ((size_t)b * Q + (size_t)(has ? q : 0)) * stride;
  double total = 0.0;
  for (int k = k0; k < k1; ++k) {      // (uniform in the workgroup)
    double sum = 0.0;
    const int t1 = (k + 1) * SH_WN_BLOCK_TILES < tiles ? (k + 1) * SH_WN_BLOCK_TILES : tiles;
    for (int t = k * SH_WN_BLOCK_TILES; t < t1; ++t) {
      bool live; long long fi; double V[9];
      (void)resect_tile_face(verts, faces, voff, foff, b, t, tid, &live, &fi, V);      // (t < tiles: the tile is there)
      __syncthreads();      // the walk of the tile before is over
      {
        double* tr = s_tri[tid];
#pragma unroll
        for (int j = 0; j < 9; ++j) tr[j] = V[j];
      }
      __syncthreads();
      const long long f0 = (long long)t * SH_WN_TILE;
      const int n = (int)(nf - f0 < SH_WN_TILE ? nf - f0 : SH_WN_TILE);
      for (int j = 0; j < n; ++j) {
        const double* tr = s_tri[j];      // (the same address in every lane)
        const double A[3] = {tr[0], tr[1], tr[2]}, B[3] = {tr[3], tr[4], tr[5]}, C[3] = {tr[6], tr[7], tr[8]};
        sum += solid_angle_tri(p, A, B, C);
      }
    }
    if (S == 1) total += sum;
    else if (has) out[k] = sum;
  }
  if (S == 1 && has) out[0] = total;
}

__global__ void __launch_bounds__(256)
k_wn_join(const long long* __restrict__ foff, int Q, int S, int stride, const double* __restrict__ part, long long n /* B x Q */,
          sh_winding* __restrict__ out /* B x Q */) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* pp = part + (size_t)i * stride;
  double total;
  if (S == 1) total = pp[0];
  else {
    const int b = (int)(i / Q);
    const long long nf = foff[b + 1] - foff[b];
    const int blocks = (int)((nf + SH_WIND_BLOCK - 1) / SH_WIND_BLOCK);      // (<= stride: the blocks of the largest humerus)
    total = 0.0;
    for (int k = 0; k < blocks; ++k) total += pp[k];
  }
  sh_winding o;
  int inside, status;
  winding_record(total, &o.winding, &inside, &status, SH_ERR_GEOMETRY_DEV);
  o.inside = inside; o.status = status;
  out[i] = o;
}

}  // namespace sh
