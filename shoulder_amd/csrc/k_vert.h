// k_vert.h -- vertex normals and discrete curvatures of the resident batch (include/shoulder_hip.h sh_vertex_fields): the per-vertex
// work the incidence of sh_mesh_topology ("topo.vrow", "topo.vface", "topo.adj") is for.  The scalar rules are sh_scalar.h vert_*;
// everything is float64 in the written order.  Grids are (block of SH_VERT_BLOCK = 256 faces or vertices, mesh), one per lane.
//   k_vert_face    (face block, mesh).  Three index loads, three corner gathers, one sqrt, three atan2, three divisions: the 80-byte
//                  record of "vert.face" (array of structs: the gather reads whole records by scattered face index, and consecutive
//                  lanes still write contiguous lines) and A2 alone into "vert.a2" for the smoothing; a workgroup with a face that is
//                  not flat sets the mesh's word of "vert.state" with one integer atomic.
//   k_vert_gather  (vertex block, mesh).  A lane walks its vertex's row in order (vert_gather): no row length is assumed, the centre of
//                  a fan walks the whole fan.  The corners of L are gathered again from "verts" (nine float32 per face, lines the face
//                  pass has just read) instead of kept per corner: nothing is indexed at run time, so nothing lives in scratch.
//                  Writes "vert.normal", fields 0 .. 4 and 7 of "vert.fields", "vert.flags", and the raw gauss and mean into planes
//                  0 and 1 of "vert.plane".
//   k_vert_smooth  (vertex block, mesh), once per round.  "vert.plane" has four planes of sumV doubles: round r reads gauss and mean
//                  from planes 2 (r & 1) and 2 (r & 1) + 1 and writes the other pair (vert_smooth).  The values a lane gathers are
//                  8-byte words of a structure-of-arrays plane, and the areas come from "vert.a2", not from the 80-byte records.
//   k_vert_pack    (vertex block, mesh).  Fields 5 and 6 from the pair the last round wrote (the raw pair without a round); the first
//                  workgroup of a mesh writes "vert.status": SH_ERR_GEOMETRY for a mesh without a face that is not flat.
// No floating-point atomics: the order of every sum is the row's.  Every index is below its array's size by construction: rows hold
// face indices of the vertex's own mesh (k_topo.h), faces hold vertex indices checked at upload.
#pragma once
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_VERT_BLOCK 256

static_assert(SH_VERT_FIELDS == SH_VTX_FIELDS && SH_VERT_WEIGHT_AREA == 0 && SH_VERT_WEIGHT_ANGLE == SH_VTX_ANGLE, "sh_scalar.h: the fields of a vertex, the weights");
static_assert(SH_VERT_USED == SH_VTX_USED && SH_VERT_BORDER == SH_VTX_BORDER && SH_VERT_NONMANIFOLD == SH_VTX_NONMANIFOLD && SH_VERT_FLAT == SH_VTX_FLAT,
              "sh_scalar.h: the flags of a vertex");
static_assert(SH_ADJ_BORDER == SH_TOPO_BORDER && SH_ADJ_NONMANIFOLD == SH_TOPO_NONMANIFOLD, "sh_scalar.h: the adjacency codes");

__global__ void __launch_bounds__(SH_VERT_BLOCK)
k_vert_face(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
            double* __restrict__ frec, double* __restrict__ a2, int* __restrict__ state /* B */) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_VERT_BLOCK;
  if (f0 >= nf) return;      // (uniform in the workgroup)
  const long long fi = f0 + tid;
  int solid = 0;
  if (fi < nf) {
    const int* f = faces + 3 * (foff[b] + fi);
    const bool deg = topo_degenerate(f, (int)(voff[b + 1] - voff[b]));
    double P[3][3], rec[SH_VTX_FACE];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) P[k][c] = 0.0;
    if (!deg) vert_corners(verts + 3 * voff[b], f, P);
    solid = vert_face(P, deg, rec) ? 0 : 1;
    double* out = frec + SH_VTX_FACE * (size_t)(foff[b] + fi);
#pragma unroll
    for (int i = 0; i < SH_VTX_FACE; ++i) out[i] = rec[i];
    a2[foff[b] + fi] = rec[3];
  }
  if (__syncthreads_or(solid) && tid == 0) atomicOr(state + b, 1);
}

__global__ void __launch_bounds__(SH_VERT_BLOCK)
k_vert_gather(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const int* __restrict__ vrow, const int* __restrict__ vface, const int* __restrict__ adj, const double* __restrict__ frec, int weight,
              long long sumV, double* __restrict__ normal, double* __restrict__ fields, int* __restrict__ flags, double* __restrict__ plane) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_VERT_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int* row = vrow + voff[b] + b;
  const int s = row[v], n = row[v + 1] - s;
  double nrm[3], fl[5];
  int fg;
  vert_gather(verts + 3 * voff[b], faces + 3 * foff[b], adj + 3 * foff[b], frec + SH_VTX_FACE * (size_t)foff[b], vface + 3 * foff[b] + s, n, (int)v, weight, nrm, fl, &fg);
  const size_t g = (size_t)(voff[b] + v);
  normal[3 * g] = nrm[0]; normal[3 * g + 1] = nrm[1]; normal[3 * g + 2] = nrm[2];
  double* o = fields + SH_VTX_FIELDS * g;
  o[0] = fl[0]; o[1] = fl[1]; o[2] = fl[2]; o[3] = fl[3]; o[4] = fl[4]; o[7] = 0.0;
  flags[g] = fg;
  plane[g] = fl[3]; plane[(size_t)sumV + g] = fl[4];
}

__global__ void __launch_bounds__(SH_VERT_BLOCK)
k_vert_smooth(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
              const int* __restrict__ vface, const double* __restrict__ a2, long long sumV, int round, double* plane) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_VERT_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int* row = vrow + voff[b] + b;
  const int s = row[v], n = row[v + 1] - s;
  const double* in = plane + (size_t)(round & 1) * 2 * (size_t)sumV + voff[b];
  double* out = plane + (size_t)((round + 1) & 1) * 2 * (size_t)sumV + voff[b];
  double g, m;
  vert_smooth(faces + 3 * foff[b], a2 + foff[b], vface + 3 * foff[b] + s, n, in, in + sumV, &g, &m);
  out[v] = g; out[(size_t)sumV + v] = m;
}

__global__ void __launch_bounds__(SH_VERT_BLOCK)
k_vert_pack(const long long* __restrict__ voff, const double* __restrict__ plane, long long sumV, int rounds, const int* __restrict__ state,
            double* __restrict__ fields, int* __restrict__ status /* B */) {
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = state[b] ? 0 : SH_ERR_GEOMETRY_DEV;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_VERT_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const size_t g = (size_t)(voff[b] + v);
  const double* fin = plane + (size_t)(rounds & 1) * 2 * (size_t)sumV;
  fields[SH_VTX_FIELDS * g + 5] = fin[g]; fields[SH_VTX_FIELDS * g + 6] = fin[(size_t)sumV + g];
}

}  // namespace sh
