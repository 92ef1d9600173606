// k_smooth.h -- smoothing of the vertices of the resident batch (include/shoulder_hip.h sh_smooth_vertices): the vertex -> vertex rows
// over the incidence of sh_mesh_topology ("topo.vrow", "topo.vface", "topo.adj") and the Laplacian, Taubin and HC filters on them.  The
// scalar rules are sh_scalar.h smooth_*; everything is float64 in the written order.  Grids are (block of SH_SMOOTH_BLOCK = 256 vertices
// or faces, mesh), one per lane, but for the three kernels with one workgroup per mesh.
//   k_smooth_count  (vertex block, mesh).  A lane walks its vertex's row with smooth_next until it has every distinct neighbour: the
//                   count into "smooth.nrow"[v].  No row length is assumed and nothing is kept per lane, so the centre of a fan of 300
//                   walks its 300 faces 301 times from L2; a bone's vertex walks 6 faces 7 times.  "topo.adj" is not used: the rule is
//                   the same at a manifold, a border and a non-manifold edge.  Built once per batch.
//   k_smooth_scan   (mesh).  The exclusive scan of the counts in chunks of 256 (integer: any tree; topo_block_scan), in place.
//   k_smooth_fill   (vertex block, mesh).  The same walk again: "smooth.nbr" and, beside it, the stored weight of the pair (smooth_weight).
//   k_smooth_init   (vertex block, mesh).  Plane 0 = P0, the float32 "verts" widened; "smooth.pin" from the mask and the border test.
//   k_smooth_round  (vertex block, mesh), one launch per M(.) evaluation.  THE HOT PATH.  A lane walks its row in order and gathers whole
//                   24-byte positions by index from an array-of-structs plane (a structure-of-arrays plane would touch three lines per
//                   neighbour); it reads one plane and writes another.  MODE 0: a step.  MODE 1: p = M(q) and b of the HC filter.
//                   MODE 2: P of the HC filter from M(b), b and p.  The planes live in memory and are served by L2: 389 KB of float64
//                   positions of a humerus do not fit a workgroup's LDS.
//   k_smooth_vol    (face block, mesh).  Terms 13 .. 16 of the mass sum (mass_face_terms) of the faces on P0 (START) or on a plane, through
//                   the LDS tree of k_mass_sum into a block row.
//   k_smooth_scale  (mesh), one wave.  The block rows added in block order; smooth_scale; the volumes, the scale and the status of the
//                   info record and the mesh's head for k_smooth_apply.
//   k_smooth_apply  (vertex block, mesh).  "smooth.pos" from the last plane, scaled when the head says so; |P - P0|^2 of the block through
//                   the same tree and the block's largest |P - P0| into a row of two doubles.
//   k_smooth_info   (mesh).  The rows added in block order, the largest, the pinned and the isolated vertices counted: the info record.
// No floating-point atomics: the order of every sum is the row's or the tree's.  Every index is below its array's size by construction:
// rows of "topo.vface" hold faces of the vertex's own mesh, faces hold vertex indices checked at upload, a mesh's rows of "smooth.nbr" start
// at 6 foff[b] and hold at most two entries per corner of a non-degenerate face.
#pragma once
#include "k_topo.h"      // topo_block_scan
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_SMOOTH_BLOCK 256

static_assert(SH_SMOOTH_LAPLACIAN == SH_SMO_LAPLACIAN && SH_SMOOTH_TAUBIN == SH_SMO_TAUBIN && SH_SMOOTH_HC == SH_SMO_HC && SH_SMOOTH_UNIFORM == 0 &&
              SH_SMOOTH_INVLEN == SH_SMO_INVLEN && SH_SMOOTH_PIN_BORDER == SH_SMO_PIN_BORDER && SH_SMOOTH_KEEP_VOLUME == SH_SMO_KEEP_VOLUME &&
              SH_SMOOTH_INFO_BYTES == sizeof(SmoothInfo), "sh_scalar.h: the filters, weights and flags of the smoothing, the info record");
static_assert(SH_SMOOTH_BLOCK == SH_MASS_BLOCK && SH_SMOOTH_BLOCK == SH_TOPO_BLOCK, "the tree of the mass sum; topo_block_scan");

// the tree of k_mass_sum for one value per lane: slot[i] += slot[i + h], h = 128 .. 1; every lane of the workgroup calls it -> slot[0]
__device__ inline double smooth_tree(double x, double* slot, int tid) {
  slot[tid] = x;
  __syncthreads();
  for (int h = SH_SMOOTH_BLOCK / 2; h >= 1; h >>= 1) {
    if (tid < h) slot[tid] += slot[tid + h];
    __syncthreads();
  }
  const double r = slot[0];
  __syncthreads();      // the next call overwrites the slots
  return r;
}

__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_count(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
               const int* __restrict__ vface, int* __restrict__ nrow) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SMOOTH_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int* row = vrow + voff[b] + b;
  const int s = row[v], n = row[v + 1] - s;
  const int *fc = faces + 3 * foff[b], *fr = vface + 3 * foff[b] + s;
  int count = 0;
  for (int u = smooth_next(fc, fr, n, (int)v, -1); u != SH_TOPO_NONE; u = smooth_next(fc, fr, n, (int)v, u)) ++count;
  nrow[voff[b] + b + v] = count;
}

__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_scan(const long long* __restrict__ voff, int* __restrict__ nrow) {
  __shared__ int s[SH_SMOOTH_BLOCK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = (int)(voff[b + 1] - voff[b]);
  int* row = nrow + voff[b] + b;
  int run = 0;
  for (int v0 = 0; v0 < nv; v0 += SH_SMOOTH_BLOCK) {
    const int v = v0 + tid;
    const int c = v < nv ? row[v] : 0;
    const int incl = topo_block_scan(c, s, tid);
    if (v < nv) row[v] = run + incl - c;
    s[tid] = incl;
    __syncthreads();
    run += s[SH_SMOOTH_BLOCK - 1];
    __syncthreads();
  }
  if (tid == 0) row[nv] = run;
}

__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_fill(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const int* __restrict__ vrow, const int* __restrict__ vface, const int* __restrict__ nrow, int* __restrict__ nbr, double* __restrict__ w) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SMOOTH_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int* row = vrow + voff[b] + b;
  const int s = row[v], n = row[v + 1] - s;
  const int *fc = faces + 3 * foff[b], *fr = vface + 3 * foff[b] + s;
  const float* vb = verts + 3 * voff[b];
  const int* nr = nrow + voff[b] + b;
  const size_t at = 6 * (size_t)foff[b] + (size_t)nr[v];
  const int room = nr[v + 1] - nr[v];      // (what k_smooth_count found: the walk below finds the same)
  int i = 0;
  for (int u = smooth_next(fc, fr, n, (int)v, -1); u != SH_TOPO_NONE && i < room; u = smooth_next(fc, fr, n, (int)v, u), ++i) {
    nbr[at + i] = u;
    w[at + i] = smooth_weight(vb, (int)v, u);
  }
}

__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_init(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const int* __restrict__ vrow, const int* __restrict__ vface, const int* __restrict__ adj, const unsigned char* __restrict__ mask /* sumV, or null */,
              int pin_border, double* __restrict__ plane, int* __restrict__ pin) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SMOOTH_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const size_t g = (size_t)(voff[b] + v);
  plane[3 * g] = (double)verts[3 * g]; plane[3 * g + 1] = (double)verts[3 * g + 1]; plane[3 * g + 2] = (double)verts[3 * g + 2];
  bool p = mask && mask[g] != 0;
  if (pin_border && !p) {
    const int* row = vrow + voff[b] + b;
    const int s = row[v];
    p = smooth_border(faces + 3 * foff[b], adj + 3 * foff[b], vface + 3 * foff[b] + s, row[v + 1] - s, (int)v);
  }
  pin[g] = p ? 1 : 0;
}

// x: the plane whose neighbours are gathered; y: the plane read at the vertex itself in MODE 2 (p); out: the plane written; bout: b in
// MODE 1.  a: lambda or mu (MODE 0), alpha (MODE 1), beta (MODE 2).  x, y, out and bout are different planes.
template <int MODE>
__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_round(const float* __restrict__ verts, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ nrow,
               const int* __restrict__ nbr, const double* __restrict__ w, const int* __restrict__ pin, int weight, double a, const double* __restrict__ x,
               const double* __restrict__ y, double* __restrict__ out, double* __restrict__ bout) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SMOOTH_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int* nr = nrow + voff[b] + b;
  const int s = nr[v], n = nr[v + 1] - s;
  const size_t at = 6 * (size_t)foff[b] + (size_t)s, g = (size_t)(voff[b] + v);
  const bool pinned = pin[g] != 0;
  const double* xm = x + 3 * (size_t)voff[b];
  double m[3];
  smooth_mean(nbr + at, w + at, n, weight, pinned, xm, (int)v, m);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double xv = xm[3 * (size_t)v + c];
    if (MODE == 0) out[3 * g + c] = smooth_step(xv, m[c], a);
    if (MODE == 1) {
      out[3 * g + c] = m[c];
      bout[3 * g + c] = pinned ? 0.0 : smooth_hc_b(m[c], (double)verts[3 * g + c], xv, a);
    }
    if (MODE == 2) out[3 * g + c] = smooth_hc_p(y[3 * g + c], xv, m[c], a);
  }
}

// START: the corners are P0, the widened "verts"; else those of `plane`.  The pivot is P0 of vertex 0 either way.
template <bool START>
__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_vol(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
             const double* __restrict__ plane, double* __restrict__ part /* B x gridDim.x x SH_SMO_TERMS */) {
  __shared__ double slot[SH_SMOOTH_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b];
  if ((long long)blockIdx.x * SH_SMOOTH_BLOCK >= nf) return;      // (uniform in the workgroup)
  const long long fi = (long long)blockIdx.x * SH_SMOOTH_BLOCK + tid;
  double t[SH_MASS_TERMS];
#pragma unroll
  for (int i = 0; i < SH_MASS_TERMS; ++i) t[i] = 0.0;
  if (fi < nf) {
    const float* vb = verts + 3 * voff[b];
    const int* f = faces + 3 * (foff[b] + fi);
    const double o[3] = {(double)vb[0], (double)vb[1], (double)vb[2]};
    double P[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) P[k][c] = START ? (double)vb[3 * (size_t)f[k] + c] : plane[3 * ((size_t)voff[b] + (size_t)f[k]) + c];
    mass_face_terms(o, P[0], P[1], P[2], t);
  }
  double* row = part + ((size_t)b * gridDim.x + blockIdx.x) * SH_SMO_TERMS;
#pragma unroll
  for (int j = 0; j < SH_SMO_TERMS; ++j) {
    const double r = smooth_tree(t[13 + j], slot, tid);
    if (tid == 0) row[j] = r;
  }
}

__global__ void __launch_bounds__(64)
k_smooth_scale(const float* __restrict__ verts, const long long* __restrict__ voff, const long long* __restrict__ foff, const double* __restrict__ part0,
               const double* __restrict__ part1, int blocks /* rows per mesh */, int keep_volume, double* __restrict__ head /* B x SH_SMO_HEAD */,
               SmoothInfo* __restrict__ info /* B */) {
  __shared__ double tot[2 * SH_SMO_TERMS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b];
  long long nblk = (nf + SH_SMOOTH_BLOCK - 1) / SH_SMOOTH_BLOCK;
  if (nblk > blocks) nblk = blocks;
  if (tid < 2 * SH_SMO_TERMS) {
    const double* part = tid < SH_SMO_TERMS ? part0 : part1;
    const int j = tid % SH_SMO_TERMS;
    double s = 0.0;
    for (long long blk = 0; blk < nblk; ++blk) s += part[((size_t)b * blocks + blk) * SH_SMO_TERMS + j];
    tot[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double T0[SH_SMO_TERMS], T1[SH_SMO_TERMS], o[3] = {0.0, 0.0, 0.0}, hd[SH_SMO_HEAD], vb, va;
  for (int j = 0; j < SH_SMO_TERMS; ++j) { T0[j] = tot[j]; T1[j] = tot[SH_SMO_TERMS + j]; }
  if (voff[b + 1] > voff[b]) {
    const float* p = verts + 3 * voff[b];
    o[0] = (double)p[0]; o[1] = (double)p[1]; o[2] = (double)p[2];
  }
  const int status = smooth_scale(T0, T1, o, keep_volume != 0, &vb, &va, hd);
  for (int i = 0; i < SH_SMO_HEAD; ++i) head[(size_t)b * SH_SMO_HEAD + i] = hd[i];
  info[b].volume_before = vb; info[b].volume_after = va; info[b].scale = hd[3]; info[b].status = status;
}

__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_apply(const float* __restrict__ verts, const long long* __restrict__ voff, const double* __restrict__ plane, const double* __restrict__ head,
               double* __restrict__ pos, double* __restrict__ rows /* B x gridDim.x x 2 */) {
  __shared__ double slot[SH_SMOOTH_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nv = voff[b + 1] - voff[b];
  if ((long long)blockIdx.x * SH_SMOOTH_BLOCK >= nv) return;      // (uniform in the workgroup)
  const long long v = (long long)blockIdx.x * SH_SMOOTH_BLOCK + tid;
  double d2 = 0.0, far = 0.0;
  if (v < nv) {
    const size_t g = (size_t)(voff[b] + v);
    const double* hd = head + (size_t)b * SH_SMO_HEAD;
    const bool scale = hd[4] != 0.0;
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p = plane[3 * g + c], q = scale ? smooth_scaled(p, hd[c], hd[3]) : p;
      pos[3 * g + c] = q;
      d[c] = q - (double)verts[3 * g + c];
    }
    d2 = dot3(d, d);
    far = smooth_disp(d2);
  }
  const double sum = smooth_tree(d2, slot, tid);
  slot[tid] = far;
  __syncthreads();
  for (int h = SH_SMOOTH_BLOCK / 2; h >= 1; h >>= 1) {
    if (tid < h && slot[tid + h] > slot[tid]) slot[tid] = slot[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    double* row = rows + ((size_t)b * gridDim.x + blockIdx.x) * 2;
    row[0] = sum; row[1] = slot[0];
  }
}

__global__ void __launch_bounds__(SH_SMOOTH_BLOCK)
k_smooth_info(const long long* __restrict__ voff, const int* __restrict__ nrow, const int* __restrict__ pin, const double* __restrict__ rows,
              int blocks /* rows per mesh */, SmoothInfo* __restrict__ info /* B */) {
  __shared__ int cnt[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long nv = voff[b + 1] - voff[b];
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  const int* nr = nrow + voff[b] + b;
  int pinned = 0, isolated = 0;
  for (long long v = tid; v < nv; v += SH_SMOOTH_BLOCK) {
    pinned += pin[voff[b] + v] != 0 ? 1 : 0;
    isolated += nr[v + 1] == nr[v] ? 1 : 0;
  }
  if (pinned) atomicAdd(&cnt[0], pinned);
  if (isolated) atomicAdd(&cnt[1], isolated);
  __syncthreads();
  if (tid != 0) return;
  long long nblk = (nv + SH_SMOOTH_BLOCK - 1) / SH_SMOOTH_BLOCK;
  if (nblk > blocks) nblk = blocks;
  double sum = 0.0, far = 0.0;
  for (long long blk = 0; blk < nblk; ++blk) {
    const double* row = rows + ((size_t)b * blocks + blk) * 2;
    sum += row[0];
    far = row[1] > far ? row[1] : far;
  }
  info[b].max_disp = far; info[b].sum_sq_disp = sum;
  info[b].pinned = cnt[0]; info[b].isolated = cnt[1];
  info[b].pad[0] = 0; info[b].pad[1] = 0; info[b].pad[2] = 0;
}

}  // namespace sh
