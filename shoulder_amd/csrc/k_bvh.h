// k_bvh.h -- the face hierarchy of the resident batch (include/shoulder_hip.h sh_mesh_bvh) and the closest-point walk that descends it
// (sh_set_query_accel).  The scalar rules are sh_scalar.h bvh_*; the index is the same bytes on the device, in the host twin and in
// tests/bvh_oracle.py.  Build grids are (block of SH_BVH_BLOCK = 256 faces or nodes, mesh), one per lane.
//   k_bvh_class   (block, mesh).  A face is loose or tight (bvh_face_loose).  The tight faces' corners go into the mesh's box -- minima and
//                 maxima of topo_enc words, first in LDS, then six integer atomics per workgroup into "bvh.state" -- and are counted.
//   k_bvh_key     (block, mesh).  The sort key of every face (bvh_key) from the finished box into "bvh.key".
//   (sort)        rocprim::segmented_radix_sort_keys, one segment per mesh, "bvh.key" -> "bvh.sorted".  The key (code, id) is unique, so
//                 any correct sort gives these bytes; the loose faces carry a code above every other and come out behind the tight
//                 ones, ascending by id.  rocPRIM because a long run of equal codes (a mesh in one cell) must not cost more than any
//                 other input, which a rank by counting smaller entries (k_topo_rows) would not give.
//   k_bvh_emit    (block, mesh).  "bvh.order", "bvh.loose" (tails -1) and "bvh.tri" from the sorted keys; the first lane of a mesh writes
//                 its row of "bvh.off" (bvh_off_row) and its sh_bvh_info.
//   k_bvh_leaves  (block of leaves, mesh).  The box of a leaf from its entries of "bvh.tri".
//   k_bvh_level   (block of nodes, mesh), once per level above the leaves, for as many levels as the largest mesh could have.
//   k_cp_tree     (chunk of SH_BVH_CHUNK = 64 points, mesh): one wave, one query point per lane, held in registers with its best
//                 (d2, face).  A lane owns a stack of SH_BVH_STACK node words (level << 28 | node) in LDS, laid out [depth][lane]: the
//                 lanes of a wave hit 64 different banks, and no dynamically indexed private array goes to scratch.  The descent is
//                 sh_scalar.h bvh_descend, the function the host twin runs: pop a node, test its box again (the best may have fallen
//                 since it was pushed); a leaf folds its entries of "bvh.tri" into the best with closest_pt_tri and closest_key_less;
//                 an inner node pushes the children whose box survives, the nearest one last, so it is descended first.  The loose
//                 faces are walked at the end from the mesh itself (cp_face).  The lane
//                 writes one CpPart {d2, face}: k_cp_join (k_closest.h) with S = 1 finishes the record as it does behind k_cp_walk.
// No floating-point atomics; no lane talks to another.  Every index is below its array's size by construction: "bvh.off" is written
// from the counts of the same build, a node word is formed from it alone, and the depth of a stack is bounded by SH_BVH_STACK for every
// tree the upload admits (static_asserts of sh_scalar.h).
//
// THE PRUNING RULE (bvh_box_skip).  The result must be the bytes of the walk over all faces, so a node may be skipped only if the d2 that
// closest_pt_tri would COMPUTE for every face in it is strictly above the lane's best (a tie with a smaller face id must survive).  A
// lane skips a node with box [lo, hi] (float32, widened) when
//     near2 > ((best_r + pad)^2) (1 + 2^-20)   and   far2 <= 1e8,
// near2 = the squared distance from p to the box and far2 = that to its farthest corner, both as computed in float64, best_r =
// sqrt(best d2) (1 + 2^-40), pad = (max(|lo_x|, |hi_x|) + .. y + .. z) 2^-40.  This is (1) - (4) of k_closest.h with the sphere (c, R)
// replaced by the box:
//   (1) closest_pt_tri returns fl(|p - q|^2) for a computed q that lies in the triangle up to the rounding of tri_point, a few ulp of
//       |A| + |ab| + |ac|.  Every corner of every face of the node is inside the box, and so is the triangle (a box is convex);
//       |A| + |ab| + |ac| <= 5 (m_x + m_y + m_z), m the largest absolute coordinate of the box per axis, so q is within
//       pad / 100 of the box: pad is about 1e-9 mm at 1000 mm against 1e-12 mm needed.
//   (2) then |p - q| >= dist(p, box) - pad, and with the skip condition dist(p, box) >= sqrt(near2) (1 - 3 ulp) > (best_r + pad)
//       (1 + 2^-21 - 3 ulp), so |p - q| > best_r (1 + 2^-22) and fl(|p - q|^2) >= |p - q|^2 (1 - 4 ulp) > best d2.  (The differences
//       lo - p and p - hi are single roundings of exact float64 operands; the margin of 2^-20 on the square is ten thousand million ulp.)
//   (3) the interior branch reached with a va, vb or vc that is not positive leaves the triangle by at most ~64 ulp D^2 / g at a
//       distance D.  A face with g < 2^-7 mm is LOOSE: it is in no node, and every lane tests it.  For the tight faces the excursion is
//       below 1e-12 D^2 mm and the margin leaves D 2^-21 mm: enough up to D = 1e4 mm.  The bound must hold for EVERY face of the node,
//       and the farthest any of them can be is the box's far corner: hence far2 <= 1e8.  Beyond ten metres nothing is skipped.
//   (4) a best that is not yet set is +inf: best_r + pad = +inf and nothing is skipped.
#pragma once
#include "k_closest.h"

#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace sh {

#define SH_BVH_BLOCK 256
#define SH_BVH_HEAD 8            // words of a mesh in "bvh.state": lo[3] and hi[3] as topo_enc words (start: ~0 and 0), the tight faces, 0
#define SH_BVH_W_TIGHT 6
#define SH_BVH_CHUNK 64          // points per workgroup of k_cp_tree: one wave

static_assert(sizeof(sh_bvh_info) == SH_BVH_INFO_BYTES && offsetof(sh_bvh_info, lo) == 24, "sh_bvh_info");

// the corners of face fi of mesh b, as stored
__device__ __forceinline__ void bvh_corners(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                            const long long* __restrict__ foff, int b, long long fi, const float** v0, const float** v1, const float** v2) {
  const int* f = faces + 3 * (foff[b] + fi);
  const float* vb = verts + 3 * voff[b];
  *v0 = vb + 3 * (size_t)f[0]; *v1 = vb + 3 * (size_t)f[1]; *v2 = vb + 3 * (size_t)f[2];
}

__global__ void __launch_bounds__(SH_BVH_BLOCK)
k_bvh_class(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
            unsigned* __restrict__ state) {
  __shared__ unsigned s_box[6];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_BVH_BLOCK;
  if (f0 >= nf) return;      // (uniform in the workgroup)
  if (tid < 6) s_box[tid] = tid < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  const long long fi = f0 + tid;
  int tight = 0;
  if (fi < nf) {
    const float *v0, *v1, *v2;
    bvh_corners(verts, faces, voff, foff, b, fi, &v0, &v1, &v2);
    if (!bvh_face_loose(v0, v1, v2)) {
      tight = 1;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const unsigned e0 = topo_enc(v0[k]), e1 = topo_enc(v1[k]), e2 = topo_enc(v2[k]);
        atomicMin(&s_box[k], min(e0, min(e1, e2)));
        atomicMax(&s_box[3 + k], max(e0, max(e1, e2)));
      }
    }
  }
  const int n = __syncthreads_count(tight);
  if (n == 0) return;      // (uniform)
  unsigned* head = state + (size_t)b * SH_BVH_HEAD;
  if (tid < 3) atomicMin(head + tid, s_box[tid]);
  else if (tid < 6) atomicMax(head + tid, s_box[tid]);
  else if (tid == 6) atomicAdd(head + SH_BVH_W_TIGHT, (unsigned)n);
}

__global__ void __launch_bounds__(SH_BVH_BLOCK)
k_bvh_key(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
          const unsigned* __restrict__ state, unsigned long long* __restrict__ key /* sumF */) {
  const int b = blockIdx.y;
  const long long nf = foff[b + 1] - foff[b], fi = (long long)blockIdx.x * SH_BVH_BLOCK + threadIdx.x;
  if (fi >= nf) return;
  const unsigned* head = state + (size_t)b * SH_BVH_HEAD;
  const float lo[3] = {topo_dec(head[0]), topo_dec(head[1]), topo_dec(head[2])}, hi[3] = {topo_dec(head[3]), topo_dec(head[4]), topo_dec(head[5])};
  const float *v0, *v1, *v2;
  bvh_corners(verts, faces, voff, foff, b, fi, &v0, &v1, &v2);
  const bool loose = bvh_face_loose(v0, v1, v2);
  key[foff[b] + fi] = bvh_key(loose, loose ? 0u : bvh_face_code(v0, v1, v2, lo, hi), (int)fi);
}

__global__ void __launch_bounds__(SH_BVH_BLOCK)
k_bvh_emit(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
           const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ state, const int* __restrict__ base /* B */, int* __restrict__ order,
           int* __restrict__ loose, float* __restrict__ tri, int* __restrict__ off, sh_bvh_info* __restrict__ info) {
  const int b = blockIdx.y;
  const long long f0 = foff[b], nf = foff[b + 1] - f0, i = (long long)blockIdx.x * SH_BVH_BLOCK + threadIdx.x;
  if (i >= nf) return;
  const unsigned* head = state + (size_t)b * SH_BVH_HEAD;
  const long long T = (long long)head[SH_BVH_W_TIGHT];      // (<= nf: it counted faces of this mesh)
  const int id = (int)(unsigned)(sorted[f0 + i] & 0xffffffffull);
  if (i < T) {
    order[f0 + i] = id;
    const float *v0, *v1, *v2;
    bvh_corners(verts, faces, voff, foff, b, id, &v0, &v1, &v2);      // (id < nf: a key of this mesh's segment)
    float* t = tri + 9 * (size_t)(f0 + i);
#pragma unroll
    for (int k = 0; k < 3; ++k) { t[k] = v0[k]; t[3 + k] = v1[k]; t[6 + k] = v2[k]; }
  } else order[f0 + i] = -1;
  loose[f0 + i] = i < nf - T ? (int)(unsigned)(sorted[f0 + T + i] & 0xffffffffull) : -1;
  if (i == 0) {
    int row[SH_BVH_OFF_WORDS];
    bvh_off_row((int)T, (int)(nf - T), base[b], row);
    for (int k = 0; k < SH_BVH_OFF_WORDS; ++k) off[(size_t)b * SH_BVH_OFF_WORDS + k] = row[k];
    sh_bvh_info r;
    r.tight = row[0]; r.loose = row[1]; r.leaves = row[2]; r.levels = row[3]; r.nodes = row[4]; r.reserved = 0;
    for (int k = 0; k < 3; ++k) { r.lo[k] = T > 0 ? topo_dec(head[k]) : 0.0f; r.hi[k] = T > 0 ? topo_dec(head[3 + k]) : 0.0f; }
    info[b] = r;
  }
}

__global__ void __launch_bounds__(SH_BVH_BLOCK)
k_bvh_leaves(const long long* __restrict__ foff, const float* __restrict__ tri, const int* __restrict__ off, float* __restrict__ box) {
  const int b = blockIdx.y;
  const int* row = off + (size_t)b * SH_BVH_OFF_WORDS;
  const int T = row[0], leaves = row[2], j = (int)(blockIdx.x * SH_BVH_BLOCK + threadIdx.x);
  if (j >= leaves) return;
  const float* t = tri + 9 * (size_t)foff[b];
  const int i0 = j * SH_BVH_LEAF, i1 = i0 + SH_BVH_LEAF < T ? i0 + SH_BVH_LEAF : T;
  float bx[6];
  for (int k = 0; k < 3; ++k) bx[k] = bx[3 + k] = t[9 * (size_t)i0 + k];
  for (int i = i0; i < i1; ++i)
    for (int c = 0; c < 3; ++c) bvh_box_point(bx, t + 9 * (size_t)i + 3 * c);
  float* o = box + 6 * ((size_t)row[5] + (size_t)j);      // (level 0 starts at the mesh's first node)
  for (int k = 0; k < 6; ++k) o[k] = bx[k];
}

__global__ void __launch_bounds__(SH_BVH_BLOCK)
k_bvh_level(const int* __restrict__ off, float* __restrict__ box, int level /* >= 1 */) {
  const int b = blockIdx.y;
  const int* row = off + (size_t)b * SH_BVH_OFF_WORDS;
  if (level >= row[3]) return;      // (uniform in the workgroup)
  const int* lv = row + SH_BVH_OFF_LEVEL;
  const int n = lv[level + 1] - lv[level], below = lv[level] - lv[level - 1], j = (int)(blockIdx.x * SH_BVH_BLOCK + threadIdx.x);
  if (j >= n) return;
  const float* ch = box + 6 * ((size_t)row[5] + (size_t)lv[level - 1]);
  const int c0 = j * SH_BVH_WIDTH, c1 = c0 + SH_BVH_WIDTH < below ? c0 + SH_BVH_WIDTH : below;
  float bx[6];
  for (int k = 0; k < 6; ++k) bx[k] = ch[6 * (size_t)c0 + k];
  for (int c = c0 + 1; c < c1; ++c) bvh_box_box(bx, ch + 6 * (size_t)c);
  float* o = box + 6 * ((size_t)row[5] + (size_t)lv[level] + (size_t)j);
  for (int k = 0; k < 6; ++k) o[k] = bx[k];
}

// a lane's stack: word i of lane l at [i][l], so the lanes of a wave hit different banks whatever their depths
struct LdsStack {
  unsigned (*s)[SH_BVH_CHUNK];
  int lane;
  __device__ __forceinline__ unsigned& at(int i) { return s[i][lane]; }
};

__global__ void __launch_bounds__(SH_BVH_CHUNK)
k_cp_tree(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
          const int* __restrict__ order, const int* __restrict__ loose, const int* __restrict__ off, const float* __restrict__ box,
          const float* __restrict__ tri, const double* __restrict__ points /* Q x 3, or B x Q x 3 */, int Q, int per_humerus,
          CpPart* __restrict__ part /* B x Q */) {
  __shared__ unsigned s_stack[SH_BVH_STACK][SH_BVH_CHUNK];
  __shared__ int s_row[SH_BVH_OFF_WORDS];
  const int b = blockIdx.y, lane = threadIdx.x;
  if (lane < SH_BVH_OFF_WORDS) s_row[lane] = off[(size_t)b * SH_BVH_OFF_WORDS + lane];
  __syncthreads();
  const int q = (int)blockIdx.x * SH_BVH_CHUNK + lane;
  if (q >= Q) return;      // (no barrier below)
  const double* pg = points + 3 * ((per_humerus ? (size_t)b * Q : (size_t)0) + (size_t)q);
  const double p[3] = {pg[0], pg[1], pg[2]};
  const int nl = s_row[1];
  const float* bx = box + 6 * (size_t)s_row[5];
  const float* tr = tri + 9 * (size_t)foff[b];
  const int* ord = order + foff[b];
  double best = INFINITY;
  int best_f = -1;
  LdsStack st{s_stack, lane};
  bvh_descend<false>(p, s_row, bx, tr, ord, st, &best, &best_f, nullptr);
  const int* lf = loose + foff[b];
  for (int i = 0; i < nl; ++i) {
    const int f = lf[i];
    double A[3], ab[3], ac[3], u, w;
    int region;
    cp_face(verts, faces, voff, foff, b, f, A, ab, ac);
    const double d2 = closest_pt_tri(p, A, ab, ac, &u, &w, &region);
    if (closest_key_less(d2, f, best, best_f)) { best = d2; best_f = f; }
  }
  CpPart o; o.d2 = best; o.face = best_f; o.pad = 0;
  part[(size_t)b * Q + q] = o;
}

}  // namespace sh
