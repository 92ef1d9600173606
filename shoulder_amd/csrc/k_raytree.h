// k_raytree.h -- the rays of the resident batch through its face hierarchy (include/shoulder_hip.h sh_ray_cast with SH_ACCEL_BVH, and
// sh_ray_nearest).  The index is k_bvh.h's ("bvh.*"), the hit rule k_rays.h's (sh_scalar.h ray_tri_hit), the descent sh_scalar.h
// bvh_ray_descend -- the function the host twin runs (tests/hostcheck/raytree_check.cpp).  Grids are (chunk of SH_BVH_CHUNK = 64 rays,
// mesh): one wave, one ray per lane, its stack of SH_BVH_STACK node words in LDS as [depth][lane] (LdsStack of k_bvh.h: 64 banks, no
// private array that could go to scratch).
//   k_ray_tree<false>  the lane counts its hits -- the tree, then the loose faces from the mesh itself, as k_cp_tree walks them -- and
//                      stores counts[b][r] with a plain store.  No atomics: a ray belongs to one lane.
//   (k_ray_scan, the total to the host, "ray.pool": k_rays.h, unchanged)
//   k_ray_tree<true>   a lane with a non-zero count walks again and writes RayKeys at offs[i] + n++, each write guarded by
//                      slot < offs[i + 1] as the brute fill's; every lane stores cursor[i] = n (0 without a hit).
//   (k_ray_sort: k_rays.h, unchanged.  It ranks by the total key (t, face), so the order in the pool does not matter: "ray.hits" and
//   "ray.counts" are the bytes of the brute chain.)
//   k_ray_near         sh_ray_nearest with SH_ACCEL_BVH in one launch: the lane folds its hits into the least (t, face) under ray_key_less
//                      and writes the record, the point formed as k_ray_sort forms it; a miss is zero with face = -1.  No count, no scan,
//                      no pool, no sort, nothing read by the host before the result.
// sh_anp_axis_hits (the BOX variant of k_rays.h) stays on the brute walk in both modes: it casts four rays per humerus, and its corners are
// the vertices under "obb_transform", which the index does not hold.
// No lane talks to another; no floating-point atomics.  Indices: as k_cp_tree's -- "bvh.off" is written from the counts of the same build,
// a node word is formed from it alone, the stack depth is bounded by SH_BVH_STACK (static_asserts of sh_scalar.h).
//
// THE SKIP RULE (sh_scalar.h bvh_ray_box_skip).  The result must be the bytes of the walk over all faces, so a node may be skipped only if
// ray_tri_hit AS COMPUTED rejects every face in it.  A plain slab test is not that: ray_tri_hit accepts on the computed
// u >= 0, w >= 0, u + w <= 1, t > 1e-9 behind a division by det that is guarded by |det| > 1e-12 alone, and for a grazing ray the point it
// accepts can lie outside the triangle.  A lane skips a node with box [lo, hi] (float32, widened) when the half-line {o + s d, s >= 0}
// misses the box grown on every side by
//     pad = 2^-8 |d| D E^2 + 2^-40 m1
// (D: from o to the box's far corner; E: the box's diagonal; m1 = sum over the axes of max(|lo|, |hi|)), and skips nothing when |d|^2 or
// D^2 is above 2^40.  eps = 2^-53 below; -ffp-contract=off, so every operation rounds once.
//   (1) What the face is.  ray_tri_hit sees A, e1, e2 as float64.  A is a corner; e1 = fl(B - A) and e2 = fl(C - A) differ from the edges
//       by eps |e| at most.  All corners of all (tight) faces of the node are in the box, so |e1|, |e2| <= E (1 + eps) and
//       |tv| = |o - A| <= D.
//   (2) What is computed.  With N_u = tv . (d x e2), N_w = d . (tv x e1), N_t = e2 . (tv x e1), det = e1 . (d x e2), the computed values
//       differ from these by absolute errors that contain no division: a cross product's component is off by at most
//       2.01 eps (|a_j b_k| + |a_k b_j|), its vector by 3.5 eps |a| |b|; a dot product of three terms by 3.01 eps |a| |b|; tv by eps |tv|.
//       That gives |det_c - det| <= 6.5 eps |d| |e1| |e2| and |N_c - N| <= 7.5 eps |tv| |e1| |e2| (times |d| for N_u and N_w).
//   (3) Cramer's rule is an identity of polynomials, true whatever det is:  det tv = N_u e1 + N_w e2 - N_t d.  Put the computed numbers in:
//       with u~ = N_uc / det_c, w~ = N_wc / det_c and P~ = A + u~ e1 + w~ e2,
//           o + (N_t / det_c) d = P~ + r,   |r| <= (6.5 + 7.5 + 7.5) eps |d| |tv| |e1| |e2| / |det_c|.
//       An accepted face has computed u, w >= 0 and fl(u + w) <= 1; u = fl(N_uc fl(1 / det_c)) has the sign of u~ and differs from it by
//       2.01 eps relative, so P~ is in the triangle up to 3.1 eps (|e1| + |e2|), and in the box up to 8 eps E.
//   (4) The half-line.  The accepted t_c = fl(N_tc / det_c) > 1e-9 > 0, and N_t / det_c >= N_tc / det_c - 7.5 eps |tv| |e1| |e2| / |det_c|: the
//       point of (3) lies on the half-line, or behind o by at most 7.5 eps |d| |tv| |e1| |e2| / |det_c|, and then o itself is that near.
//   (5) The only thing known about det_c of an accepted face is |det_c| > 1e-12 -- its size depends on the face's normal, which a node does
//       not state.  So the half-line passes within 29 eps |d| D E^2 / 1e-12 + 8 eps E = 3.22e-3 |d| D E^2 + 8 eps E of the box.
//       2^-8 = 3.91e-3 covers the first term with a fifth to spare, which takes the roundings of |d|, D, E^2 as computed (a few eps each)
//       and of lo - pad, hi + pad (eps pad); 2^-40 m1 = 9.1e-13 m1 covers 8 eps E <= 3.1e-15 m1 (E <= 2 sqrt 3 max |coordinate|) and
//       eps |lo|.  The pad is absolute, not a share of the box: where it exceeds the distance from o to the box the grown box holds o and
//       the test cannot skip -- that is the refusal for a long d, a far origin or a large node, and it needs no constant of its own.
//       At |d| = 1 and D = 50 mm a leaf of E = 3 mm is grown by 1.8 mm, a node of E = 12 mm by 28 mm; the upper levels are always entered.
//   (6) The slab test itself.  The reciprocals 1 / d_k are formed once per ray (bvh_ray_set).  Per axis with d_k != 0 and a finite
//       reciprocal: t1 = fl(fl(l - o_k) fl(1 / d_k)), t2 likewise, each within 3.01 eps relative of the true parameter and of its sign;
//       tn = max(0, min's), tf = min(max's).  The lane skips when tn > tf + |tf| 2^-40: then the true near parameter is above the true far
//       one (a negative tf is below tn >= 0: the box is behind the origin).  An axis with d_k = 0 has no parameters: the ray keeps o_k,
//       and it skips when o_k < l or o_k > h -- two comparisons of finite numbers, no 0 * inf, no 0 / 0.  An axis whose |d_k| is so small
//       that 1 / d_k overflows decides nothing: a finite difference is only ever multiplied by a finite, non-zero reciprocal, and an
//       axis left out can only skip less.  A box that is flat on an axis (a sheet mesh) is a slab of thickness 2 pad > 0 there (m1 > 0
//       for every box that holds a tight face: such a face has area).  A ray lying exactly in a face plane of the box has o_k = lo_k
//       or hi_k and d_k = 0: o_k is inside [l, h] by pad, that axis does not skip.  A product may overflow to +-inf: inf > finite skips
//       rightly, inf > inf and every comparison with a NaN are false.  The guards keep pad finite (|d|, D <= 2^20, E^2 <= 1.4e78 in
//       float32), so no NaN arises from finite rays; if one did, no comparison that skips would hold.
//   (7) Underflow.  An accepted face needs |det| > 1e-12 with |det| <= |d| E^2: impossible for |d| < 1e-90, so a |d|^2 that underflows
//       skips at worst what is rejected anyway.  Elsewhere an underflowing product adds 2^-1074 to an absolute error: below 2^-40 m1.
//   (8) The loose faces (slivers, point triangles) are in no node: every ray tests them from the mesh.  A mesh without tight faces has no
//       levels and is its loose list.
// PRUNING BY t (sh_ray_nearest only; built, with the same pad).  The point of (3) is in the grown box, so N_t / det_c is not below the
// parameter tn at which the half-line enters it, and by (4) the accepted t_c >= (tn (1 - 2.01 eps) - 0.22 pad / |d|)(1 - 2.01 eps).  The lane
// skips a node when (tn - pad / |d|)(1 - 2^-40) > best t: then every t_c in it is STRICTLY above the best, and a tie at equal t with a
// smaller face id is never skipped.  A best that is not set is +inf and skips nothing.  Children are pushed with the one entered first
// on top; a popped node is tested again, the best may have fallen.
#pragma once
#include "k_rays.h"
#include "k_bvh.h"

namespace sh {

// a ray's segment of "ray.pool": n counts every hit, a write needs room
struct RayHitFill {
  static constexpr bool PRUNE = false;
  RayKey* seg;
  unsigned long long room;
  int n;
  __device__ __forceinline__ double bound() const { return INFINITY; }
  __device__ __forceinline__ void operator()(double t, int f, int s) {
    if ((unsigned long long)(unsigned)n < room) { RayKey k; k.t = t; k.face = f; k.side = s; seg[n] = k; }
    ++n;
  }
};

// the loose faces of mesh b from the mesh itself, corners widened and edges taken as ray_walk takes them
template <typename Hit>
__device__ __forceinline__ void ray_loose(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                          const long long* __restrict__ foff, int b, const int* __restrict__ lf, int nl, const double* o, const double* d, Hit& hit) {
  for (int i = 0; i < nl; ++i) {
    const int f = lf[i];
    const float *v0, *v1, *v2;
    bvh_corners(verts, faces, voff, foff, b, f, &v0, &v1, &v2);
    const double A[3] = {(double)v0[0], (double)v0[1], (double)v0[2]};
    const double e1[3] = {(double)v1[0] - A[0], (double)v1[1] - A[1], (double)v1[2] - A[2]}, e2[3] = {(double)v2[0] - A[0], (double)v2[1] - A[1], (double)v2[2] - A[2]};
    double t = 0.0;
    int side = 0;
    if (ray_tri_hit(o, d, A, e1, e2, &t, &side)) hit(t, f, side);
  }
}

// tree, then loose list, of mesh b for the ray (o, d) of this lane; s_row: the mesh's words of "bvh.off" in LDS
template <typename Hit>
__device__ __forceinline__ void ray_tree_walk(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                              const long long* __restrict__ foff, const int* __restrict__ order, const int* __restrict__ loose,
                                              const float* __restrict__ box, const float* __restrict__ tri, const int* s_row, LdsStack& st, int b,
                                              const double* o, const double* d, Hit& hit) {
  bvh_ray_descend<false>(o, d, s_row, box + 6 * (size_t)s_row[5], tri + 9 * (size_t)foff[b], order + foff[b], st, hit, nullptr);
  ray_loose(verts, faces, voff, foff, b, loose + foff[b], s_row[1], o, d, hit);
}

template <bool FILL>
__global__ void __launch_bounds__(SH_BVH_CHUNK)
k_ray_tree(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
           const int* __restrict__ order, const int* __restrict__ loose, const int* __restrict__ off, const float* __restrict__ box,
           const float* __restrict__ tri, const double* __restrict__ rays, int R, int per_humerus, int* __restrict__ counts /* B x R */,
           const unsigned long long* __restrict__ offs /* B x R + 1 (FILL) */, int* __restrict__ cursor /* B x R (FILL) */, RayKey* __restrict__ pool) {
  __shared__ unsigned s_stack[SH_BVH_STACK][SH_BVH_CHUNK];
  __shared__ int s_row[SH_BVH_OFF_WORDS];
  const int b = blockIdx.y, lane = threadIdx.x;
  if (lane < SH_BVH_OFF_WORDS) s_row[lane] = off[(size_t)b * SH_BVH_OFF_WORDS + lane];
  __syncthreads();
  const int r = (int)blockIdx.x * SH_BVH_CHUNK + lane;
  if (r >= R) return;      // (no barrier below)
  const size_t i = (size_t)b * R + r;
  if (FILL && counts[i] == 0) { cursor[i] = 0; return; }
  const double* rg = rays + 6 * ((per_humerus ? (size_t)b * R : (size_t)0) + (size_t)r);
  const double o[3] = {rg[0], rg[1], rg[2]}, d[3] = {rg[3], rg[4], rg[5]};
  LdsStack st{s_stack, lane};
  if (!FILL) {
    RayHitCount h;
    ray_tree_walk(verts, faces, voff, foff, order, loose, box, tri, s_row, st, b, o, d, h);
    counts[i] = h.n;
  } else {
    const unsigned long long base = offs[i];
    RayHitFill h{pool + base, offs[i + 1] - base, 0};
    ray_tree_walk(verts, faces, voff, foff, order, loose, box, tri, s_row, st, b, o, d, h);
    cursor[i] = h.n;
  }
}

__global__ void __launch_bounds__(SH_BVH_CHUNK)
k_ray_near(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
           const int* __restrict__ order, const int* __restrict__ loose, const int* __restrict__ off, const float* __restrict__ box,
           const float* __restrict__ tri, const double* __restrict__ rays, int R, int per_humerus, sh_ray_hit* __restrict__ near /* B x R */) {
  __shared__ unsigned s_stack[SH_BVH_STACK][SH_BVH_CHUNK];
  __shared__ int s_row[SH_BVH_OFF_WORDS];
  const int b = blockIdx.y, lane = threadIdx.x;
  if (lane < SH_BVH_OFF_WORDS) s_row[lane] = off[(size_t)b * SH_BVH_OFF_WORDS + lane];
  __syncthreads();
  const int r = (int)blockIdx.x * SH_BVH_CHUNK + lane;
  if (r >= R) return;      // (no barrier below)
  const double* rg = rays + 6 * ((per_humerus ? (size_t)b * R : (size_t)0) + (size_t)r);
  const double o[3] = {rg[0], rg[1], rg[2]}, d[3] = {rg[3], rg[4], rg[5]};
  LdsStack st{s_stack, lane};
  RayHitNear h;
  ray_tree_walk(verts, faces, voff, foff, order, loose, box, tri, s_row, st, b, o, d, h);
  sh_ray_hit* out = near + ((size_t)b * R + r);
  if (h.face < 0) {      // zero with face = -1, the words k_ray_sort writes
    long long* w = (long long*)out;
    w[0] = 0; w[1] = 0; w[2] = 0; w[3] = 0; w[4] = 0x00000000ffffffffll;
    return;
  }
  out->t = h.t;
#pragma unroll
  for (int k = 0; k < 3; ++k) out->point[k] = o[k] + d[k] * h.t;
  out->face = h.face; out->side = h.side;
}

}  // namespace sh
