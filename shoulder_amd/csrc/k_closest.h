// k_closest.h -- closest surface points of the resident batch (include/shoulder_hip.h sh_closest_points): for every (humerus, query
// point) the smallest (d2, face) over the faces of the humerus, d2 by sh_scalar.h closest_pt_tri.  Brute force over the faces with a
// conservative cull; a minimum under a total order (closest_key_less) does not depend on the order or the grouping of its candidates,
// so no lane talks to another: no floating-point atomics, no floating-point sums across lanes, and a (humerus, point) result depends
// on that mesh and that point alone -- not on the batch, the point list, the face split or the tiling.
//   k_cp_walk   (chunk of 256 points, humerus, face split s of S) workgroups of 256 lanes.  One query point per lane, held in
//               registers with its running best (d2, face).  The workgroup walks the tiles cp_split_range(tiles, S, s) of the humerus:
//               the lanes load the 256 faces of a tile together (resect_tile_face: the float32 vertices widened) and put them into LDS
//               as (A, ab, ac), 72 B per face, beside a bounding sphere of 32 B.  Then every lane reads the same LDS address face
//               after face (one address: a broadcast, no bank conflicts) and folds closest_pt_tri into its best.  At the end each lane
//               writes one partial {d2, face} to "cp.part"[b][q][s].  A call with few points wastes lanes: Q = 4 costs what Q = 256 costs.
//   k_cp_join   one thread per (humerus, point): the minimum of the S partials under the same order, closest_pt_tri once more on the
//               winning face from the mesh, and the sh_closest; without a finite candidate SH_ERR_GEOMETRY_DEV, face -1, zeros.
//
// THE CULL.  Beside (A, ab, ac) a tile holds for each face a sphere (c, R): c the centroid, R >= the largest distance from c to a
// corner.  A lane skips face j when  dc2 > ((best_r + R)^2) (1 + 2^-20)  and dc2 <= 1e8, dc2 = |p - c|^2 as computed and best_r =
// sqrt(best d2) (1 + 2^-40).  The result must be the bytes of the walk without the cull, so a face may be skipped only if the d2 that
// closest_pt_tri would COMPUTE for it is strictly above the lane's best (a tie with a smaller face id must survive: strictly).
//   (1) closest_pt_tri returns fl(|p - q|^2) for a computed q.  In the vertex and edge branches q is a convex combination of the
//       corners by the branch's own guards (u, w in [0, 1], u + w = 1 on BC), and so it is in the interior branch when va, vb, vc are all
//       positive: q lies in the triangle up to the rounding of tri_point, at most a few ulp of |A| + |ab| + |ac|.  R is widened for
//       that at staging: R = r (1 + 2^-30) + (|c|_1 + r) 2^-40, about 1e-9 mm at |c| = 1000 mm against 1e-13 mm needed.
//   (2) then |p - q| >= |p - c| - R, and with the skip condition |p - c| >= sqrt(dc2) (1 - 3 ulp) > (best_r + R) (1 + 2^-21 - 3 ulp), so
//       |p - q| > best_r (1 + 2^-22) and fl(|p - q|^2) >= |p - q|^2 (1 - 4 ulp) > best d2.  The margin of 2^-20 on the square is ten
//       thousand million ulp; it costs nothing (a sphere within a millionth of the best distance is walked instead of skipped).
//   (3) the interior branch reached with a va, vb or vc that is not positive (possible only when that product lies within its own
//       rounding of zero, |v| <= ~32 ulp |ab| |ac| D^2 at a distance D) leaves the triangle by at most ~64 ulp D^2 / g,
//       g = |ab x ac|^2 / Lmax^3 (about the shortest height times its sine).  A face with g < 2^-7 mm -- slivers, collinear and point
//       triangles -- gets R = +inf and is never skipped.  For the others the excursion is below 1e-12 D^2 mm, and the margin leaves
//       D 2^-21 = 4.8e-7 D mm: enough up to D = 1e4 mm, hence dc2 <= 1e8.  Beyond ten metres nothing is skipped.
//   (4) a best that is not yet set is +inf: best_r + R = +inf and nothing is skipped.
// Nearly every face is skipped for eleven operations once the best is small; the exact test is about a hundred with up to one division.
#pragma once
#include "k_resect.h"

namespace sh {

#define SH_CP_TILE SH_RS_TILE
#define SH_CP_CHUNK 256      // points per workgroup: one per lane

struct __attribute__((aligned(16))) CpPart { double d2; int face, pad; };      // one partial in "cp.part"
static_assert(sizeof(CpPart) == 16, "CpPart must be 16 bytes");
static_assert(sizeof(sh_closest) == 48, "sh_closest is four doubles and four int32");
static_assert(SH_CP_TILE == SH_CP_CHUNK, "k_cp_walk: a lane stages one face and owns one point");

// face fi of humerus b as (A, ab, ac): the float32 vertices widened as resect_tile_face widens them
__device__ __forceinline__ void cp_face(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                        const long long* __restrict__ foff, int b, long long fi, double* A, double* ab, double* ac) {
  const int* f = faces + 3 * (foff[b] + fi);
  const float* vb = verts + 3 * voff[b];
  const float *v0 = vb + 3 * (size_t)f[0], *v1 = vb + 3 * (size_t)f[1], *v2 = vb + 3 * (size_t)f[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) { A[k] = (double)v0[k]; ab[k] = (double)v1[k] - A[k]; ac[k] = (double)v2[k] - A[k]; }
}

__global__ void __launch_bounds__(SH_CP_CHUNK)
k_cp_walk(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
          const double* __restrict__ points /* Q x 3, or B x Q x 3 */, int Q, int per_humerus, int S, CpPart* __restrict__ part /* B x Q x S */) {
  __shared__ double s_tri[SH_CP_TILE][9];      // A, ab, ac
  __shared__ double s_sph[SH_CP_TILE][4];      // c, R
  const int b = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
  const int q = (int)blockIdx.x * SH_CP_CHUNK + tid;
  const bool has = q < Q;      // (a lane without a point still stages its face; it walks point 0 of the chunk's humerus and stores nothing)
  const double* pg = points + 3 * ((per_humerus ? (size_t)b * Q : (size_t)0) + (size_t)(has ? q : 0));
  const double p[3] = {pg[0], pg[1], pg[2]};
  double best = INFINITY, best_r = INFINITY;
  int best_f = -1;
  const long long nf = foff[b + 1] - foff[b];
  const int tiles = (int)((nf + SH_CP_TILE - 1) / SH_CP_TILE);
  int t0, t1;
  cp_split_range(tiles, S, s, &t0, &t1);
  for (int t = t0; t < t1; ++t) {      // (uniform in the workgroup)
    bool live; long long fi; double V[9];
    (void)resect_tile_face(verts, faces, voff, foff, b, t, tid, &live, &fi, V);      // (t < tiles: the tile is there)
    __syncthreads();      // the walk of the tile before is over
    {
      double* tr = s_tri[tid];
      const double ab[3] = {V[3] - V[0], V[4] - V[1], V[5] - V[2]}, ac[3] = {V[6] - V[0], V[7] - V[1], V[8] - V[2]};
      const double bc[3] = {ac[0] - ab[0], ac[1] - ab[1], ac[2] - ab[2]};
      double c[3], da[3], db[3], dc[3], n[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        tr[k] = V[k]; tr[3 + k] = ab[k]; tr[6 + k] = ac[k];
        c[k] = V[k] + (ab[k] + ac[k]) * (1.0 / 3.0);
        da[k] = V[k] - c[k]; db[k] = da[k] + ab[k]; dc[k] = da[k] + ac[k];
      }
      const double r = sqrt(fmax(dot3(da, da), fmax(dot3(db, db), dot3(dc, dc))));
      cross3(ab, ac, n);
      const double l2 = fmax(dot3(ab, ab), fmax(dot3(ac, ac), dot3(bc, bc)));
      const double g = dot3(n, n) / (l2 * sqrt(l2));
      double R = r * (1.0 + 0x1p-30) + (((fabs(c[0]) + fabs(c[1])) + fabs(c[2])) + r) * 0x1p-40;
      if (!(g >= 0x1p-7)) R = INFINITY;
      double* sp = s_sph[tid];
      sp[0] = c[0]; sp[1] = c[1]; sp[2] = c[2]; sp[3] = R;
    }
    __syncthreads();
    const long long f0 = (long long)t * SH_CP_TILE;
    const int n = (int)(nf - f0 < SH_CP_TILE ? nf - f0 : SH_CP_TILE);
    for (int j = 0; j < n; ++j) {
      const double* sp = s_sph[j];      // (the same address in every lane)
      const double dx = p[0] - sp[0], dy = p[1] - sp[1], dz = p[2] - sp[2];
      const double dc2 = (dx * dx + dy * dy) + dz * dz;
      const double thr = best_r + sp[3];
      if (dc2 > (thr * thr) * (1.0 + 0x1p-20) && dc2 <= 1e8) continue;
      const double* tr = s_tri[j];
      const double A[3] = {tr[0], tr[1], tr[2]}, ab[3] = {tr[3], tr[4], tr[5]}, ac[3] = {tr[6], tr[7], tr[8]};
      double u, w;
      int region;
      const double d2 = closest_pt_tri(p, A, ab, ac, &u, &w, &region);
      const int f = (int)(f0 + j);
      if (closest_key_less(d2, f, best, best_f)) { best = d2; best_f = f; best_r = sqrt(d2) * (1.0 + 0x1p-40); }
    }
  }
  if (has) { CpPart o; o.d2 = best; o.face = best_f; o.pad = 0; part[((size_t)b * Q + q) * S + s] = o; }
}

__global__ void __launch_bounds__(256)
k_cp_join(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
          const double* __restrict__ points, int Q, int per_humerus, int S, const CpPart* __restrict__ part, long long n /* B x Q */,
          sh_closest* __restrict__ out /* B x Q */) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = (int)(i / Q), q = (int)(i - (long long)b * Q);
  const CpPart* pp = part + (size_t)i * S;
  double best = INFINITY;
  int best_f = -1;
  for (int s = 0; s < S; ++s) {
    const CpPart c = pp[s];
    if (c.face >= 0 && closest_key_less(c.d2, c.face, best, best_f)) { best = c.d2; best_f = c.face; }
  }
  sh_closest o;
  if (best_f < 0) {
    o.dist = 0.0; o.point[0] = 0.0; o.point[1] = 0.0; o.point[2] = 0.0; o.face = -1; o.region = 0; o.side = 0; o.status = SH_ERR_GEOMETRY_DEV;
  } else {
    const double* pg = points + 3 * ((per_humerus ? (size_t)b * Q : (size_t)0) + (size_t)q);
    const double p[3] = {pg[0], pg[1], pg[2]};
    double A[3], ab[3], ac[3], u, w, pt[3];
    int region;
    cp_face(verts, faces, voff, foff, b, best_f, A, ab, ac);
    const double d2 = closest_pt_tri(p, A, ab, ac, &u, &w, &region);
    tri_point(A, ab, ac, u, w, pt);
    const double r[3] = {p[0] - pt[0], p[1] - pt[1], p[2] - pt[2]};
    o.dist = sqrt(d2); o.point[0] = pt[0]; o.point[1] = pt[1]; o.point[2] = pt[2];
    o.face = best_f; o.region = region; o.side = closest_side(r, ab, ac); o.status = 0;
  }
  out[i] = o;
}

}  // namespace sh
