// k_resect.h -- batched head resection: B resident humeri x P planes, one measurement record per cut
// (`HumeralHeadOsteotomy`, reference src/shoulder/arthroplasty.py:13-175: `points()` :69-78, `resect_mesh()` :80-87 and what
// users compute from its result -- head volume, area, height; cut semantics of oracle/clip.py = k_clip.h).
//   k_resect_make_planes  sh_resect_offsets: the B x P planes from the device records (sh_scalar.h resect_plane_from_offsets)
//   k_resect_faces        one workgroup per (humerus, tile of SH_RS_TILE faces): the tile's faces and float32 vertices are loaded
//                         ONCE (-> float64 registers), then a loop over the humerus' planes (wave-uniform loads): sign of the three
//                         vertices, class of the face, its terms of volume / area / height.  Per (humerus, plane, tile) the terms
//                         are reduced inside the wave (fixed shuffle tree) and over the four waves in order and STORED (the slab);
//                         no floating-point atomics.  A tile is faces [256 t, 256 t + 256) of its humerus whatever the batch, so a
//                         humerus' partial sums do not depend on B, on its position in the batch or on P.  Every cut face appends
//                         its id to the cut's slot range: one integer atomic per (tile, plane) that has crossings, the slots of
//                         the tile handed out by ballot rank.
//   k_resect_join         one workgroup per cut: adds the cut's slab in a fixed order (lane-strided, shuffle tree) and joins the
//                         crossing segments into loops -- LDS hash join on edge keys, one pointer-jumping pass for the canonical
//                         start (rule B-1) and the rank of every segment (the scheme of slice_link_plane, k_slices.h, whose
//                         instantiations are untouched: this join computes 3-D crossings of a general plane from the face itself),
//                         loop areas in base.Section's basis, the largest loop's area / perimeter / centroid, the record.  With
//                         ring_out: the largest loop's points (sh_resect_ring joins one cut again).
// The mesh is read once for all P planes: bytes per humerus = faces (12 B) + gathered vertices, not times P.
#pragma once
#include "../../include/shoulder_hip.h"
#include "sh_scalar.h"
#include "sh_cutmath.h"

namespace sh {

#define SH_RS_TILE 256
#define SH_RS_JOIN_THREADS 256

struct __attribute__((aligned(16))) ResectPart { double vol, area, hmax; int n_cut, pad; };      // one (humerus, plane, tile)
static_assert(sizeof(ResectPart) == 32, "ResectPart must be 32 bytes");

__global__ void k_resect_make_planes(const sh_landmarks* __restrict__ lm, const double* __restrict__ offs /* P x 7 */, int P,
                                     double* __restrict__ planes /* B x P x 6 */, int* __restrict__ cut_status /* B x P */) {
  const int b = blockIdx.x;
  const sh_landmarks* L = lm + b;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    double pl[6] = {0, 0, 0, 0, 0, 0};
    int st = L->status;
    if (st == 0) {
      bool ok = resect_plane_from_offsets(L->csys_articular, L->anp_plane_point, L->anp_plane_normal, L->side, offs + 7 * p, pl, pl + 3);
      for (int k = 0; k < 6; ++k) ok = ok && isfinite(pl[k]);
      if (!ok || !((pl[3] * pl[3] + pl[4] * pl[4]) + pl[5] * pl[5] > 0.0)) st = SH_ERR_GEOMETRY_DEV;
    }
    double* o = planes + ((size_t)b * P + p) * 6;
    for (int k = 0; k < 6; ++k) o[k] = st == 0 ? pl[k] : 0.0;
    cut_status[(size_t)b * P + p] = st;
  }
}

// signs of a face's vertices and its class for one plane: slice_faces_plane's dots, tolerance and classes (k_clip.h), with the
// in-plane face decided by its normal
__device__ inline int resect_class(const double* V /* 3 x 3 */, const double* pl, int* s, double* d) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double dx = V[3 * j] - pl[0], dy = V[3 * j + 1] - pl[1], dz = V[3 * j + 2] - pl[2];
    d[j] = (dx * pl[3] + dy * pl[4]) + dz * pl[5];
    s[j] = d[j] < -SH_CLIP_TOL ? 1 : (d[j] > SH_CLIP_TOL ? -1 : 0);      // -1 = the normal's side (kept)
  }
  int k = clip_class(s[0], s[1], s[2]);
  if (k == 4) {
    const double ux = V[3] - V[0], uy = V[4] - V[1], uz = V[5] - V[2], vx = V[6] - V[0], vy = V[7] - V[1], vz = V[8] - V[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
    k = (nn > 1e-13 && ((nx / nn) * pl[3] + (ny / nn) * pl[4]) + (nz / nn) * pl[5] < 0.0) ? 1 : 0;
  }
  return k;
}

// det(a - o, b - o, c - o) (test_oracle_clip.volume_about's term: t0 . (t1 x t2)) and |(b - a) x (c - a)|
__device__ inline void resect_tri_terms(const double* a, const double* b, const double* c, const double* o, double* det, double* ar) {
  const double ax = a[0] - o[0], ay = a[1] - o[1], az = a[2] - o[2];
  const double bx = b[0] - o[0], by = b[1] - o[1], bz = b[2] - o[2];
  const double cx = c[0] - o[0], cy = c[1] - o[1], cz = c[2] - o[2];
  *det += (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  *ar += sqrt((nx * nx + ny * ny) + nz * nz);
}

// a lane's face of tile t of humerus b for k_resect_faces and k_headfit_faces: false when the tile lies behind the humerus' faces (uniform);
// else *live: the lane has a face, *fi its index in the humerus, V its float32 vertices widened (a lane without a face holds face 0)
__device__ __forceinline__ bool resect_tile_face(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                                 const long long* __restrict__ foff, int b, int t, int tid, bool* live, long long* fi, double* V /* 3 x 3 */) {
  const long long f0 = foff[b], nf = foff[b + 1] - f0;
  if ((long long)t * SH_RS_TILE >= nf) return false;
  *fi = (long long)t * SH_RS_TILE + tid;
  *live = *fi < nf;
  const int* f = faces + 3 * (f0 + (*live ? *fi : 0));
  const float* vb = verts + 3 * voff[b];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float* v = vb + 3 * (size_t)f[j];
    V[3 * j] = (double)v[0]; V[3 * j + 1] = (double)v[1]; V[3 * j + 2] = (double)v[2];
  }
  return true;
}

__global__ void __launch_bounds__(SH_RS_TILE)
k_resect_faces(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
               const double* __restrict__ planes /* B x P x 6 */, int P, int p0, int pc /* planes p0 .. p0 + pc of this pass */,
               int b0 /* first humerus of the grid */, int tstride /* tiles per humerus in the slab */,
               ResectPart* __restrict__ slab /* [grid.y][pc][tstride] */, int* __restrict__ seg_count /* [grid.y][pc] */,
               int* __restrict__ segs /* [grid.y][pc][SH_MAXSEG] face ids */) {
  __shared__ double s_red[2][SH_RS_TILE / 64][3];
  __shared__ int s_cnt[2][SH_RS_TILE / 64];
  __shared__ int s_base[2];
  const int bi = blockIdx.y, b = b0 + bi, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool live; long long fi; double V[9];
  if (!resect_tile_face(verts, faces, voff, foff, b, t, tid, &live, &fi, V)) return;      // (uniform)
  for (int q = 0; q < pc; ++q) {
    const double* plg = planes + ((size_t)b * P + (p0 + q)) * 6;
    const double pl[6] = {plg[0], plg[1], plg[2], plg[3], plg[4], plg[5]};      // (the same address in every lane)
    double det = 0.0, ar = 0.0, hm = 0.0;
    bool cut = false;
    if (live) {
      int s[3]; double d[3];
      const int k = resect_class(V, pl, s, d);
      hm = fmax(0.0, fmax(d[0], fmax(d[1], d[2])));
      if (k == 1) resect_tri_terms(V, V + 3, V + 6, pl, &det, &ar);
      else if (k == 2) {      // one vertex cut away: the quad's two triangles (a, b, n0), (n0, n1, a)
        const int qi = s[0] == 1 ? 0 : (s[1] == 1 ? 1 : 2);
        double n0[3], n1[3];
        clip_cross(V, (qi + 2) % 3, pl, n0);
        clip_cross(V, qi, pl, n1);
        const double* a = V + 3 * ((qi + 1) % 3); const double* bb = V + 3 * ((qi + 2) % 3);
        resect_tri_terms(a, bb, n0, pl, &det, &ar);
        resect_tri_terms(n0, n1, a, pl, &det, &ar);
        cut = true;
      } else if (k == 3) {    // one vertex kept: (v, m0, m1)
        const int ti = s[0] == -1 ? 0 : (s[1] == -1 ? 1 : 2);
        double m0[3], m1[3];
        clip_cross(V, ti, pl, m0);
        clip_cross(V, (ti + 2) % 3, pl, m1);
        resect_tri_terms(V + 3 * ti, m0, m1, pl, &det, &ar);
        cut = true;
      }
    }
    const unsigned long long bal = __ballot(cut);
    const int wc = __popcll(bal), rank = __popcll(bal & ((1ull << lane) - 1ull));
    for (int off = 32; off > 0; off >>= 1) {
      det += __shfl_down(det, off); ar += __shfl_down(ar, off); hm = fmax(hm, __shfl_down(hm, off));
    }
    const int bf = q & 1;
    if (lane == 0) { s_red[bf][wave][0] = det; s_red[bf][wave][1] = ar; s_red[bf][wave][2] = hm; s_cnt[bf][wave] = wc; }
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SH_RS_TILE / 64; ++w) { const int cw = s_cnt[bf][w]; if (w < wave) before += cw; total += cw; }
    const size_t cut_id = (size_t)bi * pc + q;
    if (tid == 0) {
      ResectPart r;
      r.vol = ((s_red[bf][0][0] + s_red[bf][1][0]) + s_red[bf][2][0]) + s_red[bf][3][0];
      r.area = ((s_red[bf][0][1] + s_red[bf][1][1]) + s_red[bf][2][1]) + s_red[bf][3][1];
      r.hmax = fmax(fmax(s_red[bf][0][2], s_red[bf][1][2]), fmax(s_red[bf][2][2], s_red[bf][3][2]));
      r.n_cut = total; r.pad = 0;
      slab[cut_id * tstride + t] = r;
      if (total > 0) s_base[bf] = atomicAdd(&seg_count[cut_id], total);
    }
    if (total > 0) {      // (uniform)
      __syncthreads();
      const int slot = s_base[bf] + before + rank;
      if (cut && slot < SH_MAXSEG) segs[cut_id * SH_MAXSEG + slot] = (int)fi;      // beyond: the cut's status says so, the count keeps counting
    }
  }
}

// the two ends of the section segment of a cut face: the mesh-edge key (a crossing on a vertex of the plane: that vertex) and the
// crossing point as this face computes it (slice_faces_plane's expression, face edge order).  Start = the edge walked from the
// kept side to the far side, end = the edge walked back: with consistently oriented faces the end of a segment is the start of
// the next.  is_tri: cut to a triangle (their new vertices come behind the quads' in slice_plane's pre-merge numbering).
struct ResectEnds { unsigned long long skey, ekey; bool ok, is_tri; int sj, ej; };
__device__ inline unsigned long long resect_edge_key(const int* id, const int* s, int j) {
  const int a = id[j], b = id[(j + 1) % 3];
  if (s[j] == 0) return ((unsigned long long)(unsigned)a << 32) | (unsigned)a;
  if (s[(j + 1) % 3] == 0) return ((unsigned long long)(unsigned)b << 32) | (unsigned)b;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return ((unsigned long long)(unsigned)lo << 32) | (unsigned)hi;
}
__device__ inline ResectEnds resect_ends(const double* V, const int* id, const double* pl) {
  int s[3]; double d[3];
  ResectEnds e;
  const int k = resect_class(V, pl, s, d);
  e.ok = k == 2 || k == 3;
  e.is_tri = k == 3;
  if (k == 2) { const int qi = s[0] == 1 ? 0 : (s[1] == 1 ? 1 : 2); e.sj = (qi + 2) % 3; e.ej = qi; }
  else { const int ti = s[0] == -1 ? 0 : (s[1] == -1 ? 1 : 2); e.sj = ti; e.ej = (ti + 2) % 3; }
  e.skey = resect_edge_key(id, s, e.sj);
  e.ekey = resect_edge_key(id, s, e.ej);
  return e;
}
__device__ inline void resect_load_face(const float* __restrict__ vb, const int* __restrict__ fb, int f, int* id, double* V) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    id[j] = fb[3 * (size_t)f + j];
    const float* v = vb + 3 * (size_t)id[j];
    V[3 * j] = (double)v[0]; V[3 * j + 1] = (double)v[1]; V[3 * j + 2] = (double)v[2];
  }
}
// the crossing with key `key` on face edge j: the vertex itself when the crossing is a vertex of the plane
__device__ inline void resect_point(const double* V, const int* id, int j, unsigned long long key, const double* pl, double* out) {
  if ((unsigned)(key >> 32) == (unsigned)key) {
    const int jj = (unsigned)id[j] == (unsigned)key ? j : (j + 1) % 3;
    out[0] = V[3 * jj]; out[1] = V[3 * jj + 1]; out[2] = V[3 * jj + 2];
  } else clip_cross(V, j, pl, out);
}

// base.Section's in-plane basis for the unit normal un (see sh_resection): u = un x e_x, or un x e_y when |un_x| >= 0.9, normalised;
// w = un x u.  The one statement of it: the join's areas, the ring coordinates it stores, k_headfit_solve and k_seat all use this.
__device__ inline void resect_basis(const double* un, double* u, double* w) {
  const double ex[3] = {1.0, 0.0, 0.0}, ey[3] = {0.0, 1.0, 0.0};
  cross3(un, fabs(un[0]) < 0.9 ? ex : ey, u);
  const double ul = norm3(u);
  u[0] /= ul; u[1] /= ul; u[2] /= ul;
  cross3(un, u, w);
}

#define SH_RJ_NAME k_resect_join
#define SH_RJ_FIT 0
#define SH_RJ_SEAT 0
#include "k_resect_join.h"
#undef SH_RJ_NAME
#undef SH_RJ_FIT
#define SH_RJ_NAME k_resect_join_fit
#define SH_RJ_FIT 1
#include "k_resect_join.h"
#undef SH_RJ_NAME
#undef SH_RJ_SEAT
#define SH_RJ_NAME k_resect_join_seat
#define SH_RJ_SEAT 1
#include "k_resect_join.h"
#undef SH_RJ_NAME
#undef SH_RJ_FIT
#undef SH_RJ_SEAT

}  // namespace sh
