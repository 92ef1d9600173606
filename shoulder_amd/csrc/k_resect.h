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
#include "k_slices.h"
#include "k_clip.h"

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
  const long long f0 = foff[b], nf = foff[b + 1] - f0;
  if ((long long)t * SH_RS_TILE >= nf) return;      // (uniform)
  const long long fi = (long long)t * SH_RS_TILE + tid;
  const bool live = fi < nf;
  double V[9];
  {
    const int* f = faces + 3 * (f0 + (live ? fi : 0));
    const float* vb = verts + 3 * voff[b];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float* v = vb + 3 * (size_t)f[j];
      V[3 * j] = (double)v[0]; V[3 * j + 1] = (double)v[1]; V[3 * j + 2] = (double)v[2];
    }
  }
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

__global__ void __launch_bounds__(SH_RS_JOIN_THREADS)
k_resect_join(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const double* __restrict__ planes, int P, int p0, int pc, int b0, int tstride, const int* __restrict__ cut_status /* B x P */,
              const ResectPart* __restrict__ slab, const int* __restrict__ seg_count, const int* __restrict__ segs,
              sh_resection* __restrict__ out /* B x P */, sh_resection* __restrict__ out_one /* nullable: the record goes here instead */,
              double* __restrict__ ring_out /* nullable: (SH_MAXSEG + 1) x 3 */) {
  constexpr int CAP = SH_MAXSEG, HASH = 2048, T = SH_RS_JOIN_THREADS;
  __shared__ unsigned long long skey[CAP];      // start keys; then the ring's z
  __shared__ unsigned long long bufA[CAP];      // end keys, label ping; then the ring's x
  __shared__ unsigned long long bufB[CAP];      // hash table, label pong; then the ring's y
  __shared__ int nxt[CAP], prd[CAP], jmpA[CAP], jmpB[CAP], offA[CAP], offB[CAP], fid[CAP];
  __shared__ unsigned long long l_key[SH_MAXLOOPS];
  __shared__ int l_start[SH_MAXLOOPS], l_len[SH_MAXLOOPS], l_off[SH_MAXLOOPS];
  __shared__ double l_area[SH_MAXLOOPS];
  __shared__ int n_loops, bad;
  __shared__ double s_sum[3];
  __shared__ int s_ncut;
  __shared__ double s_best[4][T / 64];
  int* const table = (int*)bufB;

  const int cut = blockIdx.x, bi = cut / pc, q = cut - bi * pc, b = b0 + bi, p = p0 + q, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  sh_resection* rec = out_one ? out_one : out + (size_t)b * P + p;
  const int st0 = cut_status[(size_t)b * P + p];
  const double* plg = planes + ((size_t)b * P + p) * 6;
  const double pl[6] = {plg[0], plg[1], plg[2], plg[3], plg[4], plg[5]};
  if (st0 != 0) {      // the humerus' record failed: its status, nothing else
    if (tid == 0) {
      sh_resection r;
      memset(&r, 0, sizeof r);
      r.status = st0;
      *rec = r;
    }
    return;
  }
  const long long f0 = foff[b], nf = foff[b + 1] - f0;
  const int ntile = (int)((nf + SH_RS_TILE - 1) / SH_RS_TILE);
  if (tid == 0) { n_loops = 0; bad = 0; }
  // the face sums: tiles lane-strided in order, then the shuffle tree -- a fixed order for a given face count
  if (wave == 0) {
    const ResectPart* sp = slab + (size_t)cut * tstride;
    double vol = 0.0, ar = 0.0, hm = 0.0; int nc = 0;
    for (int t = lane; t < ntile; t += 64) { const ResectPart r = sp[t]; vol += r.vol; ar += r.area; hm = fmax(hm, r.hmax); nc += r.n_cut; }
    for (int off = 32; off > 0; off >>= 1) {
      vol += __shfl_down(vol, off); ar += __shfl_down(ar, off); hm = fmax(hm, __shfl_down(hm, off)); nc += __shfl_down(nc, off);
    }
    if (lane == 0) { s_sum[0] = vol; s_sum[1] = ar; s_sum[2] = hm; s_ncut = nc; }
  }
  for (int i = tid; i < HASH; i += T) table[i] = -1;
  const int n = seg_count[cut];
  __syncthreads();
  const double nlen = sqrt((pl[3] * pl[3] + pl[4] * pl[4]) + pl[5] * pl[5]);
  // base.Section's in-plane basis
  double un[3] = {pl[3] / nlen, pl[4] / nlen, pl[5] / nlen}, u[3], w[3];
  {
    const double ex[3] = {1.0, 0.0, 0.0}, ey[3] = {0.0, 1.0, 0.0};
    cross3(un, fabs(un[0]) < 0.9 ? ex : ey, u);
    const double ul = norm3(u);
    u[0] /= ul; u[1] /= ul; u[2] /= ul;
    cross3(un, u, w);
  }
  int status = 0, nl = 0, best = 0;
  const float* vb = verts + 3 * voff[b];
  const int* fb = faces + 3 * f0;
  if (n > CAP) status = SH_ERR_CAPACITY_DEV;
  else if (n > 0) {
    const int* sg = segs + (size_t)cut * SH_MAXSEG;
    for (int i = tid; i < n; i += T) {
      const int f = sg[i];
      int id[3]; double V[9];
      resect_load_face(vb, fb, f, id, V);
      const ResectEnds e = resect_ends(V, id, pl);
      fid[i] = f; skey[i] = e.skey; bufA[i] = e.ekey; prd[i] = -1;
      if (!e.ok || e.skey == e.ekey) bad = 1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
      const unsigned long long k = skey[i];
      uint32_t h = hash_key64(k) & (HASH - 1);
      for (;;) {
        const int o = atomicCAS(&table[h], -1, i);
        if (o == -1) break;
        if (skey[o] == k) { bad = 1; break; }      // two segments leave one crossing: no simple loop
        h = (h + 1) & (HASH - 1);
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
      const unsigned long long k = bufA[i];
      uint32_t h = hash_key64(k) & (HASH - 1);
      int t, found = -1;
      while ((t = table[h]) != -1) {
        if (skey[t] == k) { found = t; break; }
        h = (h + 1) & (HASH - 1);
      }
      if (found < 0) { found = i; bad = 1; }      // an open chain
      else if (atomicExch(&prd[found], i) != -1) bad = 1;      // two segments arrive at one crossing
      nxt[i] = found;
    }
    __syncthreads();
    if (bad) status = SH_ERR_GEOMETRY_DEV;      // (uniform)
    else {
      // nxt is a permutation: every segment lies on one closed loop.  One pointer-jumping pass: the loop's smallest start key and
      // the forward distance to its node (slice_link_plane's scheme).
      unsigned long long* labA = bufA; unsigned long long* labB = bufB;
      int* ja = jmpA; int* jb = jmpB; int* ra = offA; int* rb = offB;
      for (int i = tid; i < n; i += T) { labA[i] = skey[i]; ja[i] = nxt[i]; ra[i] = 0; }
      __syncthreads();
      for (int span = 1; span < n; span <<= 1) {
        for (int i = tid; i < n; i += T) {
          const int j = ja[i];
          const unsigned long long a = labA[i], c = labA[j];
          const bool own = a <= c;
          labB[i] = own ? a : c;
          rb[i] = own ? ra[i] : span + ra[j];
          jb[i] = ja[j];
        }
        __syncthreads();
        unsigned long long* tl = labA; labA = labB; labB = tl;
        int* tj = ja; ja = jb; jb = tj;
        int* tr = ra; ra = rb; rb = tr;
      }
      for (int i = tid; i < n; i += T)
        if (ra[i] == 0) { const int l = atomicAdd(&n_loops, 1); if (l < SH_MAXLOOPS) l_start[l] = i; }
      __syncthreads();
      nl = n_loops;
      if (nl > SH_MAXLOOPS) { status = SH_ERR_CAPACITY_DEV; nl = 0; }      // (uniform)
      else {
        if (tid == 0) {      // canonical loop order: ascending start key
          for (int a = 1; a < nl; ++a) {
            const int v = l_start[a]; int c = a - 1;
            while (c >= 0 && skey[l_start[c]] > skey[v]) { l_start[c + 1] = l_start[c]; --c; }
            l_start[c + 1] = v;
          }
          int off = 0;
          for (int l = 0; l < nl; ++l) {
            const int s = l_start[l], L = ra[nxt[s]] + 1;
            l_len[l] = L; l_off[l] = off; off += L; l_key[l] = skey[s];
          }
        }
        __syncthreads();
        // ring position of every segment's start crossing; its point: of the two faces that compute this crossing the one whose
        // new vertex slice_plane's merge keeps (smallest pre-merge index: quads before triangles, then face order)
        int my_pos[CAP / T]; double my_pt[CAP / T][3];
        {
          int c = 0;
          for (int i = tid; i < n; i += T, ++c) {
            const unsigned long long key = labA[i];
            int l = 0;
            for (int qq = 0; qq < nl; ++qq) if (l_key[qq] == key) { l = qq; break; }
            const int r = ra[i];
            my_pos[c] = l_off[l] + (r == 0 ? 0 : l_len[l] - r);
            int id[3]; double V[9];
            const int f = fid[i];
            resect_load_face(vb, fb, f, id, V);
            const ResectEnds e = resect_ends(V, id, pl);
            const int g = fid[prd[i]];
            int idg[3]; double Vg[9];
            resect_load_face(vb, fb, g, idg, Vg);
            const ResectEnds eg = resect_ends(Vg, idg, pl);
            const bool own = e.is_tri != eg.is_tri ? !e.is_tri : f < g;
            if (own) resect_point(V, id, e.sj, e.skey, pl, my_pt[c]);
            else resect_point(Vg, idg, eg.ej, eg.ekey, pl, my_pt[c]);
          }
        }
        __syncthreads();      // labels, keys and ranks are dead: the ring takes their place
        double* rx = (double*)bufA; double* ry = (double*)bufB; double* rz = (double*)skey;
        {
          int c = 0;
          for (int i = tid; i < n; i += T, ++c) { rx[my_pos[c]] = my_pt[c][0]; ry[my_pos[c]] = my_pt[c][1]; rz[my_pos[c]] = my_pt[c][2]; }
        }
        __syncthreads();
        // shoelace area of every loop about the plane point: one wave per loop, lane-strided terms in ring order, fixed tree
        for (int l = wave; l < nl; l += T / 64) {
          const int o = l_off[l], L = l_len[l];
          double a2 = 0.0;
          for (int k = lane; k < L; k += 64) {
            const int kn = k + 1 == L ? 0 : k + 1;
            const double ax = rx[o + k] - pl[0], ay = ry[o + k] - pl[1], az = rz[o + k] - pl[2];
            const double bx = rx[o + kn] - pl[0], by = ry[o + kn] - pl[1], bz = rz[o + kn] - pl[2];
            const double x0 = (ax * u[0] + ay * u[1]) + az * u[2], y0 = (ax * w[0] + ay * w[1]) + az * w[2];
            const double x1 = (bx * u[0] + by * u[1]) + bz * u[2], y1 = (bx * w[0] + by * w[1]) + bz * w[2];
            a2 += x0 * y1 - x1 * y0;
          }
          for (int off = 32; off > 0; off >>= 1) a2 += __shfl_down(a2, off);
          if (lane == 0) l_area[l] = 0.5 * a2;
        }
        __syncthreads();
        for (int l = 1; l < nl; ++l) if (fabs(l_area[l]) > fabs(l_area[best])) best = l;
      }
    }
  }
  __syncthreads();
  // the largest loop: perimeter and centroid sums (all waves, lane-strided in ring order, fixed tree, waves added in order)
  double per = 0.0, sx = 0.0, sy = 0.0, a2b = 0.0;
  if (nl > 0) {
    const double* rx = (const double*)bufA; const double* ry = (const double*)bufB; const double* rz = (const double*)skey;
    const int o = l_off[best], L = l_len[best];
    for (int k = tid; k < L; k += T) {
      const int kn = k + 1 == L ? 0 : k + 1;
      const double dx = rx[o + kn] - rx[o + k], dy = ry[o + kn] - ry[o + k], dz = rz[o + kn] - rz[o + k];
      per += sqrt((dx * dx + dy * dy) + dz * dz);
      const double ax = rx[o + k] - pl[0], ay = ry[o + k] - pl[1], az = rz[o + k] - pl[2];
      const double bx = rx[o + kn] - pl[0], by = ry[o + kn] - pl[1], bz = rz[o + kn] - pl[2];
      const double x0 = (ax * u[0] + ay * u[1]) + az * u[2], y0 = (ax * w[0] + ay * w[1]) + az * w[2];
      const double x1 = (bx * u[0] + by * u[1]) + bz * u[2], y1 = (bx * w[0] + by * w[1]) + bz * w[2];
      const double cr = x0 * y1 - x1 * y0;
      a2b += cr; sx += (x0 + x1) * cr; sy += (y0 + y1) * cr;
    }
    for (int off = 32; off > 0; off >>= 1) {
      per += __shfl_down(per, off); sx += __shfl_down(sx, off); sy += __shfl_down(sy, off); a2b += __shfl_down(a2b, off);
    }
    if (lane == 0) { s_best[0][wave] = per; s_best[1][wave] = sx; s_best[2][wave] = sy; s_best[3][wave] = a2b; }
  }
  __syncthreads();
  if (tid == 0) {
    sh_resection r;
    memset(&r, 0, sizeof r);
    for (int k = 0; k < 3; ++k) { r.plane_point[k] = pl[k]; r.plane_normal[k] = pl[3 + k]; }
    r.head_volume = s_sum[0] / 6.0;
    r.head_area = 0.5 * s_sum[1];
    r.head_height = s_sum[2] / nlen;
    r.n_cut_faces = s_ncut;
    r.status = status;
    if (nl > 0) {
      double v[4];
      for (int k = 0; k < 4; ++k) v[k] = ((s_best[k][0] + s_best[k][1]) + s_best[k][2]) + s_best[k][3];
      r.cut_area = fabs(l_area[best]);
      r.cut_perimeter = v[0];
      const double cx = v[1] / (3.0 * v[3]), cy = v[2] / (3.0 * v[3]);      // polygon centroid: sum (x0 + x1) cr / (6 A), A = sum cr / 2
      for (int k = 0; k < 3; ++k) r.cut_centroid[k] = (pl[k] + cx * u[k]) + cy * w[k];
      double tot = 0.0;
      for (int l = 0; l < nl; ++l) tot += l_area[l];
      r.cap_area = fabs(tot);
      r.n_loops = nl; r.n_ring = l_len[best];
    }
    *rec = r;
  }
  if (ring_out && nl > 0) {
    const double* rx = (const double*)bufA; const double* ry = (const double*)bufB; const double* rz = (const double*)skey;
    const int o = l_off[best], L = l_len[best];
    const bool rev = l_area[best] < 0;      // clockwise seen from the normal's tip: backwards from the same start
    for (int k = tid; k <= L; k += T) {
      const int kk = k == L ? 0 : k, src = rev ? (kk == 0 ? 0 : L - kk) : kk;
      ring_out[3 * k] = rx[o + src]; ring_out[3 * k + 1] = ry[o + src]; ring_out[3 * k + 2] = rz[o + src];
    }
  }
}

}  // namespace sh
