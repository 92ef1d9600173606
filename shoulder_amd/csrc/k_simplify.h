// k_simplify.h -- simplification of the resident batch by vertex clustering with quadric placement (include/shoulder_hip.h
// sh_mesh_simplify).  The scalar rules are sh_scalar.h simp_*; the result is the same bytes on the device, in the host twin
// (tests/hostcheck/simplify_check.cpp) and in tests/simplify_oracle.py.  Grids are (block of SH_SIMP_BLOCK = 256 vertices, clusters or
// faces, mesh), one per lane, but for the scan.  A fixed list of launches; the host reads nothing in between:
//   k_simp_box      (vertex block, mesh).  A vertex is used when its incidence row is not empty.  The used vertices' coordinates go into
//                   the mesh's box -- minima and maxima of topo_enc words, first in LDS, then six integer atomics per workgroup into
//                   "simp.state" -- and are counted.
//   k_simp_key      (vertex block, mesh).  The cell key of every used vertex from the finished box into "simp.key"; SH_SIMP_NO_KEY for
//                   the others and for a mesh whose grid is refused (word SH_SIMP_W_GRID of its head says so).
//   (sort)          rocprim::segmented_radix_sort_keys, one segment per mesh, "simp.key" -> "simp.sorted".  Keys alone: equal keys are
//                   the same bytes, so any correct sort gives this array.
//   k_simp_heads    (vertex block, mesh).  Marks the first place of every key in the sorted array.
//   k_simp_scan     (mesh), 1 024 lanes: the exclusive scan of an int32 array of a mesh and its total into a word of the head.  Run
//                   three times: the heads (-> the cluster numbers, ascending by key), the kept faces, the named clusters.
//   k_simp_ukey     (vertex block, mesh).  The key and the first sorted place of every cluster: "simp.ukey", "simp.start".
//   k_simp_assign   (vertex block, mesh).  A vertex finds its cluster by bisection of "simp.ukey" -> "simp.cid", and overwrites its key
//                   by (cluster << 32 | vertex): unique, so the second sort gives the members of every cluster ascending by vertex index
//                   whatever the sort does with equal keys.
//   k_simp_quadric  (vertex block, mesh).  The quadric of a vertex over its row, relative to the centre of its cell.
//   (sort)          "simp.key" -> "simp.sorted" once more: the member lists.  A cluster's members stand where its keys stood.
//   k_simp_cluster  (cluster block, mesh).  A lane per cluster: the sums over its members in order, the solve, "simp.pos".
//   k_simp_faces    (face block, mesh).  The clusters of a face; collapsed, or a duplicate when a face of smaller index has the same
//                   three clusters -- looked for in the rows of the members of the smallest of its clusters, which hold every face that
//                   names it; a kept face marks its clusters as named.  No sort: the smallest index of a set does not depend on an order.
//   k_simp_emit     (block, mesh).  The kept faces with the output numbers of their clusters, the positions of the named clusters, the
//                   map, and the largest move (a maximum of float64 bit patterns, all >= 0, in LDS and then one atomic per workgroup).
//   k_simp_info     (mesh block).  The records.
// No floating-point atomics (the largest move is an integer maximum of the bits of non-negative doubles); integer atomics for minima,
// maxima, counts and flags only.  Every index is below its array's size by construction: keys, places and cluster numbers of a mesh are
// below its V, a face index from a row below its F.
#pragma once
#include "sh_common.h"
#include "sh_scalar.h"

#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace sh {

#define SH_SIMP_BLOCK 256
#define SH_SIMP_SCAN 1024
#define SH_SIMP_HEAD 20          // words of a mesh in "simp.state": lo[3] and hi[3] as topo_enc words (start: ~0 and 0), then the words below
#define SH_SIMP_W_USED 6
#define SH_SIMP_W_GRID 7         // 1: an axis has more than SH_SIMP_MAX_CELLS cells
#define SH_SIMP_W_CLUSTERS 8
#define SH_SIMP_W_COLLAPSED 9
#define SH_SIMP_W_DUPLICATE 10
#define SH_SIMP_W_FALLBACKS 11
#define SH_SIMP_W_LARGEST 12
#define SH_SIMP_W_FACES 13
#define SH_SIMP_W_VERTS 14
#define SH_SIMP_W_MOVE 16        // two words: the bits of the largest move

static_assert(sizeof(sh_simplify_info) == 64 && sizeof(sh_simplify_options) == 24 && offsetof(sh_simplify_info, cell) == 40, "the records of sh_mesh_simplify");
static_assert(SH_SIMPLIFY_MEAN == SH_SIMP_MEAN && SH_SIMPLIFY_QUADRIC == SH_SIMP_QUADRIC && SH_SIMPLIFY_MAX_CELLS == SH_SIMP_MAX_CELLS &&
              SH_SIMPLIFY_MAX_CLUSTERS == SH_SIMP_MAX_CLUSTERS, "the modes and limits of sh_mesh_simplify");

struct SimpGrid { float lo[3]; long long n[3]; double h; bool ok; };      // ok: the mesh has a used vertex and its grid is admitted

__device__ __forceinline__ SimpGrid simp_grid_of(const unsigned* __restrict__ head, double h) {
  SimpGrid g;
  float hi[3];
  for (int k = 0; k < 3; ++k) { g.lo[k] = topo_dec(head[k]); hi[k] = topo_dec(head[3 + k]); }
  g.h = h;
  g.ok = head[SH_SIMP_W_USED] > 0u && simp_grid(g.lo, hi, h, g.n);
  return g;
}
// a mesh whose outputs stay empty: its grid is refused or it has too many clusters
__device__ __forceinline__ bool simp_refused(const unsigned* __restrict__ head) { return head[SH_SIMP_W_GRID] != 0u || head[SH_SIMP_W_CLUSTERS] > (unsigned)SH_SIMP_MAX_CLUSTERS; }

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_box(const float* __restrict__ verts, const long long* __restrict__ voff, const int* __restrict__ vrow, unsigned* __restrict__ state) {
  __shared__ unsigned s_box[6];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nv = voff[b + 1] - voff[b], v0 = (long long)blockIdx.x * SH_SIMP_BLOCK;
  if (v0 >= nv) return;      // (uniform in the workgroup)
  if (tid < 6) s_box[tid] = tid < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  const long long v = v0 + tid;
  int used = 0;
  if (v < nv) {
    const int* row = vrow + voff[b] + b;
    if (row[v + 1] > row[v]) {
      used = 1;
      const float* x = verts + 3 * (size_t)(voff[b] + v);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const unsigned e = topo_enc(x[k]);
        atomicMin(&s_box[k], e);
        atomicMax(&s_box[3 + k], e);
      }
    }
  }
  const int n = __syncthreads_count(used);
  if (n == 0) return;      // (uniform)
  unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  if (tid < 3) atomicMin(head + tid, s_box[tid]);
  else if (tid < 6) atomicMax(head + tid, s_box[tid]);
  else if (tid == 6) atomicAdd(head + SH_SIMP_W_USED, (unsigned)n);
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_key(const float* __restrict__ verts, const long long* __restrict__ voff, const int* __restrict__ vrow, const double* __restrict__ cell,
           unsigned* __restrict__ state, unsigned long long* __restrict__ key /* sumV */) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SIMP_BLOCK + threadIdx.x;
  unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  const SimpGrid g = simp_grid_of(head, cell[b]);
  if (blockIdx.x == 0 && threadIdx.x == 0) head[SH_SIMP_W_GRID] = head[SH_SIMP_W_USED] > 0u && !g.ok ? 1u : 0u;      // (read by later launches only)
  if (v >= nv) return;
  const int* row = vrow + voff[b] + b;
  unsigned long long k = SH_SIMP_NO_KEY;
  if (g.ok && row[v + 1] > row[v]) {
    const float* x = verts + 3 * (size_t)(voff[b] + v);
    long long i[3];
    for (int a = 0; a < 3; ++a) i[a] = simp_cell(x[a], g.lo[a], g.h, g.n[a]);
    k = simp_key(i, g.n);
  }
  key[voff[b] + v] = k;
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_heads(const unsigned long long* __restrict__ sorted, const long long* __restrict__ voff, int* __restrict__ mark) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], i = (long long)blockIdx.x * SH_SIMP_BLOCK + threadIdx.x;
  if (i >= nv) return;
  const unsigned long long* s = sorted + voff[b];
  mark[voff[b] + i] = s[i] != SH_SIMP_NO_KEY && (i == 0 || s[i - 1] != s[i]) ? 1 : 0;
}

// the exclusive scan of flag over the elements [off[b], off[b + 1]) of mesh b -> rank, the total -> word `word` of the mesh's head
__global__ void __launch_bounds__(SH_SIMP_SCAN)
k_simp_scan(const int* __restrict__ flag, const long long* __restrict__ off, int word, int* __restrict__ rank, unsigned* __restrict__ state) {
  __shared__ int s_wave[SH_SIMP_SCAN / 64];
  __shared__ int s_carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long base = off[b], n = off[b + 1] - base;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (long long i0 = 0; i0 < n; i0 += SH_SIMP_SCAN) {      // (uniform)
    const long long i = i0 + tid;
    const int x = i < n ? flag[base + i] : 0;
    int inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int before = s_carry;
    for (int k = 0; k < w; ++k) before += s_wave[k];
    if (i < n) rank[base + i] = before + inc - x;
    __syncthreads();
    if (tid == SH_SIMP_SCAN - 1) s_carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) state[(size_t)b * SH_SIMP_HEAD + word] = (unsigned)s_carry;
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_ukey(const unsigned long long* __restrict__ sorted, const int* __restrict__ mark, const int* __restrict__ rank, const long long* __restrict__ voff,
            unsigned long long* __restrict__ ukey, int* __restrict__ start) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], i = (long long)blockIdx.x * SH_SIMP_BLOCK + threadIdx.x;
  if (i >= nv || !mark[voff[b] + i]) return;
  const int c = rank[voff[b] + i];      // (< the heads of this mesh <= nv)
  ukey[voff[b] + c] = sorted[voff[b] + i];
  start[voff[b] + c] = (int)i;
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_assign(const unsigned long long* __restrict__ ukey, const long long* __restrict__ voff, const unsigned* __restrict__ state, int* __restrict__ cid,
              unsigned long long* __restrict__ key /* in: the cell keys; out: cluster << 32 | vertex */) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SIMP_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  const unsigned long long k = key[voff[b] + v];
  int c = -1;
  if (k != SH_SIMP_NO_KEY && !simp_refused(head)) {
    const unsigned long long* u = ukey + voff[b];
    int lo = 0, hi = (int)head[SH_SIMP_W_CLUSTERS] - 1;      // (k is one of the keys: u[lo] <= k <= u[hi] throughout)
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (u[mid] < k) lo = mid + 1; else hi = mid;
    }
    c = lo;
  }
  cid[voff[b] + v] = c;
  key[voff[b] + v] = c >= 0 ? ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)v : SH_SIMP_NO_KEY;
}

// the corners of face f of the mesh at (vb, fb), widened
__device__ __forceinline__ void simp_corners(const float* __restrict__ vb, const int* __restrict__ fb, int f, double* A, double* B, double* C) {
  const int* t = fb + 3 * (size_t)f;
  const float *a = vb + 3 * (size_t)t[0], *bq = vb + 3 * (size_t)t[1], *cq = vb + 3 * (size_t)t[2];
  for (int k = 0; k < 3; ++k) { A[k] = (double)a[k]; B[k] = (double)bq[k]; C[k] = (double)cq[k]; }
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_quadric(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
               const int* __restrict__ vrow, const int* __restrict__ vface, const double* __restrict__ cell, const unsigned* __restrict__ state,
               const int* __restrict__ cid, double* __restrict__ quad /* SH_SIMP_Q x sumV */) {
  const int b = blockIdx.y;
  const long long nv = voff[b + 1] - voff[b], v = (long long)blockIdx.x * SH_SIMP_BLOCK + threadIdx.x;
  if (v >= nv || cid[voff[b] + v] < 0) return;
  const SimpGrid g = simp_grid_of(state + (size_t)b * SH_SIMP_HEAD, cell[b]);      // (ok: the vertex has a cluster)
  const float* vb = verts + 3 * (size_t)voff[b];
  const int* fb = faces + 3 * (size_t)foff[b];
  const int* row = vrow + voff[b] + b;
  const int* vf = vface + 3 * (size_t)foff[b];
  double o[3], q[SH_SIMP_Q];
  for (int a = 0; a < 3; ++a) o[a] = simp_center(simp_cell(vb[3 * (size_t)v + a], g.lo[a], g.h, g.n[a]), g.lo[a], g.h);
  for (int k = 0; k < SH_SIMP_Q; ++k) q[k] = 0.0;
  for (int i = row[v]; i < row[v + 1]; ++i) {
    double A[3], B[3], C[3];
    simp_corners(vb, fb, vf[i], A, B, C);
    simp_face_quadric(A, B, C, o, q);
  }
  double* out = quad + SH_SIMP_Q * (size_t)(voff[b] + v);
  for (int k = 0; k < SH_SIMP_Q; ++k) out[k] = q[k];
}

// the members of cluster c of a mesh with C clusters and U used vertices: the places [*i0, *i1) of the second sort
__device__ __forceinline__ void simp_members(const int* __restrict__ start, int c, int C, int U, int* i0, int* i1) {
  *i0 = start[c];
  *i1 = c + 1 < C ? start[c + 1] : U;
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_cluster(const float* __restrict__ verts, const long long* __restrict__ voff, const double* __restrict__ cell, unsigned* __restrict__ state,
               const unsigned long long* __restrict__ sorted, const unsigned long long* __restrict__ ukey, const int* __restrict__ start,
               const double* __restrict__ quad, int place, double reg, double clamp, float* __restrict__ pos /* 3 x sumV, by cluster */) {
  const int b = blockIdx.y;
  unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  if (simp_refused(head)) return;
  const int C = (int)head[SH_SIMP_W_CLUSTERS], U = (int)head[SH_SIMP_W_USED];
  const long long c = (long long)blockIdx.x * SH_SIMP_BLOCK + threadIdx.x;
  if (c >= C) return;
  const SimpGrid g = simp_grid_of(head, cell[b]);
  const float* vb = verts + 3 * (size_t)voff[b];
  const unsigned long long* s = sorted + voff[b];
  const double* qb = quad + SH_SIMP_Q * (size_t)voff[b];
  int i0, i1;
  simp_members(start + voff[b], (int)c, C, U, &i0, &i1);
  double S[3] = {0.0, 0.0, 0.0}, q[SH_SIMP_Q];
  for (int k = 0; k < SH_SIMP_Q; ++k) q[k] = 0.0;
  for (int i = i0; i < i1; ++i) {
    const size_t v = (size_t)(unsigned)(s[i] & 0xffffffffull);
    for (int k = 0; k < 3; ++k) S[k] = S[k] + (double)vb[3 * v + k];
    for (int k = 0; k < SH_SIMP_Q; ++k) q[k] = q[k] + qb[SH_SIMP_Q * v + k];
  }
  const double count = (double)(i1 - i0);
  double m[3], o[3], x[3];
  long long ic[3];
  simp_unkey(ukey[voff[b] + c], g.n, ic);
  for (int k = 0; k < 3; ++k) { m[k] = S[k] / count; o[k] = simp_center(ic[k], g.lo[k], g.h); }
  float* p = pos + 3 * (size_t)(voff[b] + c);
  bool solved = false;
  if (place == SH_SIMP_QUADRIC) {
    solved = simp_solve(q, m, o, g.h, reg, clamp, x);
    if (!solved) atomicAdd(head + SH_SIMP_W_FALLBACKS, 1u);
  }
  for (int k = 0; k < 3; ++k) p[k] = solved ? (float)(o[k] + x[k]) : (float)m[k];
  atomicMax(head + SH_SIMP_W_LARGEST, (unsigned)(i1 - i0));
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_faces(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
             const int* __restrict__ vface, unsigned* __restrict__ state, const int* __restrict__ cid, const unsigned long long* __restrict__ sorted,
             const int* __restrict__ start, int* __restrict__ keep /* sumF */, int* __restrict__ named /* sumV, by cluster; zero on entry */) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], nv = voff[b + 1] - voff[b], f = (long long)blockIdx.x * SH_SIMP_BLOCK + tid;
  if ((long long)blockIdx.x * SH_SIMP_BLOCK >= nf) return;      // (uniform in the workgroup)
  unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  const bool refused = simp_refused(head);
  const int C = (int)head[SH_SIMP_W_CLUSTERS], U = (int)head[SH_SIMP_W_USED];
  const int* fb = faces + 3 * (size_t)foff[b];
  const int* cb = cid + voff[b];
  int collapsed = 0, dup = 0, kept = 0;
  if (f < nf && !refused && !topo_degenerate(fb + 3 * (size_t)f, (int)nv)) {
    const int* t = fb + 3 * (size_t)f;
    int s[3];
    if (!simp_triple(cb[t[0]], cb[t[1]], cb[t[2]], s)) collapsed = 1;
    else {
      // the smallest of the three clusters: every face that names it stands in a row of one of its members
      const int* st = start + voff[b];
      int i0 = 0, i1 = 0;
      for (int k = 0; k < 3; ++k) {
        int j0, j1;
        simp_members(st, s[k], C, U, &j0, &j1);
        if (k == 0 || j1 - j0 < i1 - i0) { i0 = j0; i1 = j1; }
      }
      const unsigned long long* so = sorted + voff[b];
      const int* row = vrow + voff[b] + b;
      const int* vf = vface + 3 * (size_t)foff[b];
      for (int i = i0; i < i1 && !dup; ++i) {
        const size_t u = (size_t)(unsigned)(so[i] & 0xffffffffull);
        for (int j = row[u]; j < row[u + 1]; ++j) {
          const int g = vf[j];
          if (g >= f) break;      // (a row ascends)
          const int* tg = fb + 3 * (size_t)g;
          int sg[3];
          if (simp_triple(cb[tg[0]], cb[tg[1]], cb[tg[2]], sg) && sg[0] == s[0] && sg[1] == s[1] && sg[2] == s[2]) { dup = 1; break; }
        }
      }
      if (!dup) {
        kept = 1;
        for (int k = 0; k < 3; ++k) named[voff[b] + s[k]] = 1;      // (a flag: every writer stores 1)
      }
    }
  }
  if (f < nf) keep[foff[b] + f] = kept;
  const int nc = __syncthreads_count(collapsed), nd = __syncthreads_count(dup);
  if (tid == 0 && nc) atomicAdd(head + SH_SIMP_W_COLLAPSED, (unsigned)nc);
  if (tid == 0 && nd) atomicAdd(head + SH_SIMP_W_DUPLICATE, (unsigned)nd);
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_emit(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
            unsigned* __restrict__ state, const int* __restrict__ cid, const float* __restrict__ pos, const int* __restrict__ keep, const int* __restrict__ frank,
            const int* __restrict__ named, const int* __restrict__ vrank, float* __restrict__ overts, int* __restrict__ ofaces, int* __restrict__ map) {
  __shared__ unsigned long long s_move;
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], nv = voff[b + 1] - voff[b], i = (long long)blockIdx.x * SH_SIMP_BLOCK + tid;
  if (tid == 0) s_move = 0ull;
  __syncthreads();
  unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  const int C = simp_refused(head) ? 0 : (int)head[SH_SIMP_W_CLUSTERS];
  const int* cb = cid + voff[b];
  const int* nb = named + voff[b];
  const int* rb = vrank + voff[b];
  if (i < nf && keep[foff[b] + i]) {
    const int* t = faces + 3 * (size_t)(foff[b] + i);
    int* o = ofaces + 3 * (size_t)(foff[b] + frank[foff[b] + i]);
    for (int k = 0; k < 3; ++k) o[k] = rb[cb[t[k]]];
  }
  if (i < C && nb[i]) {
    const float* p = pos + 3 * (size_t)(voff[b] + i);
    float* o = overts + 3 * (size_t)(voff[b] + rb[i]);
    for (int k = 0; k < 3; ++k) o[k] = p[k];
  }
  if (i < nv) {
    const int c = cb[i];
    map[voff[b] + i] = c >= 0 && nb[c] ? rb[c] : -1;
    if (c >= 0) {
      const double d = simp_move(verts + 3 * (size_t)(voff[b] + i), pos + 3 * (size_t)(voff[b] + c));      // (>= 0: its bits order as it does)
      atomicMax(&s_move, (unsigned long long)__double_as_longlong(d));
    }
  }
  __syncthreads();
  if (tid == 0 && s_move) atomicMax((unsigned long long*)(head + SH_SIMP_W_MOVE), s_move);
}

__global__ void __launch_bounds__(SH_SIMP_BLOCK)
k_simp_info(const unsigned* __restrict__ state, const double* __restrict__ cell, int B, sh_simplify_info* __restrict__ info) {
  const int b = (int)(blockIdx.x * SH_SIMP_BLOCK + threadIdx.x);
  if (b >= B) return;
  const unsigned* head = state + (size_t)b * SH_SIMP_HEAD;
  const bool refused = simp_refused(head);
  sh_simplify_info r;
  r.status = refused ? SH_ERR_CAPACITY_DEV : head[SH_SIMP_W_FACES] == 0u ? SH_ERR_GEOMETRY_DEV : 0;
  r.verts_used = (int)head[SH_SIMP_W_USED]; r.clusters = (int)head[SH_SIMP_W_CLUSTERS];
  r.verts_out = (int)head[SH_SIMP_W_VERTS]; r.faces_out = (int)head[SH_SIMP_W_FACES];
  r.faces_collapsed = (int)head[SH_SIMP_W_COLLAPSED]; r.faces_duplicate = (int)head[SH_SIMP_W_DUPLICATE];
  r.fallbacks = (int)head[SH_SIMP_W_FALLBACKS]; r.largest_cluster = (int)head[SH_SIMP_W_LARGEST]; r.reserved = 0;
  r.cell = cell[b];
  r.max_move = __longlong_as_double((long long)*(const unsigned long long*)(head + SH_SIMP_W_MOVE));
  r.pad[0] = 0; r.pad[1] = 0;
  info[b] = r;
}

}  // namespace sh
