// k_geo.h -- geodesic distances and shortest paths on the resident batch (include/shoulder_hip.h sh_geodesic): the second reader of the
// incidence of sh_mesh_topology and the first of "topo.adj" across an edge.  The scalar rules are sh_scalar.h geo_*; everything is
// float64 in the written order.  A (mesh b, set k) pair is p = b K + k; its planes ("geo.dist", "geo.plane", "geo.pred", "geo.source",
// "geo.jump") lie at K voff[b] + k V_b.  The result is the fixed point of the relaxation and depends on no schedule.
//   k_geo_face   (face block, mesh).  The 48-byte record of "geo.face" (len[3], unf[3]) and the vertex across each slot into "geo.opp":
//                a round then reads one int32 per unfolded arc instead of the neighbour's three indices.
//   k_geo_init   (vertex block, set, mesh).  +inf into "geo.dist", no label into "geo.source"; the first lane of a pair writes its words
//                of "geo.state": word 0 is 1 for a pair of the general path.
//   k_geo_seed   (pair).  The lanes walk the pair's source list on the device: a d0 of at most max_dist enters "geo.dist" with an
//                UNSIGNED 64-bit integer atomic minimum on its bits -- distances are >= +0.0, so their bits order as integers, and an
//                integer atomic is indivisible by definition (a vertex may be listed more than once).
//   k_geo_lds    (set, mesh), SH_GEO_LDS_BLOCK = 1024 lanes, THE HOT PATH.  A pair with V_b <= lds_vertices relaxes inside one workgroup:
//                its plane of V_b doubles (at most SH_GEO_LDS_VERTICES: 160 000 B of the 163 840 B of LDS one workgroup of gfx950 may
//                declare) is loaded once, relaxed until a sweep changes nothing and written back once.  A lane owns the vertices
//                v = lane + 1024 j, j < 20.  A sweep relaxes them in SH_GEO_LDS_PARTS = 2 parts, one after the other (ten values per
//                lane wait in registers; twenty interleaved walks did not fit the 128 registers a lane of 1 024 has, and the second
//                part already sees the first's values, which only helps).  A part: every lane forms the new values of its vertices
//                from the plane; a barrier; every lane writes the values that fell, each into a word no other lane touches; a barrier
//                that also ORs "something fell".  So no 64-bit word is ever read while it is written: nothing rests on a plain 64-bit
//                LDS access being indivisible.  One bit per vertex in 2 560 B more of LDS says whether a neighbour fell since the vertex
//                was relaxed last: a vertex whose bit is clear is skipped (its value could not change), a vertex that falls sets the
//                bits of the vertices its arcs lead to (32-bit integer atomics), and the bits a part has served are cleared between
//                two barriers of their own.  Away from the front a sweep costs twenty bit tests per lane; the schedule changes no
//                value.  "geo.face", "geo.opp", the rows and the faces come from L2.
//   k_geo_round  (vertex block, set, mesh), once per round of the general path: Jacobi on the two planes "geo.dist" (read in even rounds)
//                and "geo.plane".  Words 0..2 of a pair rotate: round r returns at once when word r % 3 is 0 (round r - 1 changed
//                nothing: the pair is finished and both planes hold the result), ORs "changed" into word (r + 1) % 3 and its first
//                lane zeroes word (r + 2) % 3, which no one else touches in round r.  The same three words exist once for the call:
//                the host reads ONE of them per SH_GEO_CHUNK rounds.  A pair of the LDS path returns at once.
//   k_geo_root   (pair).  From the converged plane: a listed d0 that equals d[v] makes v a root; its label is the smallest list position
//                (integer atomic minimum into "geo.source").
//   k_geo_pred   (vertex block, set, mesh).  "geo.pred" (geo_pred) and the start of the pointer jumping: "geo.jump"[v] = pred[v], or v
//                itself at a root, at a vertex without predecessor and at an unreached one.
//   k_geo_jump   (vertex block, set, mesh), ceil(log2(max V_b)) times: jump[v] = jump[jump[v]] in place.  The words are 32-bit and every
//                value a lane can read is an ancestor of v or v's top itself, so a round at least halves what is left of every chain
//                whatever the order; after the rounds jump[v] is the top of v's tree.
//   k_geo_info   (set, mesh).  "geo.source" of the vertices that are no roots (the label of the top when the top is a root, else -1:
//                only roots' words are read, and they are not written), and the info record: the counts, the largest finite distance
//                with the smallest index among equals (geo_far), the sweeps and the status.
// No floating-point atomics.  Every index is below its array's size by construction: rows hold face indices of the vertex's own mesh
// (k_topo.h), faces hold vertex indices checked at upload, "geo.opp" holds -1 or a vertex of a face, and the host has checked every
// source index against V_b before anything is enqueued.
#pragma once
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_GEO_BLOCK 256
#define SH_GEO_LDS_BLOCK 1024
#define SH_GEO_LDS_PER_LANE ((SH_GEO_LDS_VERTICES + SH_GEO_LDS_BLOCK - 1) / SH_GEO_LDS_BLOCK)
#define SH_GEO_LDS_PARTS 2       // a sweep of the LDS kernel relaxes the vertices in this many parts, one after the other
#define SH_GEO_LDS_PART (SH_GEO_LDS_PER_LANE / SH_GEO_LDS_PARTS)
#define SH_GEO_LDS_WORDS (SH_GEO_LDS_PER_LANE * SH_GEO_LDS_BLOCK / 32)      // one bit per vertex slot of the LDS kernel: 640 words
#define SH_GEO_STATE 8           // int32 per pair in "geo.state", and once more behind the last pair for the call
#define SH_GEO_W_SWEEPS 3        // (words 0..2 rotate)
#define SH_GEO_W_FAILED 4        // the LDS kernel ran out of rounds (the rule cannot: V_b + 1)

static_assert(SH_GEO_EDGES == 0 && SH_GEO_UNFOLD == SH_GEOD_UNFOLD && SH_GEO_ROOT == SH_GEOD_ROOT && SH_GEO_NO_PRED == SH_GEOD_NO_PRED &&
              SH_GEO_UNREACHED == SH_GEOD_UNREACHED && SH_GEO_INFO_BYTES == sizeof(GeoInfo), "sh_scalar.h: the modes, the codes of a predecessor, the info record");
static_assert(SH_GEO_LDS_PER_LANE == 20 && SH_GEO_LDS_PART * SH_GEO_LDS_PARTS == SH_GEO_LDS_PER_LANE && SH_GEO_LDS_VERTICES * 8 + SH_GEO_LDS_WORDS * 4 + 1024 <= 163840, "the plane of a pair in the LDS of one workgroup");

struct GeoMesh { int b, k, nv; size_t base; };      // a pair's mesh, set, vertices and the start of its planes
__device__ inline GeoMesh geo_pair(const long long* voff, int K) {
  GeoMesh m;
  m.b = blockIdx.z; m.k = blockIdx.y;
  m.nv = (int)(voff[m.b + 1] - voff[m.b]);
  m.base = (size_t)K * (size_t)voff[m.b] + (size_t)m.k * (size_t)m.nv;
  return m;
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_face(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
           const int* __restrict__ adj, double* __restrict__ frec, int* __restrict__ opp) {
  const int b = blockIdx.y;
  const long long nf = foff[b + 1] - foff[b], fi = (long long)blockIdx.x * SH_GEO_BLOCK + threadIdx.x;
  if (fi >= nf) return;
  const int* f = faces + 3 * foff[b];
  double rec[SH_GEOD_FACE];
  int q[3];
  geo_face(verts + 3 * voff[b], f, adj + 3 * foff[b], (int)fi, topo_degenerate(f + 3 * fi, (int)(voff[b + 1] - voff[b])), rec, q);
  double* out = frec + SH_GEOD_FACE * (size_t)(foff[b] + fi);
#pragma unroll
  for (int i = 0; i < SH_GEOD_FACE; ++i) out[i] = rec[i];
  int* o = opp + 3 * (size_t)(foff[b] + fi);
  o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_init(const long long* __restrict__ voff, int K, int lds_vertices, double* __restrict__ dist, int* __restrict__ source, int* __restrict__ state) {
  const GeoMesh m = geo_pair(voff, K);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int* st = state + SH_GEO_STATE * (size_t)(m.b * K + m.k);
    const int general = m.nv > lds_vertices ? 1 : 0;
    st[0] = general;
#pragma unroll
    for (int i = 1; i < SH_GEO_STATE; ++i) st[i] = 0;
    if (general) atomicOr(state + SH_GEO_STATE * (size_t)(gridDim.z * K), 1);      // (the call's words: zeroed by the host)
  }
  const long long v = (long long)blockIdx.x * SH_GEO_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  dist[m.base + v] = geo_inf();
  source[m.base + v] = SH_GEOD_NO_LABEL;
}

// the bits of a distance: >= +0.0 or +inf, so they order as unsigned integers
__device__ inline unsigned long long geo_bits(double x) { return (unsigned long long)__double_as_longlong(x); }

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_seed(const long long* __restrict__ voff, int K, const int* __restrict__ src_off, const int* __restrict__ src, const double* __restrict__ d0, double max_dist,
           double* __restrict__ dist) {
  const int p = blockIdx.x, b = p / K, k = p - b * K;
  const size_t base = (size_t)K * (size_t)voff[b] + (size_t)k * (size_t)(voff[b + 1] - voff[b]);
  for (int i = src_off[p] + threadIdx.x; i < src_off[p + 1]; i += SH_GEO_BLOCK) {
    const double z = d0[i] + 0.0;      // (-0.0 becomes +0.0)
    if (z <= max_dist) atomicMin((unsigned long long*)(dist + base + src[i]), geo_bits(z));
  }
}

// vertex v fell: every vertex an arc of v leads to has to be relaxed again (32-bit integer atomics on the bits in LDS)
__device__ inline void geo_mark(const int* faces, const int* opp, const int* row, int n, int v, int mode, unsigned* need) {
  for (int i = 0; i < n; ++i) {
    const int f = row[i];
    const int* fc = faces + 3 * (size_t)f;
    const int k = vert_corner(fc, v), k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const int u1 = fc[k1], u2 = fc[k2];
    atomicOr(need + (u1 >> 5), 1u << (u1 & 31));
    atomicOr(need + (u2 >> 5), 1u << (u2 & 31));
    if (mode == SH_GEOD_UNFOLD) {
      const int q = opp[3 * (size_t)f + k1];
      if (q >= 0) atomicOr(need + (q >> 5), 1u << (q & 31));
    }
  }
}

__global__ void __launch_bounds__(SH_GEO_LDS_BLOCK)
k_geo_lds(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
          const int* __restrict__ vface, const double* __restrict__ frec, const int* __restrict__ opp, int K, int mode, double max_dist, int lds_vertices,
          double* __restrict__ dist, int* __restrict__ state) {
  __shared__ double d[SH_GEO_LDS_VERTICES];
  __shared__ unsigned need[SH_GEO_LDS_WORDS];      // bit v: a neighbour of v fell since v was relaxed last (all set at the start)
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const int nv = (int)(voff[b + 1] - voff[b]);
  if (nv > lds_vertices || nv > SH_GEO_LDS_VERTICES) return;      // (uniform: a pair of the general path)
  double* plane = dist + (size_t)K * (size_t)voff[b] + (size_t)k * (size_t)nv;
  for (int i = tid; i < nv; i += SH_GEO_LDS_BLOCK) d[i] = plane[i];
  if (tid < SH_GEO_LDS_WORDS) need[tid] = 0xffffffffu;
  __syncthreads();
  const int* row = vrow + voff[b] + b;
  const int* fc = faces + 3 * foff[b];
  const int* rows = vface + 3 * foff[b];
  const double* fr = frec + SH_GEOD_FACE * (size_t)foff[b];
  const int* op = opp + 3 * foff[b];
  int sweeps = 0, failed = 1;
  while (sweeps <= nv) {      // (the rule needs at most V_b rounds that change something and one that does not)
    int fell = 0;
#pragma unroll 1
    for (int part = 0; part < SH_GEO_LDS_PARTS; ++part) {
      const int v0 = tid + part * (SH_GEO_LDS_PART * SH_GEO_LDS_BLOCK);
      double nw[SH_GEO_LDS_PART];
      unsigned mine = 0;      // bit j: vertex j of the part was relaxed
#pragma unroll
      for (int j = 0; j < SH_GEO_LDS_PART; ++j) {
        const int v = v0 + j * SH_GEO_LDS_BLOCK;
        nw[j] = 0.0;
        if (v < nv && ((need[v >> 5] >> (v & 31)) & 1u)) {
          const int s = row[v];
          nw[j] = geo_relax(fc, fr, op, rows + s, row[v + 1] - s, v, mode, max_dist, d[v], d);
          mine |= 1u << j;
        }
      }
      __syncthreads();      // every read of the part, of the plane and of the bits, lies in front of every write
      // every set bit of the part's words has been served: lane 32 i of a wave owns bits 32 i .. 32 i + 31 of each of its ten words
      if ((tid & 31) == 0) {
#pragma unroll
        for (int j = 0; j < SH_GEO_LDS_PART; ++j) need[(v0 + j * SH_GEO_LDS_BLOCK) >> 5] = 0u;
      }
      __syncthreads();      // the bits are cleared in front of the ones this part sets
      int low = 0;
#pragma unroll
      for (int j = 0; j < SH_GEO_LDS_PART; ++j) {
        const int v = v0 + j * SH_GEO_LDS_BLOCK;
        if (((mine >> j) & 1u) && nw[j] < d[v]) {
          d[v] = nw[j]; low = 1;      // (its own word: no other lane reads or writes it here)
          const int s = row[v];
          geo_mark(fc, op, rows + s, row[v + 1] - s, v, mode, need);
        }
      }
      fell |= __syncthreads_or(low);      // every write of the part lies in front of the next read
    }
    ++sweeps;
    if (!fell) { failed = 0; break; }
  }
  for (int i = tid; i < nv; i += SH_GEO_LDS_BLOCK) plane[i] = d[i];
  if (tid == 0) {
    int* st = state + SH_GEO_STATE * (size_t)(b * K + k);
    st[SH_GEO_W_SWEEPS] = sweeps; st[SH_GEO_W_FAILED] = failed;
  }
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_round(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
            const int* __restrict__ vface, const double* __restrict__ frec, const int* __restrict__ opp, int K, int mode, double max_dist, int lds_vertices,
            int round, double* dist, double* plane, int* state) {
  const GeoMesh m = geo_pair(voff, K);
  int* st = state + SH_GEO_STATE * (size_t)(m.b * K + m.k);
  int* call = state + SH_GEO_STATE * (size_t)(gridDim.z * K);
  const int now = round % 3, next = (round + 1) % 3, after = (round + 2) % 3;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (first) st[after] = 0;
  if (first && m.b == 0 && m.k == 0) call[after] = 0;
  if (m.nv <= lds_vertices || st[now] == 0) return;      // (uniform in the workgroup)
  const long long v0 = (long long)blockIdx.x * SH_GEO_BLOCK;
  if (v0 >= m.nv) return;
  const int v = (int)v0 + threadIdx.x;
  int fell = 0;
  if (v < m.nv) {
    const double* in = ((round & 1) ? plane : dist) + m.base;
    double* out = ((round & 1) ? dist : plane) + m.base;
    const int* row = vrow + voff[m.b] + m.b;
    const int s = row[v];
    const double dv = in[v];
    const double nw = geo_relax(faces + 3 * foff[m.b], frec + SH_GEOD_FACE * (size_t)foff[m.b], opp + 3 * foff[m.b], vface + 3 * foff[m.b] + s, row[v + 1] - s, v, mode,
                                max_dist, dv, in);
    out[v] = nw;
    fell = nw < dv ? 1 : 0;
  }
  if (__syncthreads_or(fell) && threadIdx.x == 0) { atomicOr(st + next, 1); atomicOr(call + next, 1); }
  if (first) st[SH_GEO_W_SWEEPS] = round + 1;
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_root(const long long* __restrict__ voff, int K, const int* __restrict__ src_off, const int* __restrict__ src, const double* __restrict__ d0,
           const double* __restrict__ dist, int* __restrict__ source) {
  const int p = blockIdx.x, b = p / K, k = p - b * K;
  const size_t base = (size_t)K * (size_t)voff[b] + (size_t)k * (size_t)(voff[b + 1] - voff[b]);
  const int first = src_off[p];
  for (int i = first + threadIdx.x; i < src_off[p + 1]; i += SH_GEO_BLOCK) {
    const double z = d0[i] + 0.0;
    if (z == dist[base + src[i]]) atomicMin(source + base + src[i], i - first);
  }
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_pred(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
           const int* __restrict__ vface, const double* __restrict__ frec, const int* __restrict__ opp, int K, int mode, const double* __restrict__ dist,
           int* __restrict__ pred, int* __restrict__ source, int* __restrict__ jump) {
  const GeoMesh m = geo_pair(voff, K);
  const long long vl = (long long)blockIdx.x * SH_GEO_BLOCK + threadIdx.x;
  if (vl >= m.nv) return;
  const int v = (int)vl;
  const double* d = dist + m.base;
  int pr, up = v;
  if (!(d[v] < geo_inf())) {
    pr = SH_GEOD_UNREACHED;
    source[m.base + v] = -1;
  } else if (source[m.base + v] != SH_GEOD_NO_LABEL) {
    pr = SH_GEOD_ROOT;
  } else {
    const int* row = vrow + voff[m.b] + m.b;
    const int s = row[v];
    pr = geo_pred(faces + 3 * foff[m.b], frec + SH_GEOD_FACE * (size_t)foff[m.b], opp + 3 * foff[m.b], vface + 3 * foff[m.b] + s, row[v + 1] - s, v, mode, d);
    source[m.base + v] = -1;
    if (pr >= 0) up = pr;
  }
  pred[m.base + v] = pr;
  jump[m.base + v] = up;
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_jump(const long long* __restrict__ voff, int K, int* jump) {
  const GeoMesh m = geo_pair(voff, K);
  const long long v = (long long)blockIdx.x * SH_GEO_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  int* j = jump + m.base;
  const int up = j[v];
  const int top = j[up];
  if (top != up) j[v] = top;
}

__global__ void __launch_bounds__(SH_GEO_BLOCK)
k_geo_info(const long long* __restrict__ voff, int K, const double* __restrict__ dist, const int* __restrict__ pred, const int* __restrict__ jump,
           const int* __restrict__ state, int* source, GeoInfo* __restrict__ info) {
  __shared__ double s_d[SH_GEO_BLOCK];
  __shared__ int s_v[SH_GEO_BLOCK], s_n[3][SH_GEO_BLOCK];
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const int nv = (int)(voff[b + 1] - voff[b]);
  const size_t base = (size_t)K * (size_t)voff[b] + (size_t)k * (size_t)nv;
  double far_d = 0.0;
  int far_v = -1, reached = 0, roots = 0, no_pred = 0;
  for (int v = tid; v < nv; v += SH_GEO_BLOCK) {
    const int pr = pred[base + v];
    if (pr == SH_GEOD_UNREACHED) continue;
    ++reached;
    roots += pr == SH_GEOD_ROOT ? 1 : 0;
    no_pred += pr == SH_GEOD_NO_PRED ? 1 : 0;
    geo_far(dist[base + v], v, &far_d, &far_v);
    if (pr >= 0) {
      const int top = jump[base + v];
      source[base + v] = pred[base + top] == SH_GEOD_ROOT ? source[base + top] : -1;
    }
  }
  s_d[tid] = far_d; s_v[tid] = far_v; s_n[0][tid] = reached; s_n[1][tid] = roots; s_n[2][tid] = no_pred;
  __syncthreads();
  for (int off = SH_GEO_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) {
      geo_far(s_d[tid + off], s_v[tid + off], &s_d[tid], &s_v[tid]);
      s_n[0][tid] += s_n[0][tid + off]; s_n[1][tid] += s_n[1][tid + off]; s_n[2][tid] += s_n[2][tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int* st = state + SH_GEO_STATE * (size_t)(b * K + k);
    GeoInfo r;
    r.far_dist = s_v[0] < 0 ? 0.0 : s_d[0]; r.reached = s_n[0][0]; r.roots = s_n[1][0]; r.no_pred = s_n[2][0]; r.farthest = s_v[0];
    r.sweeps = st[SH_GEO_W_SWEEPS]; r.status = st[SH_GEO_W_FAILED] ? SH_ERR_INTERNAL_DEV : 0;
    info[b * K + k] = r;
  }
}

}  // namespace sh
