// k_topo.h -- mesh topology of the resident batch (include/shoulder_hip.h sh_mesh_topology): the vertex -> face incidence, the face
// adjacency, the shells (connected components over manifold edges) and their counts.  Everything is integer; the scalar rules are
// sh_scalar.h topo_*.  Grids are (block of SH_TOPO_BLOCK = 256 faces, mesh) with one face per lane, or (mesh) with 256 lanes.
//   k_topo_count  (block, mesh).  p[f] = f in both arrays of "topo.p"; a non-degenerate face adds 1 to the count of each of its vertices
//                 ("topo.cursor", zeroed by the host) with integer atomics; the degenerate faces are counted per workgroup.
//   k_topo_scan   (mesh).  The exclusive scan of the counts in chunks of 256 (integer: any tree) into "topo.vrow" and, as the rows'
//                 cursors, back into "topo.cursor"; vertices_used and max_valence; word 0 of the head becomes 1.
//   k_topo_fill   (block, mesh).  A non-degenerate face takes a place in each of its vertices' rows through the cursor, in "topo.tmp":
//                 the rows' CONTENT is defined, the order of the atomics is not.
//   k_topo_rows   (block, mesh).  The defined order without a sort: an entry's place in its row of "topo.vface" is the number of smaller
//                 entries of that row in "topo.tmp" (the entries of a row are distinct).  A lane reads valence entries per corner: 6 on a
//                 bone, the whole fan on a cap's centre, where the lanes of the fan read the same words.  No row length is assumed.
//   k_topo_adj    (block, mesh).  A lane walks, for each of its face's three slots, the SHORTER of the rows of the edge's two vertices
//                 (both hold every user of the edge; the spokes of a fan walk the rim's rows) and finds the users, the other face, the
//                 owner (the smallest user: rows ascend, so the first one met) and the direction (topo_slot); the edge counts are taken at
//                 the owner's slot, summed in LDS and added to the head with one integer atomic per workgroup and count.
//   k_topo_round  (block, mesh), once per round.  THE HOT PATH.  A workgroup whose mesh is finished (word `round` of the head is 0)
//                 returns at once.  A lane forms topo_round of its face from the old array alone: gathers of in[u], in[in[u]] and the
//                 same for three neighbours, no LDS (nothing is shared between the lanes of a block: the neighbours of consecutive
//                 faces are wherever the mesher put them).  The new array still holds round r - 2, which is >= everything written into
//                 it, so only LOWER values are written: one atomicMin for the face itself, left out when the word already holds
//                 no more (values only fall, so a stale read only costs the atomic), and one for its parent when a neighbour hooks it
//                 lower.  A converged region issues no atomic at all.  Whether the round changed something is decided from the old array
//                 (topo_round), so it does not depend on the order of the atomics; one atomicOr per workgroup sets word round + 1.
//   k_topo_rank   (mesh).  The rounds from the head; the roots (p[f] == f, non-degenerate) scanned in face order into shell indices
//                 ("topo.tmp" [0, F)), the shells' face counts zeroed ("topo.tmp" [F, 2 F)), the first max_shells records initialised.
//   k_topo_label  (block, mesh).  "topo.label"; the faces per shell and, for the first max_shells shells, the slot counts and the box
//                 corners (integer atomics on topo_enc): the lanes that share the label of the workgroup's first labelled face sum in
//                 LDS and cost one global atomic per field and workgroup, the others go to global memory directly.
//   k_topo_finish (mesh).  The largest shell (ties to the smaller index), the records decoded (slots -> edges, topo_dec), "topo.info".
// No floating-point atomics.  Every index is below its array's size by construction: face indices are checked at upload and again by
// topo_degenerate, rows hold 3 (F - degenerate) entries, p holds face indices of the face's own mesh.
#pragma once
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_TOPO_BLOCK 256
#define SH_TOPO_HEAD 64          // int32 per mesh in "topo.state": word r = round r - 1 changed something (word 0: 1), then the counts
#define SH_TOPO_W_DEGENERATE 40
#define SH_TOPO_W_USED 41
#define SH_TOPO_W_EDGES 42       // edges, border, non-manifold, inconsistent: four words in this order
#define SH_TOPO_W_VALENCE 46
#define SH_TOPO_W_SHELLS 47
#define SH_TOPO_W_ROUNDS 48
#define SH_TOPO_W_FULL 49
#define SH_TOPO_SHELL_WORDS 12   // an sh_shell as int32: six counts, lo[3], hi[3]

static_assert(SH_ADJ_BORDER == SH_TOPO_BORDER && SH_ADJ_NONMANIFOLD == SH_TOPO_NONMANIFOLD && SH_ADJ_DEGENERATE == SH_TOPO_DEGENERATE, "sh_scalar.h: the adjacency codes");
static_assert(SH_TOPO_MAX_ROUNDS + 1 <= SH_TOPO_W_DEGENERATE && SH_TOPO_W_FULL < SH_TOPO_HEAD, "topo.state: the head of a mesh");
static_assert(sizeof(sh_topology) == 64 && offsetof(sh_topology, euler) == 32 && offsetof(sh_topology, flags) == 56, "sh_topology");
static_assert(sizeof(sh_shell) == 4 * SH_TOPO_SHELL_WORDS && offsetof(sh_shell, lo) == 24 && offsetof(sh_shell, hi) == 36, "sh_shell");
static_assert(sizeof(sh_topology_options) == 12, "sh_topology_options");

// the inclusive sums of one value per lane of a 256-lane workgroup (s: 256 int32 of LDS, free again on return)
__device__ inline int topo_block_scan(int c, int* s, int tid) {
  s[tid] = c;
  __syncthreads();
  for (int off = 1; off < SH_TOPO_BLOCK; off <<= 1) {
    const int t = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  const int r = s[tid];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(SH_TOPO_BLOCK)
k_topo_count(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, int* __restrict__ cursor,
             int* __restrict__ p, int* __restrict__ state) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_TOPO_BLOCK;
  if (f0 >= nf) return;      // (uniform in the workgroup)
  const int nv = (int)(voff[b + 1] - voff[b]);
  const long long fi = f0 + tid;
  int deg = 0;
  if (fi < nf) {
    const int* f = faces + 3 * (foff[b] + fi);
    int* pb = p + 2 * foff[b];
    pb[fi] = (int)fi; pb[nf + fi] = (int)fi;
    int* cnt = cursor + voff[b] + b;
    if (topo_degenerate(f, nv)) deg = 1;
    else for (int k = 0; k < 3; ++k) atomicAdd(cnt + f[k], 1);
  }
  const int n = __syncthreads_count(deg);
  if (tid == 0 && n) atomicAdd(state + (size_t)b * SH_TOPO_HEAD + SH_TOPO_W_DEGENERATE, n);
}

__global__ void __launch_bounds__(256)
k_topo_scan(const long long* __restrict__ voff, int* __restrict__ cursor, int* __restrict__ vrow, int* __restrict__ state) {
  __shared__ int s[256];
  __shared__ int smax;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = (int)(voff[b + 1] - voff[b]);
  int* cnt = cursor + voff[b] + b;
  int* row = vrow + voff[b] + b;
  if (tid == 0) smax = 0;
  int run = 0, used = 0, maxv = 0;
  for (int v0 = 0; v0 < nv; v0 += 256) {
    const int v = v0 + tid;
    const int c = v < nv ? cnt[v] : 0;
    const int incl = topo_block_scan(c, s, tid);
    if (v < nv) { row[v] = run + incl - c; cnt[v] = run + incl - c; }
    maxv = c > maxv ? c : maxv;
    used += __syncthreads_count(c > 0);
    s[tid] = incl;
    __syncthreads();
    run += s[255];
    __syncthreads();
  }
  if (maxv) atomicMax(&smax, maxv);
  __syncthreads();
  if (tid == 0) {
    int* head = state + (size_t)b * SH_TOPO_HEAD;
    row[nv] = run; cnt[nv] = run;
    head[0] = 1; head[SH_TOPO_W_USED] = used; head[SH_TOPO_W_VALENCE] = smax;
  }
}

__global__ void __launch_bounds__(SH_TOPO_BLOCK)
k_topo_fill(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, int* __restrict__ cursor,
            int* __restrict__ tmp) {
  const int b = blockIdx.y;
  const long long nf = foff[b + 1] - foff[b], fi = (long long)blockIdx.x * SH_TOPO_BLOCK + threadIdx.x;
  if (fi >= nf) return;
  const int* f = faces + 3 * (foff[b] + fi);
  if (topo_degenerate(f, (int)(voff[b + 1] - voff[b]))) return;
  int* cur = cursor + voff[b] + b;
  int* t = tmp + 3 * foff[b];
  for (int k = 0; k < 3; ++k) {
    const int pos = atomicAdd(cur + f[k], 1);
    if (pos >= 0 && pos < 3 * nf) t[pos] = (int)fi;      // (always: the rows hold 3 (F - degenerate) entries)
  }
}

__global__ void __launch_bounds__(SH_TOPO_BLOCK)
k_topo_rows(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
            const int* __restrict__ tmp, int* __restrict__ vface) {
  const int b = blockIdx.y;
  const long long nf = foff[b + 1] - foff[b], fi = (long long)blockIdx.x * SH_TOPO_BLOCK + threadIdx.x;
  if (fi >= nf) return;
  const int* f = faces + 3 * (foff[b] + fi);
  if (topo_degenerate(f, (int)(voff[b + 1] - voff[b]))) return;
  const int* row = vrow + voff[b] + b;
  const int* t = tmp + 3 * foff[b];
  int* vf = vface + 3 * foff[b];
  for (int k = 0; k < 3; ++k) {
    const int s = row[f[k]], e = row[f[k] + 1];
    int rank = 0;
    for (int j = s; j < e; ++j) rank += t[j] < (int)fi ? 1 : 0;
    vf[s + rank] = (int)fi;
  }
}

__global__ void __launch_bounds__(SH_TOPO_BLOCK)
k_topo_adj(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff, const int* __restrict__ vrow,
           const int* __restrict__ vface, int* __restrict__ adj, int* __restrict__ state) {
  __shared__ int acc[4];      // edges, border, non-manifold, inconsistent: at their owners' slots
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_TOPO_BLOCK;
  if (f0 >= nf) return;      // (uniform in the workgroup)
  if (tid < 4) acc[tid] = 0;
  __syncthreads();
  const long long fi = f0 + tid;
  if (fi < nf) {
    const int* fb = faces + 3 * foff[b];
    const int* f = fb + 3 * fi;
    int* out = adj + 3 * (foff[b] + fi);
    if (topo_degenerate(f, (int)(voff[b + 1] - voff[b]))) {
      out[0] = SH_TOPO_DEGENERATE; out[1] = SH_TOPO_DEGENERATE; out[2] = SH_TOPO_DEGENERATE;
    } else {
      const int* row = vrow + voff[b] + b;
      const int* vf = vface + 3 * foff[b];
      int mine[4] = {0, 0, 0, 0};
      for (int e = 0; e < 3; ++e) {
        const int a = f[e], c = f[e == 2 ? 0 : e + 1];
        const int na = row[a + 1] - row[a], nc = row[c + 1] - row[c];
        const int pick = nc < na ? c : a;
        int owner, same;
        const int val = topo_slot(fb, vf + row[pick], nc < na ? nc : na, (int)fi, e, &owner, &same);
        out[e] = val;
        if (owner) { mine[0] += 1; mine[1] += val == SH_TOPO_BORDER ? 1 : 0; mine[2] += val == SH_TOPO_NONMANIFOLD ? 1 : 0; mine[3] += same; }
      }
      for (int k = 0; k < 4; ++k)
        if (mine[k]) atomicAdd(&acc[k], mine[k]);
    }
  }
  __syncthreads();
  if (tid < 4 && acc[tid]) atomicAdd(state + (size_t)b * SH_TOPO_HEAD + SH_TOPO_W_EDGES + tid, acc[tid]);
}

__global__ void __launch_bounds__(SH_TOPO_BLOCK)
k_topo_round(const long long* __restrict__ foff, const int* __restrict__ adj, int* p, int* __restrict__ state, int round) {
  const int b = blockIdx.y, tid = threadIdx.x;
  int* head = state + (size_t)b * SH_TOPO_HEAD;
  if (head[round] == 0) return;      // this mesh is finished (uniform in the workgroup; written by the launch before this one)
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_TOPO_BLOCK;
  if (f0 >= nf) return;
  const int* in = p + 2 * foff[b] + (size_t)(round & 1) * nf;
  int* nxt = p + 2 * foff[b] + (size_t)((round + 1) & 1) * nf;
  const long long fi = f0 + tid;
  int changed = 0;
  if (fi < nf) {
    int self, hook;
    changed = topo_round(in, adj + 3 * (foff[b] + fi), (int)fi, &self, &hook);
    const int pu = in[fi];
    if (nxt[fi] > self) atomicMin(nxt + fi, self);
    if (hook < in[pu]) atomicMin(nxt + pu, hook);
  }
  if (__syncthreads_or(changed) && tid == 0) atomicOr(head + round + 1, 1);
}

__global__ void __launch_bounds__(256)
k_topo_rank(const long long* __restrict__ foff, const int* __restrict__ adj, const int* __restrict__ p, int* __restrict__ state, int* __restrict__ tmp,
            int* __restrict__ shells /* B x max_shells x SH_TOPO_SHELL_WORDS */, int max_shells, int max_rounds) {
  __shared__ int s[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int* head = state + (size_t)b * SH_TOPO_HEAD;
  const int nf = (int)(foff[b + 1] - foff[b]);
  int full;
  const int rounds = topo_rounds(head, max_rounds, &full);      // (every lane: uniform)
  int n_shells = 0;
  if (!full) {
    const int* fin = p + 2 * foff[b] + (size_t)(rounds & 1) * nf;      // launch r wrote array (r + 1) & 1; the launches behind `rounds` returned at once
    const int* ad = adj + 3 * foff[b];
    int* rank = tmp + 3 * foff[b];
    int* cnt = rank + nf;
    for (int f0 = 0; f0 < nf; f0 += 256) {
      const int f = f0 + tid;
      const int root = f < nf && ad[3 * (size_t)f] != SH_TOPO_DEGENERATE && fin[f] == f ? 1 : 0;
      const int incl = topo_block_scan(root, s, tid);
      if (f < nf) { rank[f] = root ? n_shells + incl - 1 : -1; cnt[f] = 0; }
      s[tid] = incl;
      __syncthreads();
      n_shells += s[255];
      __syncthreads();
    }
  }
  int* rec = shells + (size_t)b * max_shells * SH_TOPO_SHELL_WORDS;
  for (int k = tid; k < max_shells; k += 256)
    for (int w = 0; w < SH_TOPO_SHELL_WORDS; ++w) rec[(size_t)k * SH_TOPO_SHELL_WORDS + w] = k < n_shells && w >= 6 && w < 9 ? -1 : 0;      // lo: above every topo_enc
  if (tid == 0) { head[SH_TOPO_W_SHELLS] = n_shells; head[SH_TOPO_W_ROUNDS] = rounds; head[SH_TOPO_W_FULL] = full; }
}

__global__ void __launch_bounds__(SH_TOPO_BLOCK)
k_topo_label(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
             const int* __restrict__ adj, const int* __restrict__ p, const int* __restrict__ state, int* __restrict__ tmp, int* __restrict__ label,
             int* __restrict__ shells, int max_shells) {
  __shared__ int s_first;
  __shared__ int s_acc[5];      // faces, border slots, non-manifold slots, manifold slots, inconsistent slots
  __shared__ unsigned s_lo[3], s_hi[3];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_TOPO_BLOCK;
  if (f0 >= nf) return;      // (uniform in the workgroup)
  const int* head = state + (size_t)b * SH_TOPO_HEAD;
  const int full = head[SH_TOPO_W_FULL], rounds = head[SH_TOPO_W_ROUNDS];
  const long long fi = f0 + tid;
  const int* ad = adj + 3 * (foff[b] + fi);
  const int* fin = p + 2 * foff[b] + (size_t)(rounds & 1) * nf;
  int* rank = tmp + 3 * foff[b];
  int* cnt = rank + nf;
  int lab = -1;
  if (fi < nf) {
    if (!full && ad[0] != SH_TOPO_DEGENERATE) lab = rank[fin[fi]];
    label[foff[b] + fi] = lab;
  }
  if (full) return;      // (uniform: a word of the mesh's head)
  if (tid == 0) s_first = -1;
  if (tid < 5) s_acc[tid] = 0;
  if (tid < 3) { s_lo[tid] = ~0u; s_hi[tid] = 0u; }
  __syncthreads();
  if (lab >= 0) atomicCAS(&s_first, -1, lab);      // (whichever lane wins: the sums do not depend on the choice)
  __syncthreads();
  const int first = s_first;
  if (first < 0) return;      // only degenerate faces here (uniform)
  int* recs = shells + (size_t)b * max_shells * SH_TOPO_SHELL_WORDS;
  if (lab >= 0) {
    const int* fb = faces + 3 * foff[b];
    const int* f = fb + 3 * fi;
    int mine[5] = {1, 0, 0, 0, 0};
    for (int e = 0; e < 3; ++e) {
      const int v = ad[e];
      if (v == SH_TOPO_BORDER) mine[1] += 1;
      else if (v == SH_TOPO_NONMANIFOLD) mine[2] += 1;
      else if (v >= 0) {
        const int a = f[e], c = f[e == 2 ? 0 : e + 1];
        const int* g = fb + 3 * (size_t)v;
        const int ge = topo_edge_slot(g, a, c);
        mine[3] += 1;
        mine[4] += ge >= 0 && g[ge] == a ? 1 : 0;
      }
    }
    unsigned lo[3], hi[3];
    const float* vb = verts + 3 * voff[b];
    for (int k = 0; k < 3; ++k) {
      const unsigned x = topo_enc(vb[3 * (size_t)f[0] + k]), y = topo_enc(vb[3 * (size_t)f[1] + k]), z = topo_enc(vb[3 * (size_t)f[2] + k]);
      lo[k] = x < y ? (x < z ? x : z) : (y < z ? y : z);
      hi[k] = x > y ? (x > z ? x : z) : (y > z ? y : z);
    }
    const bool recorded = lab < max_shells;
    int* rec = recs + (size_t)(recorded ? lab : 0) * SH_TOPO_SHELL_WORDS;
    if (recorded && fin[fi] == (int)fi) rec[0] = (int)fi;      // the shell's root is its first face
    if (lab == first) {
      for (int k = 0; k < 5; ++k)
        if (mine[k]) atomicAdd(&s_acc[k], mine[k]);
      for (int k = 0; k < 3; ++k) { atomicMin(&s_lo[k], lo[k]); atomicMax(&s_hi[k], hi[k]); }
    } else {
      atomicAdd(cnt + lab, 1);
      if (recorded) {
        for (int k = 0; k < 5; ++k)
          if (mine[k]) atomicAdd(rec + 1 + k, mine[k]);
        for (int k = 0; k < 3; ++k) { atomicMin((unsigned*)rec + 6 + k, lo[k]); atomicMax((unsigned*)rec + 9 + k, hi[k]); }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    atomicAdd(cnt + first, s_acc[0]);
    if (first < max_shells) {
      int* rec = recs + (size_t)first * SH_TOPO_SHELL_WORDS;
      for (int k = 0; k < 5; ++k)
        if (s_acc[k]) atomicAdd(rec + 1 + k, s_acc[k]);
      for (int k = 0; k < 3; ++k) { atomicMin((unsigned*)rec + 6 + k, s_lo[k]); atomicMax((unsigned*)rec + 9 + k, s_hi[k]); }
    }
  }
}

__global__ void __launch_bounds__(256)
k_topo_finish(const long long* __restrict__ foff, const int* __restrict__ state, const int* __restrict__ tmp, int* __restrict__ shells, int max_shells,
              sh_topology* __restrict__ info /* B */) {
  __shared__ int s_c[256], s_k[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* head = state + (size_t)b * SH_TOPO_HEAD;
  const int nf = (int)(foff[b + 1] - foff[b]), n_shells = head[SH_TOPO_W_SHELLS];
  const int* cnt = tmp + 3 * foff[b] + nf;
  int bc = 0, bk = -1;
  for (int k = tid; k < n_shells; k += 256) {      // (ascending k: a tie keeps the smaller index)
    const int c = cnt[k];
    if (c > bc) { bc = c; bk = k; }
  }
  s_c[tid] = bc; s_k[tid] = bk;
  const int written = n_shells < max_shells ? n_shells : max_shells;
  int* recs = shells + (size_t)b * max_shells * SH_TOPO_SHELL_WORDS;
  for (int k = tid; k < written; k += 256) {
    int* rec = recs + (size_t)k * SH_TOPO_SHELL_WORDS;
    rec[4] = rec[4] / 2; rec[5] = rec[5] / 2;      // every manifold edge was seen from both of its faces
    for (int w = 6; w < 12; ++w) {
      const float x = topo_dec((unsigned)rec[w]);
      __builtin_memcpy(rec + w, &x, 4);
    }
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 256; ++i)
      if (s_c[i] > bc || (s_c[i] == bc && s_k[i] >= 0 && s_k[i] < bk)) { bc = s_c[i]; bk = s_k[i]; }
    sh_topology r;
    const int deg = head[SH_TOPO_W_DEGENERATE];
    r.status = head[SH_TOPO_W_FULL] ? SH_ERR_CAPACITY_DEV : 0; r.rounds = head[SH_TOPO_W_ROUNDS];
    r.faces_degenerate = deg; r.vertices_used = head[SH_TOPO_W_USED];
    r.edges = head[SH_TOPO_W_EDGES]; r.border_edges = head[SH_TOPO_W_EDGES + 1]; r.nonmanifold_edges = head[SH_TOPO_W_EDGES + 2];
    r.inconsistent_edges = head[SH_TOPO_W_EDGES + 3];
    r.euler = r.vertices_used - r.edges + (nf - deg); r.max_valence = head[SH_TOPO_W_VALENCE];
    r.n_shells = n_shells; r.shells_written = written; r.largest_shell = bk; r.largest_faces = bk >= 0 ? bc : 0;
    r.flags = (r.border_edges == 0 && r.nonmanifold_edges == 0 && deg == 0 ? SH_TOPO_WATERTIGHT : 0) | (r.inconsistent_edges == 0 ? SH_TOPO_CONSISTENT : 0);
    r.reserved = 0;
    info[b] = r;
  }
}

}  // namespace sh
