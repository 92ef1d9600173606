// k_repair.h -- repair of the resident batch (include/shoulder_hip.h sh_mesh_repair): one winding per shell, outward shells (optionally by
// nesting depth) and filled holes, on the adjacency, the labels and the shell records of sh_mesh_topology.  The scalar rules are
// sh_scalar.h rep_*.  "repair.work" holds, per mesh, the smallest face of every label ("first", at foff[b]), the shells that are not
// orientable ("bad", at sumF + foff[b]), the two queues of the walk (at 2 sumF + 2 foff[b]), the shells' face lists (at 4 sumF + foff[b])
// and SH_REPAIR_HEAD words of state (at 5 sumF + b SH_REPAIR_HEAD).
//   k_repair_seed    (block of 256 faces, mesh).  first[label]: a written shell's record names its first face (32 440 atomics on one word
//                    per bone cost 0.98 ms for the bench batch); a shell behind the records takes an integer atomicMin, whose result is
//                    unique whatever the order.
//   k_repair_parity  (mesh), 1024 lanes.  THE PARITY PASS.  A face graph of a bone is 300 to 400 levels deep, so the walk is not a launch
//                    per level: one workgroup walks the mesh breadth first from the first faces of all shells at once.  Two bits per
//                    face live in LDS (seen, parity: 32 KB for SH_REPAIR_LDS_FACES faces); a lane takes a face of the level, and for
//                    each neighbour it is the first to see (atomicOr on the seen word: one winner) sets the parity bit and appends the
//                    neighbour to the next level's queue in "repair.work".  Then every manifold slot is held against the parities
//                    (a contradiction marks the shell in `bad`; which parity a shell that is not orientable got is never used) and
//                    "repair.flip" / "repair.par" get the winding flips.  A mesh that does not fit, is deeper than max_rounds levels or
//                    has no finished topology gets its status into the state and no flips.
//   k_repair_shell   (shell k, mesh).  The shell's faces ascending into its list (per chunk of 256 faces a ballot of label == k in every wave and the
//                    waves' counts through LDS: two barriers a chunk; a block scan per chunk cost 0.94 ms for the bench batch);
//                    with orient >= OUTWARD the terms of V6 by list place into "repair.term", the sums of blocks of SH_REP_V6_BLOCK places
//                    one lane each, the block sums one after the other by lane 0; an inverted shell's faces are flipped once more.
//                    "repair.par" keeps the outward orientation; the shell's record.
//   k_repair_nest    (shell k, mesh), orient == NESTED.  W_k at the first corner of the shell's first face over the faces of the other
//                    closed orientable shells as "repair.par" orients them (nobody writes it here), a lane per block of SH_WIND_BLOCK
//                    faces, the block sums one after the other; a shell of odd depth gets flip = par ^ 1.
//   k_repair_emit    (block of 256, mesh).  The oriented faces and the vertices into the mesh's regions of "repair.faces" / "repair.verts".
//   k_repair_holes   (mesh).  Touches the border half-edges only ("repair.edge", 18 int32 arrays of the mesh's border count): they are
//                    compacted once, ascending by id; a lane per half-edge walks to its successor (rep_succ) and finds it in the list by
//                    bisection; the cycle's smallest id and the places along the cycle come from two runs of pointer doubling inside
//                    this workgroup, a barrier per round and no launch; a cycle that passes a vertex twice is cut there (the head's
//                    incidence row names the candidates) and the doubling runs once more, only then; the holes are ranked by a scan over the starts, their faces,
//                    vertices and edges by three more; every half-edge writes its fill face, a lane per hole its new vertex; then the
//                    hole records, the holes per shell and the mesh's info record.
// No floating-point atomics.  Integer atomics only where the value is unique whatever the order (a minimum, a count, a flag, a winner
// whose prize is the same for every winner).  Every index is below its array's size by construction: a queue takes a face once (the winner
// of its seen bit), a list has the shell's face count of the topology, the border arrays have the mesh's border count of the topology and
// every write into them is guarded by it, a hole adds at most as many faces as it has edges and one vertex per three.
#pragma once
#include "k_topo.h"      // topo_block_scan
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_REPAIR_BLOCK 256
#define SH_REPAIR_WALK 1024          // lanes of k_repair_parity
#define SH_REPAIR_HEAD 16            // int32 per mesh of state: 0 status, 1 levels, 2 border half-edges, 3 holes
#define SH_REPAIR_EDGE_ARRAYS 18
#define SH_REPAIR_NEST_BLOCKS (SH_REPAIR_LDS_FACES / SH_WIND_BLOCK)

static_assert(SH_REPAIR_NONE == SH_REP_ORIENT_NONE && SH_REPAIR_WINDING == SH_REP_ORIENT_WINDING && SH_REPAIR_OUTWARD == SH_REP_ORIENT_OUTWARD &&
              SH_REPAIR_NESTED == SH_REP_ORIENT_NESTED && SH_REPAIR_FILL_NONE == SH_REP_FILL_NONE && SH_REPAIR_FAN == SH_REP_FILL_FAN &&
              SH_REPAIR_CENTROID == SH_REP_FILL_CENTROID && SH_REPAIR_NONORIENTABLE == SH_REP_SHELL_NONORIENTABLE && SH_REPAIR_AMBIGUOUS == SH_REP_SHELL_AMBIGUOUS &&
              SH_REPAIR_HOLE_FILLED == SH_REP_HOLE_FILLED && SH_REPAIR_HOLE_TOO_LONG == SH_REP_HOLE_TOO_LONG && SH_REPAIR_HOLE_SHELL == SH_REP_HOLE_SHELL &&
              SH_REPAIR_HOLE_OPEN == SH_REP_HOLE_OPEN && SH_REPAIR_HOLE_TOO_SHORT == SH_REP_HOLE_TOO_SHORT, "sh_scalar.h: the modes and statuses of the repair");
static_assert(sizeof(sh_repair_options) == 24 && sizeof(sh_repair_info) == 64 && sizeof(sh_repair_shell) == 40 && sizeof(sh_repair_hole) == 32, "the records of sh_mesh_repair");
static_assert(SH_REPAIR_BLOCK == SH_TOPO_BLOCK, "topo_block_scan");
static_assert(SH_REPAIR_LDS_FACES % 32 == 0 && SH_REPAIR_LDS_FACES % SH_WIND_BLOCK == 0 && SH_REPAIR_NEST_BLOCKS <= SH_REPAIR_BLOCK, "the walk's bits; a lane per winding block");

// the parts of "repair.work" of mesh b
struct RepairWork { int *first, *bad, *queue, *list, *state; };
__device__ inline RepairWork repair_work(int* work, long long sumF, const long long* foff, int b) {
  return {work + foff[b], work + sumF + foff[b], work + 2 * sumF + 2 * foff[b], work + 4 * sumF + foff[b], work + 5 * sumF + (long long)b * SH_REPAIR_HEAD};
}
__device__ inline int repair_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(SH_REPAIR_BLOCK)
k_repair_seed(const long long* __restrict__ foff, const int* __restrict__ label, const sh_topology* __restrict__ tinfo, const sh_shell* __restrict__ tshells, int S,
              long long sumF, int* __restrict__ work) {
  const int b = blockIdx.y;
  const long long nf = foff[b + 1] - foff[b], f = (long long)blockIdx.x * SH_REPAIR_BLOCK + threadIdx.x;
  if (f >= nf) return;
  const int lab = label[foff[b] + f];
  if (lab < 0 || lab >= nf) return;
  int* first = work + foff[b] + lab;
  if (lab < tinfo[b].shells_written && lab < S) {      // a written shell's record names its first face: one plain store, by that face
    if (tshells[(size_t)b * S + lab].first_face == (int)f) *first = (int)f;
  } else if (*first > (int)f) {                        // (values only fall: a stale read only costs the atomic)
    atomicMin(first, (int)f);
  }
}

__global__ void __launch_bounds__(SH_REPAIR_WALK)
k_repair_parity(const int* __restrict__ faces, const long long* __restrict__ foff, const int* __restrict__ adj, const int* __restrict__ label,
                const sh_topology* __restrict__ tinfo, long long sumF, int orient, int max_rounds, int* work, unsigned char* __restrict__ flip,
                unsigned char* __restrict__ par) {
  __shared__ unsigned seen[SH_REPAIR_LDS_FACES / 32], bits[SH_REPAIR_LDS_FACES / 32];
  __shared__ int qn[2];
  __shared__ int s_status;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long nfl = foff[b + 1] - foff[b];
  const RepairWork w = repair_work(work, sumF, foff, b);
  const int status = tinfo[b].status != 0 || nfl > SH_REPAIR_LDS_FACES ? SH_ERR_CAPACITY_DEV : 0;
  const int nf = (int)nfl;
  const int* fb = faces + 3 * foff[b];
  const int* ab = adj + 3 * foff[b];
  const int* lb = label + foff[b];
  unsigned char *fl = flip + foff[b], *pr = par + foff[b];
  if (tid < SH_REPAIR_HEAD) w.state[tid] = tid == 0 ? status : 0;
  if (status) {      // (uniform) an unchanged copy
    for (long long f = tid; f < nfl; f += SH_REPAIR_WALK) { fl[f] = 0; pr[f] = 0; }
    return;
  }
  for (int i = tid; i < SH_REPAIR_LDS_FACES / 32; i += SH_REPAIR_WALK) { seen[i] = 0u; bits[i] = 0u; }
  if (tid < 2) qn[tid] = 0;
  if (tid == 0) s_status = 0;
  __syncthreads();
  int *q0 = w.queue, *q1 = w.queue + nf;
  for (int f = tid; f < nf; f += SH_REPAIR_WALK) {
    const int lab = lb[f];
    if (lab >= 0 && w.first[lab] == f) {
      atomicOr(&seen[f >> 5], 1u << (f & 31));
      q0[atomicAdd(&qn[0], 1)] = f;
    }
  }
  __syncthreads();
  int cur = 0, level = 0;
  while (true) {
    const int n = qn[cur];
    if (n == 0) break;
    if (level >= max_rounds) { if (tid == 0) s_status = SH_ERR_CAPACITY_DEV; break; }      // (uniform: n and level are)
    __syncthreads();
    if (tid == 0) qn[cur ^ 1] = 0;
    __syncthreads();
    const int* qi = cur ? q1 : q0;
    int* qo = cur ? q0 : q1;
    for (int i = tid; i < n; i += SH_REPAIR_WALK) {
      const int f = qi[i];
      const int pf = (bits[f >> 5] >> (f & 31)) & 1u;
      for (int e = 0; e < 3; ++e) {
        const int g = ab[3 * (size_t)f + e];
        if (g < 0 || g >= nf) continue;
        const unsigned bit = 1u << (g & 31);
        if (seen[g >> 5] & bit) continue;      // (values only rise: a stale read costs the atomic)
        if (atomicOr(&seen[g >> 5], bit) & bit) continue;
        if (pf ^ rep_same(fb, f, e, g)) atomicOr(&bits[g >> 5], bit);
        const int at = atomicAdd(&qn[cur ^ 1], 1);
        if (at < nf) qo[at] = g;
      }
    }
    __syncthreads();
    cur ^= 1;
    ++level;
  }
  __syncthreads();
  if (s_status) {      // (uniform)
    if (tid == 0) w.state[0] = s_status;
    for (int f = tid; f < nf; f += SH_REPAIR_WALK) { fl[f] = 0; pr[f] = 0; }
    return;
  }
  if (tid == 0) w.state[1] = level;
  for (int f = tid; f < nf; f += SH_REPAIR_WALK) {
    const int lab = lb[f];
    if (lab < 0) continue;
    const int pf = (bits[f >> 5] >> (f & 31)) & 1u;
    for (int e = 0; e < 3; ++e) {
      const int g = ab[3 * (size_t)f + e];
      if (g <= f || g >= nf) continue;      // (each manifold edge once, from its smaller face)
      const int pg = (bits[g >> 5] >> (g & 31)) & 1u;
      if ((pf ^ pg) != rep_same(fb, f, e, g)) atomicOr(w.bad + lab, 1);
    }
  }
  __threadfence();
  __syncthreads();
  for (int f = tid; f < nf; f += SH_REPAIR_WALK) {
    const int lab = lb[f];
    const int pf = (bits[f >> 5] >> (f & 31)) & 1u;
    const unsigned char v = orient >= SH_REP_ORIENT_WINDING && lab >= 0 && repair_load(w.bad + lab) == 0 ? (unsigned char)pf : (unsigned char)0;
    fl[f] = v; pr[f] = v;
  }
}

__global__ void __launch_bounds__(SH_REPAIR_BLOCK)
k_repair_shell(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
               const int* __restrict__ label, const sh_topology* __restrict__ tinfo, const sh_shell* __restrict__ tshells, int S, long long sumF, int orient,
               int* work, double* term, unsigned char* flip, unsigned char* par, sh_repair_shell* __restrict__ shells) {
  __shared__ int s[SH_REPAIR_BLOCK];
  __shared__ int s_off, s_flips, s_inv;
  __shared__ double s_v6;
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const RepairWork w = repair_work(work, sumF, foff, b);
  if (w.state[0] != 0 || k >= tinfo[b].shells_written || k >= S) return;      // (uniform)
  const int nf = (int)(foff[b + 1] - foff[b]);
  const sh_shell* recs = tshells + (size_t)b * S;
  const sh_shell rec = recs[k];
  if (tid == 0) { s_off = 0; s_flips = 0; s_inv = 0; s_v6 = 0.0; }
  __syncthreads();
  int before = 0;
  for (int j = tid; j < k; j += SH_REPAIR_BLOCK) before += recs[j].faces;
  if (before) atomicAdd(&s_off, before);
  __syncthreads();
  const int off = s_off, n = rec.faces;
  if (off < 0 || n < 0 || (long long)off + n > nf) return;      // (never: the counts are the topology's)
  const int* lb = label + foff[b];
  int* list = w.list + off;
  int run = 0;
  for (int f0 = rec.first_face / SH_REPAIR_BLOCK * SH_REPAIR_BLOCK; f0 < nf && run < n; f0 += SH_REPAIR_BLOCK) {
    const int f = f0 + tid;
    const int hit = f < nf && lb[f] == k ? 1 : 0;
    const unsigned long long m = __ballot(hit);      // the hits of this wave: a place is the hits before it, in the wave and in the waves before
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s[wave] = __popcll(m);
    __syncthreads();
    int at = run + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
    for (int v = 0; v < SH_REPAIR_BLOCK / 64; ++v) { at += v < wave ? s[v] : 0; total += s[v]; }
    if (hit && at < n) list[at] = f;
    run += total;
    __syncthreads();
  }
  const bool ok = w.bad[k] == 0;
  const int* fb = faces + 3 * foff[b];
  const float* vb = verts + 3 * voff[b];
  unsigned char *fl = flip + foff[b], *pr = par + foff[b];
  if (ok && orient >= SH_REP_ORIENT_OUTWARD) {
    const double o[3] = {rep_center(rec.lo[0], rec.hi[0]), rep_center(rec.lo[1], rec.hi[1]), rep_center(rec.lo[2], rec.hi[2])};
    double* tm = term + foff[b] + off;
    double* bs = term + sumF + foff[b] + off;
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
      const int f = list[i];
      int c[3];
      rep_face(fb, f, fl[f], c);
      tm[i] = rep_v6_term(vb, c, o);
    }
    __syncthreads();
    const int nblk = (n + SH_REP_V6_BLOCK - 1) / SH_REP_V6_BLOCK;
    for (int j = tid; j < nblk; j += SH_REPAIR_BLOCK) {
      const int i1 = (j + 1) * SH_REP_V6_BLOCK < n ? (j + 1) * SH_REP_V6_BLOCK : n;
      double sum = 0.0;
      int i = j * SH_REP_V6_BLOCK;
      for (; i + 32 <= i1; i += 32) {      // 32 loads in flight, then the 32 additions in order: one lane alone would wait for every line
        double t[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) t[u] = tm[i + u];
#pragma unroll
        for (int u = 0; u < 32; ++u) sum += t[u];
      }
      for (; i < i1; ++i) sum += tm[i];
      bs[j] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      double v6 = 0.0;
      for (int j = 0; j < nblk; ++j) v6 += bs[j];
      s_v6 = v6; s_inv = v6 < 0.0 ? 1 : 0;
    }
    __syncthreads();
  }
  const int inv = s_inv;
  int flips = 0;
  for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
    const int f = list[i];
    const int p = fl[f];
    flips += p;
    const unsigned char v = (unsigned char)(p ^ inv);
    fl[f] = v; pr[f] = v;
  }
  if (flips) atomicAdd(&s_flips, flips);
  __syncthreads();
  if (tid == 0) {
    sh_repair_shell r;
    r.status = ok ? 0 : SH_REP_SHELL_NONORIENTABLE; r.parity_flips = s_flips; r.inverted = inv; r.depth = -1; r.holes = 0; r.holes_filled = 0;
    r.V6 = s_v6; r.W = 0.0;
    shells[(size_t)b * S + k] = r;
  }
}

__global__ void __launch_bounds__(SH_REPAIR_BLOCK)
k_repair_nest(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const int* __restrict__ label, const sh_topology* __restrict__ tinfo, const sh_shell* __restrict__ tshells, int S, long long sumF, int* work,
              const unsigned char* __restrict__ par, unsigned char* __restrict__ flip, sh_repair_shell* __restrict__ shells) {
  __shared__ double bsum[SH_REPAIR_NEST_BLOCKS];
  __shared__ int s_off, s_odd;
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const RepairWork w = repair_work(work, sumF, foff, b);
  const int written = tinfo[b].shells_written;
  if (w.state[0] != 0 || k >= written || k >= S || tinfo[b].n_shells > written) return;      // (uniform; more shells than records: OUTWARD)
  const int nf = (int)(foff[b + 1] - foff[b]);
  const sh_shell* recs = tshells + (size_t)b * S;
  const sh_shell rec = recs[k];
  sh_repair_shell* out = shells + (size_t)b * S + k;
  if (w.bad[k] != 0) {      // never flipped, no depth
    if (tid == 0) { out->depth = 0; out->W = 0.0; }
    return;
  }
  if (tid == 0) { s_off = 0; s_odd = 0; }
  __syncthreads();
  int before = 0;
  for (int j = tid; j < k; j += SH_REPAIR_BLOCK) before += recs[j].faces;
  if (before) atomicAdd(&s_off, before);
  const int* fb = faces + 3 * foff[b];
  const float* vb = verts + 3 * voff[b];
  const int* lb = label + foff[b];
  const unsigned char* pr = par + foff[b];
  const int blocks = (nf + SH_WIND_BLOCK - 1) / SH_WIND_BLOCK;      // (<= SH_REPAIR_NEST_BLOCKS: the mesh fits the walk)
  if (tid < blocks && tid < SH_REPAIR_NEST_BLOCKS) {
    const float* pk = vb + 3 * (size_t)fb[3 * (size_t)rec.first_face];
    const double p[3] = {(double)pk[0], (double)pk[1], (double)pk[2]};
    const int f1 = (tid + 1) * SH_WIND_BLOCK < nf ? (tid + 1) * SH_WIND_BLOCK : nf;
    double sum = 0.0;
    for (int f = tid * SH_WIND_BLOCK; f < f1; ++f) {
      const int lab = lb[f];
      if (lab < 0 || lab == k || lab >= written) continue;
      if (w.bad[lab] != 0 || recs[lab].border_slots != 0 || recs[lab].nonmanifold_slots != 0) continue;
      int c[3];
      rep_face(fb, f, pr[f], c);
      double P[3][3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) P[i][j] = (double)vb[3 * (size_t)c[i] + j];
      sum += solid_angle_tri(p, P[0], P[1], P[2]);
    }
    bsum[tid] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int j = 0; j < blocks && j < SH_REPAIR_NEST_BLOCKS; ++j) total += bsum[j];
    const double W = total / (4.0 * M_PI);
    int ambiguous;
    const int depth = rep_depth(W, &ambiguous);
    out->W = W; out->depth = depth;
    if (ambiguous) out->status = SH_REP_SHELL_AMBIGUOUS;
    s_odd = depth & 1;
  }
  __syncthreads();
  if (!s_odd) return;
  const int off = s_off, n = rec.faces;
  if (off < 0 || n < 0 || (long long)off + n > nf) return;
  unsigned char* fl = flip + foff[b];
  for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
    const int f = w.list[off + i];
    fl[f] = (unsigned char)(pr[f] ^ 1);
  }
}

__global__ void __launch_bounds__(SH_REPAIR_BLOCK)
k_repair_emit(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const unsigned char* __restrict__ flip, const long long* __restrict__ off, int B, int* __restrict__ rfaces, float* __restrict__ rverts) {
  const int b = blockIdx.y;
  const long long nf = foff[b + 1] - foff[b], nv = voff[b + 1] - voff[b], i = (long long)blockIdx.x * SH_REPAIR_BLOCK + threadIdx.x;
  if (i < nf) {
    int c[3];
    rep_face(faces + 3 * foff[b], (int)i, flip[foff[b] + i], c);
    int* o = rfaces + 3 * (off[b] + i);
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  }
  if (i < nv) {
    const float* p = verts + 3 * (voff[b] + i);
    float* o = rverts + 3 * (off[B + 1 + b] + i);
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  }
}

// the exclusive sums of a[0 .. n) in place, by the whole workgroup -> the total
__device__ inline int repair_scan(int* a, int n, int* s, int tid) {
  int run = 0;
  for (int i0 = 0; i0 < n; i0 += SH_REPAIR_BLOCK) {
    const int i = i0 + tid;
    const int c = i < n ? a[i] : 0;
    const int incl = topo_block_scan(c, s, tid);
    if (i < n) a[i] = run + incl - c;
    s[tid] = incl;
    __syncthreads();
    run += s[SH_REPAIR_BLOCK - 1];
    __syncthreads();
  }
  return run;
}

// The cycles of the injective map succ over n places, by the whole workgroup: cyc[i] = i lies on a cycle, start[i] = the smallest place of
// its cycle (-1 on a chain), dist[i] = the steps from i to the last place of its cycle when the cycle is cut open in front of its start
// (so the cycle has dist[start] + 1 places and i the place dist[start] - dist[i]).  Two runs of pointer doubling of R rounds, 2^R >= n,
// each round reading one pair of arrays and writing the other.
__device__ __forceinline__ void repair_loops(const int* succ, int n, int R, int* pa, int* pb, int* ma, int* mb, int* cyc, int* start, int* dist, int tid) {
  for (int i = tid; i < n; i += SH_REPAIR_BLOCK) { pa[i] = succ[i]; ma[i] = i; }
  __syncthreads();
  int *pi = pa, *po = pb, *mi = ma, *mo = mb;
  for (int r = 0; r < R; ++r) {
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
      const int p = pi[i];
      const int m0 = mi[i], m1 = p >= 0 ? mi[p] : m0;
      mo[i] = m1 < m0 ? m1 : m0;
      po[i] = p >= 0 ? pi[p] : -1;
    }
    __syncthreads();
    int* t = pi; pi = po; po = t;
    t = mi; mi = mo; mo = t;
  }
  for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
    const int on = pi[i] >= 0 ? 1 : 0;
    cyc[i] = on; start[i] = on ? mi[i] : -1;
  }
  __syncthreads();
  int *ni = pa, *no = pb, *di = ma, *dq = mb;
  for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
    const int nx = cyc[i] && succ[i] != start[i] ? succ[i] : -1;
    ni[i] = nx; di[i] = nx >= 0 ? 1 : 0;
  }
  __syncthreads();
  for (int r = 0; r < R; ++r) {
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
      const int p = ni[i];
      dq[i] = di[i] + (p >= 0 ? di[p] : 0);
      no[i] = p >= 0 ? ni[p] : -1;
    }
    __syncthreads();
    int* t = ni; ni = no; no = t;
    t = di; di = dq; dq = t;
  }
  for (int i = tid; i < n; i += SH_REPAIR_BLOCK) dist[i] = di[i];
  __syncthreads();
}

__global__ void __launch_bounds__(SH_REPAIR_BLOCK)
k_repair_holes(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
               const int* __restrict__ adj, const int* __restrict__ label, const int* __restrict__ vrow, const int* __restrict__ vface,
               const sh_topology* __restrict__ tinfo, const unsigned char* __restrict__ flip, const long long* __restrict__ off, int B, int S, long long sumF, int orient, int fill, int max_hole_edges, int max_holes, int* work, int* edge,
               int* __restrict__ rfaces, float* __restrict__ rverts, sh_repair_info* __restrict__ info, sh_repair_shell* shells, sh_repair_hole* __restrict__ holes) {
  __shared__ int s[SH_REPAIR_BLOCK];
  __shared__ int acc[6];      // blocked, filled, largest, flipped, not orientable, inverted
  const int b = blockIdx.x, tid = threadIdx.x;
  const RepairWork w = repair_work(work, sumF, foff, b);
  const int nf = (int)(foff[b + 1] - foff[b]), nv = (int)(voff[b + 1] - voff[b]);
  const int status = w.state[0];
  const long long RF0 = off[b], RV0 = off[B + 1 + b], E0 = off[2 * (B + 1) + b];
  const int cap = (int)(off[2 * (B + 1) + b + 1] - E0);
  int* base = edge + SH_REPAIR_EDGE_ARRAYS * E0;
  int *half = base, *succ = base + cap, *pa = base + 2 * (size_t)cap, *pb = base + 3 * (size_t)cap, *ma = base + 4 * (size_t)cap, *mb = base + 5 * (size_t)cap;
  int *dist = base + 6 * (size_t)cap, *cut = base + 7 * (size_t)cap, *hidx = base + 8 * (size_t)cap, *cyc = base + 9 * (size_t)cap, *hL = base + 10 * (size_t)cap;
  int *hst = base + 11 * (size_t)cap, *hff = base + 12 * (size_t)cap, *hvv = base + 13 * (size_t)cap, *heo = base + 14 * (size_t)cap, *order = base + 15 * (size_t)cap;
  int *hsta = base + 16 * (size_t)cap, *start = base + 17 * (size_t)cap;
  const int* fb = faces + 3 * foff[b];
  const int* ab = adj + 3 * foff[b];
  const int* lb = label + foff[b];
  const float* vb = verts + 3 * voff[b];
  const unsigned char* fl = flip + foff[b];
  if (tid < 6) acc[tid] = 0;
  __syncthreads();
  int n = 0, H = 0, faces_added = 0, verts_added = 0;
  if (status == 0) {      // (uniform)
    // the border half-edges of the oriented faces, ascending by id
    int run = 0;
    for (int f0 = 0; f0 < nf; f0 += SH_REPAIR_BLOCK) {
      const int f = f0 + tid;
      int c = 0;
      if (f < nf)
        for (int e = 0; e < 3; ++e) c += ab[3 * (size_t)f + e] == SH_TOPO_BORDER ? 1 : 0;
      const int incl = topo_block_scan(c, s, tid);
      if (c) {
        int at = run + incl - c;
        for (int e = 0; e < 3; ++e)
          if (ab[3 * (size_t)f + rep_slot(e, fl[f])] == SH_TOPO_BORDER) {
            if (at < cap) half[at] = 3 * f + e;
            ++at;
          }
      }
      s[tid] = incl;
      __syncthreads();
      run += s[SH_REPAIR_BLOCK - 1];
      __syncthreads();
    }
    n = run < cap ? run : cap;
    // the successors
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
      const int id = half[i];
      int sf, se, at = -1;
      if (rep_succ(fb, ab, fl, nf, id / 3, id % 3, &sf, &se)) {
        const int want = 3 * sf + se;
        int lo = 0, hi = n - 1;
        while (lo <= hi) {
          const int mid = (lo + hi) >> 1, x = half[mid];
          if (x == want) { at = mid; break; }
          if (x < want) lo = mid + 1; else hi = mid - 1;
        }
      }
      succ[i] = at;
    }
    __syncthreads();
    int R = 1;
    while ((1 << (R - 1)) < n) ++R;
    repair_loops(succ, n, R, pa, pb, ma, mb, cyc, start, dist, tid);
    // A cycle that passes a vertex more than once is cut there: a half-edge takes the successor of the half-edge of its cycle with the
    // same head that comes last before it (its own when there is no other).  The candidates are the border slots that end at the head
    // in the faces of the head's incidence row.
    int pinched = 0;
    const int* row = vrow + voff[b] + b;
    const int* vf = vface + 3 * foff[b];
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
      int to = succ[i];
      if (cyc[i]) {
        const int id = half[i];
        const int e = id % 3, w = rep_corner(fb, id / 3, fl[id / 3], e == 2 ? 0 : e + 1);
        const int top = dist[start[i]], mine = top - dist[i];      // the places of the cycle count from its start
        int best = -1, best_at = -1;                                // the largest place below mine, else the largest of all: the one before, cyclically
        for (int j = row[w]; j < row[w + 1]; ++j) {
          const int g = vf[j];
          const int ge = rep_corner(fb, g, fl[g], 1) == w ? 0 : rep_corner(fb, g, fl[g], 2) == w ? 1 : 2;        // the slot of g that ends at w
          if (ab[3 * (size_t)g + rep_slot(ge, fl[g])] != SH_TOPO_BORDER) continue;
          const int want = 3 * g + ge;
          int lo = 0, hi = n - 1, at = -1;
          while (lo <= hi) {
            const int mid = (lo + hi) >> 1, x = half[mid];
            if (x == want) { at = mid; break; }
            if (x < want) lo = mid + 1; else hi = mid - 1;
          }
          if (at < 0 || at == i || !cyc[at] || start[at] != start[i]) continue;
          const int place = top - dist[at];
          const int key = place < mine ? place + top + 1 : place;  // below mine ranks above everything behind mine
          if (key > best) { best = key; best_at = at; }
        }
        if (best_at >= 0) { to = succ[best_at]; pinched = 1; }
      }
      cut[i] = to;
    }
    if (__syncthreads_or(pinched)) repair_loops(cut, n, R, pa, pb, ma, mb, cyc, start, dist, tid);      // (uniform)
    int blocked = 0;
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) blocked += 1 - cyc[i];
    if (blocked) atomicAdd(&acc[0], blocked);
    // the holes in the order of their starts
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) hidx[i] = cyc[i] && start[i] == i ? 1 : 0;
    __syncthreads();
    H = repair_scan(hidx, n, s, tid);
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK)
      if (cyc[i] && start[i] == i) {
        const int h = hidx[i], L = dist[i] + 1;
        const int lab = lb[half[i] / 3];
        const int st = rep_hole_status(L, lab >= 0 && w.bad[lab] == 0 ? 1 : 0, fill, max_hole_edges);
        hst[h] = i; hL[h] = L; hsta[h] = st; heo[h] = L;
        hff[h] = st == SH_REP_HOLE_FILLED ? rep_fill_faces(L, fill) : 0;
        hvv[h] = st == SH_REP_HOLE_FILLED ? rep_fill_verts(fill) : 0;
      }
    __syncthreads();
    faces_added = repair_scan(hff, H, s, tid);
    verts_added = repair_scan(hvv, H, s, tid);
    (void)repair_scan(heo, H, s, tid);
    // the tails in loop order and the fill faces
    for (int i = tid; i < n; i += SH_REPAIR_BLOCK) {
      if (!cyc[i]) continue;
      const int si = start[i], h = hidx[si], L = hL[h], j = L - 1 - dist[i];
      if (j < 0 || j >= L) continue;      // (never)
      const int id = half[i], f = id / 3, e = id % 3;
      const int tail = rep_corner(fb, f, fl[f], e), head = rep_corner(fb, f, fl[f], e == 2 ? 0 : e + 1);
      if (heo[h] + j < cap) order[heo[h] + j] = tail;
      if (hsta[h] != SH_REP_HOLE_FILLED) continue;
      int out[3];
      const int sid = half[si];
      const int k = rep_fill_face(fill, L, j, rep_corner(fb, sid / 3, fl[sid / 3], sid % 3), tail, head, nv + hvv[h], out);
      if (k >= 0 && hff[h] + k < cap) {
        int* o = rfaces + 3 * (RF0 + nf + hff[h] + k);
        o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
      }
    }
    __syncthreads();
    const int written = tinfo[b].shells_written < S ? tinfo[b].shells_written : S;
    for (int h = tid; h < H; h += SH_REPAIR_BLOCK) {
      const int filled = hsta[h] == SH_REP_HOLE_FILLED ? 1 : 0, L = hL[h];
      if (filled && fill == SH_REP_FILL_CENTROID && 3 * (long long)hvv[h] < cap) rep_centroid(vb, order + heo[h], L, rverts + 3 * (RV0 + nv + hvv[h]));
      const int id = half[hst[h]], lab = lb[id / 3];
      if (lab >= 0 && lab < written) {
        atomicAdd(&shells[(size_t)b * S + lab].holes, 1);
        if (filled) atomicAdd(&shells[(size_t)b * S + lab].holes_filled, 1);
      }
      if (filled) atomicAdd(&acc[1], 1);
      atomicMax(&acc[2], L);
      if (h < max_holes) {
        sh_repair_hole r;
        r.shell = lab; r.start_face = id / 3; r.start_slot = id % 3; r.edges = L; r.status = hsta[h];
        r.first_face = filled ? nf + hff[h] : -1; r.faces_added = filled ? rep_fill_faces(L, fill) : 0;
        r.vertex = filled && fill == SH_REP_FILL_CENTROID ? nv + hvv[h] : -1;
        holes[(size_t)b * max_holes + h] = r;
      }
    }
    int flipped = 0, bad = 0, inverted = 0;
    for (int f = tid; f < nf; f += SH_REPAIR_BLOCK) flipped += fl[f];
    const int n_shells = tinfo[b].n_shells;
    for (int k = tid; k < n_shells && k < nf; k += SH_REPAIR_BLOCK) bad += w.bad[k] != 0 ? 1 : 0;
    for (int k = tid; k < written; k += SH_REPAIR_BLOCK) inverted += shells[(size_t)b * S + k].inverted;
    if (flipped) atomicAdd(&acc[3], flipped);
    if (bad) atomicAdd(&acc[4], bad);
    if (inverted) atomicAdd(&acc[5], inverted);
  }
  __syncthreads();
  if (tid == 0) {
    sh_repair_info r;
    const bool left = status == 0 && tinfo[b].n_shells > tinfo[b].shells_written;
    r.status = status != 0 ? status : (left && orient == SH_REP_ORIENT_NESTED ? SH_ERR_CAPACITY_DEV : 0);
    r.shells_nonorientable = acc[4]; r.shells_inverted = acc[5]; r.faces_flipped = acc[3];
    r.holes = H; r.holes_written = H < max_holes ? H : max_holes; r.holes_filled = acc[1]; r.largest_hole = acc[2]; r.blocked_edges = acc[0];
    r.faces_added = faces_added; r.verts_added = verts_added; r.faces_out = nf + faces_added; r.verts_out = nv + verts_added;
    r.flags = (acc[3] > 0 || faces_added > 0 ? SH_REPAIR_CHANGED : 0) | (left && orient >= SH_REP_ORIENT_OUTWARD ? SH_REPAIR_SHELLS_LEFT : 0);
    r.shell_records = S; r.reserved = 0;
    info[b] = r;
    w.state[2] = n; w.state[3] = H;
  }
}

}  // namespace sh
