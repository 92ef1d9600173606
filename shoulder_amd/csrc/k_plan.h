// k_plan.h -- implant plans: the cuts of the last seated resection, the heads seated on them and the stems fitted below them joined
// into (cut, head, stem) triples and ranked per humerus under one rule (include/shoulder_hip.h sh_resect_plan).  The step the
// reference leaves open (arthroplasty.py:178-182, the commented-out `HumeralImplantation` that "continues from the humeral head
// osteotomy and places the implant"); k_headfit.h / k_seat.h / k_stem.h measure, this joins.  All arithmetic is sh_scalar.h plan_*,
// one source for the device and the host tests.
//   k_plan_ref       (tile of 256 vertices, humerus) workgroups, one vertex per lane: the vertex is widened, its side of the reference
//                    plane and its frame height taken (plan_side, canal_map_point), and the two (z, vid) maxima of the tile -- head
//                    side, tuberosity side -- go through one fixed shuffle tree and LDS across the four waves into the tile's slab
//                    entry: the per-tile-slab pattern of k_resect_faces.  z and the id are never packed into one atomic word.
//   k_plan_ref_join  one wave per humerus adds the tiles in tile order (lanes stride them, the same tree) and writes sh_plan_ref, as
//                    k_resect_join adds k_resect_faces' slab.  A maximum under a total order does not depend on the order: the record
//                    is the same bytes whatever the batch, the humerus' position in it or the tiling.
//   k_plan_terms     one workgroup of 128 per cut: lane k < 64 takes head k (and lane 0 the cut part, from the seat record k_h = 0
//                    it holds anyway), lane 64 + k stem k.  Every 232-byte seat record and every 128-byte stem record is read once,
//                    here; what is left of it is a 16-byte PlanTerm {cost, feasible} and the unweighted terms a plan record shows.
//   k_plan_select    one workgroup of 256 per humerus, N rounds.  A round is an arg-min of the key (cost, i) over the lane-strided
//                    candidates whose key is greater than the previous round's winner; a candidate is two 16-byte loads (its head
//                    and stem parts; the cut part and the compat word repeat) and two adds.  The winner is reduced by one fixed
//                    shuffle tree, then through LDS across the waves.  N P K_h K_s / 256 evaluations per lane: nothing at a
//                    planning sweep, slow at the limits (see the header); there is one variant.
// No floating-point atomics and no floating-point sums across lanes anywhere; the only cross-lane sum is the integer n_feasible.
#pragma once
#include "k_stem.h"

namespace sh {

#define SH_PLAN_TILE 256
#define SH_PLAN_TERM_THREADS 128
#define SH_PLAN_THREADS 256

struct __attribute__((aligned(16))) PlanTop { double z; int vid, pad; };      // one side's maximum of one (humerus, tile); vid < 0: none
static_assert(sizeof(PlanTop) == 16 && sizeof(PlanTerm) == 16, "PlanTop and PlanTerm are 16 bytes");
static_assert(sizeof(sh_plan_ref) == 96 && sizeof(sh_plan) == 112 && sizeof(sh_plan_rule) == 96, "sh_plan_ref, sh_plan, sh_plan_rule");

// the reference plane of humerus b (the caller's row, or the record's anatomic-neck plane) and the humerus' status
__device__ inline int plan_ref_plane(const sh_landmarks* __restrict__ lm, const double* __restrict__ ref_planes, const int* __restrict__ hstatus, int b,
                                     double* pl /* 6 */) {
  int st = 0;
  if (ref_planes) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pl[k] = ref_planes[6 * (size_t)b + k];
  } else {
    const sh_landmarks* L = lm + b;
    st = L->status;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { pl[k] = L->anp_plane_point[k]; pl[3 + k] = L->anp_plane_normal[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(pl[k]);
    if (st == 0 && (!ok || !((pl[3] * pl[3] + pl[4] * pl[4]) + pl[5] * pl[5] > 0.0))) st = SH_ERR_GEOMETRY_DEV;
  }
  if (st == 0) st = hstatus[b];
  return st;
}

// the wave's maximum of (z, vid) in lane 0
__device__ __forceinline__ void plan_top_tree(double* z, int* vid) {
  for (int off = 32; off > 0; off >>= 1) {
    const double oz = __shfl_down(*z, off);
    const int ov = __shfl_down(*vid, off);
    if (ov >= 0 && plan_ref_better(oz, ov, *z, *vid)) { *z = oz; *vid = ov; }
  }
}

__global__ void __launch_bounds__(SH_PLAN_TILE)
k_plan_ref(const float* __restrict__ verts, const long long* __restrict__ voff, const double* __restrict__ frames /* B x 16 */,
           const int* __restrict__ hstatus /* B */, const sh_landmarks* __restrict__ lm /* null: ref_planes */, const double* __restrict__ ref_planes /* B x 6 or null */,
           double margin, int tstride /* tiles per humerus in the slab */, PlanTop* __restrict__ slab /* [B][tstride][2] */) {
  __shared__ PlanTop s_top[SH_PLAN_TILE / 64][2];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long v0 = voff[b], nv = voff[b + 1] - v0;
  if ((long long)t * SH_PLAN_TILE >= nv) return;      // (uniform) the tile lies behind the humerus' vertices
  double pl[6];
  if (plan_ref_plane(lm, ref_planes, hstatus, b, pl) != 0) return;      // (uniform) the join writes the status
  const long long vi = (long long)t * SH_PLAN_TILE + tid;
  double hz = 0.0, tz = 0.0;
  int hv = -1, tv = -1;
  if (vi < nv) {
    const float* v = verts + 3 * (v0 + vi);
    const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
    const double s = plan_side(pl, pl + 3, x, y, z);
    double q[3];
    canal_map_point(frames + 16 * (size_t)b, x, y, z, q);
    if (s > 0.0) { hz = q[2]; hv = (int)vi; }
    if (s <= plan_tuberosity_bound(margin, pl + 3)) { tz = q[2]; tv = (int)vi; }
  }
  plan_top_tree(&hz, &hv);
  plan_top_tree(&tz, &tv);
  if (lane == 0) { s_top[wave][0] = PlanTop{hz, hv, 0}; s_top[wave][1] = PlanTop{tz, tv, 0}; }
  __syncthreads();
  if (tid < 2) {      // the four waves in order
    PlanTop m = s_top[0][tid];
    for (int w = 1; w < SH_PLAN_TILE / 64; ++w) {
      const PlanTop o = s_top[w][tid];
      if (o.vid >= 0 && plan_ref_better(o.z, o.vid, m.z, m.vid)) m = o;
    }
    slab[((size_t)b * tstride + t) * 2 + tid] = m;
  }
}

__global__ void __launch_bounds__(64)
k_plan_ref_join(const float* __restrict__ verts, const long long* __restrict__ voff, const int* __restrict__ hstatus, const sh_landmarks* __restrict__ lm,
                const double* __restrict__ ref_planes, int tstride, const PlanTop* __restrict__ slab, sh_plan_ref* __restrict__ out /* B */) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long v0 = voff[b], nv = voff[b + 1] - v0;
  double pl[6];
  int st = plan_ref_plane(lm, ref_planes, hstatus, b, pl);
  double hz = 0.0, tz = 0.0;
  int hv = -1, tv = -1;
  if (st == 0) {      // (uniform) a failed humerus has no slab
    const int tiles = (int)((nv + SH_PLAN_TILE - 1) / SH_PLAN_TILE);      // <= tstride
    for (int t = lane; t < tiles; t += 64) {
      const PlanTop h = slab[((size_t)b * tstride + t) * 2], u = slab[((size_t)b * tstride + t) * 2 + 1];
      if (h.vid >= 0 && plan_ref_better(h.z, h.vid, hz, hv)) { hz = h.z; hv = h.vid; }
      if (u.vid >= 0 && plan_ref_better(u.z, u.vid, tz, tv)) { tz = u.z; tv = u.vid; }
    }
    plan_top_tree(&hz, &hv);
    plan_top_tree(&tz, &tv);
  }
  if (lane != 0) return;
  if (st == 0 && (hv < 0 || tv < 0)) st = SH_ERR_GEOMETRY_DEV;
  sh_plan_ref* r = out + b;
  const bool ok = st == 0;
  const float* vh = verts + 3 * (v0 + (ok ? hv : 0));      // (read only when ok: hv, tv < nv)
  const float* vt = verts + 3 * (v0 + (ok ? tv : 0));
#pragma unroll
  for (int i = 0; i < 3; ++i) { r->tuberosity_top[i] = ok ? (double)vt[i] : 0.0; r->head_apex[i] = ok ? (double)vh[i] : 0.0; }
  r->tuberosity_z = ok ? tz : 0.0; r->head_apex_z = ok ? hz : 0.0; r->head_height = ok ? hz - tz : 0.0;
  r->n_feasible = 0;
  r->tuberosity_vid = ok ? tv : -1; r->head_apex_vid = ok ? hv : -1; r->status = st; r->pad = 0;
}

__global__ void __launch_bounds__(SH_PLAN_TERM_THREADS)
k_plan_terms(const double* __restrict__ planes /* B x P x 6 */, const int* __restrict__ cut_status /* B x P */, const sh_resection* __restrict__ recs /* B x P */,
             const sh_head_fit* __restrict__ fits /* B x P */, const sh_seat* __restrict__ seats /* B x P x Kh */, const sh_implant_head* __restrict__ heads, int Kh,
             const sh_stem_fit* __restrict__ stems /* B x P x Ks */, int Ks, const double* __restrict__ frames /* B x 16 */, const sh_plan_ref* __restrict__ refs /* B */,
             sh_plan_rule rule, int P, PlanTerm* __restrict__ cut_terms /* B x P */, PlanTerm* __restrict__ head_terms /* B x P x Kh */,
             PlanTerm* __restrict__ stem_terms /* B x P x Ks */, double* __restrict__ cut_vals /* B x P */, double* __restrict__ head_vals /* B x P x Kh x 8 */,
             double* __restrict__ stem_vals /* B x P x Ks */) {
  const int cut = blockIdx.x, b = cut / P, tid = threadIdx.x;
  if (tid < 64) {
    const int k = tid;
    if (k >= Kh) return;
    const sh_seat* s = seats + (size_t)cut * Kh + k;
    const double* T = frames + 16 * (size_t)b;
    const double* pl = planes + 6 * (size_t)cut;
    const double sc[3] = {s->seat_center[0], s->seat_center[1], s->seat_center[2]};
    const double cs[3] = {s->cor_shift[0], s->cor_shift[1], s->cor_shift[2]};
    const double n[3] = {pl[3], pl[4], pl[5]};
    const int seat_status = s->status;
    double vals[8];
    const PlanTerm ht = plan_head_term(rule.w_uncovered, rule.w_overhang, rule.w_cor, rule.w_height, rule.max_overhang, rule.min_coverage, s->coverage,
                                       s->max_overhang, cs, sc, n, heads[k].thickness, T, refs[b].head_apex_z, vals);
    head_terms[(size_t)cut * Kh + k] = ht;
    double* hv = head_vals + 8 * ((size_t)cut * Kh + k);
#pragma unroll
    for (int i = 0; i < 8; ++i) hv[i] = vals[i];
    if (k == 0) {      // the cut part, from the seat record this lane holds
      int cst = cut_status[cut];
      if (cst == 0) cst = recs[cut].status;
      double ecc;
      cut_terms[cut] = plan_cut_term(rule.w_eccentricity, rule.max_eccentricity, rule.w_cor, refs[b].status, cst, recs[cut].n_loops, seat_status,
                                     fits[cut].sphere_status, sc, T, pl, n, &ecc);
      cut_vals[cut] = ecc;
    }
  } else {
    const int k = tid - 64;
    if (k >= Ks) return;
    const sh_stem_fit* f = stems + (size_t)cut * Ks + k;
    double fill;
    stem_terms[(size_t)cut * Ks + k] = plan_stem_term(rule.w_fill, rule.fill_target, rule.min_clearance, f->status, f->fits, f->min_clearance, f->fill_mean, &fill);
    stem_vals[(size_t)cut * Ks + k] = fill;
  }
}

// a slot without a plan: indices -1, the status, zeros
__device__ inline void plan_write_none(sh_plan* r, int status) {
  r->cost = 0.0; r->uncovered = 0.0; r->overhang = 0.0; r->cor = 0.0; r->height = 0.0; r->eccentricity = 0.0; r->fill = 0.0;
  r->apex[0] = 0.0; r->apex[1] = 0.0; r->apex[2] = 0.0; r->apex_z = 0.0; r->head_height = 0.0;
  r->cut = -1; r->head = -1; r->stem = -1; r->status = status;
}

__global__ void __launch_bounds__(SH_PLAN_THREADS)
k_plan_select(const PlanTerm* __restrict__ cut_terms, const PlanTerm* __restrict__ head_terms, const PlanTerm* __restrict__ stem_terms,
              const double* __restrict__ cut_vals, const double* __restrict__ head_vals, const double* __restrict__ stem_vals,
              const unsigned long long* __restrict__ compat /* Kh words */, int P, int Kh, int Ks, int N, sh_plan_ref* __restrict__ refs /* B */,
              sh_plan* __restrict__ out /* B x N */) {
  __shared__ double s_c[SH_PLAN_THREADS / 64];
  __shared__ int s_i[SH_PLAN_THREADS / 64];
  __shared__ long long s_n[SH_PLAN_THREADS / 64];
  __shared__ double w_c;
  __shared__ int w_i;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  sh_plan* const dst = out + (size_t)b * N;
  const int hst = refs[b].status;
  if (hst != 0) {      // (uniform) every plan carries the humerus' status; n_feasible stays 0
    if (tid < N) plan_write_none(dst + tid, hst);
    return;
  }
  const double tub_z = refs[b].tuberosity_z;
  const int total = (P * Kh) * Ks;      // <= 4 096 x 64 x 64 = 2^24
  const PlanTerm* ct = cut_terms + (size_t)b * P;
  const PlanTerm* ht = head_terms + (size_t)b * P * Kh;
  const PlanTerm* st = stem_terms + (size_t)b * P * Ks;
  double prev_c = 0.0;
  int prev_i = -1, r = 0;
  for (; r < N; ++r) {
    double best_c = 0.0;
    int best_i = -1;
    long long cnt = 0;
    for (int i = tid; i < total; i += SH_PLAN_THREADS) {
      const int q = i / Ks, ks = i - q * Ks, p = q / Kh, kh = q - p * Kh;      // q = p Kh + kh
      double cost;
      if (!plan_candidate(ct[p], ht[q], st[(size_t)p * Ks + ks], compat[kh], ks, &cost)) continue;
      ++cnt;
      if (r > 0 && !plan_key_less(prev_c, prev_i, cost, i)) continue;
      if (best_i < 0 || plan_key_less(cost, i, best_c, best_i)) { best_c = cost; best_i = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double oc = __shfl_down(best_c, off);
      const int oi = __shfl_down(best_i, off);
      if (oi >= 0 && (best_i < 0 || plan_key_less(oc, oi, best_c, best_i))) { best_c = oc; best_i = oi; }
      cnt += __shfl_down(cnt, off);
    }
    if (lane == 0) { s_c[wave] = best_c; s_i[wave] = best_i; s_n[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
      double c = s_c[0];
      int i = s_i[0];
      long long n = s_n[0];
      for (int w = 1; w < SH_PLAN_THREADS / 64; ++w) {
        if (s_i[w] >= 0 && (i < 0 || plan_key_less(s_c[w], s_i[w], c, i))) { c = s_c[w]; i = s_i[w]; }
        n += s_n[w];
      }
      w_c = c; w_i = i;
      if (r == 0) refs[b].n_feasible = n;
      if (i >= 0) {      // the round's plan, field by field
        const int q = i / Ks, ks = i - q * Ks, p = q / Kh, kh = q - p * Kh;
        const double* hv = head_vals + 8 * ((size_t)b * P * Kh + q);
        sh_plan* o = dst + r;
        o->cost = c; o->uncovered = hv[0]; o->overhang = hv[1]; o->cor = hv[2]; o->height = hv[3];
        o->eccentricity = cut_vals[(size_t)b * P + p]; o->fill = stem_vals[((size_t)b * P + p) * Ks + ks];
        o->apex[0] = hv[4]; o->apex[1] = hv[5]; o->apex[2] = hv[6]; o->apex_z = hv[7]; o->head_height = hv[7] - tub_z;
        o->cut = p; o->head = kh; o->stem = ks; o->status = 0;
      }
    }
    __syncthreads();
    prev_c = w_c; prev_i = w_i;
    if (prev_i < 0) break;      // (uniform) no candidate is left
  }
  if (tid < N - r) plan_write_none(dst + r + tid, SH_ERR_GEOMETRY_DEV);      // the slots beyond n_feasible
}

}  // namespace sh
