// Test shim (NOT product): the implant-plan arithmetic of shoulder_amd/csrc/sh_scalar.h (plan_side, plan_tuberosity_bound,
// plan_ref_better, plan_cut_term, plan_head_term, plan_stem_term, plan_candidate, plan_key_less -- the source k_plan.h runs on the
// device) on the host, for tests/test_plan_host.py.  pc_ref walks the vertices as k_plan_ref / k_plan_ref_join do (tiles of 256, four
// waves of 64 lanes, the shuffle tree where lane l takes lane l + off for off = 32, 16, ..., 1, the waves in order, then the tiles
// lane-strided and the tree again); pc_select runs k_plan_select's rounds with 256 lanes striding the candidates.  Its own main()
// runs all of it on a small prism and a small catalogue, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

namespace {
struct Top { double z; int vid; };
// one wave's tree: a lane beyond the wave keeps its own value, as __shfl_down does
template <typename Better>
void tree64(Top* w, Better better) {
  for (int off = 32; off > 0; off >>= 1) {
    Top old[64];
    memcpy(old, w, sizeof old);
    for (int l = 0; l < 64; ++l) {
      const Top o = old[l + off < 64 ? l + off : l];
      if (better(o, w[l])) w[l] = o;
    }
  }
}
bool top_better(const Top& o, const Top& m) { return o.vid >= 0 && sh::plan_ref_better(o.z, o.vid, m.z, m.vid); }
struct Key { double c; int i; };
bool key_better(const Key& o, const Key& m) { return o.i >= 0 && (m.i < 0 || sh::plan_key_less(o.c, o.i, m.c, m.i)); }
void key_tree64(Key* w) {
  for (int off = 32; off > 0; off >>= 1) {
    Key old[64];
    memcpy(old, w, sizeof old);
    for (int l = 0; l < 64; ++l) {
      const Key o = old[l + off < 64 ? l + off : l];
      if (key_better(o, w[l])) w[l] = o;
    }
  }
}
void plan_none(sh_plan* r, int status) {
  memset(r, 0, sizeof *r);
  r->cut = r->head = r->stem = -1; r->status = status;
}
}  // namespace

extern "C" void pc_ref(const float* verts, int nv, const double* T, const double* plane /* 6 */, double margin, int status, sh_plan_ref* out) {
  const int tiles = (nv + 255) / 256;
  std::vector<Top> slab(2 * (size_t)(tiles > 0 ? tiles : 1), Top{0.0, -1});
  const double bound = sh::plan_tuberosity_bound(margin, plane + 3);
  for (int t = 0; t < tiles && status == 0; ++t) {
    Top w[2][4][64];
    for (int tid = 0; tid < 256; ++tid) {
      Top h = {0.0, -1}, u = {0.0, -1};
      const int vi = t * 256 + tid;
      if (vi < nv) {
        const double x = (double)verts[3 * vi], y = (double)verts[3 * vi + 1], z = (double)verts[3 * vi + 2];
        const double s = sh::plan_side(plane, plane + 3, x, y, z);
        double q[3];
        sh::canal_map_point(T, x, y, z, q);
        if (s > 0.0) h = Top{q[2], vi};
        if (s <= bound) u = Top{q[2], vi};
      }
      w[0][tid >> 6][tid & 63] = h; w[1][tid >> 6][tid & 63] = u;
    }
    for (int side = 0; side < 2; ++side) {
      for (int wv = 0; wv < 4; ++wv) tree64(w[side][wv], top_better);
      Top m = w[side][0][0];
      for (int wv = 1; wv < 4; ++wv)
        if (top_better(w[side][wv][0], m)) m = w[side][wv][0];
      slab[2 * (size_t)t + side] = m;
    }
  }
  Top best[2] = {{0.0, -1}, {0.0, -1}};
  if (status == 0)
    for (int side = 0; side < 2; ++side) {
      Top w[64];
      for (int l = 0; l < 64; ++l) {
        w[l] = Top{0.0, -1};
        for (int t = l; t < tiles; t += 64)
          if (top_better(slab[2 * (size_t)t + side], w[l])) w[l] = slab[2 * (size_t)t + side];
      }
      tree64(w, top_better);
      best[side] = w[0];
    }
  if (status == 0 && (best[0].vid < 0 || best[1].vid < 0)) status = SH_ERR_GEOMETRY;
  memset(out, 0, sizeof *out);
  out->status = status; out->tuberosity_vid = -1; out->head_apex_vid = -1;
  if (status != 0) return;
  for (int i = 0; i < 3; ++i) { out->head_apex[i] = (double)verts[3 * best[0].vid + i]; out->tuberosity_top[i] = (double)verts[3 * best[1].vid + i]; }
  out->head_apex_z = best[0].z; out->tuberosity_z = best[1].z; out->head_height = best[0].z - best[1].z;
  out->head_apex_vid = best[0].vid; out->tuberosity_vid = best[1].vid;
}

extern "C" void pc_cut_term(const sh_plan_rule* r, int humerus_status, int cut_status, int n_loops, int seat0_status, int sphere_status,
                            const double* seat_center, const double* T, const double* plane /* 6 */, double* out /* cost, feasible, ecc */) {
  double ecc;
  const sh::PlanTerm t = sh::plan_cut_term(r->w_eccentricity, r->max_eccentricity, r->w_cor, humerus_status, cut_status, n_loops, seat0_status, sphere_status,
                                           seat_center, T, plane, plane + 3, &ecc);
  out[0] = t.cost; out[1] = (double)t.feasible; out[2] = ecc;
}
extern "C" void pc_head_term(const sh_plan_rule* r, double coverage, double max_overhang, const double* cor_shift, const double* seat_center, const double* n,
                             double h, const double* T, double head_apex_z, double* vals /* 8 */, double* out /* cost, feasible */) {
  const sh::PlanTerm t = sh::plan_head_term(r->w_uncovered, r->w_overhang, r->w_cor, r->w_height, r->max_overhang, r->min_coverage, coverage, max_overhang,
                                            cor_shift, seat_center, n, h, T, head_apex_z, vals);
  out[0] = t.cost; out[1] = (double)t.feasible;
}
extern "C" void pc_stem_term(const sh_plan_rule* r, int status, int fits, double min_clearance, double fill_mean, double* out /* cost, feasible, fill */) {
  double fill;
  const sh::PlanTerm t = sh::plan_stem_term(r->w_fill, r->fill_target, r->min_clearance, status, fits, min_clearance, fill_mean, &fill);
  out[0] = t.cost; out[1] = (double)t.feasible; out[2] = fill;
}
extern "C" int pc_candidate(const sh::PlanTerm* cut, const sh::PlanTerm* head, const sh::PlanTerm* stem, unsigned long long word, int ks, double* cost) {
  return sh::plan_candidate(*cut, *head, *stem, word, ks, cost) ? 1 : 0;
}

// k_plan_select for one humerus: the arrays are the humerus' own (P, P x Kh, P x Ks); ref->status and ref->tuberosity_z are read,
// ref->n_feasible is written
extern "C" void pc_select(const sh::PlanTerm* ct, const sh::PlanTerm* ht, const sh::PlanTerm* st, const double* cut_vals, const double* head_vals /* x 8 */,
                          const double* stem_vals, const unsigned long long* compat, int P, int Kh, int Ks, int N, sh_plan_ref* ref, sh_plan* out) {
  if (ref->status != 0) {
    for (int r = 0; r < N; ++r) plan_none(out + r, ref->status);
    return;
  }
  const int total = (P * Kh) * Ks;
  Key prev = {0.0, -1};
  int r = 0;
  for (; r < N; ++r) {
    Key w[4][64];
    long long cnt = 0;
    for (int tid = 0; tid < 256; ++tid) {
      Key best = {0.0, -1};
      for (int i = tid; i < total; i += 256) {
        const int q = i / Ks, ks = i - q * Ks, p = q / Kh, kh = q - p * Kh;
        double cost;
        if (!sh::plan_candidate(ct[p], ht[q], st[(size_t)p * Ks + ks], compat[kh], ks, &cost)) continue;
        ++cnt;
        if (r > 0 && !sh::plan_key_less(prev.c, prev.i, cost, i)) continue;
        if (best.i < 0 || sh::plan_key_less(cost, i, best.c, best.i)) best = Key{cost, i};
      }
      w[tid >> 6][tid & 63] = best;
    }
    for (int wv = 0; wv < 4; ++wv) key_tree64(w[wv]);
    Key m = w[0][0];
    for (int wv = 1; wv < 4; ++wv)
      if (key_better(w[wv][0], m)) m = w[wv][0];
    if (r == 0) ref->n_feasible = cnt;
    prev = m;
    if (m.i < 0) break;
    const int q = m.i / Ks, ks = m.i - q * Ks, p = q / Kh, kh = q - p * Kh;
    const double* hv = head_vals + 8 * (size_t)q;
    sh_plan* o = out + r;
    o->cost = m.c; o->uncovered = hv[0]; o->overhang = hv[1]; o->cor = hv[2]; o->height = hv[3];
    o->eccentricity = cut_vals[p]; o->fill = stem_vals[(size_t)p * Ks + ks];
    o->apex[0] = hv[4]; o->apex[1] = hv[5]; o->apex[2] = hv[6]; o->apex_z = hv[7]; o->head_height = hv[7] - ref->tuberosity_z;
    o->cut = p; o->head = kh; o->stem = ks; o->status = 0;
  }
  for (; r < N; ++r) plan_none(out + r, SH_ERR_GEOMETRY);
}

// stand-alone run (sanitizer build): a prism's reference, the three parts of a few candidates, a selection with ties
int main() {
  const int n = 300;      // two tiles
  std::vector<float> v(3 * (size_t)(2 * n));
  for (int i = 0; i < n; ++i) {
    const double t = 0.01 + 6.283185307179586 * i / n;
    for (int k = 0; k < 2; ++k) { v[3 * (k * n + i)] = (float)(5.0 * cos(t)); v[3 * (k * n + i) + 1] = (float)(5.0 * sin(t)); v[3 * (k * n + i) + 2] = k ? 6.0f : -4.0f; }
  }
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double plane[6] = {0, 0, 0, 1, 0, 0.5};
  sh_plan_ref ref;
  pc_ref(v.data(), 2 * n, T, plane, 0.5, 0, &ref);
  if (ref.status != 0 || ref.head_apex_vid < n || ref.tuberosity_vid < n) { printf("plan_check: reference %d %d %d\n", ref.status, ref.head_apex_vid, ref.tuberosity_vid); return 1; }
  pc_ref(v.data(), 2 * n, T, plane, 1e9, 0, &ref);
  if (ref.status != SH_ERR_GEOMETRY) { printf("plan_check: margin\n"); return 1; }
  pc_ref(v.data(), 0, T, plane, 0.0, 0, &ref);
  if (ref.status != SH_ERR_GEOMETRY) { printf("plan_check: empty mesh\n"); return 1; }
  ref.status = 0; ref.tuberosity_z = 1.0;
  sh_plan_rule rule = {INFINITY, -INFINITY, -INFINITY, INFINITY, 0.8, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
  const double sc[3] = {3.0, 4.0, 2.0}, cs[3] = {1.0, 2.0, 2.0}, cut_plane[6] = {0, 0, 2.0, 0, 0, 2.0};
  double out3[3], vals[8];
  pc_cut_term(&rule, 0, 0, 1, 0, 0, sc, T, cut_plane, out3);
  if (out3[2] != 5.0 || out3[1] != 1.0) { printf("plan_check: eccentricity %g\n", out3[2]); return 1; }
  pc_head_term(&rule, 0.75, 1.5, cs, sc, cut_plane + 3, 18.0, T, 20.0, vals, out3);
  if (vals[7] != 20.0 || vals[3] != 0.0 || vals[2] != 3.0) { printf("plan_check: head term\n"); return 1; }
  pc_stem_term(&rule, 0, 1, 0.5, 0.7, out3);
  const int P = 3, Kh = 5, Ks = 7, N = 64;
  std::vector<sh::PlanTerm> ct(P), ht(P * Kh), st(P * Ks);
  std::vector<double> cv(P, 0.0), hv(8 * (size_t)P * Kh, 0.0), sv((size_t)P * Ks, 0.0);
  for (int i = 0; i < P; ++i) ct[i] = sh::PlanTerm{(double)(i % 2), 1, 0};
  for (int i = 0; i < P * Kh; ++i) ht[i] = sh::PlanTerm{(double)(i % 3), i % 4 != 0, 0};
  for (int i = 0; i < P * Ks; ++i) st[i] = sh::PlanTerm{(double)(i % 2), 1, 0};
  unsigned long long compat[64];
  for (int k = 0; k < 64; ++k) compat[k] = ~0ull;
  compat[1] = 0;
  std::vector<sh_plan> plans(N);
  pc_select(ct.data(), ht.data(), st.data(), cv.data(), hv.data(), sv.data(), compat, P, Kh, Ks, N, &ref, plans.data());
  long long got = 0;
  for (int r = 0; r < N; ++r) {
    if (plans[r].status != 0) continue;
    ++got;
    if (r > 0 && plans[r].cost < plans[r - 1].cost) { printf("plan_check: order\n"); return 1; }
  }
  if (got != (ref.n_feasible < N ? ref.n_feasible : N)) { printf("plan_check: count %lld %lld\n", got, (long long)ref.n_feasible); return 1; }
  printf("plan_check: ok (n_feasible %lld)\n", (long long)ref.n_feasible);
  return 0;
}
