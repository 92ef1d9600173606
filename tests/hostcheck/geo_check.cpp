// Test shim (NOT product): the geodesic rules of shoulder_amd/csrc/sh_scalar.h (geo_face, geo_relax, geo_pred, geo_far -- the source
// k_geo.h runs on the device) and, of sh_query.h, the argument checks of sh_geodesic and its buffer plan, on the host, for
// tests/test_geo_host.py.  gc_geodesic makes the buffers of one mesh as the kernels do: the face records and the vertices across the
// slots, the seeded plane, the relaxation in either of the device's two schedules (lds: every read of a round in front of every write,
// in ONE array and in the kernel's two parts, as k_geo_lds -- which also skips a vertex none of whose neighbours fell, and so changes
// no value; otherwise all vertices at once, as the two planes of k_geo_round), the roots, the predecessors, the pointer jumping in place
// and the info records.  Its own main() builds the incidence and the adjacency of a box, two boxes, a fan and a box with a twin vertex with the
// topo_* rules and walks them and the checks, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(SH_GEO_UNFOLD == SH_GEOD_UNFOLD && SH_GEO_ROOT == SH_GEOD_ROOT && SH_GEO_NO_PRED == SH_GEOD_NO_PRED && SH_GEO_UNREACHED == SH_GEOD_UNREACHED &&
              SH_GEO_INFO_BYTES == sizeof(sh::GeoInfo) && sh::AR_GEO_FACE == SH_GEOD_FACE, "the constants of sh_geodesic");

// -> 0, or SH_ERR_INTERNAL when a relaxation goes past nv + 1 rounds
extern "C" int gc_geodesic(const float* verts, int nv, const int* faces, int nf, const int32_t* vrow /* nv + 1 */, const int32_t* vface /* 3 nf */,
                           const int32_t* adj /* 3 nf */, int mode, int K, double max_dist, const int32_t* src_off /* K + 1 */, const int32_t* src, const double* d0,
                           int lds, double* frec /* 6 nf */, double* dist /* K nv */, int32_t* pred /* K nv */, int32_t* source /* K nv */, sh::GeoInfo* info /* K */) {
  // k_geo_face
  std::vector<int32_t> opp(3 * (size_t)nf + 1, -1);
  for (int f = 0; f < nf; ++f) sh::geo_face(verts, faces, adj, f, sh::topo_degenerate(faces + 3 * (size_t)f, nv), frec + SH_GEOD_FACE * (size_t)f, opp.data() + 3 * (size_t)f);
  std::vector<double> other((size_t)nv + 1), fresh((size_t)nv + 1);
  std::vector<int32_t> jump((size_t)nv + 1);
  for (int k = 0; k < K; ++k) {
    double* d = dist + (size_t)k * nv;
    int32_t *pr = pred + (size_t)k * nv, *so = source + (size_t)k * nv;
    // k_geo_init, k_geo_seed
    for (int v = 0; v < nv; ++v) { d[v] = sh::geo_inf(); so[v] = SH_GEOD_NO_LABEL; }
    for (int i = src_off[k]; i < src_off[k + 1]; ++i) {
      const double z = d0[i] + 0.0;
      if (z <= max_dist && z < d[src[i]]) d[src[i]] = z;
    }
    // k_geo_lds / k_geo_round
    int sweeps = 0;
    for (bool fell = true; fell;) {
      if (sweeps > nv) return SH_ERR_INTERNAL;
      fell = false;
      double* out = lds ? fresh.data() : other.data();
      const int part = lds ? 10 * 1024 : nv;      // k_geo_lds relaxes the vertices [0, 10 240) and [10 240, 20 000) one after the other
      for (int v0 = 0; v0 < nv; v0 += part) {
        const int v1 = v0 + part < nv ? v0 + part : nv;
        for (int v = v0; v < v1; ++v) out[v] = sh::geo_relax(faces, frec, opp.data(), vface + vrow[v], vrow[v + 1] - vrow[v], v, mode, max_dist, d[v], d);
        for (int v = v0; v < v1; ++v) {
          if (out[v] < d[v]) fell = true;
          if (lds ? out[v] < d[v] : true) d[v] = out[v];
        }
      }
      ++sweeps;
    }
    // k_geo_root, k_geo_pred
    for (int i = src_off[k]; i < src_off[k + 1]; ++i)
      if (d0[i] + 0.0 == d[src[i]] && i - src_off[k] < so[src[i]]) so[src[i]] = i - src_off[k];
    for (int v = 0; v < nv; ++v) {
      jump[v] = v;
      if (!(d[v] < sh::geo_inf())) { pr[v] = SH_GEOD_UNREACHED; so[v] = -1; continue; }
      if (so[v] != SH_GEOD_NO_LABEL) { pr[v] = SH_GEOD_ROOT; continue; }
      pr[v] = sh::geo_pred(faces, frec, opp.data(), vface + vrow[v], vrow[v + 1] - vrow[v], v, mode, d);
      so[v] = -1;
      if (pr[v] >= 0) jump[v] = pr[v];
    }
    // k_geo_jump, as many rounds as the plan says; k_geo_info
    const sh::GeoPlan plan = sh::geo_plan(1, K, src_off[K], SH_GEO_LDS_VERTICES, nv, nf, nv, nf);
    for (int r = 0; r < plan.jumps; ++r)
      for (int v = 0; v < nv; ++v) jump[v] = jump[jump[v]];
    sh::GeoInfo g = {0.0, 0, 0, 0, -1, sweeps, 0};
    for (int v = 0; v < nv; ++v) {
      if (pr[v] == SH_GEOD_UNREACHED) continue;
      ++g.reached;
      g.roots += pr[v] == SH_GEOD_ROOT;
      g.no_pred += pr[v] == SH_GEOD_NO_PRED;
      sh::geo_far(d[v], v, &g.far_dist, &g.farthest);
      if (pr[v] >= 0) so[v] = pr[jump[v]] == SH_GEOD_ROOT ? so[jump[v]] : -1;
    }
    if (g.farthest < 0) g.far_dist = 0.0;
    info[k] = g;
  }
  return 0;
}

// precheck_geodesic; the refusal's text to `text`.  voff: B + 1 vertex offsets (null: no resident batch to read the lists against)
extern "C" int gc_precheck(int ctx, int mode, int K, double max_dist, int has_off, int has_src, const int32_t* src_off, const int32_t* src, const double* d0,
                           const long long* voff, int incidence, int B, int n_pending, char* text, int cap) {
  const sh::ArthroState st;
  const sh::ArthroError e = sh::precheck_geodesic(mode, K, max_dist, has_off ? src_off : nullptr, has_src ? src : nullptr, d0, voff, incidence != 0,
                                                  sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: face blocks, vertex blocks, jumps, general, rounds_max, then the eleven sizes of GEO_BUFS
extern "C" void gc_plan(int B, int K, long long S, long long lds_vertices, long long maxV, long long maxF, long long sumV, long long sumF, size_t* out) {
  const sh::GeoPlan p = sh::geo_plan(B, K, S, (int)lds_vertices, maxV, maxF, sumV, sumF);
  size_t* o = out;
  *o++ = (size_t)p.fblocks; *o++ = (size_t)p.vblocks; *o++ = (size_t)p.jumps; *o++ = p.general ? 1 : 0; *o++ = (size_t)p.rounds_max;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  GEO_BUFS(X)
#undef X
}

// ---- stand-alone run (sanitizer build) ----
struct Result {
  std::vector<double> face, dist;
  std::vector<int32_t> pred, source;
  std::vector<sh::GeoInfo> info;
  int rc;
};
// the incidence in ascending order and the adjacency by the topo_* rules, then gc_geodesic with one set per entry of `sets`
static Result run(const std::vector<float>& v, const std::vector<int>& f, int mode, const std::vector<std::vector<int>>& sets, double max_dist, int lds) {
  const int nv = (int)v.size() / 3, nf = (int)f.size() / 3, K = (int)sets.size();
  std::vector<int32_t> vrow((size_t)nv + 1, 0), vface(3 * (size_t)nf + 1, -1), adj(3 * (size_t)nf + 1, SH_TOPO_DEGENERATE);
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) ++vrow[f[3 * (size_t)i + k] + 1];
  for (int i = 0; i < nv; ++i) vrow[i + 1] += vrow[i];
  std::vector<int> cur(vrow.begin(), vrow.end());
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) vface[cur[f[3 * (size_t)i + k]]++] = i;
  for (int i = 0; i < nf; ++i) {
    if (sh::topo_degenerate(&f[3 * (size_t)i], nv)) continue;
    for (int e = 0; e < 3; ++e) {
      const int a = f[3 * (size_t)i + e];
      int owner, same;
      adj[3 * (size_t)i + e] = sh::topo_slot(f.data(), vface.data() + vrow[a], vrow[a + 1] - vrow[a], i, e, &owner, &same);
    }
  }
  std::vector<int32_t> off(1, 0), src;
  for (const auto& s : sets) { src.insert(src.end(), s.begin(), s.end()); off.push_back((int32_t)src.size()); }
  std::vector<double> d0(src.size() + 1, 0.0);
  src.push_back(0);
  Result r;
  r.face.resize(SH_GEOD_FACE * (size_t)nf + 1); r.dist.resize((size_t)K * nv + 1); r.pred.resize((size_t)K * nv + 1); r.source.resize((size_t)K * nv + 1); r.info.resize((size_t)K);
  r.rc = gc_geodesic(v.data(), nv, f.data(), nf, vrow.data(), vface.data(), adj.data(), mode, K, max_dist, off.data(), src.data(), d0.data(), lds, r.face.data(), r.dist.data(),
                     r.pred.data(), r.source.data(), r.info.data());
  return r;
}
static bool same(const Result& a, const Result& b) {
  return a.rc == b.rc && a.pred == b.pred && a.source == b.source && memcmp(a.dist.data(), b.dist.data(), a.dist.size() * 8) == 0 && memcmp(a.face.data(), b.face.data(), a.face.size() * 8) == 0;
}

int main() {
  const double inf = sh::geo_inf();
  std::vector<float> bv(24);
  const std::vector<int> bf = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  // the 30 x 20 x 10 box from corner 0: along the edges the far corner is 60 away, over the unfolded faces sqrt(30^2 + 30^2) = 42.43 at best;
  // both schedules give the same bytes
  for (int mode = 0; mode < 2; ++mode) {
    const Result a = run(bv, bf, mode, {{0}, {0, 7}, {}}, inf, 1), b = run(bv, bf, mode, {{0}, {0, 7}, {}}, inf, 0);
    if (a.rc != 0 || !same(a, b)) { printf("geo_check: box, mode %d: the two schedules differ\n", mode); return 1; }
    const sh::GeoInfo& g = a.info[0];
    if (g.reached != 8 || g.roots != 1 || g.no_pred != 0 || g.farthest != 7 || a.pred[0] != SH_GEO_ROOT || a.source[7] != 0 || a.dist[0] != 0.0 ||
        (mode == 0 ? g.far_dist != 60.0 : !(g.far_dist > 42.4 && g.far_dist < 46.1))) {
      printf("geo_check: box, mode %d (far %.17g at %d, reached %d)\n", mode, g.far_dist, g.farthest, g.reached); return 1;
    }
    if (a.info[1].roots != 2 || a.source[8 + 7] != 1 || a.pred[8 + 7] != SH_GEO_ROOT || a.info[2].reached != 0 || a.info[2].farthest != -1 || a.info[2].far_dist != 0.0 ||
        a.pred[16] != SH_GEO_UNREACHED || a.source[16] != -1 || a.dist[16] != inf) { printf("geo_check: box, two sources / no source\n"); return 1; }
    for (int v = 1; v < 8; ++v) {      // d falls strictly along pred
      const int u = a.pred[v];
      if (u < 0 || !(a.dist[u] < a.dist[v])) { printf("geo_check: box, pred of %d\n", v); return 1; }
    }
    const Result c = run(bv, bf, mode, {{0}}, 25.0, 1);      // a cut-off: what is kept is the same bytes, the rest +inf
    for (int v = 0; v < 8; ++v)
      if (c.dist[v] != (a.dist[v] <= 25.0 ? a.dist[v] : inf)) { printf("geo_check: box, max_dist at %d\n", v); return 1; }
  }
  // two boxes in one mesh: the second is not reached
  {
    std::vector<float> tv = bv;
    std::vector<int> tf = bf;
    for (int i = 0; i < 24; ++i) tv.push_back(bv[i] + (i % 3 == 0 ? 100.f : 0.f));
    for (int x : bf) tf.push_back(x + 8);
    const Result r = run(tv, tf, 1, {{0}}, inf, 0);
    bool ok = r.rc == 0 && r.info[0].reached == 8;
    for (int v = 8; v < 16; ++v) ok = ok && r.pred[v] == SH_GEO_UNREACHED && r.source[v] == -1 && r.dist[v] == inf;
    if (!ok) { printf("geo_check: two boxes\n"); return 1; }
  }
  // a fan of 300 around vertex 0: one row of 300 faces, from the centre and from the rim
  {
    std::vector<float> av(3 * 302, 0.f);
    std::vector<int> af;
    for (int i = 0; i < 302; ++i) { av[3 * i] = (float)cos(0.02 * i) * (i ? 40.f : 0.f); av[3 * i + 1] = (float)sin(0.02 * i) * (i ? 40.f : 0.f); }
    av[2] = 25.f;
    for (int i = 1; i <= 300; ++i) { af.push_back(0); af.push_back(i); af.push_back(i + 1); }
    const Result a = run(av, af, 1, {{0}, {150}}, inf, 1), b = run(av, af, 1, {{0}, {150}}, inf, 0);
    if (a.rc != 0 || !same(a, b) || a.info[0].reached != 302 || a.info[1].reached != 302 || a.pred[5] != 0 || a.pred[302] < 0) { printf("geo_check: fan\n"); return 1; }
  }
  // vertex 0 a second time as vertex 8 and the face [0, 8, 1]: from 8 its twin is reached over an arc of length 0 and has no predecessor
  {
    std::vector<float> wv = bv;
    std::vector<int> wf = bf;
    for (int c = 0; c < 3; ++c) wv.push_back(bv[c]);
    wf.insert(wf.end(), {0, 8, 1});
    const Result r = run(wv, wf, 1, {{8}}, inf, 1);
    if (r.rc != 0 || r.pred[8] != SH_GEO_ROOT || r.pred[0] != SH_GEO_NO_PRED || r.dist[0] != 0.0 || r.source[0] != -1 || r.info[0].no_pred != 1 || r.info[0].reached != 9) {
      printf("geo_check: twin vertex (pred %d, no_pred %d)\n", r.pred[0], r.info[0].no_pred); return 1;
    }
  }
  // the checks of sh_geodesic in their order, and the plan
  char text[256];
  const long long voff[3] = {0, 8, 20};
  const int32_t off[5] = {0, 1, 1, 3, 4}, src[4] = {7, 0, 11, 3};
  const double d0[4] = {0.0, 1.5, 0.0, 2.0};
  auto pre = [&](int ctx, int mode, int K, double md, const int32_t* s, const double* z, int inc, int B, int pend) {
    return gc_precheck(ctx, mode, K, md, 1, 1, off, s, z, B ? voff : nullptr, inc, B, pend, text, (int)sizeof text);
  };
  int32_t bad_src[4] = {7, 0, 12, 3};
  double bad_d0[4] = {0.0, 1.5, 0.0, -1.0};
  if (pre(1, 1, 2, inf, src, d0, 1, 2, 0) != SH_OK || pre(1, 0, 2, 30.0, src, nullptr, 1, 2, 0) != SH_OK || pre(0, 5, 0, 0.0, src, d0, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "no context") ||
      pre(1, 2, 2, inf, src, d0, 1, 2, 0) != SH_ERR_ARG || !strstr(text, "mode 0 or 1") || pre(1, 1, 0, inf, src, d0, 1, 2, 0) != SH_ERR_ARG || pre(1, 1, 17, inf, src, d0, 1, 2, 0) != SH_ERR_ARG ||
      pre(1, 1, 2, 0.0, src, d0, 1, 2, 0) != SH_ERR_ARG || pre(1, 1, 2, std::nan(""), src, d0, 1, 2, 0) != SH_ERR_ARG || pre(1, 1, 2, inf, bad_src, d0, 0, 2, 1) != SH_ERR_ARG ||
      !strstr(text, "mesh 1, set 0, position 1: source vertex 12 is not in [0, 12)") || pre(1, 1, 2, inf, src, bad_d0, 0, 2, 1) != SH_ERR_ARG ||
      !strstr(text, "mesh 1, set 1, position 0: d0 is not finite and >= 0") || pre(1, 1, 2, inf, src, d0, 0, 0, 0) != SH_ERR_STATE || pre(1, 1, 2, inf, src, d0, 0, 2, 1) != SH_ERR_STATE ||
      !strstr(text, "in flight") || pre(1, 1, 2, inf, src, d0, 0, 2, 0) != SH_ERR_STATE || !strstr(text, "sh_mesh_topology first")) {
    printf("geo_check: precheck_geodesic (%s)\n", text); return 1;
  }
  size_t plan[16];
  gc_plan(3, 2, 5, 20000, 300, 513, 900, 1200, plan);
  const size_t want[16] = {3, 2, 9, 0, 0, 57600, 14400, 7200, 7200, 192, 14400, 0, 7200, 48, 40, 224};
  for (int i = 0; i < 16; ++i)
    if (plan[i] != want[i]) { printf("geo_check: plan[%d] = %zu\n", i, plan[i]); return 1; }
  printf("geo_check: ok\n");
  return 0;
}
