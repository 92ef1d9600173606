// Test shim (NOT product): the smoothing rules of shoulder_amd/csrc/sh_scalar.h (smooth_next, smooth_weight, smooth_border, smooth_mean,
// smooth_step, smooth_hc_b, smooth_hc_p, smooth_scale ... -- the source k_smooth.h runs on the device) and, of sh_query.h, the argument
// checks of sh_smooth_vertices and its buffer plan, on the host, for tests/test_smooth_host.py.  sc_smooth makes the buffers of one mesh
// as the kernels do: count, scan and fill of the rows, the pins, one pass over the vertices per M(.) evaluation on three planes, the two
// volume sums through the tree of 256-face blocks, the scaling, the displacement rows and the info record.  Its own main() builds the
// incidence and the adjacency of a box, an open box, two boxes sharing an edge, a fan and degenerate faces with the topo_* rules and
// walks them and the checks, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(SH_SMOOTH_LAPLACIAN == SH_SMO_LAPLACIAN && SH_SMOOTH_TAUBIN == SH_SMO_TAUBIN && SH_SMOOTH_HC == SH_SMO_HC && SH_SMOOTH_INVLEN == SH_SMO_INVLEN &&
              SH_SMOOTH_PIN_BORDER == SH_SMO_PIN_BORDER && SH_SMOOTH_KEEP_VOLUME == SH_SMO_KEEP_VOLUME && SH_SMOOTH_INFO_BYTES == sizeof(sh::SmoothInfo),
              "the constants of sh_smooth_vertices");

// the tree of one block: 256 slots, the missing ones +0.0
static double tree256(const double* vals, int n, int stride) {
  double slot[SH_MASS_BLOCK];
  for (int i = 0; i < SH_MASS_BLOCK; ++i) slot[i] = i < n ? vals[(size_t)i * stride] : 0.0;
  for (int h = SH_MASS_BLOCK / 2; h >= 1; h >>= 1)
    for (int i = 0; i < h; ++i) slot[i] += slot[i + h];
  return slot[0];
}

// k_smooth_vol and the sums of k_smooth_scale: terms 13 .. 16 of the faces on the corners P about the pivot o
static void volume_sums(const double* P, const int* faces, int nf, const double* o, double* T /* SH_SMO_TERMS */) {
  std::vector<double> t((size_t)(nf > 0 ? nf : 1) * SH_SMO_TERMS, 0.0);
  for (int f = 0; f < nf; ++f) {
    double all[SH_MASS_TERMS];
    const int* fc = faces + 3 * (size_t)f;
    sh::mass_face_terms(o, P + 3 * (size_t)fc[0], P + 3 * (size_t)fc[1], P + 3 * (size_t)fc[2], all);
    for (int j = 0; j < SH_SMO_TERMS; ++j) t[(size_t)f * SH_SMO_TERMS + j] = all[13 + j];
  }
  for (int j = 0; j < SH_SMO_TERMS; ++j) T[j] = 0.0;
  for (int f0 = 0; f0 < nf; f0 += SH_MASS_BLOCK) {
    const int n = nf - f0 < SH_MASS_BLOCK ? nf - f0 : SH_MASS_BLOCK;
    for (int j = 0; j < SH_SMO_TERMS; ++j) T[j] += tree256(&t[(size_t)f0 * SH_SMO_TERMS + j], n, SH_SMO_TERMS);
  }
}

extern "C" void sc_smooth(const float* verts, int nv, const int* faces, int nf, const int32_t* vrow /* nv + 1 */, const int32_t* vface /* 3 nf */,
                          const int32_t* adj /* 3 nf */, int filter, int weight, int iterations, int flags, double p0, double p1, const unsigned char* mask /* nv, nullable */,
                          int32_t* nrow /* nv + 1 */, int32_t* nbr /* 6 nf */, double* w /* 6 nf */, double* pos /* 3 nv */, void* info_out) {
  // k_smooth_count, k_smooth_scan, k_smooth_fill
  int run = 0;
  for (int v = 0; v < nv; ++v) {
    const int32_t* row = vface + vrow[v];
    const int n = vrow[v + 1] - vrow[v];
    nrow[v] = run;
    for (int u = sh::smooth_next(faces, row, n, v, -1); u != SH_TOPO_NONE; u = sh::smooth_next(faces, row, n, v, u)) {
      nbr[run] = u;
      w[run] = sh::smooth_weight(verts, v, u);
      ++run;
    }
  }
  nrow[nv] = run;
  // k_smooth_init
  const size_t n3 = 3 * (size_t)nv;
  std::vector<double> P0(n3 + 1), plane[3];
  std::vector<int> pin((size_t)nv + 1, 0);
  for (auto& p : plane) p.assign(n3 + 1, 0.0);
  for (size_t i = 0; i < n3; ++i) plane[0][i] = P0[i] = (double)verts[i];
  for (int v = 0; v < nv; ++v)
    pin[v] = (mask && mask[v] != 0) || ((flags & SH_SMOOTH_PIN_BORDER) && sh::smooth_border(faces, adj, vface + vrow[v], vrow[v + 1] - vrow[v], v));
  // k_smooth_round, once per M(.) evaluation
  auto round = [&](int mode, double a, const double* x, const double* y, double* out, double* bout) {
    for (int v = 0; v < nv; ++v) {
      double m[3];
      sh::smooth_mean(nbr + nrow[v], w + nrow[v], nrow[v + 1] - nrow[v], weight, pin[v] != 0, x, v, m);
      for (int c = 0; c < 3; ++c) {
        const size_t g = 3 * (size_t)v + c;
        if (mode == 0) out[g] = sh::smooth_step(x[g], m[c], a);
        if (mode == 1) { out[g] = m[c]; bout[g] = pin[v] ? 0.0 : sh::smooth_hc_b(m[c], P0[g], x[g], a); }
        if (mode == 2) out[g] = sh::smooth_hc_p(y[g], x[g], m[c], a);
      }
    }
  };
  int last = 0;
  for (int it = 0; it < iterations; ++it) {
    if (filter == SH_SMOOTH_HC) {
      round(1, p0, plane[0].data(), nullptr, plane[1].data(), plane[2].data());
      round(2, p1, plane[2].data(), plane[1].data(), plane[0].data(), nullptr);
      continue;
    }
    const int per = filter == SH_SMOOTH_TAUBIN ? 2 : 1;
    for (int k = 0; k < per; ++k) {
      const int s = it * per + k;
      round(0, k == 0 ? p0 : p1, plane[s & 1].data(), nullptr, plane[(s + 1) & 1].data(), nullptr);
      last = (s + 1) & 1;
    }
  }
  const double* fin = plane[last].data();
  // k_smooth_vol twice, k_smooth_scale
  sh::SmoothInfo info;
  memset(&info, 0, sizeof info);
  double T0[SH_SMO_TERMS], T1[SH_SMO_TERMS], head[SH_SMO_HEAD], o[3] = {0.0, 0.0, 0.0};
  if (nv > 0) for (int k = 0; k < 3; ++k) o[k] = P0[k];
  volume_sums(P0.data(), faces, nf, o, T0);
  volume_sums(fin, faces, nf, o, T1);
  info.status = sh::smooth_scale(T0, T1, o, (flags & SH_SMOOTH_KEEP_VOLUME) != 0, &info.volume_before, &info.volume_after, head);
  info.scale = head[3];
  // k_smooth_apply, k_smooth_info
  std::vector<double> d2((size_t)nv + 1, 0.0);
  double far = 0.0, sum = 0.0;
  for (int v = 0; v < nv; ++v) {
    double d[3];
    for (int c = 0; c < 3; ++c) {
      const size_t g = 3 * (size_t)v + c;
      pos[g] = head[4] != 0.0 ? sh::smooth_scaled(fin[g], head[c], head[3]) : fin[g];
      d[c] = pos[g] - P0[g];
    }
    d2[v] = sh::dot3(d, d);
    const double x = sh::smooth_disp(d2[v]);
    far = x > far ? x : far;
    info.pinned += pin[v] ? 1 : 0;
    info.isolated += nrow[v + 1] == nrow[v] ? 1 : 0;
  }
  for (int v0 = 0; v0 < nv; v0 += SH_MASS_BLOCK) sum += tree256(&d2[v0], nv - v0 < SH_MASS_BLOCK ? nv - v0 : SH_MASS_BLOCK, 1);
  info.max_disp = far; info.sum_sq_disp = sum;
  memcpy(info_out, &info, sizeof info);
}

extern "C" double sc_cbrt(double r) { return sh::smooth_cbrt(r); }

// precheck_smooth; the refusal's text to `text`
extern "C" int sc_precheck(int ctx, int filter, int weight, int iterations, int flags, double p0, double p1, int has_pin, int incidence, long long maxF, int B, int n_pending,
                           char* text, int cap) {
  const sh::ArthroState st;
  const sh::ArthroError e = sh::precheck_smooth(filter, weight, iterations, flags, p0, p1, has_pin != 0, incidence != 0, maxF, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: face blocks, vertex blocks, steps, last, the offsets vol1, disp and head in doubles, then the nine sizes of SMOOTH_BUFS
extern "C" void sc_plan(int B, int filter, int iterations, long long maxV, long long maxF, long long sumV, long long sumF, size_t* out) {
  const sh::SmoothPlan p = sh::smooth_plan(B, filter, iterations, maxV, maxF, sumV, sumF);
  size_t* o = out;
  *o++ = (size_t)p.fblocks; *o++ = (size_t)p.vblocks; *o++ = (size_t)p.steps; *o++ = (size_t)p.last; *o++ = p.vol1; *o++ = p.disp; *o++ = p.head;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  SMOOTH_BUFS(X)
#undef X
}

// ---- stand-alone run (sanitizer build) ----
struct Result {
  std::vector<int32_t> nrow, nbr;
  std::vector<double> w, pos;
  sh::SmoothInfo info;
};
// the incidence in ascending order and the adjacency by the topo_* rules, then sc_smooth
static Result run(const std::vector<float>& v, const std::vector<int>& f, int filter, int weight, int iterations, int flags, double p0, double p1, const unsigned char* mask = nullptr) {
  const int nv = (int)v.size() / 3, nf = (int)f.size() / 3;
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
  Result r;
  r.nrow.resize((size_t)nv + 1); r.nbr.resize(6 * (size_t)nf + 1); r.w.resize(6 * (size_t)nf + 1); r.pos.resize(3 * (size_t)nv + 1);
  sc_smooth(v.data(), nv, f.data(), nf, vrow.data(), vface.data(), adj.data(), filter, weight, iterations, flags, p0, p1, mask, r.nrow.data(), r.nbr.data(), r.w.data(),
            r.pos.data(), &r.info);
  return r;
}
static bool is_start(const Result& r, const std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i)
    if (r.pos[i] != (double)v[i]) return false;
  return true;
}

int main() {
  std::vector<float> bv(24);
  const std::vector<int> bf = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  // the box: 18 edges, so 36 row entries, ascending; nothing pinned without a border; 0 iterations and lambda 0 give P0
  {
    const Result r = run(bv, bf, SH_SMOOTH_TAUBIN, SH_SMOOTH_INVLEN, 0, SH_SMOOTH_PIN_BORDER, 0.5, -0.53);
    bool asc = r.nrow[8] == 36;
    for (int v = 0; v < 8; ++v)
      for (int i = r.nrow[v]; i + 1 < r.nrow[v + 1]; ++i) asc = asc && r.nbr[i] < r.nbr[i + 1];
    if (!asc || r.info.pinned != 0 || r.info.isolated != 0 || !is_start(r, bv) || r.info.volume_before != 6000.0 || r.info.volume_after != 6000.0 || r.info.scale != 1.0 ||
        r.info.max_disp != 0.0 || r.w[0] != 1.0 / 30.0) {
      printf("smooth_check: box rows (%d entries, %d pinned, volume %.17g)\n", r.nrow[8], r.info.pinned, r.info.volume_before); return 1;
    }
    for (int filter = 0; filter < 2; ++filter)
      if (!is_start(run(bv, bf, filter, SH_SMOOTH_UNIFORM, 5, 0, 0.0, 0.0), bv)) { printf("smooth_check: lambda 0 moves the box\n"); return 1; }
    const unsigned char all[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int filter = 0; filter < 3; ++filter)
      if (!is_start(run(bv, bf, filter, SH_SMOOTH_INVLEN, 4, 0, 0.5, filter == SH_SMOOTH_TAUBIN ? -0.53 : 0.5, all), bv)) { printf("smooth_check: a pinned box moves\n"); return 1; }
  }
  // every filter shrinks the box; with the flag the volume comes back; a box that lost seven eighths has the status
  for (int filter = 0; filter < 3; ++filter) {
    const double p0 = filter == SH_SMOOTH_HC ? 0.1 : 0.2, p1 = filter == SH_SMOOTH_TAUBIN ? -0.21 : 0.5;      // (eight vertices: a second HC iteration leaves less than an eighth)
    const Result a = run(bv, bf, filter, SH_SMOOTH_UNIFORM, 1, 0, p0, p1), k = run(bv, bf, filter, SH_SMOOTH_UNIFORM, 1, SH_SMOOTH_KEEP_VOLUME, p0, p1);
    if (a.info.status != 0 || !(a.info.max_disp > 0.0) || !(a.info.sum_sq_disp > 0.0) || k.info.status != 0 || k.info.volume_after != a.info.volume_after ||
        !(std::fabs((k.info.scale * k.info.scale) * k.info.scale * k.info.volume_after / k.info.volume_before - 1.0) < 1e-14)) {
      printf("smooth_check: box filter %d (disp %.17g scale %.17g)\n", filter, a.info.max_disp, k.info.scale); return 1;
    }
  }
  if (run(bv, bf, SH_SMOOTH_HC, SH_SMOOTH_UNIFORM, 2, SH_SMOOTH_KEEP_VOLUME, 0.1, 0.5).info.status != SH_ERR_GEOMETRY) { printf("smooth_check: a collapsed box is scaled\n"); return 1; }
  // without face 0 and SH_SMOOTH_PIN_BORDER: its three corners are pinned and stay
  {
    const std::vector<int> open(bf.begin() + 3, bf.end());
    const Result r = run(bv, open, SH_SMOOTH_LAPLACIAN, SH_SMOOTH_UNIFORM, 3, SH_SMOOTH_PIN_BORDER, 0.5, 0.0);
    bool stay = r.info.pinned == 3;
    for (int v : {0, 2, 1})
      for (int c = 0; c < 3; ++c) stay = stay && r.pos[3 * v + c] == (double)bv[3 * v + c];
    if (!stay || r.pos[9] == (double)bv[9]) { printf("smooth_check: open box (%d pinned)\n", r.info.pinned); return 1; }
  }
  // two boxes sharing the edge {0, 1}: its ends see each other through four faces, once in the row
  {
    std::vector<float> tv(bv);
    for (int i = 0; i < 8; ++i) { tv.push_back(bv[3 * i] + 100.f); tv.push_back(bv[3 * i + 1]); tv.push_back(bv[3 * i + 2]); }
    std::vector<int> tf(bf);
    for (int x : bf) tf.push_back(x == 0 ? 0 : x == 1 ? 1 : x + 8);
    const Result r = run(tv, tf, SH_SMOOTH_HC, SH_SMOOTH_INVLEN, 2, SH_SMOOTH_PIN_BORDER, 0.1, 0.5);
    int ones = 0;
    for (int i = r.nrow[0]; i < r.nrow[1]; ++i) ones += r.nbr[i] == 1;
    if (ones != 1 || r.info.pinned != 2 || r.info.isolated != 2 || r.nrow[8] != r.nrow[10]) { printf("smooth_check: shared edge (%d, %d pinned, %d isolated)\n", ones, r.info.pinned, r.info.isolated); return 1; }
  }
  // a fan of 300 around vertex 0: one row of 301 neighbours
  {
    std::vector<float> av(3 * 302, 0.f);
    std::vector<int> af;
    for (int i = 0; i < 302; ++i) { av[3 * i] = (float)cos(0.02 * i) * (i ? 40.f : 0.f); av[3 * i + 1] = (float)sin(0.02 * i) * (i ? 40.f : 0.f); }
    av[2] = 25.f;
    for (int i = 1; i <= 300; ++i) { af.push_back(0); af.push_back(i); af.push_back(i + 1); }
    const Result r = run(av, af, SH_SMOOTH_TAUBIN, SH_SMOOTH_INVLEN, 3, 0, 0.5, -0.53);
    if (r.nrow[1] != 301 || r.nbr[0] != 1 || r.nbr[300] != 301 || r.nrow[302] != 301 + 2 + 299 * 3 + 2 || !(r.pos[2] < 25.0)) { printf("smooth_check: fan (%d)\n", r.nrow[1]); return 1; }
  }
  // degenerate faces take no part; a mesh of them alone has empty rows, and with the flag the status
  {
    std::vector<int> df = {0, 0, 1};
    df.insert(df.end(), bf.begin(), bf.end());
    df.insert(df.end(), {5, 7, 5});
    const Result plain = run(bv, bf, SH_SMOOTH_HC, SH_SMOOTH_INVLEN, 2, 0, 0.1, 0.5), r = run(bv, df, SH_SMOOTH_HC, SH_SMOOTH_INVLEN, 2, 0, 0.1, 0.5);
    if (plain.nrow != r.nrow || memcmp(plain.pos.data(), r.pos.data(), 24 * 8) != 0 || memcmp(plain.nbr.data(), r.nbr.data(), 36 * 4) != 0) { printf("smooth_check: degenerate faces take part\n"); return 1; }
    const std::vector<int> only = {0, 1, 1, 2, 2, 3, 4, 5, 4, 6, 6, 6};
    const Result o = run(bv, only, SH_SMOOTH_LAPLACIAN, SH_SMOOTH_UNIFORM, 2, SH_SMOOTH_KEEP_VOLUME, 0.5, 0.0);
    if (o.nrow[8] != 0 || o.info.isolated != 8 || o.info.status != SH_ERR_GEOMETRY || o.info.scale != 1.0 || !is_start(o, bv)) { printf("smooth_check: only degenerate faces\n"); return 1; }
  }
  // ten Newton steps
  for (double r : {0.125, 0.3, 1.0, 2.5, 8.0}) {
    const double s = sc_cbrt(r);
    if (!(std::fabs((s * s) * s / r - 1.0) <= 0x1p-48)) { printf("smooth_check: cube root of %g\n", r); return 1; }
  }
  // the checks of sh_smooth_vertices in their order, and the plan
  char text[256];
  auto pre = [&](int ctx, int filter, int weight, int it, int flags, double p0, double p1, int has_pin, int inc, int B, int pend) {
    return sc_precheck(ctx, filter, weight, it, flags, p0, p1, has_pin, inc, 1000, B, pend, text, (int)sizeof text);
  };
  if (pre(1, 1, 0, 10, 0, 0.5, -0.53, 0, 1, 1, 0) != SH_OK || pre(1, 2, 1, 256, 2, 0.0, 1.0, 0, 1, 1, 0) != SH_OK || pre(0, 9, 0, 0, 0, 0.5, 0.0, 0, 0, 0, 0) != SH_ERR_ARG ||
      !strstr(text, "no context") || pre(1, 3, 0, 0, 0, 0.5, 0.0, 0, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "filter") || pre(1, 0, 2, 0, 0, 0.5, 0.0, 0, 1, 1, 0) != SH_ERR_ARG ||
      pre(1, 0, 0, -1, 0, 0.5, 0.0, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, 0, 257, 0, 0.5, 0.0, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, 0, 1, 4, 0.5, 0.0, 0, 1, 1, 0) != SH_ERR_ARG ||
      pre(1, 0, 0, 1, 0, 1.5, 0.0, 0, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "lambda") || pre(1, 1, 0, 1, 0, 0.5, 0.1, 0, 1, 1, 0) != SH_ERR_ARG || !strstr(text, "mu") ||
      pre(1, 2, 0, 1, 0, -0.1, 0.5, 0, 1, 1, 0) != SH_ERR_ARG || !strstr(text, "alpha") || pre(1, 2, 0, 1, 0, 0.1, 1.5, 0, 1, 1, 0) != SH_ERR_ARG || !strstr(text, "beta") ||
      pre(1, 0, 0, 1, 0, NAN, 0.0, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, 0, 1, 0, 0.5, NAN, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, 0, 1, 3, 0.5, 0.0, 0, 0, 0, 0) != SH_ERR_ARG ||
      !strstr(text, "SH_SMOOTH_KEEP_VOLUME") || pre(1, 0, 0, 1, 2, 0.5, 0.0, 1, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, 0, 1, 0, 0.5, 0.0, 0, 0, 0, 0) != SH_ERR_STATE ||
      pre(1, 0, 0, 1, 0, 0.5, 0.0, 0, 0, 1, 1) != SH_ERR_STATE || !strstr(text, "in flight") || pre(1, 0, 0, 1, 0, 0.5, 0.0, 0, 0, 1, 0) != SH_ERR_STATE ||
      !strstr(text, "sh_mesh_topology first")) {
    printf("smooth_check: precheck_smooth (%s)\n", text); return 1;
  }
  size_t plan[16];
  sc_plan(3, SH_SMOOTH_TAUBIN, 3, 300, 513, 900, 1200, plan);
  const size_t want[16] = {3, 2, 6, 0, 36, 72, 84, 28800, 57600, 21600, 192, 64800, 3600, 900, 864, 3612};
  if (memcmp(plan, want, sizeof want) != 0) { printf("smooth_check: plan\n"); return 1; }
  printf("smooth_check: ok\n");
  return 0;
}
