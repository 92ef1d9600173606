// Test shim (NOT product): the surface-sample arithmetic of shoulder_amd/csrc/sh_scalar.h (samp_word, samp_unit, samp_area2,
// samp_scan_block, samp_search, samp_point, samp_thin_see / samp_thin_verdict -- the source k_sample.h runs on the device) and, of
// sh_query.h, the argument checks of sh_sample_surface and its buffer plan, on the host, for tests/test_sample_host.py.  sc_sample makes
// the records of one mesh as the kernels do: the areas scanned block by block, the bases in block order, a sample from its three words,
// the thinning in Jacobi rounds on two state arrays with a count of the undecided per round.  Its own main() samples a box and
// degenerate meshes, thins a line of points and walks the checks, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(sizeof(sh_sample) == 48 && sizeof(sh_sample_info) == 24 && sizeof(sh_sample_options) == 16, "the records of sh_sample_surface");

extern "C" void sc_words(uint64_t seed, uint64_t n0, int count, uint64_t* out) {
  for (int i = 0; i < count; ++i) out[i] = sh::samp_word(seed, n0 + (uint64_t)i);
}
extern "C" double sc_unit(uint64_t w) { return sh::samp_unit(w); }

// k_samp_thin round after round and k_samp_finish on n points: keep (n), res = kept, rounds, status
extern "C" void sc_thin(const double* pts, int n, double radius, int max_rounds, int32_t* keep, int32_t* res) {
  const double r2 = radius * radius;
  std::vector<int> a((size_t)n, SH_SAMP_UNDECIDED), b((size_t)n, SH_SAMP_UNDECIDED);
  std::vector<int> count((size_t)max_rounds + 1, 0);
  count[0] = n;
  int rounds = max_rounds, full = 1;
  for (int r = 0; r <= max_rounds; ++r) {
    if (count[r] == 0) { rounds = r; full = 0; break; }
    if (r == max_rounds) break;
    const std::vector<int>& in = (r & 1) ? b : a;
    std::vector<int>& nxt = (r & 1) ? a : b;
    for (int j = 0; j < n; ++j) {
      int ns = in[j];
      if (ns == SH_SAMP_UNDECIDED) {
        int flags = 0;
        for (int i = 0; i < j && !(flags & 1); ++i) {
          if (in[i] == SH_SAMP_REMOVED) continue;
          flags = sh::samp_thin_see(flags, in[i], sh::samp_d2(pts + 3 * (size_t)j, pts + 3 * (size_t)i), r2);
        }
        ns = sh::samp_thin_verdict(flags);
      }
      nxt[j] = ns;
      if (ns == SH_SAMP_UNDECIDED) ++count[r + 1];
    }
  }
  const std::vector<int>& fin = (rounds & 1) ? b : a;
  int kept = 0;
  for (int j = 0; j < n; ++j) { keep[j] = fin[j]; kept += fin[j] == SH_SAMP_KEPT ? 1 : 0; }
  res[0] = kept; res[1] = rounds; res[2] = full ? SH_ERR_CAPACITY : 0;
}

// k_samp_scan, k_samp_base, k_samp_draw and the thinning for one mesh; cdf: nf doubles (nullable)
extern "C" void sc_sample(const float* verts, int nv, const int* faces, int nf, int N, uint64_t seed, double radius, int max_rounds, double* cdf_out,
                          sh_sample* out, sh_sample_info* info) {
  (void)nv;
  std::vector<double> cdf((size_t)nf), base;
  auto corner = [&](int f, int j, double* P) { for (int k = 0; k < 3; ++k) P[k] = (double)verts[3 * (size_t)faces[3 * f + j] + k]; };
  for (int f0 = 0; f0 < nf; f0 += SH_SAMPLE_BLOCK) {
    const int n = nf - f0 < SH_SAMPLE_BLOCK ? nf - f0 : SH_SAMPLE_BLOCK;
    for (int i = 0; i < n; ++i) {
      double A[3], B[3], C[3];
      corner(f0 + i, 0, A); corner(f0 + i, 1, B); corner(f0 + i, 2, C);
      cdf[(size_t)f0 + i] = sh::samp_area2(A, B, C);
    }
    sh::samp_scan_block(&cdf[f0], n);
    base.push_back(cdf[(size_t)f0 + n - 1]);
  }
  double run = 0.0;
  for (double& t : base) { const double s = t; t = run; run = run + s; }
  for (int f = 0; f < nf; ++f) cdf[f] = base[(size_t)f / SH_SAMPLE_BLOCK] + cdf[f];
  if (cdf_out) for (int f = 0; f < nf; ++f) cdf_out[f] = cdf[f];
  const bool ok = nf > 0 && run != 0.0 && sh::icp_finite(run), thin = radius > 0.0;
  memset(out, 0, (size_t)N * sizeof(sh_sample));
  memset(info, 0, sizeof *info);
  info->status = ok ? 0 : SH_ERR_GEOMETRY;
  if (!ok) return;
  info->area = run / 2.0; info->kept = thin ? 0 : N;
  for (int j = 0; j < N; ++j) {
    const double target = sh::samp_unit(sh::samp_word(seed, 3ull * (uint64_t)j)) * cdf[(size_t)nf - 1];
    const long long fi = sh::samp_search(cdf.data(), nf, target);
    double A[3], B[3], C[3], rec[5];
    corner((int)fi, 0, A); corner((int)fi, 1, B); corner((int)fi, 2, C);
    sh::samp_point(A, B, C, sh::samp_unit(sh::samp_word(seed, 3ull * (uint64_t)j + 1ull)), sh::samp_unit(sh::samp_word(seed, 3ull * (uint64_t)j + 2ull)), rec);
    sh_sample& r = out[j];
    r.point[0] = rec[0]; r.point[1] = rec[1]; r.point[2] = rec[2]; r.u = rec[3]; r.v = rec[4]; r.face = (int32_t)fi; r.keep = SH_SAMP_KEPT;
  }
  if (!thin) return;
  std::vector<double> pts(3 * (size_t)N);
  std::vector<int32_t> keep((size_t)N);
  for (int j = 0; j < N; ++j) for (int k = 0; k < 3; ++k) pts[3 * (size_t)j + k] = out[j].point[k];
  int32_t res[3];
  sc_thin(pts.data(), N, radius, max_rounds, keep.data(), res);
  for (int j = 0; j < N; ++j) out[j].keep = keep[j];
  info->kept = res[0]; info->rounds = res[1]; info->status = res[2];
}

// precheck_sample; the refusal's text to `text`
extern "C" int sc_precheck(int ctx, int have_seeds, int have_opt, int N, double radius, int max_rounds, int reserved, int B, int n_pending, char* text, int cap) {
  const sh::ArthroState st;
  const uint64_t seeds[1] = {0};
  const sh_sample_options opt = {radius, max_rounds, reserved};
  const sh::ArthroError e = sh::precheck_sample(N, have_seeds ? seeds : nullptr, have_opt ? &opt : nullptr, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: blocks, chunks, thin, stride, then the five sizes of SAMP_BUFS
extern "C" void sc_plan(int B, int N, int thin, long long maxF, long long sumF, size_t* out) {
  const sh::SampPlan p = sh::samp_plan(B, N, thin != 0, maxF, sumF);
  size_t* o = out;
  *o++ = (size_t)p.blocks; *o++ = (size_t)p.chunks; *o++ = (size_t)p.thin; *o++ = (size_t)p.stride;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  SAMP_BUFS(X)
#undef X
}

// stand-alone run (sanitizer build)
int main() {
  uint64_t w[5];
  const uint64_t known[5] = {6457827717110365317ull, 3203168211198807973ull, 9817491932198370423ull, 4593380528125082431ull, 16408922859458223821ull};
  sc_words(1234567, 0, 5, w);
  if (memcmp(w, known, sizeof w) != 0 || sc_unit(~0ull) >= 1.0 || sc_unit(0) != 0.0) { printf("sample_check: words\n"); return 1; }
  // the 30 x 20 x 10 box at integer CT coordinates: area 2200, every sample on a face of the box
  float bv[24];
  const int bf[36] = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  const int N = 300;
  std::vector<sh_sample> out(N);
  std::vector<double> cdf(12);
  sh_sample_info info;
  sc_sample(bv, 8, bf, 12, N, 7, 0.0, 32, cdf.data(), out.data(), &info);
  if (info.status || info.area != 2200.0 || info.kept != N || info.rounds != 0 || cdf[11] != 4400.0) { printf("sample_check: box: status %d area %g\n", info.status, info.area); return 1; }
  for (int j = 0; j < N; ++j) {
    const sh_sample& r = out[j];
    const bool on = r.point[0] == 120.0 || r.point[0] == 150.0 || r.point[1] == -85.0 || r.point[1] == -65.0 || r.point[2] == 410.0 || r.point[2] == 420.0;
    if (!on || r.face < 0 || r.face > 11 || r.keep != 1 || !(r.u >= 0.0 && r.v >= 0.0 && r.u + r.v <= 1.0)) { printf("sample_check: box sample %d\n", j); return 1; }
  }
  // thinned: no two kept samples nearer than the radius, every removed one has a kept one of lower index within it
  sc_sample(bv, 8, bf, 12, N, 7, 3.0, 32, nullptr, out.data(), &info);
  if (info.status || info.kept < 1 || info.kept >= N || info.rounds < 2) { printf("sample_check: thinned box: status %d kept %d rounds %d\n", info.status, info.kept, info.rounds); return 1; }
  for (int j = 0; j < N; ++j) {
    bool near_kept = false;
    for (int i = 0; i < j; ++i) near_kept = near_kept || (out[i].keep == 1 && sh::samp_d2(out[j].point, out[i].point) < 9.0);
    if (out[j].keep != (near_kept ? 0 : 1)) { printf("sample_check: thinned box sample %d\n", j); return 1; }
  }
  // zero-area faces are never drawn; only zero-area faces, no faces: the status and zero records
  const int mixed[12] = {0, 1, 1, 0, 2, 1, 2, 2, 3, 1, 2, 3};
  sc_sample(bv, 8, mixed, 4, N, 1, 0.0, 32, cdf.data(), out.data(), &info);
  if (info.status || cdf[0] != 0.0 || cdf[2] != cdf[1]) { printf("sample_check: mixed\n"); return 1; }
  for (int j = 0; j < N; ++j) if (out[j].face != 1 && out[j].face != 3) { printf("sample_check: a zero-area face was drawn\n"); return 1; }
  const int flat[6] = {0, 1, 1, 2, 2, 3};
  sc_sample(bv, 8, flat, 2, N, 1, 2.0, 32, nullptr, out.data(), &info);
  if (info.status != SH_ERR_GEOMETRY || info.area != 0.0 || out[0].keep != 0 || out[N - 1].point[0] != 0.0) { printf("sample_check: flat\n"); return 1; }
  sc_sample(bv, 8, flat, 0, N, 1, 0.0, 32, nullptr, out.data(), &info);
  if (info.status != SH_ERR_GEOMETRY) { printf("sample_check: no faces\n"); return 1; }
  // a fan of 513 faces: past one and two blocks
  std::vector<float> fv(3 * 515);
  std::vector<int> ff(3 * 513);
  for (int i = 0; i < 515; ++i) { fv[3 * i] = i == 0 ? 0.f : (float)cos(0.01 * i) * 40.f; fv[3 * i + 1] = i == 0 ? 0.f : (float)sin(0.01 * i) * 40.f; fv[3 * i + 2] = i == 0 ? 25.f : 0.f; }
  for (int i = 0; i < 513; ++i) { ff[3 * i] = 0; ff[3 * i + 1] = i + 1; ff[3 * i + 2] = i + 2; }
  std::vector<double> fc(513);
  for (int nf : {255, 256, 257, 513}) {
    sc_sample(fv.data(), 515, ff.data(), nf, N, 3, 0.0, 32, fc.data(), out.data(), &info);
    bool up = true;
    for (int f = 1; f < nf; ++f) up = up && fc[f] >= fc[f - 1];
    if (info.status || !up || info.area * 2.0 != fc[(size_t)nf - 1]) { printf("sample_check: fan %d\n", nf); return 1; }
  }
  // a line of 40 points 0.9 r apart: every second one, one decided per round
  std::vector<double> line(3 * 40, 0.0);
  for (int j = 0; j < 40; ++j) line[3 * j] = 0.9 * j;
  int32_t keep[40], res[3];
  sc_thin(line.data(), 40, 1.0, 32, keep, res);
  bool alt = res[0] == 16 && res[1] == 32 && res[2] == SH_ERR_CAPACITY;
  for (int j = 0; j < 40; ++j) alt = alt && keep[j] == (j < 32 ? (j % 2 == 0 ? 1 : 0) : -1);
  sc_thin(line.data(), 32, 1.0, 32, keep, res);
  if (!alt || res[0] != 16 || res[1] != 32 || res[2] != 0) { printf("sample_check: line\n"); return 1; }
  // the checks of sh_sample_surface in their order
  char text[256];
  auto pre = [&](int ctx, int seeds, int opt, int n, double radius, int rounds, int reserved, int B, int pend) {
    return sc_precheck(ctx, seeds, opt, n, radius, rounds, reserved, B, pend, text, (int)sizeof text);
  };
  if (pre(1, 1, 1, 10, 0.0, 32, 0, 1, 0) != SH_OK || pre(0, 1, 1, 10, 0.0, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 0, 1, 0, 0.0, 32, 0, 0, 0) != SH_ERR_ARG ||
      pre(1, 1, 0, 10, 0.0, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 1, 0, -1.0, 32, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "N in 1..1048576") ||
      pre(1, 1, 1, SH_SAMPLE_MAX + 1, 0.0, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 1, 10, -1.0, 32, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "options") ||
      pre(1, 1, 1, 10, NAN, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 1, 10, INFINITY, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 1, 10, 1.0, 0, 0, 1, 0) != SH_ERR_ARG ||
      pre(1, 1, 1, 10, 1.0, 33, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 1, 10, 1.0, 32, 1, 1, 0) != SH_ERR_ARG || pre(1, 1, 1, SH_SAMPLE_THIN_MAX + 1, 1.0, 32, 0, 0, 0) != SH_ERR_ARG ||
      !strstr(text, "with a radius") || pre(1, 1, 1, SH_SAMPLE_THIN_MAX + 1, 0.0, 32, 0, 1, 0) != SH_OK || pre(1, 1, 1, SH_SAMPLE_THIN_MAX, 1.0, 32, 0, 1, 0) != SH_OK ||
      pre(1, 1, 1, 10, 0.0, 32, 0, 0, 0) != SH_ERR_STATE || pre(1, 1, 1, 10, 0.0, 32, 0, 1, 1) != SH_ERR_STATE) {
    printf("sample_check: precheck_sample (%s)\n", text); return 1;
  }
  size_t plan[9];
  sc_plan(3, 1000, 1, 513, 1200, plan);
  if (plan[0] != 3 || plan[1] != 4 || plan[2] != 1 || plan[3] != 2064 || plan[4] != 9600 || plan[5] != 72 || plan[6] != 144000 || plan[7] != 72 || plan[8] != 3 * 2064 * 4) {
    printf("sample_check: plan\n"); return 1;
  }
  printf("sample_check: ok\n");
  return 0;
}
