// Test shim (NOT product): the ray arithmetic of shoulder_amd/csrc/sh_scalar.h (ray_tri_hit, canal_ray_hit_side, ray_key_less -- the
// source k_rays.h runs on the device) and the argument checks of sh_query.h (precheck_ray_cast) on the host, for
// tests/test_ray_host.py.  rc_sort ranks a segment as k_ray_sort does (64 lanes striding the keys, each counting the keys below its
// own, the ranks below cap stored, the slots behind them zero with face = -1); rc_cast walks the faces of a mesh BACKWARDS into the
// pool (the device's slot order is arbitrary: the sort must remove it) with the CT or the box-frame loader and sorts.  Its own
// main() runs all of it on a tetrahedron and a stack of plates, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

extern "C" int rc_hit(const double* o, const double* d, const double* tri /* 3 x 3 */, double* t, int* side) {
  return sh::canal_ray_hit_side(o, d, tri, tri + 3, tri + 6, t, side) ? 1 : 0;
}
extern "C" int rc_hit_plain(const double* o, const double* d, const double* tri /* 3 x 3 */, double* t) { return sh::canal_ray_hit(o, d, tri, tri + 3, tri + 6, t) ? 1 : 0; }

// k_ray_sort for one segment of n keys; T: the box transform (points go to CT through its inverse) or null
extern "C" void rc_sort(const double* t, const int* face, const int* side, int n, const double* o, const double* d, const double* T, int cap, sh_ray_hit* out) {
  double Ti[16];
  if (T) sh::inv_transform(T, Ti);
  for (int lane = 0; lane < 64; ++lane)
    for (int j = lane; j < n; j += 64) {
      int rank = 0;
      for (int k = 0; k < n; ++k) rank += sh::ray_key_less(t[k], face[k], t[j], face[j]) ? 1 : 0;
      if (rank >= cap) continue;
      sh_ray_hit* h = out + rank;
      double p[3];
      for (int k = 0; k < 3; ++k) p[k] = o[k] + d[k] * t[j];
      if (T) { double q[3]; sh::xform_pt(Ti, p[0], p[1], p[2], q); p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
      h->t = t[j]; h->point[0] = p[0]; h->point[1] = p[1]; h->point[2] = p[2]; h->face = face[j]; h->side = side[j];
    }
  for (int s = n < cap ? n : cap; s < cap; ++s) { memset(out + s, 0, sizeof *out); out[s].face = -1; }
}

// one ray against the nf faces of a mesh of float32 vertices -> the count; the first min(count, cap) hits in order
extern "C" int rc_cast(const float* verts, const int* faces, int nf, const double* T, const double* o, const double* d, int cap, sh_ray_hit* out) {
  std::vector<double> t;
  std::vector<int> face, side;
  for (int f = nf - 1; f >= 0; --f) {
    double V[9];
    for (int j = 0; j < 3; ++j) {
      const float* v = verts + 3 * (size_t)faces[3 * f + j];
      V[3 * j] = (double)v[0]; V[3 * j + 1] = (double)v[1]; V[3 * j + 2] = (double)v[2];
      if (T) { double q[3]; sh::xform_pt(T, V[3 * j], V[3 * j + 1], V[3 * j + 2], q); V[3 * j] = q[0]; V[3 * j + 1] = q[1]; V[3 * j + 2] = q[2]; }
    }
    const double e1[3] = {V[3] - V[0], V[4] - V[1], V[5] - V[2]};
    const double e2[3] = {V[6] - V[0], V[7] - V[1], V[8] - V[2]};
    double th; int s;
    if (sh::ray_tri_hit(o, d, V, e1, e2, &th, &s)) { t.push_back(th); face.push_back(f); side.push_back(s); }
  }
  rc_sort(t.data(), face.data(), side.data(), (int)t.size(), o, d, T, cap, out);
  return (int)t.size();
}

// precheck_ray_cast against a context that is there, holds B humeri and has n_pending runs in flight
extern "C" int rc_precheck(const sh_ray* rays, int R, int per_humerus, int cap, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_ray_cast(rays, R, per_humerus, cap, sh::ArthroFacts{true, B, n_pending, 0, false, &st}).code;
}

// stand-alone run (sanitizer build): a tetrahedron from outside, through a vertex and missing; plates with tied pairs, cap below and above the count
int main() {
  const float tv[12] = {0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4};
  const int tf[12] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  std::vector<sh_ray_hit> h(8);
  const double o[3] = {1, 1, -2}, d[3] = {0, 0, 1};
  int n = rc_cast(tv, tf, 4, nullptr, o, d, 8, h.data());
  if (n != 2 || h[0].t != 2.0 || h[0].side != 1 || h[0].face != 0 || h[1].t != 4.0 || h[1].side != -1 || h[1].face != 3 || h[2].face != -1) {
    printf("ray_check: tetrahedron %d %g %d %g %d\n", n, h[0].t, h[0].side, h[1].t, h[1].side); return 1;
  }
  const double ov[3] = {1, 1, 6}, dv[3] = {-1, -1, -2};      // into the vertex (0, 0, 4) at t = 1: the three faces that hold it, by face
  n = rc_cast(tv, tf, 4, nullptr, ov, dv, 8, h.data());
  if (n != 3 || h[0].t != 1.0 || h[1].t != 1.0 || h[2].t != 1.0 || h[0].face != 1 || h[1].face != 2 || h[2].face != 3) { printf("ray_check: vertex %d\n", n); return 1; }
  const double om[3] = {9, 9, -2};
  if (rc_cast(tv, tf, 4, nullptr, om, d, 8, h.data()) != 0 || h[0].face != -1) { printf("ray_check: miss\n"); return 1; }
  const int P = 40;
  std::vector<float> pv(12 * (size_t)P);
  std::vector<int> pf(6 * (size_t)P);
  for (int k = 0; k < P; ++k) {
    const float z = (float)(k + 1), c[12] = {-1, -1, z, 1, -1, z, 1, 1, z, -1, 1, z};
    memcpy(&pv[12 * k], c, sizeof c);
    const int f[6] = {4 * k, 4 * k + 1, 4 * k + 2, 4 * k, 4 * k + 2, 4 * k + 3};
    memcpy(&pf[6 * k], f, sizeof f);
  }
  const double T[16] = {1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2, 0, 0, 0, 1};
  const double od[3] = {0.5, -0.25, 2.0}, oc[3] = {0, 0, 0};      // the diagonal of every plate: 80 hits in 40 tied pairs (box frame: shifted)
  for (int cap : {1, 8, 64, 128}) {
    std::vector<sh_ray_hit> g((size_t)cap);
    n = rc_cast(pv.data(), pf.data(), 2 * P, cap == 64 ? T : nullptr, cap == 64 ? od : oc, d, cap, g.data());
    if (n != 2 * P) { printf("ray_check: plates %d\n", n); return 1; }
    for (int s = 0; s < cap; ++s) {
      const bool ok = s < n ? (g[s].face == s && g[s].t == (double)(s / 2 + 1) && g[s].side == -1 && g[s].point[2] == (double)(s / 2 + 1))
                            : (g[s].face == -1 && g[s].t == 0.0 && g[s].side == 0);
      if (!ok) { printf("ray_check: plates cap %d slot %d\n", cap, s); return 1; }
    }
  }
  sh_ray r[2] = {{{0, 0, 0}, {0, 0, 1}}, {{0, 0, 0}, {0, 0, 0}}};
  if (rc_precheck(r, 1, 0, 16, 1, 0) != SH_OK || rc_precheck(r, 2, 0, 16, 1, 0) != SH_ERR_ARG || rc_precheck(r, 1, 0, 0, 1, 0) != SH_ERR_ARG ||
      rc_precheck(r, 1, 0, 16, 0, 0) != SH_ERR_STATE || rc_precheck(r, 1, 0, 16, 1, 1) != SH_ERR_STATE) { printf("ray_check: precheck\n"); return 1; }
  printf("ray_check: ok (tetrahedron 2 + 3 + 0 hits, plates %d hits in %d tied pairs)\n", 2 * P, P);
  return 0;
}
