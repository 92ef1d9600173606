// Test shim (NOT product): the canal-profile and stem arithmetic of shoulder_amd/csrc/sh_scalar.h (canal_map_point, canal_ray_hit,
// canal_level_range, canal_angle_range, stem_radius_at, stem_sample_counts, stem_entry, stem_level_span -- the source k_stem.h runs on
// the device) on the host, for tests/test_stem_host.py.  sc_profile walks the faces as k_canal_rays does (with the culling, or with
// cull = 0 every ray against every face); sc_levels and sc_stem add and compare in the kernels' order: 64 lanes striding, then the
// shuffle tree (lane l takes lane l + off for off = 32, 16, ..., 1).  Its own main() runs all of it on a small prism, so that the
// file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

extern "C" void sc_dirs(int A, double* dirs /* A x 2 */) {      // the table sh_canal_profile uploads
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int a = 0; a < A; ++a) { const double t = (two_pi * (double)a) / (double)A; dirs[2 * a] = cos(t); dirs[2 * a + 1] = sin(t); }
}
extern "C" int sc_hit(const double* o, const double* d, const double* tri /* 3 x 3 */, double* t) { return sh::canal_ray_hit(o, d, tri, tri + 3, tri + 6, t) ? 1 : 0; }
extern "C" double sc_radius(double length, double r_prox, double r_tip, double d) { return sh::stem_radius_at(length, r_prox, r_tip, d); }
extern "C" void sc_ranges(const double* tri /* 3 x 3, frame */, double z0, double dz, int L, int A, int* out /* l_lo, l_hi, a0, n */) {
  sh::canal_level_range(z0, dz, L, fmin(tri[2], fmin(tri[5], tri[8])), fmax(tri[2], fmax(tri[5], tri[8])), out, out + 1);
  const double x[3] = {tri[0], tri[3], tri[6]}, y[3] = {tri[1], tri[4], tri[7]};
  sh::canal_angle_range(x, y, A, out + 2, out + 3);
}

// near / far (L x A, +inf / 0 without a hit) of the mesh (float32 vertices, nf faces) in the frame T; returns the (face, ray) tests made
extern "C" long long sc_profile(const float* verts, const int* faces, int nf, const double* T, double z0, double dz, int L, int A, int cull,
                                double* near, double* far) {
  std::vector<double> dirs(2 * (size_t)A);
  sc_dirs(A, dirs.data());
  for (int i = 0; i < L * A; ++i) { near[i] = INFINITY; far[i] = 0.0; }
  long long tests = 0;
  for (int f = 0; f < nf; ++f) {
    double P[9];
    for (int j = 0; j < 3; ++j) {
      const float* v = verts + 3 * (size_t)faces[3 * f + j];
      sh::canal_map_point(T, (double)v[0], (double)v[1], (double)v[2], P + 3 * j);
    }
    int r[4] = {0, L - 1, 0, A};
    if (cull) sc_ranges(P, z0, dz, L, A, r);
    for (int l = r[0]; l <= r[1]; ++l) {
      const double o[3] = {0.0, 0.0, z0 - (double)l * dz};
      int a = r[2];
      for (int k = 0; k < r[3]; ++k) {
        const double d[3] = {dirs[2 * a], dirs[2 * a + 1], 0.0};
        double t;
        ++tests;
        if (sh::canal_ray_hit(o, d, P, P + 3, P + 6, &t)) {
          if (t < near[l * A + a]) near[l * A + a] = t;
          if (t > far[l * A + a]) far[l * A + a] = t;
        }
        a = a + 1 == A ? 0 : a + 1;
      }
    }
  }
  return tests;
}

extern "C" void sc_levels(const double* near, const double* far, int L, int A, sh_canal_level* out) {
  std::vector<double> dirs(2 * (size_t)A);
  sc_dirs(A, dirs.data());
  const double half_sin_step = 0.5 * sin((2.0 * 3.14159265358979323846) / (double)A);
  for (int l = 0; l < L; ++l) {
    const double* nr = near + (size_t)l * A;
    const double* fr = far + (size_t)l * A;
    sh_canal_level* r = out + l;
    memset(r, 0, sizeof *r);
    int nh = 0;
    for (int a = 0; a < A; ++a) nh += nr[a] < INFINITY ? 1 : 0;
    r->n_hit = nh;
    if (nh < A) { r->status = SH_ERR_GEOMETRY; continue; }
    double rmin[64], rmax[64], sr[64], srr[64], sc[64], scx[64], scy[64], xlo[64], xhi[64], ylo[64], yhi[64], wmin[64];
    int imin[64], imax[64];
    for (int ln = 0; ln < 64; ++ln) {
      rmin[ln] = INFINITY; rmax[ln] = -1.0; sr[ln] = srr[ln] = sc[ln] = scx[ln] = scy[ln] = 0.0;
      xlo[ln] = ylo[ln] = wmin[ln] = INFINITY; xhi[ln] = yhi[ln] = -INFINITY; imin[ln] = imax[ln] = 0x7fffffff;
      for (int a = ln; a < A; a += 64) {
        const int an = a + 1 == A ? 0 : a + 1;
        const double ra = nr[a], rb = nr[an];
        const double xa = ra * dirs[2 * a], ya = ra * dirs[2 * a + 1], xb = rb * dirs[2 * an], yb = rb * dirs[2 * an + 1];
        const double cr = xa * yb - ya * xb, w = fr[a] - ra;
        if (ra < rmin[ln]) { rmin[ln] = ra; imin[ln] = a; }
        if (ra > rmax[ln]) { rmax[ln] = ra; imax[ln] = a; }
        sr[ln] += ra; srr[ln] += ra * rb; sc[ln] += cr; scx[ln] += (xa + xb) * cr; scy[ln] += (ya + yb) * cr;
        xlo[ln] = fmin(xlo[ln], xa); xhi[ln] = fmax(xhi[ln], xa); ylo[ln] = fmin(ylo[ln], ya); yhi[ln] = fmax(yhi[ln], ya); wmin[ln] = fmin(wmin[ln], w);
      }
    }
    for (int off = 32; off > 0; off >>= 1)
      for (int ln = 0; ln < off; ++ln) {
        const int o = ln + off;
        if (rmin[o] < rmin[ln] || (rmin[o] == rmin[ln] && imin[o] < imin[ln])) { rmin[ln] = rmin[o]; imin[ln] = imin[o]; }
        if (rmax[o] > rmax[ln] || (rmax[o] == rmax[ln] && imax[o] < imax[ln])) { rmax[ln] = rmax[o]; imax[ln] = imax[o]; }
        sr[ln] += sr[o]; srr[ln] += srr[o]; sc[ln] += sc[o]; scx[ln] += scx[o]; scy[ln] += scy[o];
        xlo[ln] = fmin(xlo[ln], xlo[o]); xhi[ln] = fmax(xhi[ln], xhi[o]); ylo[ln] = fmin(ylo[ln], ylo[o]); yhi[ln] = fmax(yhi[ln], yhi[o]);
        wmin[ln] = fmin(wmin[ln], wmin[o]);
      }
    r->r_min = rmin[0]; r->r_max = rmax[0]; r->r_mean = sr[0] / (double)A; r->area = half_sin_step * srr[0];
    r->centroid[0] = sc[0] != 0.0 ? scx[0] / (3.0 * sc[0]) : 0.0; r->centroid[1] = sc[0] != 0.0 ? scy[0] / (3.0 * sc[0]) : 0.0;
    r->extent_x[0] = xlo[0]; r->extent_x[1] = xhi[0]; r->extent_y[0] = ylo[0]; r->extent_y[1] = yhi[0]; r->wall_min = wmin[0];
    r->a_min = imin[0]; r->a_max = imax[0];
  }
}

// one stem below one cut (plane: point, normal in CT) in k_stem_fit's order
extern "C" void sc_stem(const double* plane, const double* T, const double* near, const sh_canal_level* lv, double z0, double dz, int L, int A,
                        const sh_stem* stem, sh_stem_fit* r) {
  std::vector<double> dirs(2 * (size_t)A);
  sc_dirs(A, dirs.data());
  memset(r, 0, sizeof *r);
  double of[3], un[3], entry[3], ze = 0.0;
  if (int st = sh::stem_entry(T, plane, plane + 3, of, un, &ze, entry)) { r->status = st; return; }
  const double len = stem->length, rp = stem->r_prox, rt = stem->r_tip;
  int l0, l1;
  if (!sh::stem_level_span(z0, dz, L, ze, len, &l0, &l1)) { r->status = SH_ERR_ARG; return; }
  const int total = l1 >= l0 ? (l1 - l0 + 1) * A : 0;
  double cmin[64], smin[64];
  int imin[64], ns[64], nbr[64], nop[64];
  for (int ln = 0; ln < 64; ++ln) {
    cmin[ln] = smin[ln] = INFINITY; imin[ln] = 0x7fffffff; ns[ln] = nbr[ln] = nop[ln] = 0;
    for (int s = ln; s < total; s += 64) {
      const int li = s / A, a = s - li * A, l = l0 + li;
      const double d = sh::stem_level_depth(z0, dz, l, ze), rr = sh::stem_radius_at(len, rp, rt, d);
      if (!sh::stem_sample_counts(rr, dirs[2 * a], dirs[2 * a + 1], z0 - (double)l * dz, of, un)) continue;
      ++ns[ln];
      const double t = near[(size_t)l * A + a];
      if (!(t < INFINITY)) { ++nop[ln]; continue; }
      const double cl = t - rr, sc = t / rr;
      if (cl < 0.0) ++nbr[ln];
      if (cl < cmin[ln]) { cmin[ln] = cl; imin[ln] = s; }
      if (sc < smin[ln]) smin[ln] = sc;
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int ln = 0; ln < off; ++ln) {
      const int o = ln + off;
      if (cmin[o] < cmin[ln] || (cmin[o] == cmin[ln] && imin[o] < imin[ln])) { cmin[ln] = cmin[o]; imin[ln] = imin[o]; }
      smin[ln] = fmin(smin[ln], smin[o]);
      ns[ln] += ns[o]; nbr[ln] += nbr[o]; nop[ln] += nop[o];
    }
  const double pi = 3.14159265358979323846;
  double fsum = 0.0, fmax_ = 0.0, fdepth = 0.0;
  int nf = 0;
  for (int l = l0; l <= l1; ++l) {
    const double area = lv[l].area;
    if (lv[l].status != 0 || !(area > 0.0)) continue;
    const double d = sh::stem_level_depth(z0, dz, l, ze), rr = sh::stem_radius_at(len, rp, rt, d);
    const double f = (pi * (rr * rr)) / area;
    fsum += f; ++nf;
    if (f > fmax_) { fmax_ = f; fdepth = d; }
  }
  const bool any = imin[0] != 0x7fffffff;
  const int li = any ? imin[0] / A : 0, a = any ? imin[0] - li * A : -1;
  const double dv[3] = {any ? dirs[2 * a] : 0.0, any ? dirs[2 * a + 1] : 0.0, 0.0};
  double dc[3];
  sh::canal_unmap_dir(T, dv, dc);
  for (int i = 0; i < 3; ++i) { r->entry[i] = entry[i]; r->direction[i] = any ? dc[i] : 0.0; }
  r->z_entry = ze;
  r->min_clearance = any ? cmin[0] : 0.0;
  r->depth = any ? sh::stem_level_depth(z0, dz, l0 + li, ze) : 0.0;
  r->scale_max = any ? smin[0] : 0.0;
  r->fill_mean = nf > 0 ? fsum / (double)nf : 0.0;
  r->fill_max = fmax_; r->fill_max_depth = fdepth;
  r->angle_index = a; r->n_samples = ns[0]; r->n_breach = nbr[0]; r->n_open = nop[0];
  r->fits = (nbr[0] == 0 && nop[0] == 0 && ns[0] > 0) ? 1 : 0;
}

// stand-alone run: a square prism (corners (20, 6), (-6, 20), ... off every ray; apothem sqrt(218), z in [-60, 60]) about the z axis of the identity frame, profile with and without
// the culling, levels and two stems below a tilted cut
int main() {
  const float v[8][3] = {{20, 6, -60}, {-6, 20, -60}, {-20, -6, -60}, {6, -20, -60}, {20, 6, 60}, {-6, 20, 60}, {-20, -6, 60}, {6, -20, 60}};
  int f[12][3]; int nf = 0;
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) % 4;
    f[nf][0] = i; f[nf][1] = j; f[nf][2] = j + 4; ++nf;
    f[nf][0] = i; f[nf][1] = j + 4; f[nf][2] = i + 4; ++nf;
  }
  f[nf][0] = 0; f[nf][1] = 2; f[nf][2] = 1; ++nf; f[nf][0] = 0; f[nf][1] = 3; f[nf][2] = 2; ++nf;
  f[nf][0] = 4; f[nf][1] = 5; f[nf][2] = 6; ++nf; f[nf][0] = 4; f[nf][1] = 6; f[nf][2] = 7; ++nf;
  const double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const int L = 70, A = 64;
  const double z0 = 65.0, dz = 2.0;
  std::vector<double> near(L * A), far(L * A), near2(L * A), far2(L * A);
  const long long t1 = sc_profile(&v[0][0], &f[0][0], nf, T, z0, dz, L, A, 1, near.data(), far.data());
  const long long t0 = sc_profile(&v[0][0], &f[0][0], nf, T, z0, dz, L, A, 0, near2.data(), far2.data());
  const bool same = memcmp(near.data(), near2.data(), near.size() * 8) == 0 && memcmp(far.data(), far2.data(), far.size() * 8) == 0;
  std::vector<sh_canal_level> lv(L);
  sc_levels(near.data(), far.data(), L, A, lv.data());
  const double plane[6] = {0.0, 0.0, 40.0, 0.2, 0.0, 1.0};
  const sh_stem stems[2] = {{80.0, 8.0, 5.0}, {80.0, 16.0, 5.0}};
  sh_stem_fit fit[2];
  for (int k = 0; k < 2; ++k) sc_stem(plane, T, near.data(), lv.data(), z0, dz, L, A, stems + k, fit + k);
  printf("tests culled %lld of %lld, same %d; level 10: r_min %.17g area %.17g status %d; level 0 n_hit %d status %d\n", t1, t0, (int)same, lv[10].r_min,
         lv[10].area, lv[10].status, lv[0].n_hit, lv[0].status);
  for (int k = 0; k < 2; ++k)
    printf("stem %d: status %d fits %d n_samples %d n_breach %d min_clearance %.17g scale_max %.17g fill_max %.17g\n", k, fit[k].status, fit[k].fits,
           fit[k].n_samples, fit[k].n_breach, fit[k].min_clearance, fit[k].scale_max, fit[k].fill_max);
  const bool ok = same && lv[10].status == 0 && lv[10].r_min >= sqrt(218.0) - 1e-12 && lv[10].r_min < sqrt(218.0) + 0.05 && lv[0].status == SH_ERR_GEOMETRY && fit[0].fits == 1 && fit[1].fits == 0 && fit[1].n_breach > 0;
  return ok ? 0 : 1;
}
