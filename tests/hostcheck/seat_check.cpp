// Test shim (NOT product): the seat arithmetic of shoulder_amd/csrc/sh_scalar.h (seat_edge_term, seat_seg_dist2, seat_winding_term,
// seat_surface_rms -- the source k_seat runs on the device) on the host, for tests/test_seat_host.py.  st_seat adds and compares in k_seat's order: 64 lanes striding the edges in ring order, then
// the shuffle tree (lane l takes lane l + off for off = 32, 16, ..., 1), minimum and maximum with their ring index.
#include "../../shoulder_amd/csrc/sh_scalar.h"
extern "C" double st_edge(double ax, double ay, double bx, double by, double rho2) { return sh::seat_edge_term(ax, ay, bx, by, rho2); }
extern "C" double st_seg(double ax, double ay, double bx, double by, double* near2) { return sh::seat_seg_dist2(ax, ay, bx, by, near2, near2 + 1); }
extern "C" int st_wind(double ax, double ay, double bx, double by) { return sh::seat_winding_term(ax, ay, bx, by); }
extern "C" double st_rms(const double* m16, const double* c3, double R) { return sh::seat_surface_rms(m16, c3, R); }
// x, y: the L ring vertices about the seat centre.  out: signed covered area, rim_min^2, nearest point (2), rim_max^2, farthest
// vertex (2); idx: nearest segment, farthest vertex, winding number
extern "C" void st_seat(const double* x, const double* y, int L, double rho2, double* out, int* idx) {
  double a[64], dmin[64], dmax[64]; int imin[64], imax[64], wn[64];
  for (int l = 0; l < 64; ++l) {
    a[l] = 0.0; dmin[l] = INFINITY; dmax[l] = -1.0; imin[l] = imax[l] = 0x7fffffff; wn[l] = 0;
    for (int k = l; k < L; k += 64) {
      const int kn = k + 1 == L ? 0 : k + 1;
      double q[2];
      const double d2 = sh::seat_seg_dist2(x[k], y[k], x[kn], y[kn], q, q + 1), v2 = x[k] * x[k] + y[k] * y[k];
      if (d2 < dmin[l]) { dmin[l] = d2; imin[l] = k; }
      if (v2 > dmax[l]) { dmax[l] = v2; imax[l] = k; }
      wn[l] += sh::seat_winding_term(x[k], y[k], x[kn], y[kn]);
      a[l] += sh::seat_edge_term(x[k], y[k], x[kn], y[kn], rho2);
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int l = 0; l < off; ++l) {
      const int o = l + off;
      a[l] += a[o]; wn[l] += wn[o];
      if (dmin[o] < dmin[l] || (dmin[o] == dmin[l] && imin[o] < imin[l])) { dmin[l] = dmin[o]; imin[l] = imin[o]; }
      if (dmax[o] > dmax[l] || (dmax[o] == dmax[l] && imax[o] < imax[l])) { dmax[l] = dmax[o]; imax[l] = imax[o]; }
    }
  const int k = imin[0], kn = k + 1 == L ? 0 : k + 1;
  out[0] = a[0];
  out[1] = sh::seat_seg_dist2(x[k], y[k], x[kn], y[kn], out + 2, out + 3);
  out[4] = dmax[0]; out[5] = x[imax[0]]; out[6] = y[imax[0]];
  idx[0] = k; idx[1] = imax[0]; idx[2] = wn[0];
}
