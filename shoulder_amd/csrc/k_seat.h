// k_seat.h -- a catalogue of K implant heads seated on every cut of a fitted batched resection (include/shoulder_hip.h sh_seat):
// covered / overhanging / uncovered area of each head's base disk against the cut's largest loop, the radial rim distances about
// the seat centre, the implant sphere's centre against the fitted one and its rms distance from the head piece's samples.
// The reference stops in front of this step (arthroplasty.py:178-182, a commented-out `HumeralImplantation`).
//   k_resect_join_seat (k_resect.h) the fitted join; it also stores the largest loop's in-plane coordinates ("resect.seat_ring").
//   k_seat             one workgroup of four waves per cut of the pass, after k_headfit_solve of that pass.  The ring goes into LDS
//                      once (16 KB).  Wave 0 takes the measures that do not depend on the head -- nearest segment, farthest vertex,
//                      winding number about the seat centre -- lanes striding the edges in ring order, minimum and maximum carried
//                      with their ring index through the shuffle tree so that ties go to the smaller index.  Then wave j takes
//                      heads j, j + 4, ...: lanes stride the edges, every lane adds its edges' Green terms (sh_scalar.h
//                      seat_edge_term) in ring order, the fixed shuffle tree adds the lanes, lane 0 finishes and stores the record.
//                      A head's sum is taken by one wave in one order whichever wave that is: a record does not depend on K or on
//                      the head's place in the catalogue; the ring and the moments are the cut's own.  No floating-point atomics.
#pragma once
#include "k_headfit.h"

namespace sh {

#define SH_SEAT_THREADS 256

__global__ void __launch_bounds__(SH_SEAT_THREADS)
k_seat(const sh_resection* __restrict__ recs /* B x P */, const sh_head_fit* __restrict__ fits /* B x P */, const int* __restrict__ cut_status /* B x P */,
       const double* __restrict__ moments /* B x P x 16 */, const double* __restrict__ ring_uw /* [cuts of the pass][2][SH_MAXSEG] */,
       const sh_landmarks* __restrict__ lm /* nullable, as k_headfit_solve's */, const sh_implant_head* __restrict__ heads, int K, int mode,
       int P, int p0, int pc, sh_seat* __restrict__ out /* B x P x K */) {
  __shared__ double rx[SH_MAXSEG], ry[SH_MAXSEG];
  __shared__ double s_rim[6];      // rim_min^2, nearest point (2), rim_max^2, farthest vertex (2), about s
  __shared__ int s_wind;
  const int cut = blockIdx.x, b = cut / pc, p = p0 + (cut - b * pc), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t idx = (size_t)b * P + p;
  sh_seat* const dst = out + idx * K;
  const sh_resection rec = recs[idx];
  const sh_head_fit fit = fits[idx];
  const bool has_sphere = fit.sphere_status == 0 && fit.sphere_radius > 0.0;
  int status = cut_status[idx];
  if (status == 0) status = rec.status;
  const int L = rec.n_ring;
  const bool ring = status == 0 && rec.n_loops > 0 && L >= 1 && L <= SH_MAXSEG;
  if (status == 0 && ring && mode == SH_SEAT_SPHERE_AXIS) status = fit.sphere_status != 0 ? fit.sphere_status : (has_sphere ? 0 : SH_ERR_GEOMETRY_DEV);
  if (status != 0 || !ring) {      // (uniform) the status, nothing else; a cut without a loop: zeros
    static_assert(sizeof(sh_seat) == 29 * 8, "sh_seat is 28 doubles and two int32");
    for (int i = tid; i < K * 29; i += SH_SEAT_THREADS) {
      long long word = 0;
      if (i % 29 == 28) word = (long long)(unsigned long long)(unsigned)status << 32;      // (center_inside = 0 | status)
      ((long long*)dst)[i] = word;
    }
    return;
  }
  const double* o = rec.plane_point; const double* nn = rec.plane_normal;
  const double nlen = sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
  const double un[3] = {nn[0] / nlen, nn[1] / nlen, nn[2] / nlen};
  double u[3], w[3];
  resect_basis(un, u, w);
  const bool axis = mode == SH_SEAT_SPHERE_AXIS;
  const double gx = (axis ? fit.sphere_center[0] : rec.cut_centroid[0]) - o[0], gy = (axis ? fit.sphere_center[1] : rec.cut_centroid[1]) - o[1],
               gz = (axis ? fit.sphere_center[2] : rec.cut_centroid[2]) - o[2];
  const double su = (gx * u[0] + gy * u[1]) + gz * u[2], sw = (gx * w[0] + gy * w[1]) + gz * w[2];
  {      // the ring about s
    const double* g = ring_uw + (size_t)cut * 2 * SH_MAXSEG;
    for (int k = tid; k < L; k += SH_SEAT_THREADS) { rx[k] = g[k] - su; ry[k] = g[SH_MAXSEG + k] - sw; }
  }
  __syncthreads();
  if (wave == 0) {
    double dmin = INFINITY, dmax = -1.0; int imin = 0x7fffffff, imax = 0x7fffffff, wn = 0;
    for (int k = lane; k < L; k += 64) {
      const int kn = k + 1 == L ? 0 : k + 1;
      const double ax = rx[k], ay = ry[k], bx = rx[kn], by = ry[kn];
      double qx, qy;
      const double d2 = seat_seg_dist2(ax, ay, bx, by, &qx, &qy), v2 = ax * ax + ay * ay;
      if (d2 < dmin) { dmin = d2; imin = k; }
      if (v2 > dmax) { dmax = v2; imax = k; }
      wn += seat_winding_term(ax, ay, bx, by);
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_down(dmin, off), ox = __shfl_down(dmax, off);
      const int oi = __shfl_down(imin, off), oj = __shfl_down(imax, off);
      if (od < dmin || (od == dmin && oi < imin)) { dmin = od; imin = oi; }
      if (ox > dmax || (ox == dmax && oj < imax)) { dmax = ox; imax = oj; }
      wn += __shfl_down(wn, off);
    }
    if (lane == 0) {
      const int kn = imin + 1 == L ? 0 : imin + 1;
      double qx, qy;
      s_rim[0] = seat_seg_dist2(rx[imin], ry[imin], rx[kn], ry[kn], &qx, &qy);
      s_rim[1] = qx; s_rim[2] = qy;
      s_rim[3] = dmax; s_rim[4] = rx[imax]; s_rim[5] = ry[imax];
      s_wind = wn;
    }
  }
  __syncthreads();
  const double rmin = sqrt(s_rim[0]), rmax = sqrt(s_rim[3]);
  const double* m = moments + idx * 16;
  const sh_landmarks* Lm = lm ? lm + b : nullptr;
  for (int k = wave; k < K; k += SH_SEAT_THREADS / 64) {
    const double R = heads[k].radius, h = heads[k].thickness;
    const double rho2 = h * (2.0 * R - h), rho = sqrt(rho2);
    double a2 = 0.0;
    for (int e = lane; e < L; e += 64) {
      const int en = e + 1 == L ? 0 : e + 1;
      a2 += seat_edge_term(rx[e], ry[e], rx[en], ry[en], rho2);
    }
    for (int off = 32; off > 0; off >>= 1) a2 += __shfl_down(a2, off);
    if (lane == 0) {      // (the record is written field by field: a local sh_seat would live in scratch)
      sh_seat* r = dst + k;
      const double pi = 3.14159265358979323846;
      const double cov = fabs(a2);
      r->base_radius = rho;
      r->covered_area = cov;
      r->coverage = rec.cut_area > 0.0 ? cov / rec.cut_area : 0.0;
      r->overhang_area = pi * rho2 - cov;
      r->uncovered_area = rec.cut_area - cov;
      r->rim_min = rmin; r->rim_max = rmax;
      r->max_overhang = rho - rmin > 0.0 ? rho - rmin : 0.0;
      r->max_uncovered = rmax - rho > 0.0 ? rmax - rho : 0.0;
      r->center_inside = s_wind != 0 ? 1 : 0;
      r->status = 0;
      double c[3], ic[3], cs[3];      // the implant centre about the plane point, as the moments are; in CT; its shift
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        r->seat_center[i] = (o[i] + su * u[i]) + sw * w[i];
        r->overhang_dir[i] = rmin > 0.0 ? (s_rim[1] / rmin) * u[i] + (s_rim[2] / rmin) * w[i] : 0.0;
        r->uncovered_dir[i] = rmax > 0.0 ? (s_rim[4] / rmax) * u[i] + (s_rim[5] / rmax) * w[i] : 0.0;
        c[i] = (su * u[i] + sw * w[i]) + (h - R) * un[i];
        ic[i] = o[i] + c[i];
        cs[i] = has_sphere ? ic[i] - fit.sphere_center[i] : 0.0;
        r->implant_center[i] = ic[i]; r->cor_shift[i] = cs[i];
      }
      r->surface_rms = seat_surface_rms(m, c, R);
      const bool frame = Lm && Lm->status == 0;
      const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double v = qnan;
        if (frame) { const double* T = Lm->csys_articular; v = has_sphere ? (T[4 * i] * cs[0] + T[4 * i + 1] * cs[1]) + T[4 * i + 2] * cs[2] : 0.0; }
        r->cor_shift_articular[i] = v;
      }
    }
  }
}

}  // namespace sh
