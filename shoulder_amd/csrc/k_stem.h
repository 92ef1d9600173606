// k_stem.h -- the canal below a cut: a polar profile of every resident humerus about its canal axis (include/shoulder_hip.h
// sh_canal_profile) and the fit of a catalogue of K frustum stems below every cut of the last batched resection (sh_resect_stems).
// The reference names this step and leaves it empty (arthroplasty.py:178-182, a commented-out `HumeralImplantation` that
// "continues from the humeral head osteotomy and places the implant"); k_headfit.h / k_seat.h size and seat the head, this is the stem.
//   k_canal_frames  frames == NULL: the B frames and statuses from the device records (csys_articular, status)
//   k_canal_clear   near = +inf, far = 0 (the +inf bit pattern is not a byte fill)
//   k_canal_rays    (tile of 256 faces, humerus) workgroups, one face per lane as k_resect_faces: the face is fetched once, widened
//                   and mapped into the frame (sh_scalar.h canal_map_point), then the lane visits only the levels inside the face's
//                   z-extent and the angles inside the angular extent of its projection about the axis (canal_level_range /
//                   canal_angle_range: both rounded outwards and widened by one index each side, angles wrap, a projection that
//                   holds the origin takes all A angles) and runs the full test (canal_ray_hit) on each.  The culling only leaves
//                   out pairs the full test rejects.  A hit goes to memory with atomicMin / atomicMax on the double's bit pattern
//                   (t > 0 orders like its bits; k_obb.h and k_rays_hit do the same): minimum and maximum do not depend on an
//                   order, so a humerus' rows are bit-equal whatever the batch, its position in it, L or the tiling.  No
//                   floating-point sums, no LDS, no shuffles.
//   k_canal_levels  one wave per (humerus, level): lanes stride the A rays in angle order, the fixed shuffle tree adds the lanes,
//                   minima and maxima carry their angle index so that ties go to the smaller one; lane 0 writes the record.
//   k_stem_fit      one workgroup of four waves per cut.  Wave j takes stems j, j + 4, ... as k_seat takes heads: lanes stride the
//                   samples of the used levels in (l, a) order, the minimum clearance carries its sample index through the tree,
//                   integer sums are plain, the fill sum is taken by lane 0 in level order.  A record depends on its cut, its stem
//                   and the profile alone: not on B, P, K or the stem's place in the catalogue.
#pragma once
#include "k_resect.h"

namespace sh {

#define SH_CANAL_TILE SH_RS_TILE
#define SH_STEM_THREADS 256
#define SH_CANAL_INF_BITS 0x7ff0000000000000ull

__global__ void k_canal_frames(const sh_landmarks* __restrict__ lm, int B, double* __restrict__ frames /* B x 16 */, int* __restrict__ hstatus /* B */) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const sh_landmarks* L = lm + b;
  int st = L->status;
  bool fin = true;
  for (int i = 0; i < 16; ++i) fin = fin && isfinite(L->csys_articular[i]);
  if (st == 0 && !fin) st = SH_ERR_GEOMETRY_DEV;
  for (int i = 0; i < 16; ++i) frames[16 * (size_t)b + i] = st == 0 ? L->csys_articular[i] : 0.0;
  hstatus[b] = st;
}

__global__ void __launch_bounds__(256)
k_canal_clear(unsigned long long* __restrict__ near_bits, unsigned long long* __restrict__ far_bits, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) { near_bits[i] = SH_CANAL_INF_BITS; far_bits[i] = 0ull; }
}

__global__ void __launch_bounds__(SH_CANAL_TILE)
k_canal_rays(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
             const double* __restrict__ frames /* B x 16 */, const int* __restrict__ hstatus /* B */, const double* __restrict__ dirs /* A x 2 */,
             double z0, double dz, int L, int A, unsigned long long* __restrict__ near_bits /* B x L x A */, unsigned long long* __restrict__ far_bits) {
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  if (hstatus[b] != 0) return;      // (uniform) a humerus without a frame keeps near = +inf, far = 0
  bool live; long long fi; double V[9];
  if (!resect_tile_face(verts, faces, voff, foff, b, t, tid, &live, &fi, V)) return;      // (uniform)
  if (!live) return;
  const double* T = frames + 16 * (size_t)b;
  double P[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) canal_map_point(T, V[3 * j], V[3 * j + 1], V[3 * j + 2], P + 3 * j);
  int l_lo, l_hi, a0, na;
  canal_level_range(z0, dz, L, fmin(P[2], fmin(P[5], P[8])), fmax(P[2], fmax(P[5], P[8])), &l_lo, &l_hi);
  if (l_lo > l_hi) return;
  {
    const double x[3] = {P[0], P[3], P[6]}, y[3] = {P[1], P[4], P[7]};
    canal_angle_range(x, y, A, &a0, &na);
  }
  unsigned long long* const nb = near_bits + (size_t)b * L * A;
  unsigned long long* const fb = far_bits + (size_t)b * L * A;
  for (int l = l_lo; l <= l_hi; ++l) {      // 0 <= l_lo, l_hi <= L - 1
    const double o[3] = {0.0, 0.0, z0 - (double)l * dz};
    int a = a0;                             // 0 <= a0 < A, na <= A
    for (int k = 0; k < na; ++k) {
      const double d[3] = {dirs[2 * a], dirs[2 * a + 1], 0.0};
      double th;
      if (canal_ray_hit(o, d, P, P + 3, P + 6, &th)) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(th);
        atomicMin(&nb[(size_t)l * A + a], bits);
        atomicMax(&fb[(size_t)l * A + a], bits);
      }
      a = a + 1 == A ? 0 : a + 1;
    }
  }
}

__global__ void __launch_bounds__(64)
k_canal_levels(const double* __restrict__ near /* B x L x A */, const double* __restrict__ far, const int* __restrict__ hstatus /* B */,
               const double* __restrict__ dirs /* A x 2 */, double half_sin_step /* 0.5 sin(2 pi / A) */, int L, int A,
               sh_canal_level* __restrict__ out /* B x L */) {
  const int row = blockIdx.x, b = row / L, lane = threadIdx.x;
  const double* nr = near + (size_t)row * A;
  const double* fr = far + (size_t)row * A;
  sh_canal_level* r = out + row;
  const int hs = hstatus[b];
  int nh = 0;
  for (int a = lane; a < A; a += 64) nh += nr[a] < INFINITY ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) nh += __shfl_down(nh, off);
  nh = __shfl(nh, 0);
  if (hs != 0 || nh < A) {      // (uniform) the count and the status, nothing else
    static_assert(sizeof(sh_canal_level) == 13 * 8, "sh_canal_level is 11 doubles and four int32");
    if (lane < 13) {
      long long word = 0;
      if (lane == 12) word = (long long)((unsigned long long)(unsigned)(hs != 0 ? 0 : nh) | ((unsigned long long)(unsigned)(hs != 0 ? hs : SH_ERR_GEOMETRY_DEV) << 32));
      ((long long*)r)[lane] = word;
    }
    return;
  }
  double rmin = INFINITY, rmax = -1.0, sr = 0.0, srr = 0.0, sc = 0.0, scx = 0.0, scy = 0.0;
  double xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY, wmin = INFINITY;
  int imin = 0x7fffffff, imax = 0x7fffffff;
  for (int a = lane; a < A; a += 64) {
    const int an = a + 1 == A ? 0 : a + 1;
    const double ra = nr[a], rb = nr[an];
    const double xa = ra * dirs[2 * a], ya = ra * dirs[2 * a + 1], xb = rb * dirs[2 * an], yb = rb * dirs[2 * an + 1];
    const double cr = xa * yb - ya * xb, w = fr[a] - ra;
    if (ra < rmin) { rmin = ra; imin = a; }
    if (ra > rmax) { rmax = ra; imax = a; }
    sr += ra; srr += ra * rb; sc += cr; scx += (xa + xb) * cr; scy += (ya + yb) * cr;
    xlo = fmin(xlo, xa); xhi = fmax(xhi, xa); ylo = fmin(ylo, ya); yhi = fmax(yhi, ya); wmin = fmin(wmin, w);
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double on = __shfl_down(rmin, off), ox = __shfl_down(rmax, off);
    const int oi = __shfl_down(imin, off), oj = __shfl_down(imax, off);
    if (on < rmin || (on == rmin && oi < imin)) { rmin = on; imin = oi; }
    if (ox > rmax || (ox == rmax && oj < imax)) { rmax = ox; imax = oj; }
    sr += __shfl_down(sr, off); srr += __shfl_down(srr, off); sc += __shfl_down(sc, off);
    scx += __shfl_down(scx, off); scy += __shfl_down(scy, off);
    xlo = fmin(xlo, __shfl_down(xlo, off)); xhi = fmax(xhi, __shfl_down(xhi, off));
    ylo = fmin(ylo, __shfl_down(ylo, off)); yhi = fmax(yhi, __shfl_down(yhi, off));
    wmin = fmin(wmin, __shfl_down(wmin, off));
  }
  if (lane == 0) {
    r->r_min = rmin; r->r_max = rmax; r->r_mean = sr / (double)A; r->area = half_sin_step * srr;
    r->centroid[0] = sc != 0.0 ? scx / (3.0 * sc) : 0.0; r->centroid[1] = sc != 0.0 ? scy / (3.0 * sc) : 0.0;
    r->extent_x[0] = xlo; r->extent_x[1] = xhi; r->extent_y[0] = ylo; r->extent_y[1] = yhi; r->wall_min = wmin;
    r->a_min = imin; r->a_max = imax; r->n_hit = nh; r->status = 0;
  }
}

__global__ void __launch_bounds__(SH_STEM_THREADS)
k_stem_fit(const double* __restrict__ planes /* B x P x 6 */, const int* __restrict__ cut_status /* B x P */, const sh_resection* __restrict__ recs /* B x P */,
           const double* __restrict__ frames /* B x 16 */, const int* __restrict__ hstatus /* B */, const double* __restrict__ near /* B x L x A */,
           const sh_canal_level* __restrict__ levels /* B x L */, const double* __restrict__ dirs /* A x 2 */, double z0, double dz, int L, int A,
           const sh_stem* __restrict__ stems, int K, int P, sh_stem_fit* __restrict__ out /* B x P x K */) {
  static_assert(sizeof(sh_stem_fit) == 16 * 8, "sh_stem_fit is 13 doubles and six int32");
  const int cut = blockIdx.x, b = cut / P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  sh_stem_fit* const dst = out + (size_t)cut * K;
  const double* T = frames + 16 * (size_t)b;
  int status = hstatus[b];
  if (status == 0) status = cut_status[cut];
  if (status == 0) status = recs[cut].status;
  double of[3], un[3], entry[3], ze = 0.0;
  if (status == 0) status = stem_entry(T, planes + 6 * (size_t)cut, planes + 6 * (size_t)cut + 3, of, un, &ze, entry);
  if (status != 0) {      // (uniform) the status, nothing else
    for (int i = tid; i < K * 16; i += SH_STEM_THREADS) {
      long long word = 0;
      if (i % 16 == 15) word = (long long)((unsigned long long)(unsigned)status << 32);      // (fits = 0 | status)
      ((long long*)dst)[i] = word;
    }
    return;
  }
  const double* nr = near + (size_t)b * L * A;
  const sh_canal_level* lv = levels + (size_t)b * L;
  for (int k = wave; k < K; k += SH_STEM_THREADS / 64) {
    const double len = stems[k].length, rp = stems[k].r_prox, rt = stems[k].r_tip;
    sh_stem_fit* r = dst + k;
    int l0, l1;
    if (!stem_level_span(z0, dz, L, ze, len, &l0, &l1)) {      // (uniform in the wave) the grid does not reach: nothing is extrapolated
      if (lane < 16) ((long long*)r)[lane] = lane == 15 ? (long long)((unsigned long long)(unsigned)SH_ERR_ARG << 32) : 0ll;
      continue;
    }
    const int total = l1 >= l0 ? (l1 - l0 + 1) * A : 0;      // <= 1 024 x 256
    double cmin = INFINITY, smin = INFINITY;
    int imin = 0x7fffffff, ns = 0, nbr = 0, nop = 0;
    for (int s = lane; s < total; s += 64) {
      const int li = s / A, a = s - li * A, l = l0 + li;
      const double d = stem_level_depth(z0, dz, l, ze), rr = stem_radius_at(len, rp, rt, d);
      if (!stem_sample_counts(rr, dirs[2 * a], dirs[2 * a + 1], z0 - (double)l * dz, of, un)) continue;
      ++ns;
      const double t = nr[(size_t)l * A + a];
      if (!(t < INFINITY)) { ++nop; continue; }
      const double cl = t - rr, sc = t / rr;
      if (cl < 0.0) ++nbr;
      if (cl < cmin) { cmin = cl; imin = s; }
      if (sc < smin) smin = sc;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double oc = __shfl_down(cmin, off);
      const int oi = __shfl_down(imin, off);
      if (oc < cmin || (oc == cmin && oi < imin)) { cmin = oc; imin = oi; }
      smin = fmin(smin, __shfl_down(smin, off));
      ns += __shfl_down(ns, off); nbr += __shfl_down(nbr, off); nop += __shfl_down(nop, off);
    }
    if (lane == 0) {      // (field by field: a local record would live in scratch)
      const double pi = 3.14159265358979323846;
      double fsum = 0.0, fmax_ = 0.0, fdepth = 0.0;
      int nf = 0;
      for (int l = l0; l <= l1; ++l) {
        const double area = lv[l].area;
        if (lv[l].status != 0 || !(area > 0.0)) continue;
        const double d = stem_level_depth(z0, dz, l, ze), rr = stem_radius_at(len, rp, rt, d);
        const double f = (pi * (rr * rr)) / area;
        fsum += f; ++nf;
        if (f > fmax_) { fmax_ = f; fdepth = d; }
      }
      const bool any = imin != 0x7fffffff;
      const int li = any ? imin / A : 0, a = any ? imin - li * A : -1;
      const double dv[3] = {any ? dirs[2 * a] : 0.0, any ? dirs[2 * a + 1] : 0.0, 0.0};
      double dc[3];
      canal_unmap_dir(T, dv, dc);
#pragma unroll
      for (int i = 0; i < 3; ++i) { r->entry[i] = entry[i]; r->direction[i] = any ? dc[i] : 0.0; }
      r->z_entry = ze;
      r->min_clearance = any ? cmin : 0.0;
      r->depth = any ? stem_level_depth(z0, dz, l0 + li, ze) : 0.0;
      r->scale_max = any ? smin : 0.0;
      r->fill_mean = nf > 0 ? fsum / (double)nf : 0.0;
      r->fill_max = fmax_; r->fill_max_depth = fdepth;
      r->angle_index = a; r->n_samples = ns; r->n_breach = nbr; r->n_open = nop;
      r->fits = (nbr == 0 && nop == 0 && ns > 0) ? 1 : 0;
      r->status = 0;
    }
  }
}

}  // namespace sh
