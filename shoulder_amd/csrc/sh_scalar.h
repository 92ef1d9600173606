// sh_scalar.h -- the small sequential stages of the path, one call per humerus / per slice row.
// Written once as SH_HD functions: on the product path they run inside device kernels (one
// lane per item, data in HBM); tests instantiate the same source on the host
// (tests/hostcheck) to compare against the oracle without a GPU.
#pragma once
#include "sh_common.h"

namespace sh {

// ======================================================================================
// K10  ruptures.KernelCPD(kernel="rbf").fit(x).predict(n_bkps=1)   surgical_neck.py:31-33
// gamma = 1/median(pairwise sq. distances); K = exp(-clip(gamma d^2, 1e-2, 1e2));
// t* = first argmin_{t in [2, n-2]} c(0,t)+c(t,n),  c(a,b) = sum K_ii - sum_{ij} K_ij/(b-a).
// ======================================================================================
#define SH_CPD_MAXN 64
SH_HD double kth_smallest(double* a, int n, int k) {  // quickselect, destroys a
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    double p = a[(lo + hi) >> 1];
    int i = lo, j = hi;
    while (i <= j) {
      while (a[i] < p) ++i;
      while (a[j] > p) --j;
      if (i <= j) { double t = a[i]; a[i] = a[j]; a[j] = t; ++i; --j; }
    }
    if (k <= j) hi = j; else if (k >= i) lo = i; else break;
  }
  return a[k];
}

// gamma by the median heuristic; pd: scratch >= n*(n-1)/2 doubles
SH_HD double cpd_gamma(const double* x, int n, double* pd) {
  int np_ = n * (n - 1) / 2;
  int c = 0;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) { double d = x[i] - x[j]; pd[c++] = d * d; }
  double med;
  if (np_ & 1) med = kth_smallest(pd, np_, np_ / 2);
  else { double a = kth_smallest(pd, np_, np_ / 2 - 1); double b = kth_smallest(pd, np_, np_ / 2); med = (a + b) / 2.0; }
  return (med == 0.0) ? 1.0 : 1.0 / med;
}
SH_HD double cpd_kernel(double xi, double xj, double gamma) {
  double d = xi - xj;
  double v = d * d * gamma;
  v = v < 1e-2 ? 1e-2 : (v > 1e2 ? 1e2 : v);
  return exp(-v);
}
// c(0,t) + c(t,n) for the Gram matrix K (n x n)
SH_HD double cpd_cost(const double* K, int n, int t) {
  double d0 = 0, s0 = 0, d1 = 0, s1 = 0;
  for (int i = 0; i < t; ++i) { d0 += K[i * n + i]; for (int j = 0; j < t; ++j) s0 += K[i * n + j]; }
  for (int i = t; i < n; ++i) { d1 += K[i * n + i]; for (int j = t; j < n; ++j) s1 += K[i * n + j]; }
  return (d0 - s0 / (double)t) + (d1 - s1 / (double)(n - t));
}
// scratch: >= n*(n-1)/2 + n*n doubles
SH_HD int cpd_one_bkp(const double* x, int n, double* scratch) {
  const int min_size = 2;
  double* K = scratch + n * (n - 1) / 2;
  double gamma = cpd_gamma(x, n, scratch);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) K[i * n + j] = cpd_kernel(x[i], x[j], gamma);
  int best_t = -1;
  double best = 1e300;
  for (int t = min_size; t <= n - min_size; ++t) {
    double cst = cpd_cost(K, n, t);
    if (cst < best) { best = cst; best_t = t; }
  }
  return best_t;
}

// ======================================================================================
// ProxObb canal range   mesh.py:181-190
// grad = np.gradient(savgol_filter(area, 3, 1)); canal = longest run (first of the longest) of consecutive sections
// with grad < 10.  savgol(3, 1): interior = mean of 3 (scipy's least-squares taps are 1/3 + 4e-17; tolerance-level),
// ends = the line fitted to the first / last three samples evaluated at the end ((5 y0 + 2 y1 - y2) / 6).
// tmp: 2 n doubles.  Returns 0 and lo = hi = 0 when no section qualifies.
// ======================================================================================
SH_HD int prox_canal_range(const double* area, int n, double* tmp, int* lo, int* hi) {
  double* sm = tmp;
  double* g = tmp + n;
  for (int i = 1; i + 1 < n; ++i) sm[i] = ((area[i - 1] + area[i]) + area[i + 1]) / 3.0;
  sm[0] = ((5.0 * area[0] + 2.0 * area[1]) - area[2]) / 6.0;
  sm[n - 1] = ((5.0 * area[n - 1] + 2.0 * area[n - 2]) - area[n - 3]) / 6.0;
  g[0] = sm[1] - sm[0];
  g[n - 1] = sm[n - 1] - sm[n - 2];
  for (int i = 1; i + 1 < n; ++i) g[i] = (sm[i + 1] - sm[i - 1]) / 2.0;
  int best_a = 0, best_len = 0, a = -1;
  for (int i = 0; i <= n; ++i) {
    const bool in = i < n && g[i] < 10.0;
    if (in && a < 0) a = i;
    if (!in && a >= 0) { if (i - a > best_len) { best_len = i - a; best_a = a; } a = -1; }
  }
  *lo = best_a; *hi = best_len > 0 ? best_a + best_len - 1 : best_a;
  return best_len;
}

// ======================================================================================
// K4  circle_fit.least_squares_circle residual   mesh.py:102
// minimise sum (R_i - mean R)^2 over the centre from the barycentre (Levenberg-Marquardt);
// returns residu = sum (R_i - mean R)^2 at the optimum.
// ======================================================================================
SH_HD double circle_residual_at(const double* xy, int n, double cx, double cy, double* g, double* H) {
  double sr = 0, sux = 0, suy = 0;
  for (int i = 0; i < n; ++i) {
    double dx = xy[2 * i] - cx, dy = xy[2 * i + 1] - cy;
    double r = sqrt(dx * dx + dy * dy);
    sr += r; sux += dx / r; suy += dy / r;
  }
  double rm = sr / n, mux = sux / n, muy = suy / n;
  double f2 = 0;
  if (g) { g[0] = g[1] = 0; H[0] = H[1] = H[2] = 0; }
  for (int i = 0; i < n; ++i) {
    double dx = xy[2 * i] - cx, dy = xy[2 * i + 1] - cy;
    double r = sqrt(dx * dx + dy * dy);
    double f = r - rm;
    f2 += f * f;
    if (g) {  // J_i = d f_i / d c = -(u_i - mean u)
      double jx = -(dx / r - mux), jy = -(dy / r - muy);
      g[0] += jx * f; g[1] += jy * f;
      H[0] += jx * jx; H[1] += jx * jy; H[2] += jy * jy;
    }
  }
  return f2;
}

SH_HD double circle_fit_residual(const double* xy, int n, double* cx_out = nullptr, double* cy_out = nullptr) {
  double cx = 0, cy = 0;
  for (int i = 0; i < n; ++i) { cx += xy[2 * i]; cy += xy[2 * i + 1]; }
  cx /= n; cy /= n;
  double lam = 1e-3, g[2], H[3];
  double f2 = circle_residual_at(xy, n, cx, cy, g, H);
  for (int it = 0; it < 200; ++it) {
    double a = H[0] * (1 + lam), b = H[1], d = H[2] * (1 + lam);
    double det = a * d - b * b;
    if (det == 0) break;
    double sx = -(d * g[0] - b * g[1]) / det, sy = -(-b * g[0] + a * g[1]) / det;
    double g2[2], H2[3];
    double f2n = circle_residual_at(xy, n, cx + sx, cy + sy, g2, H2);
    if (f2n <= f2) {
      cx += sx; cy += sy;
      bool done = (fabs(sx) + fabs(sy)) < 1e-13 * (1.0 + fabs(cx) + fabs(cy));
      f2 = f2n; g[0] = g2[0]; g[1] = g2[1]; H[0] = H2[0]; H[1] = H2[1]; H[2] = H2[2];
      lam *= 0.2;
      if (done) break;
    } else {
      lam *= 10.0;
      if (lam > 1e12) break;
    }
  }
  if (cx_out) { *cx_out = cx; *cy_out = cy; }
  return f2;
}

// ======================================================================================
// K12/K13  scipy.signal.savgol_filter(x, 10, 1) and find_peaks(height=-10, prominence=0.6,
// width=0.1)   bicipital_groove.py:107-118
// ======================================================================================
// savgol(10,1,mode="interp"): a 10-tap box mean over x[i-4 .. i+5] for i in [5, n-5) (scipy's
// lstsq-derived coefficients are 0.1 to within 3e-17 and differ in the last bit between
// LAPACK builds, so the canonical taps here are exactly 0.1: |y - scipy| <= 4e-15*|x|);
// the first / last 5 samples are a least-squares line through the first / last 10 samples
// (scipy _fit_edges_polyfit).
SH_HD double savgol10_1_at(const double* x, int i) {     // interior sample, 5 <= i < n-5
  double s = 0.0;
  for (int j = 0; j < 10; ++j) s += 0.1 * x[i - 4 + j];
  return s;
}
SH_HD void savgol10_1_edges(const double* x, int n, double* y);
SH_HD void savgol10_1(const double* x, int n, double* y) {
  for (int i = 5; i < n - 5; ++i) y[i] = savgol10_1_at(x, i);
  savgol10_1_edges(x, n, y);
}
SH_HD void savgol10_1_edges(const double* x, int n, double* y) {
  // edges: line fit a + b*t over t = 0..9
  for (int side = 0; side < 2; ++side) {
    const double* p = side == 0 ? x : x + (n - 10);
    double sy = 0, sty = 0;
    for (int t = 0; t < 10; ++t) { sy += p[t]; sty += t * p[t]; }
    // sum t = 45, sum t^2 = 285, n = 10: b = (10*sty - 45*sy)/(10*285 - 45*45), a = (sy - 45 b)/10
    double b = (10.0 * sty - 45.0 * sy) / 825.0;
    double a = (sy - 45.0 * b) / 10.0;
    if (side == 0) for (int t = 0; t < 5; ++t) y[t] = a + b * t;
    else for (int t = 5; t < 10; ++t) y[n - 10 + t] = a + b * t;
  }
}

struct Peak {
  int idx;
  double prominence, width, width_height;
};

// scipy _local_maxima_1d for one candidate start i (x[i-1] < x[i] is the caller's test): follows the
// plateau; returns the peak index (plateau midpoint) or -1, and the index the scan resumes from.
SH_HD int local_maximum_at(const double* x, int n, int i, int* resume) {
  const int i_max = n - 1;
  int ia = i + 1;
  while (ia < i_max && x[ia] == x[i]) ++ia;
  *resume = i;
  if (x[ia] < x[i]) { *resume = ia; return (i + (ia - 1)) / 2; }
  return -1;
}

// height / prominence (wlen=-1) / width (rel_height 0.5) filters of scipy.signal.find_peaks for one
// local maximum pk; true if it passes all three.
SH_HD bool peak_eval(const double* x, int n, int pk, double hmin, double pmin, double wmin, Peak* out) {
  if (!(x[pk] >= hmin)) return false;
  double left_min = x[pk], right_min = x[pk];
  int lb = pk, rb = pk, k = pk;
  while (0 <= k && x[k] <= x[pk]) { if (x[k] < left_min) { left_min = x[k]; lb = k; } --k; }
  k = pk;
  while (k <= n - 1 && x[k] <= x[pk]) { if (x[k] < right_min) { right_min = x[k]; rb = k; } ++k; }
  double prom = x[pk] - (left_min > right_min ? left_min : right_min);
  if (!(prom >= pmin)) return false;
  double h = x[pk] - prom * 0.5;
  k = pk;
  while (lb < k && h < x[k]) --k;
  double lip = (double)k;
  if (x[k] < h) lip += (h - x[k]) / (x[k + 1] - x[k]);
  k = pk;
  while (k < rb && h < x[k]) ++k;
  double rip = (double)k;
  if (x[k] < h) rip -= (h - x[k]) / (x[k - 1] - x[k]);
  double w = rip - lip;
  if (!(w >= wmin)) return false;
  out->idx = pk; out->prominence = prom; out->width = w; out->width_height = h;
  return true;
}

// Returns number of peaks written (all that pass the filters, ascending index), cap = capacity.
SH_HD int find_peaks_hpw(const double* x, int n, double hmin, double pmin, double wmin, Peak* out, int cap) {
  int np_ = 0;
  int i = 1, i_max = n - 1;
  while (i < i_max) {
    if (x[i - 1] < x[i]) {
      int resume;
      int pk = local_maximum_at(x, n, i, &resume);
      i = resume;
      if (pk >= 0) {
        Peak p;
        if (peak_eval(x, n, pk, hmin, pmin, wmin, &p)) {
          if (np_ < cap) out[np_] = p;
          ++np_;
        }
      }
    }
    ++i;
  }
  return np_;
}

// ======================================================================================
// K14  per-row peak features   bicipital_groove.py:102-156
// polar row: theta[M], r[M] = itr_centered_start (theta rolled to argmin, r about the slice
// AABB centre).  Writes up to 7 rows of raw features X_raw[.,9] and peak thetas.
// Feature order (:144-154): radius, nearest, next_nearest, z_scaled, prominence, width,
// width_height, canal_dist, n_peaks/7.
// scratch: 3*M doubles.
// ======================================================================================
#define SH_PEAK_CAP 256     // passing peaks of a row: 512 samples hold at most 255 strict local maxima, so the cap is never met
SH_HD int groove_features_from_peaks(const double* theta, const double* r, int M, double z, double z_scaled, const double* canal_u,
                                     Peak* pk, int np_, int amin, double* Xraw, double* peak_theta, int* peak_idx);
SH_HD double wrapped_abs_diff(double v, double a) { return fabs(atan2(sin(v - a), cos(v - a))); }

SH_HD int groove_row_features(const double* theta, const double* r, int M, double z, double z_scaled,
                              const double* canal_u /*3: unit(axis0-axis1), CT*/, double* scratch,
                              double* Xraw /*7x9*/, double* peak_theta /*7*/, int* peak_idx /*7*/) {
  double* neg0 = scratch;        // -(r - mean r)
  double* filt = scratch + M;    // savgol
  double* roll = scratch + 2 * M;
  // np.mean over M=512: NumPy pairwise summation (blocks of 128, 8 accumulators)
  double mean;
  {
    double tot = 0.0;
    // pairwise_sum for n = 512: split 256/256 -> 128/128 each; leaf (<=128) uses 8 partial sums
    double leaf[8];
    int nleaf = 0;
    for (int base = 0; base < M; base += 128) {
      int len = (M - base) < 128 ? (M - base) : 128;
      double a8[8];
      const double* p = r + base;
      double res;
      if (len < 8) { res = 0.0; for (int k = 0; k < len; ++k) res += p[k]; }
      else {
        for (int k = 0; k < 8; ++k) a8[k] = p[k];
        int k8;
        for (k8 = 8; k8 < len - (len % 8); k8 += 8)
          for (int k = 0; k < 8; ++k) a8[k] += p[k8 + k];
        res = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
        for (; k8 < len; ++k8) res += p[k8];
      }
      leaf[nleaf++] = res;
    }
    // combine leaves pairwise (valid for M = 512: ((l0+l1)+(l2+l3)); generic fallback sequential)
    if (nleaf == 4) tot = (leaf[0] + leaf[1]) + (leaf[2] + leaf[3]);
    else { tot = 0.0; for (int k = 0; k < nleaf; ++k) tot += leaf[k]; }
    mean = tot / (double)M;
  }
  for (int k = 0; k < M; ++k) neg0[k] = -1.0 * (r[k] - mean);
  savgol10_1(neg0, M, filt);
  int amin = 0;
  for (int k = 1; k < M; ++k) if (filt[k] < filt[amin]) amin = k;
  // np.roll(radius, -amin): roll[k] = filt[(k + amin) % M]
  for (int k = 0; k < M; ++k) roll[k] = filt[(k + amin) % M];
  Peak pk[SH_PEAK_CAP];
  int np_ = find_peaks_hpw(roll, M, -10.0, 0.6, 0.1, pk, SH_PEAK_CAP);
  if (np_ > SH_PEAK_CAP) np_ = SH_PEAK_CAP;
  return groove_features_from_peaks(theta, r, M, z, z_scaled, canal_u, pk, np_, amin, Xraw, peak_theta, peak_idx);
}

// Second half of the per-row work (bicipital_groove.py:121-156): pk = peaks of the rolled, filtered
// row that passed find_peaks (ascending index, np_ <= SH_PEAK_CAP; modified in place), amin = roll.
SH_HD int groove_features_from_peaks(const double* theta, const double* r, int M, double z, double z_scaled, const double* canal_u,
                                     Peak* pk, int np_, int amin, double* Xraw /*7x9*/, double* peak_theta /*7*/, int* peak_idx /*7*/) {
  // keep the 7 most prominent (B-5: ascending index order among the kept)
  if (np_ > SH_MAXPEAK) {
    bool keep[SH_PEAK_CAP];
    for (int k = 0; k < np_; ++k) keep[k] = false;
    for (int s = 0; s < SH_MAXPEAK; ++s) {
      int b = -1;
      for (int k = 0; k < np_; ++k)
        if (!keep[k] && (b < 0 || pk[k].prominence > pk[b].prominence)) b = k;
      keep[b] = true;
    }
    int w = 0;
    for (int k = 0; k < np_; ++k) if (keep[k]) pk[w++] = pk[k];
    np_ = SH_MAXPEAK;
  }
  double th[SH_MAXPEAK];
  for (int k = 0; k < np_; ++k) {
    int idx = (pk[k].idx + amin) % M;     // (peaks - rmin) % interp_num with rmin = -amin
    peak_idx[k] = idx;
    th[k] = theta[idx];
    peak_theta[k] = th[k];
  }
  for (int k = 0; k < np_; ++k) {
    double near = 0.0, next = 0.0;
    if (np_ > 1) {
      // sorted wrapped distances to all peaks, dropping those that round to 0.00 (:46)
      double a[SH_MAXPEAK];
      int na = 0;
      for (int j = 0; j < np_; ++j) {
        double d = wrapped_abs_diff(th[k], th[j]);
        if (rint(d * 100.0) / 100.0 != 0.0) a[na++] = d;     // np.round(angs, 2) != 0
      }
      for (int p = 1; p < na; ++p) { double v = a[p]; int q = p - 1; while (q >= 0 && a[q] > v) { a[q + 1] = a[q]; --q; } a[q + 1] = v; }
      near = na > 0 ? a[0] : nan("");
      if (np_ > 2) next = na > 1 ? a[1] : nan("");
    }
    double rad = r[peak_idx[k]];
    double px = rad * cos(th[k]), py = rad * sin(th[k]);
    double dx = px - canal_u[0] * z, dy = py - canal_u[1] * z;
    double* X = Xraw + k * 9;
    X[0] = rad; X[1] = near; X[2] = next; X[3] = z_scaled; X[4] = pk[k].prominence; X[5] = pk[k].width;
    X[6] = pk[k].width_height; X[7] = sqrt(dx * dx + dy * dy); X[8] = (double)np_ / 7.0;
  }
  return np_;
}

// K15  onnxruntime TreeEnsembleClassifier walk (bicipital_groove.py:178-181): P(class 1) as f32.
SH_HD float rfc_proba1(const int32_t* feat, const float* thr, const int32_t* ti, const int32_t* fi,
                       const float* leafw, const int32_t* roots, int n_trees, const double* x) {
  double s = 0.0;
  for (int t = 0; t < n_trees; ++t) {
    int c = roots[t];
    while (ti[c] >= 0) c = (x[feat[c]] <= (double)thr[c]) ? ti[c] : fi[c];
    s += (double)leafw[c];
  }
  return (float)s;
}

// K17  local radius minimum near bg_theta for one row (bicipital_groove.py:199-229).
// theta/r0 = row of polar_0 (theta, r - mean r).  Returns bg_i_local (may be negative: the
// reference then indexes from the end of the row).
SH_HD int groove_local_min(const double* theta, const double* r0, int M, double bg_theta, int ivar) {
  int esti = searchsorted_left(theta, M, bg_theta);
  if (esti == M) esti = M - 1;
  int best = 0;
  double bv = 0;
  bool first = true;
  int pos = 0;
  if (ivar > esti) {
    // polar_0[:, (esti-ivar):] (negative start = tail) ++ polar_0[:, :(esti+ivar)]
    int start = M + (esti - ivar);
    if (start < 0) start = 0;      // a Python slice start below -M clamps to the beginning of the row
    for (int k = start; k < M; ++k, ++pos) if (first || r0[k] < bv) { bv = r0[k]; best = pos; first = false; }
    for (int k = 0; k < esti + ivar && k < M; ++k, ++pos) if (first || r0[k] < bv) { bv = r0[k]; best = pos; first = false; }
  } else {
    int hi = esti + ivar < M ? esti + ivar : M;
    for (int k = esti - ivar; k < hi; ++k, ++pos) if (first || r0[k] < bv) { bv = r0[k]; best = pos; first = false; }
  }
  return best + (esti - ivar);
}

// ======================================================================================
// K22  LsqEllipse().fit(xy).as_parameters() centre   anatomic_neck.py:139-144
// (Halir & Flusser).  S = the 6x6 scatter of [x^2, xy, y^2, x, y, 1] (upper triangle used).
// ======================================================================================
SH_HD bool inv3(const double* A, double* Ai) {
  double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  if (det == 0.0) return false;
  double id = 1.0 / det;
  Ai[0] = c00 * id; Ai[1] = (A[2] * A[7] - A[1] * A[8]) * id; Ai[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  Ai[3] = c01 * id; Ai[4] = (A[0] * A[8] - A[2] * A[6]) * id; Ai[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  Ai[6] = c02 * id; Ai[7] = (A[1] * A[6] - A[0] * A[7]) * id; Ai[8] = (A[0] * A[4] - A[1] * A[3]) * id;
  return true;
}

// real eigenvalues of a real 3x3 (assumed to have 3 real eigenvalues, as Halir-Flusser's M has)
SH_HD int eigvals3_real(const double* M, double* ev) {
  double tr = M[0] + M[4] + M[8];
  double c1 = (M[0] * M[4] - M[1] * M[3]) + (M[0] * M[8] - M[2] * M[6]) + (M[4] * M[8] - M[5] * M[7]);
  double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  // l^3 - tr l^2 + c1 l - det = 0 ; substitute l = t + tr/3
  double a = tr / 3.0;
  double p = c1 - tr * tr / 3.0;
  double q = -2.0 * a * a * a + a * c1 - det;   // t^3 + p t + q = 0
  int n = 0;
  if (p >= 0) {  // one real root
    double t = 0;  // Newton from 0 works since monotone
    double sq = sqrt(q * q / 4.0 + p * p * p / 27.0);
    t = cbrt(-q / 2.0 + sq) + cbrt(-q / 2.0 - sq);
    ev[n++] = t + a;
  } else {
    double m = 2.0 * sqrt(-p / 3.0);
    double arg = 3.0 * q / (p * m);
    if (arg > 1) arg = 1;
    if (arg < -1) arg = -1;
    double th = acos(arg) / 3.0;
    for (int k = 0; k < 3; ++k) ev[n++] = m * cos(th - 2.0 * M_PI * k / 3.0) + a;
  }
  // Newton polish on the characteristic polynomial
  for (int k = 0; k < n; ++k) {
    double l = ev[k];
    for (int it = 0; it < 8; ++it) {
      double f = ((l - tr) * l + c1) * l - det;
      double df = (3.0 * l - 2.0 * tr) * l + c1;
      if (df == 0) break;
      double dl = f / df;
      l -= dl;
      if (fabs(dl) <= 1e-16 * fabs(l)) break;
    }
    ev[k] = l;
  }
  return n;
}

SH_HD bool ellipse_center_from_scatter(const double* S /*6x6 row-major, symmetric*/, double* cx, double* cy) {
  double S1[9], S2[9], S3[9], S3i[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { S1[i * 3 + j] = S[i * 6 + j]; S2[i * 3 + j] = S[i * 6 + 3 + j]; S3[i * 3 + j] = S[(3 + i) * 6 + 3 + j]; }
  if (!inv3(S3, S3i)) return false;
  // T = S3^-1 S2^T ; A = S1 - S2 T ; M = C1^-1 A with C1^-1 = [[0,0,.5],[0,-1,0],[.5,0,0]]
  double T[9], A[9], Mx[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += S3i[i * 3 + k] * S2[j * 3 + k]; T[i * 3 + j] = s; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += S2[i * 3 + k] * T[k * 3 + j]; A[i * 3 + j] = S1[i * 3 + j] - s; }
  for (int j = 0; j < 3; ++j) { Mx[j] = 0.5 * A[6 + j]; Mx[3 + j] = -A[3 + j]; Mx[6 + j] = 0.5 * A[j]; }
  double ev[3];
  int ne = eigvals3_real(Mx, ev);
  for (int e = 0; e < ne; ++e) {
    // eigenvector = cross product of two rows of (M - l I), pick the largest
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = Mx[i];
    R[0] -= ev[e]; R[4] -= ev[e]; R[8] -= ev[e];
    double v[3], best[3] = {0, 0, 0}, bn = -1;
    for (int a = 0; a < 3; ++a)
      for (int b = a + 1; b < 3; ++b) {
        cross3(R + 3 * a, R + 3 * b, v);
        double nn = dot3(v, v);
        if (nn > bn) { bn = nn; best[0] = v[0]; best[1] = v[1]; best[2] = v[2]; }
      }
    if (bn <= 0) continue;
    double cond = 4.0 * best[0] * best[2] - best[1] * best[1];
    if (cond > 0) {
      // a2 = -S3^-1 S2^T a1 = -T a1
      double a2[3];
      for (int i = 0; i < 3; ++i) a2[i] = -(T[i * 3] * best[0] + T[i * 3 + 1] * best[1] + T[i * 3 + 2] * best[2]);
      double a = best[0], b = best[1] / 2.0, c = best[2], d = a2[0] / 2.0, f = a2[1] / 2.0;
      double den = b * b - a * c;
      *cx = (c * d - b * f) / den;
      *cy = (a * f - b * d) / den;
      return true;
    }
  }
  return false;
}

// orthonormal basis of the plane with unit normal n (oracle fits.plane_basis)
SH_HD void plane_basis(const double* n, double* u, double* v) {
  int k = 0;
  if (fabs(n[1]) < fabs(n[k])) k = 1;
  if (fabs(n[2]) < fabs(n[k])) k = 2;
  double e[3] = {0, 0, 0};
  e[k] = 1.0;
  cross3(n, e, u);
  double l = norm3(u);
  for (int i = 0; i < 3; ++i) u[i] /= l;
  cross3(n, u, v);
}

// ======================================================================================
// K24/K25  trans-epicondylar helpers   epicondyle.py:33-81, utils.py:36-97
// ======================================================================================
// Convex hull of a simple closed polygon given as an open CCW vertex list (Melkman, O(n)).
// hull: capacity >= n+1 ints (indices into xy), returns count (CCW, no repeated end).
SH_HD double orient2(const double* a, const double* b, const double* c) {
  return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]);
}

// Andrew monotone chain on a copy of the indices (insertion sort by (x,y)); robust for any
// point set, n <= SH_MAXSEG.  idx: scratch n ints; hull: out capacity 2n.
SH_HD int convex_hull_2d(const double* xy, int n, int* idx, int* hull) {
  for (int i = 0; i < n; ++i) idx[i] = i;
  // shell sort by (x, y)
  for (int gap = n / 2; gap > 0; gap /= 2)
    for (int i = gap; i < n; ++i) {
      int t = idx[i];
      double tx = xy[2 * t], ty = xy[2 * t + 1];
      int j = i;
      while (j >= gap) {
        int u = idx[j - gap];
        double ux = xy[2 * u], uy = xy[2 * u + 1];
        if (ux > tx || (ux == tx && uy > ty)) { idx[j] = u; j -= gap; } else break;
      }
      idx[j] = t;
    }
  int k = 0;
  for (int i = 0; i < n; ++i) {
    while (k >= 2 && orient2(xy + 2 * hull[k - 2], xy + 2 * hull[k - 1], xy + 2 * idx[i]) <= 0) --k;
    hull[k++] = idx[i];
  }
  int lo = k + 1;
  for (int i = n - 2; i >= 0; --i) {
    while (k >= lo && orient2(xy + 2 * hull[k - 2], xy + 2 * hull[k - 1], xy + 2 * idx[i]) <= 0) --k;
    hull[k++] = idx[i];
  }
  return k - 1;
}

// Convex hull of a SIMPLE polygon given as an open vertex list in boundary order (Melkman's
// O(n) deque algorithm; collinear points are dropped like the monotone chain above does).
// dq: scratch 2n+2 ints; returns the hull size, hull vertices (CCW) in hull[0..).  Falls back to
// the sort-based hull when the first three vertices are collinear.
SH_HD int convex_hull_simple_polygon(const double* xy, int n, int* dq, int* hull) {
  if (n < 3) { for (int i = 0; i < n; ++i) hull[i] = i; return n; }
  double o = orient2(xy, xy + 2, xy + 4);
  if (o == 0.0) return convex_hull_2d(xy, n, dq, hull);
  int bot = n - 2, top = bot + 3;
  dq[bot] = dq[top] = 2;
  if (o > 0) { dq[bot + 1] = 0; dq[bot + 2] = 1; } else { dq[bot + 1] = 1; dq[bot + 2] = 0; }
  for (int i = 3; i < n; ++i) {
    const double* v = xy + 2 * i;
    if (orient2(xy + 2 * dq[bot], xy + 2 * dq[bot + 1], v) > 0 && orient2(xy + 2 * dq[top - 1], xy + 2 * dq[top], v) > 0) continue;
    while (top - bot >= 2 && orient2(xy + 2 * dq[bot], xy + 2 * dq[bot + 1], v) <= 0) ++bot;
    dq[--bot] = i;
    while (top - bot >= 2 && orient2(xy + 2 * dq[top - 1], xy + 2 * dq[top], v) <= 0) --top;
    dq[++top] = i;
  }
  int nh = top - bot;
  for (int k = 0; k < nh; ++k) hull[k] = dq[bot + k];
  return nh;
}

struct Rect2 {
  double cx, cy, mx, my, L, W, area;
};

// minimum-area rectangle over hull edges, first minimum in hull order (oracle te.min_area_rect)
SH_HD bool min_area_rect(const double* xy, const int* hull, int nh, Rect2* out) {
  bool have = false;
  for (int i = 0; i < nh; ++i) {
    const double* p = xy + 2 * hull[i];
    const double* q = xy + 2 * hull[(i + 1) % nh];
    double ex = q[0] - p[0], ey = q[1] - p[1];
    double ln = hypot(ex, ey);
    if (ln == 0) continue;
    ex /= ln; ey /= ln;
    double nx = -ey, ny = ex;
    double amin = 1e300, amax = -1e300, bmin = 1e300, bmax = -1e300;
    for (int k = 0; k < nh; ++k) {
      const double* h = xy + 2 * hull[k];
      double a = h[0] * ex + h[1] * ey, b = h[0] * nx + h[1] * ny;
      amin = a < amin ? a : amin; amax = a > amax ? a : amax;
      bmin = b < bmin ? b : bmin; bmax = b > bmax ? b : bmax;
    }
    double ea = amax - amin, eb = bmax - bmin, area = ea * eb;
    if (!have || area < out->area) {
      have = true;
      double ca = 0.5 * (amax + amin), cb = 0.5 * (bmax + bmin);
      out->cx = ex * ca + nx * cb; out->cy = ey * ca + ny * cb; out->area = area;
      if (ea >= eb) { out->mx = ex; out->my = ey; out->L = ea; out->W = eb; }
      else { out->mx = nx; out->my = ny; out->L = eb; out->W = ea; }
    }
  }
  return have;
}

// Area centroid of an open vertex list about its first vertex (oracle te._poly_centroid).
SH_HD void poly_centroid(const double* p, int n, double* cx, double* cy, double* area) {
  double a2 = 0, sx = 0, sy = 0;
  for (int i = 0; i < n; ++i) {
    int j = (i + 1) % n;
    double x = p[2 * i] - p[0], y = p[2 * i + 1] - p[1], xn = p[2 * j] - p[0], yn = p[2 * j + 1] - p[1];
    double cr = x * yn - xn * y;
    a2 += cr; sx += (x + xn) * cr; sy += (y + yn) * cr;
  }
  double a = a2 / 2.0;
  *area = a;
  *cx = p[0] + sx / (6.0 * a);
  *cy = p[1] + sy / (6.0 * a);
}

// Pieces of a simple CCW ring (open list, n points) inside {(p-c).m > w0}: centroids appended to
// cents (2 doubles each); returns the number of pieces.  scratch: >= (2n + 8*maxchains) doubles.
#define SH_TE_MAXCH 32
SH_HD int clip_halfplane_pieces(const double* pts, int n, double cx, double cy, double mx, double my, double w0,
                                double* cents, int cap, double* scratch) {
  double* poly = scratch;  // up to 2*(n+2*chains) doubles
  int start = -1;
  bool any_in = false, all_in = true;
  for (int i = 0; i < n; ++i) {
    bool in = ((pts[2 * i] - cx) * mx + (pts[2 * i + 1] - cy) * my - w0) > 0;
    any_in |= in; all_in &= in;
  }
  if (!any_in) return 0;
  if (all_in) { double a; if (cap > 0) poly_centroid(pts, n, cents, cents + 1, &a); return 1; }
  for (int i = 0; i < n && start < 0; ++i) {
    int j = (i + 1) % n;
    bool ii = ((pts[2 * i] - cx) * mx + (pts[2 * i + 1] - cy) * my - w0) > 0;
    bool jj = ((pts[2 * j] - cx) * mx + (pts[2 * j + 1] - cy) * my - w0) > 0;
    if (!ii && jj) start = i;
  }
  // chains: [begin, end) into poly plus s_in/s_out along the clip line
  int cb[SH_TE_MAXCH], ce[SH_TE_MAXCH];
  double sin_[SH_TE_MAXCH], sout[SH_TE_MAXCH];
  int nc = 0, np_ = 0;
  bool open = false;
  double px = -my, py = mx;
  for (int k = 0; k < n; ++k) {
    int i = (start + k) % n, j = (start + k + 1) % n;
    double fi = (pts[2 * i] - cx) * mx + (pts[2 * i + 1] - cy) * my - w0;
    double fj = (pts[2 * j] - cx) * mx + (pts[2 * j + 1] - cy) * my - w0;
    bool ii = fi > 0, jj = fj > 0;
    if (ii != jj) {
      double t = fi / (fi - fj);
      double x = pts[2 * i] + t * (pts[2 * j] - pts[2 * i]), y = pts[2 * i + 1] + t * (pts[2 * j + 1] - pts[2 * i + 1]);
      double s = (x - cx) * px + (y - cy) * py;
      if (jj) {
        if (nc >= SH_TE_MAXCH) return -1;
        cb[nc] = np_; sin_[nc] = s; open = true;
        poly[2 * np_] = x; poly[2 * np_ + 1] = y; ++np_;
        poly[2 * np_] = pts[2 * j]; poly[2 * np_ + 1] = pts[2 * j + 1]; ++np_;
      } else if (open) {
        poly[2 * np_] = x; poly[2 * np_ + 1] = y; ++np_;
        sout[nc] = s; ce[nc] = np_; ++nc; open = false;
      }
    } else if (jj && open) {
      poly[2 * np_] = pts[2 * j]; poly[2 * np_ + 1] = pts[2 * j + 1]; ++np_;
    }
  }
  // pair the crossings along the line: sort 2*nc events by s; (0,1),(2,3),...
  int ev_chain[2 * SH_TE_MAXCH], ev_out[2 * SH_TE_MAXCH];
  double ev_s[2 * SH_TE_MAXCH];
  int ne = 0;
  for (int c = 0; c < nc; ++c) { ev_s[ne] = sin_[c]; ev_chain[ne] = c; ev_out[ne] = 0; ++ne; ev_s[ne] = sout[c]; ev_chain[ne] = c; ev_out[ne] = 1; ++ne; }
  for (int a = 1; a < ne; ++a) {
    double s = ev_s[a]; int c = ev_chain[a], o = ev_out[a]; int b = a - 1;
    while (b >= 0 && ev_s[b] > s) { ev_s[b + 1] = ev_s[b]; ev_chain[b + 1] = ev_chain[b]; ev_out[b + 1] = ev_out[b]; --b; }
    ev_s[b + 1] = s; ev_chain[b + 1] = c; ev_out[b + 1] = o;
  }
  int next_after_out[SH_TE_MAXCH];
  for (int a = 0; a + 1 < ne; a += 2) {
    if (ev_out[a]) next_after_out[ev_chain[a]] = ev_chain[a + 1];
    if (ev_out[a + 1]) next_after_out[ev_chain[a + 1]] = ev_chain[a];
  }
  bool used[SH_TE_MAXCH];
  for (int c = 0; c < nc; ++c) used[c] = false;
  double* comp = poly + 2 * np_;
  int npieces = 0;
  for (int c0 = 0; c0 < nc; ++c0) {
    if (used[c0]) continue;
    int m = 0, c = c0;
    while (!used[c]) {
      used[c] = true;
      for (int k = cb[c]; k < ce[c]; ++k) { comp[2 * m] = poly[2 * k]; comp[2 * m + 1] = poly[2 * k + 1]; ++m; }
      c = next_after_out[c];
    }
    if (npieces < cap) { double a; poly_centroid(comp, m, cents + 2 * npieces, cents + 2 * npieces + 1, &a); }
    ++npieces;
  }
  return npieces;
}

// ---- HumeralHeadOsteotomy's plane bookkeeping (arthroplasty.py:13-175; oracle/osteotomy.py operation for operation) -------
// utils.unitxyz_to_spherical (utils.py:321-332): [r, azimuth, polar angle], degrees
SH_HD void unitxyz_to_spherical(const double* v, double* s) {
  s[0] = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  s[1] = atan2(v[1], v[0]) * (180.0 / M_PI);
  s[2] = acos(v[2] / s[0]) * (180.0 / M_PI);
}
// utils.spherical_to_unitxyz (utils.py:333-339)
SH_HD void spherical_to_unitxyz(const double* s, double* v) {
  const double th = s[1] * (M_PI / 180.0), ph = s[2] * (M_PI / 180.0);
  v[0] = s[0] * sin(ph) * cos(th);
  v[1] = s[0] * sin(ph) * sin(th);
  v[2] = s[0] * cos(ph);
}
// The resection plane in CT of a humerus with the anatomic-neck plane (p_ct, n_ct), the CT -> canal / articular matrix T_anp
// (bone.py:53-62) and side (0 left, 1 right) after the calls of `off` (the seven fields of sh_cut_offset in their order:
// offset_retroversion, offest_neckshaft, offset_depth canal / anp / resection, offset_anterior_posterior,
// offset_medial_lateral; arthroplasty.py:90-175), read back as `plane` with the humerus in CT (:33-40).  A field that is
// exactly 0 is a call that is not made.  False: T_anp is singular.
SH_HD bool resect_plane_from_offsets(const double* T_anp, const double* p_ct, const double* n_ct, int side, const double* off,
                                     double* out_p, double* out_n) {
  double p[3], n[3], an[3], s[3], Ti[16];
  xform_pt(T_anp, p_ct[0], p_ct[1], p_ct[2], p);                      // transform_plane (utils.py:191-206): point, then T[:3,:3] @ normal
  for (int i = 0; i < 3; ++i) { n[i] = (T_anp[4 * i] * n_ct[0] + T_anp[4 * i + 1] * n_ct[1]) + T_anp[4 * i + 2] * n_ct[2]; an[i] = n[i]; }
  if (off[0] != 0.0) { unitxyz_to_spherical(n, s); s[1] += side == 0 ? -off[0] : off[0]; spherical_to_unitxyz(s, n); }
  if (off[1] != 0.0) { unitxyz_to_spherical(n, s); s[2] += -off[1]; spherical_to_unitxyz(s, n); }
  if (off[2] != 0.0) p[2] += off[2];
  if (off[3] != 0.0) for (int i = 0; i < 3; ++i) p[i] = p[i] + off[3] * an[i];
  if (off[4] != 0.0) for (int i = 0; i < 3; ++i) p[i] = p[i] + off[4] * n[i];
  if (off[5] != 0.0) p[0] += side == 0 ? -off[5] : off[5];
  if (off[6] != 0.0) p[1] -= off[6];
  if (!inv_transform(T_anp, Ti)) return false;
  xform_pt(Ti, p[0], p[1], p[2], out_p);
  for (int i = 0; i < 3; ++i) out_n[i] = (Ti[4 * i] * n[0] + Ti[4 * i + 1] * n[1]) + Ti[4 * i + 2] * n[2];
  return true;
}

// ---- head sizing of a cut (include/shoulder_hip.h sh_head_fit; k_headfit.h) ------------------------------------------------
// The weighted algebraic least-squares sphere (bone_props.py:114-148 `_spherefit`, with weights) from the sixteen moment words
// of a cut: m[0] = S0, m[1..3] = S1, m[4..9] = S2 (xx, xy, xz, yy, yz, zz), m[10..12] = S3, m[13] = S4, coordinates q about
// the plane point.  The moments are shifted to the weighted centroid g = S1 / S0 first: there sum w p = 0, so the normal
// equations [[4 S2, 2 S1], [2 S1^T, S0]] [c; t] = [2 S3; tr S2] fall apart into 4 C c' = 2 K3 (C the covariance, K3 = E |p|^2 p)
// and t' = tr C; C is solved by a 3 x 3 Cholesky factorisation.  c = g + c' (about the plane point), r = sqrt(t' + |c'|^2),
// rms = sqrt(max(E, 0)) / (2 r) with E = K4 - 2 K3 . c' - (tr C)^2 the minimum of the objective per unit weight.
// A pivot at or below SH_HEADFIT_PIVOT x tr(S2) / S0 is not told from zero (false): the moments are sums of n <= 2^21 terms
// added in some fixed order, so each carries up to 4 n 2^-53 = 2^-30 of its sum of magnitudes, and the shift to the centroid
// subtracts numbers of the size tr(S2) / S0; 2^-26 leaves a factor 16 on that bound.  One operation order, sqrt and divisions
// only: the host instantiation (tests/hostcheck/headfit_check.cpp) gives the device's bits.
#define SH_HEADFIT_PIVOT 1.4901161193847656e-08      /* 2^-26 */
// The moments per unit weight about the weighted centroid g = S1 / S0 (S0 > 0): C the covariance (xx, xy, xz, yy, yz, zz),
// K3 = E |p|^2 p, K4 = E |p|^4, tr = tr(S2) / S0 (the size of the numbers the shift subtracts).
SH_HD void head_central_moments(const double* m, double* g, double* C, double* K3, double* K4, double* tr_out) {
  const double S0 = m[0];
  g[0] = m[1] / S0; g[1] = m[2] / S0; g[2] = m[3] / S0;
  const double M2[6] = {m[4] / S0, m[5] / S0, m[6] / S0, m[7] / S0, m[8] / S0, m[9] / S0};
  const double M3[3] = {m[10] / S0, m[11] / S0, m[12] / S0};
  const double M4 = m[13] / S0;
  const double tr = (M2[0] + M2[3]) + M2[5];
  const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
  C[0] = M2[0] - g[0] * g[0]; C[1] = M2[1] - g[0] * g[1]; C[2] = M2[2] - g[0] * g[2];
  C[3] = M2[3] - g[1] * g[1]; C[4] = M2[4] - g[1] * g[2]; C[5] = M2[5] - g[2] * g[2];
  const double Mg[3] = {(M2[0] * g[0] + M2[1] * g[1]) + M2[2] * g[2], (M2[1] * g[0] + M2[3] * g[1]) + M2[4] * g[2],
                        (M2[2] * g[0] + M2[4] * g[1]) + M2[5] * g[2]};
  for (int i = 0; i < 3; ++i) K3[i] = ((M3[i] - 2.0 * Mg[i]) - tr * g[i]) + 2.0 * gg * g[i];
  const double gM3 = (g[0] * M3[0] + g[1] * M3[1]) + g[2] * M3[2], gMg = (g[0] * Mg[0] + g[1] * Mg[1]) + g[2] * Mg[2];
  *K4 = (((M4 - 4.0 * gM3) + 4.0 * gMg) + 2.0 * gg * tr) - 3.0 * gg * gg;
  *tr_out = tr;
}
SH_HD bool head_sphere_from_moments(const double* m, double* c, double* r, double* rms) {
  c[0] = c[1] = c[2] = 0.0; *r = 0.0; *rms = 0.0;
  const double S0 = m[0];
  if (!(S0 > 0.0)) return false;
  double g[3], C[6], K3[3], K4, tr;
  head_central_moments(m, g, C, K3, &K4, &tr);
  const double Cxx = C[0], Cxy = C[1], Cxz = C[2], Cyy = C[3], Cyz = C[4], Czz = C[5];
  const double trC = (Cxx + Cyy) + Czz;
  // Cholesky C = L L^T, pivots against the size of the numbers the shift subtracted
  const double tiny = SH_HEADFIT_PIVOT * tr;
  if (!(Cxx > tiny)) return false;
  const double l00 = sqrt(Cxx), l10 = Cxy / l00, l20 = Cxz / l00;
  const double d1 = Cyy - l10 * l10;
  if (!(d1 > tiny)) return false;
  const double l11 = sqrt(d1), l21 = (Cyz - l20 * l10) / l11;
  const double d2 = (Czz - l20 * l20) - l21 * l21;
  if (!(d2 > tiny)) return false;
  const double l22 = sqrt(d2);
  // 4 C c' = 2 K3
  const double y0 = (0.5 * K3[0]) / l00, y1 = (0.5 * K3[1] - l10 * y0) / l11, y2 = ((0.5 * K3[2] - l20 * y0) - l21 * y1) / l22;
  const double c2 = y2 / l22, c1 = (y1 - l21 * c2) / l11, c0 = ((y0 - l10 * c1) - l20 * c2) / l00;
  const double r2 = trC + ((c0 * c0 + c1 * c1) + c2 * c2);
  if (!(r2 > 0.0) || !(r2 < 1e300)) return false;
  const double E = (K4 - 2.0 * ((K3[0] * c0 + K3[1] * c1) + K3[2] * c2)) - trC * trC;
  c[0] = g[0] + c0; c[1] = g[1] + c1; c[2] = g[2] + c2;
  *r = sqrt(r2);
  *rms = sqrt(E > 0.0 ? E : 0.0) / (2.0 * *r);
  return true;
}

// The ellipse with the area second moments of a polygon from its six shoelace sums about the in-plane origin: rm[0] = sum cr
// (cr = x0 y1 - x1 y0; twice the signed area), rm[1] = sum (x0 + x1) cr, rm[2] = sum (y0 + y1) cr, rm[3] = sum cr (x0^2 + x0 x1
// + x1^2), rm[4] = the same in y, rm[5] = sum cr (x0 y1 + 2 x0 y0 + 2 x1 y1 + x1 y0).  The second-moment tensor about the area
// centroid divided by the area has eigenvalues l1 >= l2; semi-axes 2 sqrt(l1), 2 sqrt(l2); dir = unit eigenvector of l1 in the
// (x, y) basis ((1, 0) when the two are equal).  False: no area or a tensor that is not positive.
SH_HD bool ellipse_from_moments(const double* rm, double* semi_major, double* semi_minor, double* dir) {
  *semi_major = 0.0; *semi_minor = 0.0; dir[0] = 0.0; dir[1] = 0.0;
  const double a2 = rm[0];
  if (!(a2 != 0.0)) return false;
  const double cx = rm[1] / (3.0 * a2), cy = rm[2] / (3.0 * a2);
  const double mxx = rm[3] / (6.0 * a2) - cx * cx, myy = rm[4] / (6.0 * a2) - cy * cy, mxy = rm[5] / (12.0 * a2) - cx * cy;
  const double mean = 0.5 * (mxx + myy), d = 0.5 * (mxx - myy), rad = sqrt(d * d + mxy * mxy);
  const double l1 = mean + rad, l2 = mean - rad;
  if (!(l2 > 0.0) || !(l1 < 1e300)) return false;
  double vx = 1.0, vy = 0.0;
  if (rad > 0.0) {
    if (d >= 0.0) { vx = d + rad; vy = mxy; } else { vx = mxy; vy = rad - d; }
    const double vl = sqrt(vx * vx + vy * vy);
    vx /= vl; vy /= vl;
  }
  *semi_major = 2.0 * sqrt(l1); *semi_minor = 2.0 * sqrt(l2);
  dir[0] = vx; dir[1] = vy;
  return true;
}

// ---- seating an implant head on a cut (include/shoulder_hip.h sh_seat; k_seat.h) -------------------------------------------
// All in the cut's in-plane basis, coordinates about the seat centre s: a = p - s, b = q - s for the directed ring edge p -> q.
// The edge's term of area(polygon n disk of radius rho about s) by Green's theorem: the roots t_lo < t_hi of |a + t (b - a)|^2 =
// rho^2 cut [0, 1] into at most three pieces; the piece inside [t_lo, t_hi] is a chord of the polygon inside the disk and gives
// cross(x, y) / 2, every other piece follows the circle and gives the sector rho^2 atan2(cross(x, y), dot(x, y)) / 2 (x, y the
// piece's ends).  Pieces are told apart by the roots alone: a discriminant <= 0 (the line misses or touches the circle) is a
// sector over the whole edge.  The sum over the ring is the signed area.
SH_HD double seat_edge_term(double ax, double ay, double bx, double by, double rho2) {
  const double dx = bx - ax, dy = by - ay;
  const double A = dx * dx + dy * dy, Bh = ax * dx + ay * dy, Cc = (ax * ax + ay * ay) - rho2;
  const double disc = Bh * Bh - A * Cc;
  double c0 = 0.0, c1 = 0.0;      // the chord piece [c0, c1] of [0, 1]; empty when c0 >= c1
  if (disc > 0.0) {
    const double sq = sqrt(disc), tlo = (-Bh - sq) / A, thi = (-Bh + sq) / A;
    c0 = tlo > 0.0 ? tlo : 0.0; c1 = thi < 1.0 ? thi : 1.0;
  }
  if (!(c0 < c1)) return (0.5 * rho2) * atan2(ax * by - ay * bx, ax * bx + ay * by);
  const double x0 = ax + c0 * dx, y0 = ay + c0 * dy, x1 = c1 < 1.0 ? ax + c1 * dx : bx, y1 = c1 < 1.0 ? ay + c1 * dy : by;
  double t = 0.5 * (x0 * y1 - y0 * x1);
  if (c0 > 0.0) t += (0.5 * rho2) * atan2(ax * y0 - ay * x0, ax * x0 + ay * y0);
  if (c1 < 1.0) t += (0.5 * rho2) * atan2(x1 * by - y1 * bx, x1 * bx + y1 * by);
  return t;
}
// squared distance from the origin (the seat centre) to the segment a -> b, and the nearest point
SH_HD double seat_seg_dist2(double ax, double ay, double bx, double by, double* nx, double* ny) {
  const double dx = bx - ax, dy = by - ay, dd = dx * dx + dy * dy;
  double t = dd > 0.0 ? -(ax * dx + ay * dy) / dd : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double x = t < 1.0 ? ax + t * dx : bx, y = t < 1.0 ? ay + t * dy : by;
  *nx = x; *ny = y;
  return x * x + y * y;
}
// the edge's term of the winding number of the ring about the origin (crossings of the positive x axis' line y = 0, signed)
SH_HD int seat_winding_term(double ax, double ay, double bx, double by) {
  const double cr = ax * by - ay * bx;
  if (ay <= 0.0) return (by > 0.0 && cr > 0.0) ? 1 : 0;
  return (by <= 0.0 && cr < 0.0) ? -1 : 0;
}
// sqrt(sum w (|q - c|^2 - R^2)^2 / S0) / (2 R) from the sixteen moment words of a cut (head_sphere_from_moments' layout, c about
// the plane point): the first-order radial rms of the head piece's samples against the sphere (c, R).  Formed about the weighted
// centroid: with c' = c - g and t = R^2 - |c'|^2 the mean of (|p|^2 - 2 c'.p - t)^2 is K4 - 4 c'.K3 + 4 c'^T C c' - 2 t tr C + t^2
// (E p = 0), which for the fitted sphere (4 C c' = 2 K3, t = tr C) is head_sphere_from_moments' E.  0 for an empty piece.
SH_HD double seat_surface_rms(const double* m, const double* c, double R) {
  if (!(m[0] > 0.0) || !(R > 0.0)) return 0.0;
  double g[3], C[6], K3[3], K4, tr;
  head_central_moments(m, g, C, K3, &K4, &tr);
  const double c0 = c[0] - g[0], c1 = c[1] - g[1], c2 = c[2] - g[2];
  const double trC = (C[0] + C[3]) + C[5];
  const double t = R * R - ((c0 * c0 + c1 * c1) + c2 * c2);
  const double Cc[3] = {(C[0] * c0 + C[1] * c1) + C[2] * c2, (C[1] * c0 + C[3] * c1) + C[4] * c2, (C[2] * c0 + C[4] * c1) + C[5] * c2};
  const double E = (((K4 - 4.0 * ((K3[0] * c0 + K3[1] * c1) + K3[2] * c2)) + 4.0 * ((Cc[0] * c0 + Cc[1] * c1) + Cc[2] * c2)) - 2.0 * t * trC) + t * t;
  return sqrt(E > 0.0 ? E : 0.0) / (2.0 * R);
}

// ---- canal profile and stems below a cut (include/shoulder_hip.h sh_canal_profile / sh_resect_stems; k_stem.h) -------------
// A point into the canal frame T (row-major 4 x 4, CT -> frame), in this order of operations on host and device.
SH_HD void canal_map_point(const double* T, double x, double y, double z, double* q) {
  q[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  q[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  q[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}
// a direction into the frame (rotation part), and a frame direction back into CT (its transpose)
SH_HD void canal_map_dir(const double* T, const double* v, double* q) {
  q[0] = (T[0] * v[0] + T[1] * v[1]) + T[2] * v[2];
  q[1] = (T[4] * v[0] + T[5] * v[1]) + T[6] * v[2];
  q[2] = (T[8] * v[0] + T[9] * v[1]) + T[10] * v[2];
}
SH_HD void canal_unmap_dir(const double* T, const double* v, double* q) {
  q[0] = (T[0] * v[0] + T[4] * v[1]) + T[8] * v[2];
  q[1] = (T[1] * v[0] + T[5] * v[1]) + T[9] * v[2];
  q[2] = (T[2] * v[0] + T[6] * v[1]) + T[10] * v[2];
}
// Moller-Trumbore of the ray o + t d against the triangle (A, B, C), k_rays_hit's statement (k_anp.h) operation by operation:
// |det| > 1e-12, u >= 0, w >= 0, u + w <= 1 closed, t > 1e-9
SH_HD bool canal_ray_hit(const double* o, const double* d, const double* A, const double* B, const double* C, double* t_out) {
  const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  const double e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  const double tv[3] = {o[0] - A[0], o[1] - A[1], o[2] - A[2]};
  double qv[3], pv[3];
  cross3(tv, e1, qv);
  cross3(d, e2, pv);
  const double det = dot3(e1, pv);
  if (!(fabs(det) > 1e-12)) return false;
  const double inv = 1.0 / det;
  const double uu = dot3(tv, pv) * inv;
  const double ww = dot3(d, qv) * inv;
  const double t = dot3(e2, qv) * inv;
  if (!(uu >= 0 && ww >= 0 && uu + ww <= 1 && t > 1e-9)) return false;
  *t_out = t;
  return true;
}
// The same statement for a triangle kept as (A, e1 = B - A, e2 = C - A), which also returns det's sign (include/shoulder_hip.h
// sh_ray_hit.side: +1 when det > 0, the ray runs against the face's normal; -1 otherwise).  Verdict and t are canal_ray_hit's bits:
// the edges are the differences it takes first, everything behind them is its operations in its order (k_rays.h; -ffp-contract=off).
SH_HD bool ray_tri_hit(const double* o, const double* d, const double* A, const double* e1, const double* e2, double* t_out, int* side_out) {
  const double tv[3] = {o[0] - A[0], o[1] - A[1], o[2] - A[2]};
  double qv[3], pv[3];
  cross3(tv, e1, qv);
  cross3(d, e2, pv);
  const double det = dot3(e1, pv);
  if (!(fabs(det) > 1e-12)) return false;
  const double inv = 1.0 / det;
  const double uu = dot3(tv, pv) * inv;
  const double ww = dot3(d, qv) * inv;
  const double t = dot3(e2, qv) * inv;
  if (!(uu >= 0 && ww >= 0 && uu + ww <= 1 && t > 1e-9)) return false;
  *t_out = t;
  *side_out = det > 0 ? 1 : -1;
  return true;
}
SH_HD bool canal_ray_hit_side(const double* o, const double* d, const double* A, const double* B, const double* C, double* t_out, int* side_out) {
  const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  const double e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  return ray_tri_hit(o, d, A, e1, e2, t_out, side_out);
}
// hits of a ray order ascending by (t, face): total, a face is hit once (t is never NaN: it passed t > 1e-9)
SH_HD bool ray_key_less(double ta, int fa, double tb, int fb) { return ta < tb || (ta == tb && fa < fb); }
// The closest point of a triangle kept as (A, ab = B - A, ac = C - A) to p (include/shoulder_hip.h sh_closest_points, k_closest.h):
// the Voronoi-region walk of Ericson, Real-Time Collision Detection 5.1.5, the six dot products and the three products tested in his
// order -- vertex A, vertex B, edge AB, vertex C, edge CA, edge BC, interior.  bp = ap - ab and cp = ap - ac (B and C are never
// formed).  The point is q = A + ab u + ac w (tri_point); *region: 0 interior, 1 / 2 / 3 edge AB / BC / CA, 4 / 5 / 6 vertex A / B / C.
// Returns (p - q) . (p - q).  Every branch but the interior one gives a convex combination by its own guards; the interior branch of a
// collinear triangle divides by a sum of rounding noise and may return a number that is not finite, which closest_key_less never
// selects.  Operation by operation the statement of tests/closest_oracle.py (-ffp-contract=off).
SH_HD void tri_point(const double* A, const double* ab, const double* ac, double u, double w, double* q) {
  q[0] = (A[0] + ab[0] * u) + ac[0] * w;
  q[1] = (A[1] + ab[1] * u) + ac[1] * w;
  q[2] = (A[2] + ab[2] * u) + ac[2] * w;
}
SH_HD double closest_pt_tri(const double* p, const double* A, const double* ab, const double* ac, double* u_out, double* w_out, int* region_out) {
  const double ap[3] = {p[0] - A[0], p[1] - A[1], p[2] - A[2]};
  const double bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]};
  const double cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  double u, w;
  int region;
  if (d1 <= 0 && d2 <= 0) { u = 0.0; w = 0.0; region = 4; }
  else if (d3 >= 0 && d4 <= d3) { u = 1.0; w = 0.0; region = 5; }
  else {
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) { u = d1 / (d1 - d3); w = 0.0; region = 1; }
    else if (d6 >= 0 && d5 <= d6) { u = 0.0; w = 1.0; region = 6; }
    else {
      const double vb = d5 * d2 - d1 * d6;
      if (vb <= 0 && d2 >= 0 && d6 <= 0) { u = 0.0; w = d2 / (d2 - d6); region = 3; }
      else {
        const double va = d3 * d6 - d5 * d4, e = d4 - d3, g = d5 - d6;
        if (va <= 0 && e >= 0 && g >= 0) { w = e / (e + g); u = 1.0 - w; region = 2; }
        else { const double denom = 1.0 / ((va + vb) + vc); u = vb * denom; w = vc * denom; region = 0; }
      }
    }
  }
  double q[3];
  tri_point(A, ab, ac, u, w, q);
  const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  *u_out = u; *w_out = w; *region_out = region;
  return dot3(r, r);
}
// candidates order by (d2, face): total.  A d2 that is not finite (NaN or infinite) is below nothing and above everything: it never
// wins, whichever side it stands on
SH_HD bool closest_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
SH_HD bool closest_key_less(double d2a, int fa, double d2b, int fb) {
  if (!closest_finite(d2a)) return false;
  if (!closest_finite(d2b)) return true;
  return d2a < d2b || (d2a == d2b && fa < fb);
}
// the tiles [*t0, *t1) of split s of S of a humerus with `tiles` tiles: consecutive ranges that cover every tile exactly once (empty
// where S > tiles)
SH_HD void cp_split_range(int tiles, int S, int s, int* t0, int* t1) {
  *t0 = (int)(((long long)s * tiles) / S);
  *t1 = (int)(((long long)(s + 1) * tiles) / S);
}
// +1 when p lies on the side of the face its normal ab x ac points to (or in its plane), -1 otherwise; r = p - q
SH_HD int closest_side(const double* r, const double* ab, const double* ac) {
  double n[3];
  cross3(ab, ac, n);
  return dot3(r, n) >= 0 ? 1 : -1;
}
// The signed solid angle of the triangle (A, B, C) seen from p (include/shoulder_hip.h sh_winding_numbers, k_winding.h), Van Oosterom &
// Strackee, The solid angle of a plane triangle, 1983: with a = A - p, b = B - p, c = C - p, la = sqrt(a . a), lb, lc alike,
//   num = a . (b x c)          den = ((la * lb) * lc + (a . b) * lc) + ((a . c) * lb + (b . c) * la)          omega = 2.0 * atan2(num, den)
// in exactly this parenthesisation (dot3 and cross3 of sh_common.h), and omega = 0 when num == 0.0, whatever the sign of the zero and
// whatever den is: a point in the plane of a face gets nothing from that face.  Positive when p sees the corners clockwise, i.e. from
// behind a face whose normal (B - A) x (C - A) points away from p: a point inside an outward-oriented closed mesh collects + 4 pi.
// Operation by operation the statement of tests/winding_oracle.py (-ffp-contract=off); atan2 is the math library's.
SH_HD void solid_angle_terms(const double* p, const double* A, const double* B, const double* C, double* num, double* den) {
  const double a[3] = {A[0] - p[0], A[1] - p[1], A[2] - p[2]};
  const double b[3] = {B[0] - p[0], B[1] - p[1], B[2] - p[2]};
  const double c[3] = {C[0] - p[0], C[1] - p[1], C[2] - p[2]};
  const double la = sqrt(dot3(a, a)), lb = sqrt(dot3(b, b)), lc = sqrt(dot3(c, c));
  double bc[3];
  cross3(b, c, bc);
  *num = dot3(a, bc);
  *den = ((la * lb) * lc + dot3(a, b) * lc) + (dot3(a, c) * lb + dot3(b, c) * la);
}
SH_HD double solid_angle_tri(const double* p, const double* A, const double* B, const double* C) {
  double num, den;
  solid_angle_terms(p, A, B, C, &num, &den);
  return num == 0.0 ? 0.0 : 2.0 * atan2(num, den);
}
// the sum of the solid angles -> winding number, inside, status (the statement of k_wn_join): 4 pi is 4.0 * M_PI
SH_HD void winding_record(double sum, double* winding, int* inside, int* status, int err_geometry) {
  if (!(fabs(sum) <= 1.7976931348623157e308)) { *winding = 0.0; *inside = 0; *status = err_geometry; return; }      // (not finite)
  const double w = sum / (4.0 * M_PI);
  *winding = w; *inside = fabs(w) >= 0.5 ? 1 : 0; *status = 0;
}
// The levels a face with frame heights [zmin, zmax] can be hit at, z_l = z0 - l dz: z_l in [zmin, zmax] <=> (z0 - zmax) / dz <= l
// <= (z0 - zmin) / dz, rounded outwards and widened by one level each side (the full test decides), clamped to [0, L - 1];
// empty: *lo > *hi.  A superset of what canal_ray_hit accepts, never less.
SH_HD void canal_level_range(double z0, double dz, int L, double zmin, double zmax, int* lo, int* hi) {
  double a = floor((z0 - zmax) / dz) - 1.0, b = ceil((z0 - zmin) / dz) + 1.0;
  if (!(a > 0.0)) a = 0.0;
  if (!(b < (double)(L - 1))) b = (double)(L - 1);
  *lo = a > (double)L ? L : (int)a;
  *hi = b < -1.0 ? -1 : (int)b;
}
// The angle indices the projection (x, y)[3] of a face can be hit at from the axis, t_a = (2 pi a) / A: the arc of its three
// vertex angles taken about the first one, rounded outwards and widened by one index each side; *a0 in [0, A) the first index,
// *n the number of indices (they wrap: a0, a0 + 1, ... mod A).  A projection that holds the origin, has it on an edge or comes
// close to that (an arc of 3 rad or more; pi for the origin on an edge) takes all A angles, and so does an arc of A indices or more.
SH_HD void canal_angle_range(const double* x, const double* y, int A, int* a0, int* n) {
  const double pi = 3.14159265358979323846, two_pi = 2.0 * pi;
  const double p0 = atan2(y[0], x[0]);
  double d1 = atan2(y[1], x[1]) - p0, d2 = atan2(y[2], x[2]) - p0;
  d1 = d1 > pi ? d1 - two_pi : (d1 < -pi ? d1 + two_pi : d1);
  d2 = d2 > pi ? d2 - two_pi : (d2 < -pi ? d2 + two_pi : d2);
  const double lo = fmin(0.0, fmin(d1, d2)), hi = fmax(0.0, fmax(d1, d2));
  *a0 = 0; *n = A;
  if (!(hi - lo < 3.0)) return;
  const double step = two_pi / (double)A;
  const double s = floor((p0 + lo) / step) - 1.0, e = ceil((p0 + hi) / step) + 1.0;
  const double cnt = (e - s) + 1.0;
  if (!(cnt < (double)A)) return;
  const int si = (int)s;
  *a0 = ((si % A) + A) % A; *n = (int)cnt;
}
// radius of the frustum stem (length, r_prox, r_tip) at depth d below its entry
SH_HD double stem_radius_at(double length, double r_prox, double r_tip, double d) { return r_prox + ((r_tip - r_prox) * d) / length; }
// whether the stem's surface point (r ca, r sa, zl) lies on the retained side of the plane (of, un) given in the frame
SH_HD bool stem_sample_counts(double r, double ca, double sa, double zl, const double* of, const double* un) {
  const double dx = r * ca - of[0], dy = r * sa - of[1], dz = zl - of[2];
  return (dx * un[0] + dy * un[1]) + dz * un[2] <= 0.0;
}
// The plane (o, n) of a cut (CT) in the frame T: of its point, un its unit normal there, *ze the height at which the frame's z axis
// pierces it, entry that point in CT.  0, or SH_ERR_GEOMETRY when the plane does not meet the axis (|un_z| < 1e-12) or is not finite.
SH_HD int stem_entry(const double* T, const double* o, const double* n, double* of, double* un, double* ze, double* entry) {
  canal_map_point(T, o[0], o[1], o[2], of);
  canal_map_dir(T, n, un);
  const double len = norm3(un);
  if (!(len > 0.0) || !(len < 1e300)) return SH_ERR_GEOMETRY_DEV;
  un[0] /= len; un[1] /= len; un[2] /= len;
  if (!(fabs(un[2]) >= 1e-12)) return SH_ERR_GEOMETRY_DEV;
  const double z = of[2] + (of[0] * un[0] + of[1] * un[1]) / un[2];
  if (!(fabs(z) < 1e300)) return SH_ERR_GEOMETRY_DEV;
  *ze = z;
  const double back[3] = {0.0 - T[3], 0.0 - T[7], z - T[11]};
  canal_unmap_dir(T, back, entry);
  return 0;
}
// first and last level of the grid with 0 <= d_l <= length, d_l = ze - (z0 - l dz) as every user computes it (monotone in l);
// false when the grid does not reach from ze down to ze - length.  *l0 > *l1: no level falls inside.
SH_HD double stem_level_depth(double z0, double dz, int l, double ze) { return ze - (z0 - (double)l * dz); }
SH_HD bool stem_level_span(double z0, double dz, int L, double ze, double length, int* l0, int* l1) {
  if (!(z0 >= ze) || !(z0 - (double)(L - 1) * dz <= ze - length)) return false;
  double g = ceil((z0 - ze) / dz);
  int a = g < 0.0 ? 0 : (g > (double)(L - 1) ? L - 1 : (int)g);
  while (a > 0 && stem_level_depth(z0, dz, a - 1, ze) >= 0.0) --a;
  while (a < L && stem_level_depth(z0, dz, a, ze) < 0.0) ++a;
  g = floor((z0 - (ze - length)) / dz);
  int b = g < 0.0 ? 0 : (g > (double)(L - 1) ? L - 1 : (int)g);
  while (b < L - 1 && stem_level_depth(z0, dz, b + 1, ze) <= length) ++b;
  while (b >= 0 && stem_level_depth(z0, dz, b, ze) > length) --b;
  *l0 = a; *l1 = b;
  return true;
}

// ---- implant plans: cuts, heads and stems joined and ranked (include/shoulder_hip.h sh_resect_plan; k_plan.h) ---------------
// One part of a candidate's cost and whether the part passes its limits; the three compact arrays of k_plan_terms hold these.
struct __attribute__((aligned(16))) PlanTerm { double cost; int32_t feasible, pad; };
// signed distance, times |n|, of a vertex from the reference plane (o, n), the normal as given
SH_HD double plan_side(const double* o, const double* n, double x, double y, double z) {
  const double dx = x - o[0], dy = y - o[1], dz = z - o[2];
  return (dx * n[0] + dy * n[1]) + dz * n[2];
}
// the bound of the tuberosity side: s_v <= -(margin |n|)
SH_HD double plan_tuberosity_bound(double margin, const double* n) { return -(margin * norm3(n)); }
// whether the vertex (z, vid), vid >= 0, replaces the best so far (bvid < 0: none yet): the larger frame height, of equals the smaller id
SH_HD bool plan_ref_better(double z, int vid, double bz, int bvid) { return bvid < 0 || z > bz || (z == bz && vid < bvid); }
// The cut part of a cost: eccentricity = |seat_center - entry|, entry the point where the frame's z axis pierces the cut's plane
// (stem_entry, what k_stem_fit calls).  *ecc is 0 where the cut, its seat or its entry does not exist.
SH_HD PlanTerm plan_cut_term(double w_eccentricity, double max_eccentricity, double w_cor, int humerus_status, int cut_status, int n_loops,
                             int seat0_status, int sphere_status, const double* seat_center, const double* T, const double* o, const double* n,
                             double* ecc) {
  PlanTerm t = {0.0, 0, 0};
  *ecc = 0.0;
  double of[3], un[3], entry[3], ze = 0.0;
  if (humerus_status != 0 || cut_status != 0 || n_loops < 1 || seat0_status != 0 || stem_entry(T, o, n, of, un, &ze, entry) != 0) return t;
  const double d[3] = {seat_center[0] - entry[0], seat_center[1] - entry[1], seat_center[2] - entry[2]};
  *ecc = norm3(d);
  t.cost = w_eccentricity * *ecc;
  t.feasible = (!(w_cor > 0.0) || sphere_status == 0) && *ecc <= max_eccentricity ? 1 : 0;
  return t;
}
// The head part: vals = uncovered, overhang, cor, height, apex (3, CT), apex_z.  apex = seat_center + (h n) / |n|, h the head's
// thickness; height = |apex_z - head_apex_z| against the native apex of the humerus' reference.
SH_HD PlanTerm plan_head_term(double w_uncovered, double w_overhang, double w_cor, double w_height, double limit_overhang, double min_coverage,
                              double coverage, double max_overhang, const double* cor_shift, const double* seat_center, const double* n, double h,
                              const double* T, double head_apex_z, double* vals /* 8 */) {
  const double len = norm3(n);
  double q[3];
  vals[0] = 1.0 - coverage; vals[1] = max_overhang; vals[2] = norm3(cor_shift);
  for (int i = 0; i < 3; ++i) vals[4 + i] = seat_center[i] + (h * n[i]) / len;
  canal_map_point(T, vals[4], vals[5], vals[6], q);
  vals[7] = q[2];
  vals[3] = fabs(vals[7] - head_apex_z);
  PlanTerm t;
  t.cost = ((w_uncovered * vals[0] + w_overhang * vals[1]) + w_cor * vals[2]) + w_height * vals[3];
  t.feasible = (max_overhang <= limit_overhang && coverage >= min_coverage) ? 1 : 0;
  t.pad = 0;
  return t;
}
// The stem part: *fill = |fill_mean - fill_target|.
SH_HD PlanTerm plan_stem_term(double w_fill, double fill_target, double limit_clearance, int status, int fits, double min_clearance, double fill_mean,
                              double* fill) {
  *fill = fabs(fill_mean - fill_target);
  PlanTerm t;
  t.cost = w_fill * *fill;
  t.feasible = (status == 0 && fits == 1 && min_clearance >= limit_clearance) ? 1 : 0;
  t.pad = 0;
  return t;
}
// A candidate (p, k_h, k_s) from its three parts and its head's compatibility word: cost = (head + stem) + cut; feasible when the
// parts are, the cost is not NaN and bit k_s of the word is set.
SH_HD bool plan_candidate(const PlanTerm& cut, const PlanTerm& head, const PlanTerm& stem, unsigned long long compat_word, int ks, double* cost) {
  *cost = (head.cost + stem.cost) + cut.cost;
  return cut.feasible != 0 && head.feasible != 0 && stem.feasible != 0 && *cost == *cost && ((compat_word >> ks) & 1ull) != 0;
}
// the order of the ranking: ascending (cost, i), costs not NaN.  A total order: its minima do not depend on the reduction order.
SH_HD bool plan_key_less(double ca, int ia, double cb, int ib) { return ca < cb || (ca == cb && ia < ib); }

// ---- rigid registration of point sets onto the resident batch (include/shoulder_hip.h sh_register_points; k_icp.h) ----------
// Everything below is + - x / sqrt on float64 in the written order (-ffp-contract=off), restated by tests/icp_oracle.py.
// A row of sums has SH_ICP_TERMS doubles: [0] n, [1] sum e2; point metric [2..4] sum p', [5..7] sum q, [8 + 3 i + j] sum p'_i q_j;
// plane metric [2..22] the upper triangle of sum J J^T row by row (i <= j), [23..28] sum J r; the rest +0.0.  The centroid pass uses
// [0] and [2..4] (sum p over all input points).
#define SH_ICP_TERMS 32
#define SH_ICP_SWEEPS 12      // cyclic Jacobi sweeps of sym4_jacobi: fixed, converged or not
#define SH_ICP_METRIC_POINT 0
#define SH_ICP_METRIC_PLANE 1

// the terms of one pair: pm the moved point, q its closest point with its status, (ab, ac) the winning face (plane metric), c the pivot.
// A pair that is not accepted leaves +0.0 everywhere.
SH_HD void icp_pair_terms(int metric, const double* pm, const double* q, int status, double reject, const double* ab, const double* ac,
                          const double* c, double* t /* SH_ICP_TERMS */) {
  for (int i = 0; i < SH_ICP_TERMS; ++i) t[i] = 0.0;
  const double e[3] = {q[0] - pm[0], q[1] - pm[1], q[2] - pm[2]};
  const double e2 = dot3(e, e);
  bool acc = status == 0 && sqrt(e2) <= reject;
  double n[3] = {0.0, 0.0, 0.0};
  if (acc && metric == SH_ICP_METRIC_PLANE) {
    double nn[3];
    cross3(ab, ac, nn);
    const double len = sqrt(dot3(nn, nn));
    if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) acc = false;
    else { n[0] = nn[0] / len; n[1] = nn[1] / len; n[2] = nn[2] / len; }
  }
  if (!acc) return;
  t[0] = 1.0; t[1] = e2;
  if (metric == SH_ICP_METRIC_PLANE) {
    const double d[3] = {pm[0] - c[0], pm[1] - c[1], pm[2] - c[2]};
    double J[6];
    cross3(d, n, J);
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    const double r = dot3(e, n);
    int idx = 2;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) t[idx++] = J[i] * J[j];
    for (int i = 0; i < 6; ++i) t[23 + i] = J[i] * r;
  } else {
    for (int i = 0; i < 3; ++i) { t[2 + i] = pm[i]; t[5 + i] = q[i]; }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) t[8 + 3 * i + j] = pm[i] * q[j];
  }
}

// Cyclic Jacobi on a symmetric 4 x 4 (row-major, destroyed: its diagonal becomes the eigenvalues), V the eigenvectors in columns.
// SH_ICP_SWEEPS sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair whose a_pq is 0.0 is left alone; otherwise
// theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (sgn(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c,
// a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, and for the other k: a_kp' = c a_kp - s a_kq, a_kq' = s a_kp + c a_kq (mirrored);
// the same column update on V.
SH_HD void sym4_jacobi(double* A, double* V) {
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SH_ICP_SWEEPS; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[4 * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[4 * q + q] - A[4 * p + p]) / (2.0 * apq);
        const double at = fabs(theta);
        double t = 1.0 / (at + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[4 * p + p] = A[4 * p + p] - t * apq;
        A[4 * q + q] = A[4 * q + q] + t * apq;
        A[4 * p + q] = 0.0; A[4 * q + p] = 0.0;
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != q) {
            const double akp = A[4 * k + p], akq = A[4 * k + q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            A[4 * k + p] = np_; A[4 * p + k] = np_;
            A[4 * k + q] = nq_; A[4 * q + k] = nq_;
          }
          const double vkp = V[4 * k + p], vkq = V[4 * k + q];
          V[4 * k + p] = c * vkp - s * vkq;
          V[4 * k + q] = s * vkp + c * vkq;
        }
      }
}

SH_HD bool icp_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the rotation of a unit quaternion (w, x, y, z), row-major 3 x 3
SH_HD void quat_rot(double w, double x, double y, double z, double* R) {
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
// (R, t) as a row-major 4 x 4
SH_HD void icp_pack(const double* R, const double* t, double* D) {
  for (int i = 0; i < 3; ++i) { D[4 * i] = R[3 * i]; D[4 * i + 1] = R[3 * i + 1]; D[4 * i + 2] = R[3 * i + 2]; D[4 * i + 3] = t[i]; }
  D[12] = 0.0; D[13] = 0.0; D[14] = 0.0; D[15] = 1.0;
}

// Horn's closed form (Closed-form solution of absolute orientation using unit quaternions, 1987) from a row of point-metric sums:
// pbar = sum p' / n, qbar = sum q / n, S_ij = sum p'_i q_j - (sum p'_i) qbar_j, the symmetric N of S, its eigenvector of the largest
// eigenvalue (the first among equals) normalised with w >= 0, dt = qbar - R pbar.  false: N or the result is not finite.
SH_HD bool icp_horn_solve(const double* tot, double* D /* 16 */) {
  const double n = tot[0];
  double pb[3], qb[3], S[9];
  for (int i = 0; i < 3; ++i) { pb[i] = tot[2 + i] / n; qb[i] = tot[5 + i] / n; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S[3 * i + j] = tot[8 + 3 * i + j] - tot[2 + i] * qb[j];
  double N[16], V[16];
  N[0] = (S[0] + S[4]) + S[8]; N[1] = S[5] - S[7]; N[2] = S[6] - S[2]; N[3] = S[1] - S[3];
  N[5] = (S[0] - S[4]) - S[8]; N[6] = S[1] + S[3]; N[7] = S[6] + S[2];
  N[10] = (S[4] - S[0]) - S[8]; N[11] = S[5] + S[7];
  N[15] = (S[8] - S[0]) - S[4];
  N[4] = N[1]; N[8] = N[2]; N[12] = N[3]; N[9] = N[6]; N[13] = N[7]; N[14] = N[11];
  for (int i = 0; i < 16; ++i)
    if (!icp_finite(N[i])) return false;
  sym4_jacobi(N, V);
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (N[5 * i] > N[5 * best]) best = i;
  double w = V[best], x = V[4 + best], y = V[8 + best], z = V[12 + best];
  const double len = sqrt(((w * w + x * x) + y * y) + z * z);
  if (!(len > 0.0) || !icp_finite(len)) return false;
  w = w / len; x = x / len; y = y / len; z = z / len;
  if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  double R[9], t[3];
  quat_rot(w, x, y, z, R);
  for (int i = 0; i < 3; ++i) t[i] = qb[i] - ((R[3 * i] * pb[0] + R[3 * i + 1] * pb[1]) + R[3 * i + 2] * pb[2]);
  icp_pack(R, t, D);
  return true;
}

// Cholesky of a symmetric 6 x 6 given by its upper triangle row by row (21 doubles), in index order, and the solve of A x = b.
// Column j: s = A_jj - L_j0^2 - ... - L_j,j-1^2 (left to right); a pivot s that is <= 0 or not finite fails; L_jj = sqrt(s);
// below it L_ij = (A_ij - L_i0 L_j0 - ...) / L_jj.  Then L y = b forwards and L^T x = y backwards, the sums left to right with k
// ascending.  *min_pivot = min_j min(1, (L_jj L_jj) / A_jj): near 0 where the system is nearly singular.
SH_HD bool chol6_solve(const double* up, const double* b, double* x, double* min_pivot) {
  double A[36], L[36], y[6];
  int idx = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { A[6 * i + j] = up[idx]; A[6 * j + i] = up[idx]; ++idx; }
  for (int i = 0; i < 36; ++i) L[i] = 0.0;
  double mp = 1.0;
  for (int j = 0; j < 6; ++j) {
    double s = A[6 * j + j];
    for (int k = 0; k < j; ++k) s = s - L[6 * j + k] * L[6 * j + k];
    if (!(s > 0.0) || !icp_finite(s)) return false;
    const double l = sqrt(s);
    L[6 * j + j] = l;
    const double ratio = (l * l) / A[6 * j + j];
    if (ratio < mp) mp = ratio;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[6 * i + j];
      for (int k = 0; k < j; ++k) v = v - L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / l;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
    for (int k = 0; k < i; ++k) v = v - L[6 * i + k] * y[k];
    y[i] = v / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[6 * k + i] * x[k];
    x[i] = v / L[6 * i + i];
  }
  *min_pivot = mp;
  return true;
}

// the plane-metric update from a row of sums and the pivot c: x = (w, t) by chol6_solve, the rotation of the quaternion (1, w / 2)
// normalised, dt = (c - R c) + t
SH_HD bool icp_plane_solve(const double* tot, const double* c, double* D /* 16 */, double* min_pivot) {
  double x[6];
  if (!chol6_solve(tot + 2, tot + 23, x, min_pivot)) return false;
  const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
  const double len = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  if (!icp_finite(len)) return false;
  double R[9], t[3];
  quat_rot(1.0 / len, hx / len, hy / len, hz / len, R);
  for (int i = 0; i < 3; ++i) t[i] = (c[i] - ((R[3 * i] * c[0] + R[3 * i + 1] * c[1]) + R[3 * i + 2] * c[2])) + x[3 + i];
  icp_pack(R, t, D);
  return true;
}

// Tn = D T for two rigid 4 x 4 (last rows 0 0 0 1): the sums left to right, the translation added last
SH_HD void icp_compose(const double* D, const double* T, double* Tn) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) Tn[4 * i + j] = (D[4 * i] * T[j] + D[4 * i + 1] * T[4 + j]) + D[4 * i + 2] * T[8 + j];
    Tn[4 * i + 3] = Tn[4 * i + 3] + D[4 * i + 3];
  }
  Tn[12] = 0.0; Tn[13] = 0.0; Tn[14] = 0.0; Tn[15] = 1.0;
}

// Evaluation k of one humerus from its joined row of sums: report, then stop or step (include/shoulder_hip.h).  rec = {rms, rms_first,
// min_pivot} and irec = {pairs, iterations, converged, status} are the tail of its sh_registration: rec[0] comes in as the rms of
// evaluation k - 1.  T is the transform the sums were taken at; it is replaced only when an update is applied.  Returns 1 when the
// humerus is done.  rms = sqrt(sum e2 / n), and 0.0 when n = 0.
SH_HD int icp_step(int metric, int k, int max_iter, double tol, const double* tot, const double* cbar, double* T, double* rec, int* irec,
                   double* hist /* rms, pairs */) {
  const double n = tot[0];
  const double rms = n > 0.0 ? sqrt(tot[1] / n) : 0.0;
  const double prev = rec[0];
  hist[0] = rms; hist[1] = n;
  rec[0] = rms;
  if (k == 0) { rec[1] = rms; rec[2] = 1.0; }
  irec[0] = (int)n; irec[1] = k; irec[2] = 0; irec[3] = 0;
  if (k > 0 && fabs(prev - rms) <= tol) { irec[2] = 1; return 1; }
  if (k == max_iter) return 1;
  if (n < 6.0) { irec[3] = SH_ERR_GEOMETRY_DEV; return 1; }
  double D[16], Tn[16], mp = 1.0;
  bool ok;
  if (metric == SH_ICP_METRIC_PLANE) {
    double c[3];
    canal_map_point(T, cbar[0], cbar[1], cbar[2], c);
    ok = icp_plane_solve(tot, c, D, &mp);
  } else {
    ok = icp_horn_solve(tot, D);
  }
  if (ok) {
    icp_compose(D, T, Tn);
    for (int i = 0; i < 12; ++i) ok = ok && icp_finite(Tn[i]);
  }
  if (!ok) { irec[3] = SH_ERR_GEOMETRY_DEV; return 1; }
  rec[2] = mp;
  for (int i = 0; i < 16; ++i) T[i] = Tn[i];
  return 0;
}

// ---- mass properties of the resident batch (include/shoulder_hip.h sh_mass_properties; k_mass.h) ------------------------------
// Everything below is + - x / sqrt on float64 in the written order (-ffp-contract=off), restated by tests/mass_oracle.py.
// A row of sums has SH_MASS_TERMS doubles: [0] A2, [1..3] A2 s, [4..9] A2 m, [10..12] n, [13] d, [14..16] d s, [17..22] d m,
// [23] faces with A2 == 0.0; m runs over ij = 00, 01, 02, 11, 12, 22.
#define SH_MASS_TERMS 24
#define SH_MASS_DOUBLES 48      // the doubles of an sh_mass, in its order
#define SH_MASS_SWEEPS 12       // cyclic Jacobi sweeps of sym3_jacobi: fixed, converged or not

// twice the area of a face from its edges ab = B - A and ac = C - A, and its normal n = cross3(ab, ac) (mass properties, surface samples)
SH_HD double face_area2(const double* ab, const double* ac, double* n) {
  cross3(ab, ac, n);
  return sqrt(dot3(n, n));
}

// the terms of one face with the widened corners A, B, C, relative to the pivot o
SH_HD void mass_face_terms(const double* o, const double* A, const double* B, const double* C, double* t /* SH_MASS_TERMS */) {
  const double a[3] = {A[0] - o[0], A[1] - o[1], A[2] - o[2]};
  const double b[3] = {B[0] - o[0], B[1] - o[1], B[2] - o[2]};
  const double c[3] = {C[0] - o[0], C[1] - o[1], C[2] - o[2]};
  const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  const double ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  double n[3], bc[3], m[6];
  const double A2 = face_area2(ab, ac, n);
  const double s[3] = {(a[0] + b[0]) + c[0], (a[1] + b[1]) + c[1], (a[2] + b[2]) + c[2]};
  cross3(b, c, bc);
  const double d = dot3(a, bc);
  int idx = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) m[idx++] = ((s[i] * s[j] + a[i] * a[j]) + b[i] * b[j]) + c[i] * c[j];
  t[0] = A2; t[13] = d;
  for (int k = 0; k < 3; ++k) { t[1 + k] = A2 * s[k]; t[10 + k] = n[k]; t[14 + k] = d * s[k]; }
  for (int q = 0; q < 6; ++q) { t[4 + q] = A2 * m[q]; t[17 + q] = d * m[q]; }
  t[23] = A2 == 0.0 ? 1.0 : 0.0;
}

// sym4_jacobi for a symmetric 3 x 3 (row-major, destroyed: its diagonal becomes the eigenvalues), V the eigenvectors in columns:
// SH_MASS_SWEEPS sweeps over the pairs (0,1) (0,2) (1,2), the same theta, t, c and s, a pair whose a_pq is 0.0 left alone.
SH_HD void sym3_jacobi(double* A, double* V) {
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SH_MASS_SWEEPS; ++sweep)
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[3 * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[3 * q + q] - A[3 * p + p]) / (2.0 * apq);
        const double at = fabs(theta);
        double t = 1.0 / (at + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[3 * p + p] = A[3 * p + p] - t * apq;
        A[3 * q + q] = A[3 * q + q] + t * apq;
        A[3 * p + q] = 0.0; A[3 * q + p] = 0.0;
        for (int k = 0; k < 3; ++k) {
          if (k != p && k != q) {
            const double akp = A[3 * k + p], akq = A[3 * k + q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            A[3 * k + p] = np_; A[3 * p + k] = np_;
            A[3 * k + q] = nq_; A[3 * q + k] = nq_;
          }
          const double vkp = V[3 * k + p], vkq = V[3 * k + q];
          V[3 * k + p] = c * vkp - s * vkq;
          V[3 * k + q] = s * vkp + c * vkq;
        }
      }
}

// The frame of a symmetric 3 x 3 given by its upper triangle (00, 01, 02, 11, 12, 22): eigenvalues ascending or descending, among equal
// ones the first; axes[3 r + k] is component k of axis r.  Each of the first two axes is signed so that its component of largest
// magnitude is positive (the first among equals), the third is cross3(first, second).  false: something is not finite.
SH_HD bool mass_frame(const double* up, bool descending, double* eig /* 3 */, double* axes /* 9 */) {
  double A[9] = {up[0], up[1], up[2], up[1], up[3], up[4], up[2], up[4], up[5]}, V[9];
  for (int i = 0; i < 9; ++i)
    if (!icp_finite(A[i])) return false;
  sym3_jacobi(A, V);
  int ord[3] = {0, 1, 2};
  for (int i = 1; i < 3; ++i)      // insertion sort, stable: ties keep their order
    for (int j = i; j > 0; --j) {
      const double x = A[4 * ord[j]], y = A[4 * ord[j - 1]];
      if (!(descending ? x > y : x < y)) break;
      const int tmp = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = tmp;
    }
  for (int r = 0; r < 3; ++r) {
    eig[r] = A[4 * ord[r]];
    for (int k = 0; k < 3; ++k) axes[3 * r + k] = V[3 * k + ord[r]];
  }
  for (int r = 0; r < 2; ++r) {
    int big = 0;
    for (int k = 1; k < 3; ++k)
      if (fabs(axes[3 * r + k]) > fabs(axes[3 * r + big])) big = k;
    if (axes[3 * r + big] < 0.0)
      for (int k = 0; k < 3; ++k) axes[3 * r + k] = -axes[3 * r + k];
  }
  cross3(axes, axes + 3, axes + 6);
  bool ok = true;
  for (int r = 0; r < 3; ++r) ok = ok && icp_finite(eig[r]);
  for (int i = 0; i < 9; ++i) ok = ok && icp_finite(axes[i]);
  return ok;
}

// The record of one humerus from its totals T, the pivot o and its number of faces (include/shoulder_hip.h): rec is the doubles of
// an sh_mass in its order -- [0] area, [1] volume, [2] closure, [3..5] shell_centroid, [6..11] shell_cov, [12..14] shell_eig,
// [15..23] shell_axes, [24..26] center_mass, [27..35] inertia, [36..38] principal, [39..47] principal_axes -- and irec its int32:
// faces, degenerate, status, vstatus.  A part that fails leaves its fields +0.0.
SH_HD void mass_finish(const double* T, const double* o, int nf, double* rec /* SH_MASS_DOUBLES */, int* irec /* 4 */) {
  for (int i = 0; i < SH_MASS_DOUBLES; ++i) rec[i] = 0.0;
  irec[0] = nf; irec[1] = (int)T[23]; irec[2] = 0; irec[3] = 0;
  const double T0 = T[0], T13 = T[13];
  bool ok = nf > 0 && T0 != 0.0;
  if (ok) {
    const double area = T0 / 2.0;
    double cs[3], C[6], eig[3], axes[9];
    for (int k = 0; k < 3; ++k) cs[k] = T[1 + k] / (3.0 * T0);
    int q = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++q) C[q] = T[4 + q] / (12.0 * T0) - cs[i] * cs[j];
    const double closure = sqrt(dot3(T + 10, T + 10)) / T0;
    ok = icp_finite(area) && icp_finite(closure) && mass_frame(C, true, eig, axes);
    for (int k = 0; k < 3; ++k) ok = ok && icp_finite(cs[k] + o[k]);
    if (ok) {
      rec[0] = area; rec[2] = closure;
      for (int k = 0; k < 3; ++k) { rec[3 + k] = cs[k] + o[k]; rec[12 + k] = eig[k]; }
      for (int i = 0; i < 6; ++i) rec[6 + i] = C[i];
      for (int i = 0; i < 9; ++i) rec[15 + i] = axes[i];
    }
  }
  if (!ok) irec[2] = SH_ERR_GEOMETRY_DEV;
  bool vok = nf > 0 && T13 != 0.0;
  if (vok) {
    const double volume = T13 / 6.0;
    double cm[3], S[6], I[6], eig[3], axes[9];
    for (int k = 0; k < 3; ++k) cm[k] = T[14 + k] / (4.0 * T13);
    int q = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++q) S[q] = T[17 + q] / 120.0 - (volume * cm[i]) * cm[j];
    I[0] = S[3] + S[5]; I[1] = -S[1]; I[2] = -S[2]; I[3] = S[0] + S[5]; I[4] = -S[4]; I[5] = S[0] + S[3];
    vok = icp_finite(volume) && mass_frame(I, false, eig, axes);
    for (int k = 0; k < 3; ++k) vok = vok && icp_finite(cm[k] + o[k]);
    if (vok) {
      rec[1] = volume;
      for (int k = 0; k < 3; ++k) { rec[24 + k] = cm[k] + o[k]; rec[36 + k] = eig[k]; }
      rec[27] = I[0]; rec[28] = I[1]; rec[29] = I[2]; rec[30] = I[1]; rec[31] = I[3]; rec[32] = I[4]; rec[33] = I[2]; rec[34] = I[4]; rec[35] = I[5];
      for (int i = 0; i < 9; ++i) rec[39 + i] = axes[i];
    }
  }
  if (!vok) irec[3] = SH_ERR_GEOMETRY_DEV;
}

// ---- surface samples of the resident batch (include/shoulder_hip.h sh_sample_surface; k_sample.h) ----------------------------------
// Integer words, and + - x sqrt on float64 in the written order (-ffp-contract=off), restated by tests/sample_oracle.py.
#define SH_SAMP_REMOVED 0        // the states of the thinning are the values of sh_sample.keep
#define SH_SAMP_KEPT 1
#define SH_SAMP_UNDECIDED (-1)

// SplitMix64 as a counter generator: word n of a seed, and a word as a double in [0, 1) (its top 53 bits: the product is exact)
SH_HD unsigned long long samp_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
SH_HD unsigned long long samp_word(unsigned long long seed, unsigned long long n) { return samp_mix(seed + (n + 1ull) * 0x9E3779B97F4A7C15ull); }
SH_HD double samp_unit(unsigned long long w) { return (double)(w >> 11) * 1.1102230246251565e-16; }

// twice the area of the face with the widened corners A, B, C
SH_HD double samp_area2(const double* A, const double* B, const double* C) {
  const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  const double ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  double n[3];
  return face_area2(ab, ac, n);
}

// the scan of one block, in place and strictly in index order: s[0] = a[0], s[i] = s[i - 1] + a[i]
SH_HD void samp_scan_block(double* s, int n) {
  for (int i = 1; i < n; ++i) s[i] = s[i - 1] + s[i];
}

// the smallest f in [0, nf - 1] with cdf[f] > target, nf - 1 when there is none (nf >= 1, cdf non-decreasing)
SH_HD long long samp_search(const double* cdf, long long nf, double target) {
  long long lo = 0, hi = nf;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  return lo < nf ? lo : nf - 1;
}

// the point of the words' r1, r2 on the face with the widened corners A, B, C, folded into the triangle: out[0..2] the point, out[3] u, out[4] v
SH_HD void samp_point(const double* A, const double* B, const double* C, double r1, double r2, double* out /* 5 */) {
  if (r1 + r2 > 1.0) { r1 = 1.0 - r1; r2 = 1.0 - r2; }
  for (int k = 0; k < 3; ++k) {
    const double ab = B[k] - A[k], ac = C[k] - A[k];
    out[k] = A[k] + (r1 * ab + r2 * ac);
  }
  out[3] = r1; out[4] = r2;
}

// The round rule of the thinning for one undecided sample j.  samp_thin_see folds one candidate i < j -- its state at the start of the
// round and its squared distance to j -- into the flags (bit 0: a kept neighbour, bit 1: an undecided one); samp_thin_verdict is j's
// state after the round.  A kept neighbour decides j: the caller may stop looking.
SH_HD double samp_d2(const double* p, const double* q) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return (dx * dx + dy * dy) + dz * dz;
}
SH_HD int samp_thin_see(int flags, int state_i, double d2, double r2) {
  if (state_i == SH_SAMP_REMOVED || !(d2 < r2)) return flags;
  return flags | (state_i == SH_SAMP_KEPT ? 1 : 2);
}
SH_HD int samp_thin_verdict(int flags) { return (flags & 1) ? SH_SAMP_REMOVED : (flags & 2) ? SH_SAMP_UNDECIDED : SH_SAMP_KEPT; }

// ---- mesh topology of the resident batch (include/shoulder_hip.h sh_mesh_topology; k_topo.h) ----------------------------------------
// Integer rules, restated by tests/topo_oracle.py.  The adjacency codes are the header's SH_ADJ_* (k_topo.h holds them equal).
#define SH_TOPO_BORDER (-1)
#define SH_TOPO_NONMANIFOLD (-2)
#define SH_TOPO_DEGENERATE (-3)
#define SH_TOPO_NONE 0x7fffffff      // no neighbour's value: above every face index

// a face that takes no part: two equal indices (or an index outside the mesh, which an upload refuses: nothing is ever indexed by it)
SH_HD bool topo_degenerate(const int* f, int nv) {
  return f[0] == f[1] || f[1] == f[2] || f[0] == f[2] || f[0] < 0 || f[1] < 0 || f[2] < 0 || f[0] >= nv || f[1] >= nv || f[2] >= nv;
}

// the slot of the non-degenerate face g whose undirected edge is {a, c}, or -1
SH_HD int topo_edge_slot(const int* g, int a, int c) {
  for (int e = 0; e < 3; ++e) {
    const int x = g[e], y = g[e == 2 ? 0 : e + 1];
    if ((x == a && y == c) || (x == c && y == a)) return e;
  }
  return -1;
}

// Slot e of the non-degenerate face f: the users of its edge {a, c} = {f[e], f[(e + 1) % 3]} among the faces of `row`, the ascending row
// of a or of c (both hold every user).  -> the slot's adjacency value; *owner: f is the smallest user, at whose slot the edge is counted
// once; *same: two users and both traverse the edge from a to c (an inconsistent edge).
SH_HD int topo_slot(const int* faces, const int* row, int n, int f, int e, int* owner, int* same) {
  const int a = faces[3 * (size_t)f + e], c = faces[3 * (size_t)f + (e == 2 ? 0 : e + 1)];
  int users = 0, other = -1, first = -1;
  for (int i = 0; i < n; ++i) {
    const int g = row[i];
    if (topo_edge_slot(faces + 3 * (size_t)g, a, c) < 0) continue;
    if (users == 0) first = g;
    if (g != f) other = g;
    ++users;
  }
  *owner = first == f ? 1 : 0;
  *same = 0;
  if (users == 1) return SH_TOPO_BORDER;
  if (users != 2) return SH_TOPO_NONMANIFOLD;
  const int* g = faces + 3 * (size_t)other;
  *same = g[topo_edge_slot(g, a, c)] == a ? 1 : 0;
  return other;
}

// One face u in a Jacobi round of FastSV on the old array `in`: *self is the value for the new p[u] (g[u] and every g[v] of a neighbour),
// *hook the value for the new p[p[u]] (every g[v] of a neighbour; SH_TOPO_NONE without one).  -> 1 when either lowers its target below
// what the old array holds there (in[u], and in[p[u]] = g[u]): the round changed something.
SH_HD int topo_round(const int* in, const int* adj /* the 3 slots of u */, int u, int* self, int* hook) {
  const int pu = in[u], gu = in[pu];
  int h = SH_TOPO_NONE;
  for (int e = 0; e < 3; ++e) {
    const int v = adj[e];
    if (v < 0) continue;
    const int gv = in[in[v]];
    h = gv < h ? gv : h;
  }
  *self = gu < h ? gu : h;
  *hook = h;
  return (*self < pu || h < gu) ? 1 : 0;
}

// the rounds of a head (word r: round r - 1 changed something; word 0 is 1): the smallest R >= 1 with word R == 0, or max_rounds and
// *full = 1 when there is none up to max_rounds
SH_HD int topo_rounds(const int* head, int max_rounds, int* full) {
  for (int r = 1; r <= max_rounds; ++r)
    if (head[r] == 0) { *full = 0; return r; }
  *full = 1;
  return max_rounds;
}

// a float32 as an unsigned whose order is the floats' (-0 below +0), and back: minima and maxima by integer atomics
SH_HD unsigned topo_enc(float x) {
  unsigned u;
  __builtin_memcpy(&u, &x, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SH_HD float topo_dec(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// ---- vertex normals and discrete curvatures of the resident batch (include/shoulder_hip.h sh_vertex_fields; k_vert.h) ---------------
// float64, operation by operation in the written order (-ffp-contract=off), restated by tests/vert_oracle.py.  Everything but atan2 is
// + - x / sqrt, so only the fields an angle enters differ between two math libraries.  The flags and the weights are the header's
// SH_VERT_* (k_vert.h holds them equal).
#define SH_VTX_FACE 10          // doubles of a face record: n[3], A2, angle[3], cot[3]
#define SH_VTX_FIELDS 8         // doubles of a vertex: area, angle_sum, defect, gauss, mean, gauss_smooth, mean_smooth, 0.0
#define SH_VTX_USED 1
#define SH_VTX_BORDER 2
#define SH_VTX_NONMANIFOLD 4
#define SH_VTX_FLAT 8
#define SH_VTX_ANGLE 1          // the weight of the normals: 0 the faces' areas, 1 the corners' angles

SH_HD bool vert_finite(double x) { return x - x == 0.0; }

// the widened corners of face f of a mesh
SH_HD void vert_corners(const float* verts, const int* f, double P[3][3]) {
  for (int k = 0; k < 3; ++k)
    for (int c = 0; c < 3; ++c) P[k][c] = (double)verts[3 * (size_t)f[k] + c];
}

// The record of a face with the widened corners P: n, A2, the three angles and cotangents.  -> 1 and ten zeros when the face is flat
// (degenerate by its indices, or A2 zero or not finite).
SH_HD int vert_face(const double P[3][3], bool degenerate, double* rec /* SH_VTX_FACE */) {
  const double ab[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
  const double ac[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  double n[3];
  const double A2 = face_area2(ab, ac, n);
  if (degenerate || A2 == 0.0 || !vert_finite(A2)) {
    for (int i = 0; i < SH_VTX_FACE; ++i) rec[i] = 0.0;
    return 1;
  }
  rec[0] = n[0]; rec[1] = n[1]; rec[2] = n[2]; rec[3] = A2;
  for (int k = 0; k < 3; ++k) {
    const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const double e1[3] = {P[k1][0] - P[k][0], P[k1][1] - P[k][1], P[k1][2] - P[k][2]};
    const double e2[3] = {P[k2][0] - P[k][0], P[k2][1] - P[k][1], P[k2][2] - P[k][2]};
    const double d = dot3(e1, e2);
    rec[4 + k] = atan2(A2, d);
    rec[7 + k] = d / A2;
  }
  return 0;
}

// the corner of the non-degenerate face f that is v (v is one of them: f comes from v's row)
SH_HD int vert_corner(const int* f, int v) { return f[0] == v ? 0 : f[1] == v ? 1 : 2; }

// Vertex v of a mesh from its ascending row of n faces: the sums in the row's order, then normal[3], fields[0 .. 4] = area, angle_sum,
// defect, gauss, mean, and the flags.  `adj` and `frec` are the mesh's "topo.adj" and "vert.face".
SH_HD void vert_gather(const float* verts, const int* faces, const int* adj, const double* frec, const int* row, int n, int v, int weight,
                       double* normal, double* fields, int* flags_out) {
  double s = 0.0, angle_sum = 0.0, N[3] = {0.0, 0.0, 0.0}, L[3] = {0.0, 0.0, 0.0};
  int flags = n > 0 ? SH_VTX_USED : 0;
  const double Pv[3] = {(double)verts[3 * (size_t)v], (double)verts[3 * (size_t)v + 1], (double)verts[3 * (size_t)v + 2]};      // P_k of every face of the row
  for (int i = 0; i < n; ++i) {
    const int f = row[i];
    const int* fc = faces + 3 * (size_t)f;
    const int k = vert_corner(fc, v), k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const int a0 = adj[3 * (size_t)f + k], a1 = adj[3 * (size_t)f + k2];      // the slots of the edges {v, next} and {previous, v}
    if (a0 == SH_TOPO_BORDER || a1 == SH_TOPO_BORDER) flags |= SH_VTX_BORDER;
    if (a0 == SH_TOPO_NONMANIFOLD || a1 == SH_TOPO_NONMANIFOLD) flags |= SH_VTX_NONMANIFOLD;
    const double* r = frec + SH_VTX_FACE * (size_t)f;
    const double A2 = r[3];
    if (A2 == 0.0) { flags |= SH_VTX_FLAT; continue; }
    s += A2;
    angle_sum += r[4 + k];
    const double w = r[4 + k];
    for (int c = 0; c < 3; ++c) N[c] += weight == SH_VTX_ANGLE ? (r[c] / A2) * w : r[c];
    const float *p1 = verts + 3 * (size_t)fc[k1], *p2 = verts + 3 * (size_t)fc[k2];      // the corners again, by index: no array indexed by k
    const double c1 = r[7 + k1], c2 = r[7 + k2];
    for (int c = 0; c < 3; ++c) L[c] += c1 * (Pv[c] - (double)p2[c]) + c2 * (Pv[c] - (double)p1[c]);
  }
  const double len = sqrt(dot3(N, N));
  const bool unit = len != 0.0 && vert_finite(len);
  for (int c = 0; c < 3; ++c) normal[c] = unit ? N[c] / len : 0.0;
  const double area = s / 6.0;
  const double defect = ((flags & SH_VTX_BORDER) ? 3.141592653589793 : 6.283185307179586) - angle_sum;
  fields[0] = area; fields[1] = angle_sum;
  fields[2] = area == 0.0 ? 0.0 : defect;
  fields[3] = area == 0.0 ? 0.0 : defect / area;
  fields[4] = area == 0.0 ? 0.0 : dot3(L, normal) / (4.0 * area);
  *flags_out = flags;
}

// One Jacobi round of the smoothing at vertex v: the area-weighted mean over the non-flat faces of the row of the faces' means of the
// old values, for two planes at once (g: gauss, m: mean).  `a2` is the mesh's "vert.a2" (0.0: flat).
SH_HD void vert_smooth(const int* faces, const double* a2, const int* row, int n, const double* g, const double* m, double* g_out, double* m_out) {
  double den = 0.0, sg = 0.0, sm = 0.0;
  for (int i = 0; i < n; ++i) {
    const int f = row[i];
    const double A2 = a2[f];
    if (A2 == 0.0) continue;
    const int* fc = faces + 3 * (size_t)f;
    den += A2;
    sg += A2 * (((g[fc[0]] + g[fc[1]]) + g[fc[2]]) / 3.0);
    sm += A2 * (((m[fc[0]] + m[fc[1]]) + m[fc[2]]) / 3.0);
  }
  *g_out = den == 0.0 ? 0.0 : sg / den;
  *m_out = den == 0.0 ? 0.0 : sm / den;
}

// ---- geodesic distances and shortest paths on the resident batch (include/shoulder_hip.h sh_geodesic; k_geo.h) ----------------------
// float64, operation by operation in the written order (-ffp-contract=off), restated by tests/geo_oracle.py.  Nothing is
// transcendental: + - x / sqrt and comparisons, so the bytes are the same wherever the rule runs.  The modes and the codes of a
// predecessor are the header's SH_GEO_* (k_geo.h holds them equal).
#define SH_GEOD_FACE 6           // doubles of a face record: len[3], unf[3]
#define SH_GEOD_UNFOLD 1         // the mode with the unfolded diagonals (0: the mesh edges alone)
#define SH_GEOD_ROOT (-1)
#define SH_GEOD_NO_PRED (-2)
#define SH_GEOD_UNREACHED (-3)
#define SH_GEOD_NO_LABEL 0x7fffffff      // no list position: above every one

// the info record of a (mesh, set) pair as the device writes it: SH_GEO_INFO_BYTES of the header
struct GeoInfo { double far_dist; int reached, roots, no_pred, farthest, sweeps, status; };
static_assert(sizeof(GeoInfo) == 32, "GeoInfo");

SH_HD double geo_inf() { return __builtin_huge_val(); }

// The record of face f of a mesh and the vertex across each of its slots (-1 where the slot has no face behind it).  `faces` and `adj`
// are the mesh's; a degenerate face has six +inf.
SH_HD void geo_face(const float* verts, const int* faces, const int* adj, int f, bool degenerate, double* rec /* SH_GEOD_FACE */, int* opp /* 3 */) {
  const double inf = geo_inf();
  for (int e = 0; e < 3; ++e) { rec[e] = inf; rec[3 + e] = inf; opp[e] = -1; }
  if (degenerate) return;
  const int* fc = faces + 3 * (size_t)f;
  for (int e = 0; e < 3; ++e) {
    const int a = fc[e], b = fc[e == 2 ? 0 : e + 1], p = fc[e == 0 ? 2 : e - 1];
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const float *vl = verts + 3 * (size_t)lo, *vh = verts + 3 * (size_t)hi;
    const double Pl[3] = {(double)vl[0], (double)vl[1], (double)vl[2]};
    const double E[3] = {(double)vh[0] - Pl[0], (double)vh[1] - Pl[1], (double)vh[2] - Pl[2]};
    const double l = sqrt(dot3(E, E));
    rec[e] = l;
    const int g = adj[3 * (size_t)f + e];
    if (g < 0) continue;
    const int* gc = faces + 3 * (size_t)g;
    const int q = (int)((long long)gc[0] + gc[1] + gc[2] - a - b);      // g holds a and b: its third vertex
    opp[e] = q;
    const int r0 = p < q ? p : q, r1 = p < q ? q : p;
    double x[2], y[2];
    for (int i = 0; i < 2; ++i) {
      const float* vr = verts + 3 * (size_t)(i == 0 ? r0 : r1);
      const double d[3] = {(double)vr[0] - Pl[0], (double)vr[1] - Pl[1], (double)vr[2] - Pl[2]};
      x[i] = dot3(d, E) / l;
      const double t = dot3(d, d) - x[i] * x[i];
      y[i] = sqrt(t < 0.0 ? 0.0 : t);
    }
    const double s = y[0] + y[1];
    const double xc = (x[0] * y[1] + x[1] * y[0]) / s;
    const double dx = x[0] - x[1];
    const double unf = sqrt(dx * dx + s * s);
    if (p != q && s > 0.0 && xc > 0.0 && xc < l) rec[3 + e] = unf;      // (false on NaN: the line crosses the open shared edge)
  }
}

// One relaxation of vertex v over its ascending row of n faces: the minimum of dv and of fl(d[u] + w) over the arcs of v's faces that
// are finite and at most max_dist.  `d` is the plane of the (mesh, set) pair -- global memory or LDS; `frec` and `opp` are the mesh's
// "geo.face" and "geo.opp".  The arcs of the rule leave v; each has its reverse with the same bytes, so they are also the arcs that arrive.
SH_HD double geo_relax(const int* faces, const double* frec, const int* opp, const int* row, int n, int v, int mode, double max_dist, double dv, const double* d) {
  double best = dv;
  for (int i = 0; i < n; ++i) {
    const int f = row[i];
    const int* fc = faces + 3 * (size_t)f;
    const int k = vert_corner(fc, v), k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const double* r = frec + SH_GEOD_FACE * (size_t)f;
    double c = d[fc[k1]] + r[k];
    if (c <= max_dist && c < best) best = c;
    c = d[fc[k2]] + r[k2];
    if (c <= max_dist && c < best) best = c;
    if (mode == SH_GEOD_UNFOLD) {
      const int q = opp[3 * (size_t)f + k1];
      if (q >= 0) {
        c = d[q] + r[3 + k1];
        if (c <= max_dist && c < best) best = c;
      }
    }
  }
  return best;
}

// The predecessor of a reached vertex v that is no root, from the converged plane d: the smallest u with an arc to v, fl(d[u] + w) ==
// d[v] and d[u] < d[v], or SH_GEOD_NO_PRED (only behind an arc of length 0, or one that d[u] absorbs).
SH_HD int geo_pred(const int* faces, const double* frec, const int* opp, const int* row, int n, int v, int mode, const double* d) {
  const double dv = d[v];
  int best = SH_GEOD_NO_LABEL;
  for (int i = 0; i < n; ++i) {
    const int f = row[i];
    const int* fc = faces + 3 * (size_t)f;
    const int k = vert_corner(fc, v), k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const double* r = frec + SH_GEOD_FACE * (size_t)f;
    int u = fc[k1];
    double du = d[u];
    if (du + r[k] == dv && du < dv && u < best) best = u;
    u = fc[k2]; du = d[u];
    if (du + r[k2] == dv && du < dv && u < best) best = u;
    if (mode == SH_GEOD_UNFOLD) {
      u = opp[3 * (size_t)f + k1];
      if (u >= 0) {
        du = d[u];
        if (du + r[3 + k1] == dv && du < dv && u < best) best = u;
      }
    }
  }
  return best == SH_GEOD_NO_LABEL ? SH_GEOD_NO_PRED : best;
}

// the better of two candidates for the farthest vertex: the larger distance, the smaller index among equals (v < 0: none)
SH_HD void geo_far(double d, int v, double* best_d, int* best_v) {
  if (v >= 0 && (*best_v < 0 || d > *best_d || (d == *best_d && v < *best_v))) { *best_d = d; *best_v = v; }
}

// ---- smoothing of the vertices of the resident batch (include/shoulder_hip.h sh_smooth_vertices; k_smooth.h) ---------------------------
// float64, operation by operation in the written order (-ffp-contract=off), restated by tests/smooth_oracle.py.  Nothing is
// transcendental: + - x / sqrt and comparisons, so the bytes are the same wherever the rule runs.  The filters, the weights and the
// flags are the header's SH_SMOOTH_* (k_smooth.h holds them equal).
#define SH_SMO_LAPLACIAN 0
#define SH_SMO_TAUBIN 1
#define SH_SMO_HC 2
#define SH_SMO_INVLEN 1          // the weight of a neighbour: 0 uniform, 1 one over the length of the edge in P0
#define SH_SMO_PIN_BORDER 1
#define SH_SMO_KEEP_VOLUME 2
#define SH_SMO_TERMS 4           // doubles of a block row of a volume sum: terms 13 .. 16 of the mass sum (d, d s)
#define SH_SMO_HEAD 8            // doubles of a mesh between the volume sums and the scaling: c[3], s, whether to scale, three unused
#define SH_SMO_NEWTON 10

// the info record of a mesh ("smooth.info"; the header states it in words)
struct SmoothInfo { double volume_before, volume_after, scale, max_disp, sum_sq_disp; int pinned, isolated, status, pad[3]; };
static_assert(sizeof(SmoothInfo) == 64, "SmoothInfo");

// The neighbour of v behind `last` (-1: the first): the smallest u > last among the corners other than v of the faces of v's row, or
// SH_TOPO_NONE.  Called until it says so it lists the distinct neighbours in ascending order, however often a neighbour turns up in the
// row (twice in a manifold fan, once on a border, more often at a non-manifold edge) and however long the row is.
SH_HD int smooth_next(const int* faces, const int* row, int n, int v, int last) {
  int best = SH_TOPO_NONE;
  for (int i = 0; i < n; ++i) {
    const int* f = faces + 3 * (size_t)row[i];
    for (int k = 0; k < 3; ++k) {
      const int u = f[k];
      if (u != v && u > last && u < best) best = u;
    }
  }
  return best;
}

// the stored weight of the neighbour pair {v, u}: 1.0 / l with l the length of P0_hi - P0_lo in the canonical order of the two indices
// (both directions hold the same bytes), 0.0 for a pair that is skipped (l == 0.0 or not finite)
SH_HD double smooth_weight(const float* verts, int v, int u) {
  const int lo = v < u ? v : u, hi = v < u ? u : v;
  const float *a = verts + 3 * (size_t)lo, *b = verts + 3 * (size_t)hi;
  const double D[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
  const double l = sqrt(dot3(D, D));
  return (l == 0.0 || !vert_finite(l)) ? 0.0 : 1.0 / l;
}

// the test behind SH_VERT_BORDER | SH_VERT_NONMANIFOLD (vert_gather): one of the two slots that touch v in a face of its row
SH_HD bool smooth_border(const int* faces, const int* adj, const int* row, int n, int v) {
  bool hit = false;
  for (int i = 0; i < n; ++i) {
    const int f = row[i];
    const int k = vert_corner(faces + 3 * (size_t)f, v), k2 = k == 0 ? 2 : k - 1;
    const int a0 = adj[3 * (size_t)f + k], a1 = adj[3 * (size_t)f + k2];
    hit = hit || a0 == SH_TOPO_BORDER || a1 == SH_TOPO_BORDER || a0 == SH_TOPO_NONMANIFOLD || a1 == SH_TOPO_NONMANIFOLD;
  }
  return hit;
}

// M(x)[v] from v's row of n neighbours (`w` beside it) on the mesh's plane x of three doubles per vertex: the sums in the row's order
SH_HD void smooth_mean(const int* nbr, const double* w, int n, int weight, bool pinned, const double* x, int v, double* m) {
  double S[3] = {0.0, 0.0, 0.0}, W = 0.0;
  int added = 0;
  if (!pinned)
    for (int i = 0; i < n; ++i) {
      const double wi = weight == SH_SMO_INVLEN ? w[i] : 1.0;
      if (wi == 0.0) continue;
      const double* xu = x + 3 * (size_t)nbr[i];
      S[0] += wi * xu[0]; S[1] += wi * xu[1]; S[2] += wi * xu[2];
      W += wi;
      ++added;
    }
  const bool keep = pinned || added == 0 || !vert_finite(W);
  for (int c = 0; c < 3; ++c) m[c] = keep ? x[3 * (size_t)v + c] : S[c] / W;
}

SH_HD double smooth_step(double p, double m, double c) { return p + c * (m - p); }
// b of the HC filter at a vertex that is not pinned (a pinned one has 0.0: alpha x + (1 - alpha) x need not give x back), and P
SH_HD double smooth_hc_b(double p, double p0, double q, double alpha) { return p - (alpha * p0 + (1.0 - alpha) * q); }
SH_HD double smooth_hc_p(double p, double b, double mb, double beta) { return p - (beta * b + (1.0 - beta) * mb); }

// s with s^3 = r: SH_SMO_NEWTON Newton steps from 1.0
SH_HD double smooth_cbrt(double r) {
  double s = 1.0;
  for (int i = 0; i < SH_SMO_NEWTON; ++i) s = s - ((s * s) * s - r) / (3.0 * (s * s));
  return s;
}

// The volumes and the scaling of a mesh from its two rows of sums (terms 13 .. 16 of P0 and of P about the pivot o): head = c[3], s,
// 1.0 when the vertices are to be scaled.  -> the status.
SH_HD int smooth_scale(const double* T0, const double* T1, const double* o, bool keep_volume, double* volume_before, double* volume_after, double* head /* SH_SMO_HEAD */) {
  const double V0 = T0[0] / 6.0, V1 = T1[0] / 6.0;
  *volume_before = V0; *volume_after = V1;
  for (int i = 0; i < SH_SMO_HEAD; ++i) head[i] = 0.0;
  head[3] = 1.0;
  if (!keep_volume) return 0;
  if (V0 == 0.0 || V1 == 0.0 || !vert_finite(V0) || !vert_finite(V1)) return SH_ERR_GEOMETRY_DEV;
  const double r = V0 / V1;
  if (!(r >= 0.125 && r <= 8.0)) return SH_ERR_GEOMETRY_DEV;
  double c[3];
  for (int k = 0; k < 3; ++k) c[k] = T1[1 + k] / (4.0 * T1[0]) + o[k];
  if (!vert_finite(c[0]) || !vert_finite(c[1]) || !vert_finite(c[2])) return SH_ERR_GEOMETRY_DEV;
  head[0] = c[0]; head[1] = c[1]; head[2] = c[2]; head[3] = smooth_cbrt(r); head[4] = 1.0;
  return 0;
}
SH_HD double smooth_scaled(double p, double c, double s) { return c + s * (p - c); }
// what a vertex gives to the largest displacement: its |P - P0|, 0.0 when that is no number
SH_HD double smooth_disp(double d2) {
  const double d = sqrt(d2);
  return d > 0.0 ? d : 0.0;
}

// ---- repair of the resident batch (include/shoulder_hip.h sh_mesh_repair; k_repair.h) -------------------------------------------------
// Integer rules on the faces and the adjacency of sh_mesh_topology, one float64 sum per shell and one per filled hole, restated by
// tests/repair_oracle.py.  The modes and the statuses are the header's SH_REPAIR_* (k_repair.h holds them equal).
#define SH_REP_ORIENT_NONE 0
#define SH_REP_ORIENT_WINDING 1
#define SH_REP_ORIENT_OUTWARD 2
#define SH_REP_ORIENT_NESTED 3
#define SH_REP_FILL_NONE 0
#define SH_REP_FILL_FAN 1
#define SH_REP_FILL_CENTROID 2
#define SH_REP_SHELL_NONORIENTABLE 1
#define SH_REP_SHELL_AMBIGUOUS 2
#define SH_REP_HOLE_FILLED 0
#define SH_REP_HOLE_TOO_LONG 1
#define SH_REP_HOLE_SHELL 2
#define SH_REP_HOLE_OPEN 3           // fill = NONE: reported, not filled
#define SH_REP_HOLE_TOO_SHORT 4      // fewer than three edges
#define SH_REP_V6_BLOCK 2048         // entries of a shell's face list that are summed one after the other

// the corners of face f as it is oriented: (a, b, c), or (a, c, b) when it is flipped
SH_HD void rep_face(const int* faces, int f, int flip, int* c) {
  const int* p = faces + 3 * (size_t)f;
  c[0] = p[0]; c[1] = flip ? p[2] : p[1]; c[2] = flip ? p[1] : p[2];
}
// corner k of face f as it is oriented, read where it is stored (no copy of the face)
SH_HD int rep_corner(const int* faces, int f, int flip, int k) { return faces[3 * (size_t)f + (k == 0 || !flip ? k : 3 - k)]; }
// slot e of an oriented face is this slot of the stored one: a flip exchanges slots 0 and 2
SH_HD int rep_slot(int e, int flip) { return flip ? 2 - e : e; }

// same(f, g) across the stored slot e of f, whose value in "topo.adj" is the face g: both traverse the edge in the same direction
SH_HD int rep_same(const int* faces, int f, int e, int g) {
  const int a = faces[3 * (size_t)f + e], c = faces[3 * (size_t)f + (e == 2 ? 0 : e + 1)];
  const int* gf = faces + 3 * (size_t)g;
  const int ge = topo_edge_slot(gf, a, c);
  return ge >= 0 && gf[ge] == a ? 1 : 0;
}

// the centre of a shell's float32 box, per coordinate
SH_HD double rep_center(float lo, float hi) { return (double)lo + ((double)hi - (double)lo) * 0.5; }

// det[A - o, B - o, C - o] of an oriented face: a . (b x c), the numerator of solid_angle_tri
SH_HD double rep_v6_term(const float* verts, const int* c, const double* o) {
  double P[3][3];
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 3; ++j) P[k][j] = (double)verts[3 * (size_t)c[k] + j] - o[j];
  double bc[3];
  cross3(P[1], P[2], bc);
  return dot3(P[0], bc);
}

// The successor of the border half-edge (f, e) of the oriented faces: rotate about its head w.  Slot (e + 1) % 3 of f starts at w; a
// border there is the successor; a face g there is entered through its slot that runs the other way, x -> w, and the rotation goes on
// from it; a non-manifold slot, or a neighbour that runs the same way (no rotation about w), blocks the chain.  -> 1 and (*sf, *se), or 0.
// A step enters a face through a manifold slot, so no (face, slot) comes twice and the walk ends within 3 nf steps.
SH_HD int rep_succ(const int* faces, const int* adj, const unsigned char* flip, int nf, int f, int e, int* sf, int* se) {
  int cf = f, ce = e;
  for (long long step = 0; step <= 3 * (long long)nf; ++step) {
    const int fc = flip[cf];
    const int n = ce == 2 ? 0 : ce + 1;
    const int w = rep_corner(faces, cf, fc, n), x = rep_corner(faces, cf, fc, n == 2 ? 0 : n + 1);
    const int a = adj[3 * (size_t)cf + rep_slot(n, fc)];
    if (a == SH_TOPO_BORDER) { *sf = cf; *se = n; return 1; }
    if (a < 0) return 0;
    const int fa = flip[a];
    const int g0 = rep_corner(faces, a, fa, 0), g1 = rep_corner(faces, a, fa, 1), g2 = rep_corner(faces, a, fa, 2);
    const int ge = g0 == x && g1 == w ? 0 : g1 == x && g2 == w ? 1 : g2 == x && g0 == w ? 2 : -1;
    if (ge < 0) return 0;
    cf = a; ce = ge;
  }
  return 0;
}

// the status of a hole of L edges; shell_ok: its shell is orientable
SH_HD int rep_hole_status(int L, int shell_ok, int fill, int max_hole_edges) {
  if (!shell_ok) return SH_REP_HOLE_SHELL;
  if (L < 3) return SH_REP_HOLE_TOO_SHORT;
  if (L > max_hole_edges) return SH_REP_HOLE_TOO_LONG;
  return fill == SH_REP_FILL_NONE ? SH_REP_HOLE_OPEN : SH_REP_HOLE_FILLED;
}
// the faces and the vertices a filled hole of L edges adds
SH_HD int rep_fill_faces(int L, int fill) { return fill == SH_REP_FILL_FAN ? L - 2 : L; }
SH_HD int rep_fill_verts(int fill) { return fill == SH_REP_FILL_CENTROID ? 1 : 0; }

// The fill face of the half-edge at place j of a hole of L edges (u_j -> u_j1, u_0 the start's tail, cv the new vertex): its place among
// the hole's faces, or -1 when the half-edge adds none (the fan's places 0 and L - 1).  Each runs u_j1 -> u_j, against the border.
SH_HD int rep_fill_face(int fill, int L, int j, int u0, int uj, int uj1, int cv, int* out) {
  if (fill == SH_REP_FILL_FAN) {
    if (j < 1 || j > L - 2) return -1;
    out[0] = u0; out[1] = uj1; out[2] = uj;
    return j - 1;
  }
  out[0] = uj1; out[1] = uj; out[2] = cv;
  return j;
}

// the new vertex of a hole: per coordinate the float64 sum of the float32 positions of its tails in loop order from u_0, over (double) L
SH_HD void rep_centroid(const float* verts, const int* order, int L, float* out) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < L; ++j) {
    const float* p = verts + 3 * (size_t)order[j];
    s[0] += (double)p[0]; s[1] += (double)p[1]; s[2] += (double)p[2];
  }
  for (int k = 0; k < 3; ++k) out[k] = (float)(s[k] / (double)L);
}

// the nesting depth of a shell from its winding sum W (NESTED): rint(W), or 0 and *ambiguous when W is further than 0.25 from it
SH_HD int rep_depth(double W, int* ambiguous) {
  const double d = rint(W);
  *ambiguous = !(fabs(W - d) <= 0.25) ? 1 : 0;
  if (*ambiguous || !(fabs(d) < 1e9)) return 0;
  return (int)d;
}

// ---- the face hierarchy of the resident batch (include/shoulder_hip.h sh_mesh_bvh; k_bvh.h) -------------------------------------------
// float32 minima and maxima, one float64 quantisation and integer work, restated by tests/bvh_oracle.py: the device, the host twin
// (tests/hostcheck/bvh_check.cpp) and the oracle give the same bytes.  LEAF and WIDTH are powers of two in 4..16, fixed after measuring
// (4 x 4 was the fastest of six candidates on the bench batch); a lab build may set others (tools/time_bvh.py),
// everything below follows.
#ifndef SH_BVH_LEAF
#define SH_BVH_LEAF 4            // entries of the order per leaf
#endif
#ifndef SH_BVH_WIDTH
#define SH_BVH_WIDTH 4           // nodes of level k per node of level k + 1
#endif
#define SH_BVH_MAX_FACES (0x7fffffffLL / 3)      // the faces of the largest mesh an upload admits (sh_ingest.h check_mesh_arrays)
#define SH_BVH_OFF_WORDS 32      // int32 of a mesh in "bvh.off": tight, loose, leaves, levels, nodes, base, 0, 0, then the level starts
#define SH_BVH_OFF_LEVEL 8       // ... word of the start of level 0
#define SH_BVH_LOOSE_CODE 0x40000000u      // the sort code of a loose face: above every 30-bit code

// the levels of a tree over `tight` faces (0 without one) and the nodes of all of them
SH_HD constexpr int bvh_levels_of(long long tight) {
  if (tight <= 0) return 0;
  long long n = (tight + SH_BVH_LEAF - 1) / SH_BVH_LEAF;
  int k = 1;
  while (n > 1) { n = (n + SH_BVH_WIDTH - 1) / SH_BVH_WIDTH; ++k; }
  return k;
}
SH_HD constexpr long long bvh_nodes_of(long long tight) {
  if (tight <= 0) return 0;
  long long n = (tight + SH_BVH_LEAF - 1) / SH_BVH_LEAF, sum = n;
  while (n > 1) { n = (n + SH_BVH_WIDTH - 1) / SH_BVH_WIDTH; sum += n; }
  return sum;
}
constexpr int SH_BVH_MAX_LEVELS = bvh_levels_of(SH_BVH_MAX_FACES);
constexpr int SH_BVH_STACK = SH_BVH_MAX_LEVELS * (SH_BVH_WIDTH - 1) + 1;      // a depth-first walk that replaces a node by its children holds no more
static_assert(SH_BVH_LEAF >= 4 && SH_BVH_LEAF <= 16 && (SH_BVH_LEAF & (SH_BVH_LEAF - 1)) == 0, "SH_BVH_LEAF: a power of two in 4..16");
static_assert(SH_BVH_WIDTH >= 4 && SH_BVH_WIDTH <= 16 && (SH_BVH_WIDTH & (SH_BVH_WIDTH - 1)) == 0, "SH_BVH_WIDTH: a power of two in 4..16");
static_assert(SH_BVH_MAX_LEVELS <= 16 && (SH_BVH_MAX_FACES + SH_BVH_LEAF - 1) / SH_BVH_LEAF < (1LL << 28), "a stack entry is level << 28 | node");
static_assert(SH_BVH_OFF_LEVEL + SH_BVH_MAX_LEVELS + 1 <= SH_BVH_OFF_WORDS, "bvh.off: a word per level and one behind the last");
static_assert(bvh_nodes_of(SH_BVH_MAX_FACES) <= 0x7fffffffLL, "the nodes of a mesh are an int32");

// The row of a mesh in "bvh.off" from its counts and its first node in "bvh.box"
SH_HD void bvh_off_row(int tight, int loose, int base, int* row /* SH_BVH_OFF_WORDS */) {
  for (int i = 0; i < SH_BVH_OFF_WORDS; ++i) row[i] = 0;
  int levels = 0, nodes = 0, n = tight > 0 ? (tight + SH_BVH_LEAF - 1) / SH_BVH_LEAF : 0;
  const int leaves = n;
  while (n > 0) {
    row[SH_BVH_OFF_LEVEL + levels] = nodes;
    nodes += n; ++levels;
    if (n == 1) break;
    n = (n + SH_BVH_WIDTH - 1) / SH_BVH_WIDTH;
  }
  row[SH_BVH_OFF_LEVEL + levels] = nodes;
  row[0] = tight; row[1] = loose; row[2] = leaves; row[3] = levels; row[4] = nodes; row[5] = base;
}

// THE LOOSE PREDICATE, once: g = |ab x ac|^2 / Lmax^3 of the widened edges, the number k_closest.h forms at staging (point (3) of its
// cull).  !(g >= 2^-7): the face is loose -- also when g is NaN (a point triangle divides 0 by 0).
SH_HD bool bvh_loose(const double* ab, const double* ac) {
  const double bc[3] = {ac[0] - ab[0], ac[1] - ab[1], ac[2] - ab[2]};
  double n[3];
  cross3(ab, ac, n);
  const double l2 = fmax(dot3(ab, ab), fmax(dot3(ac, ac), dot3(bc, bc)));
  const double g = dot3(n, n) / (l2 * sqrt(l2));
  return !(g >= 0x1p-7);
}
// the corners of a face widened as cp_face widens them -> loose or not
SH_HD bool bvh_face_loose(const float* v0, const float* v1, const float* v2) {
  const double A[3] = {(double)v0[0], (double)v0[1], (double)v0[2]};
  const double ab[3] = {(double)v1[0] - A[0], (double)v1[1] - A[1], (double)v1[2] - A[2]}, ac[3] = {(double)v2[0] - A[0], (double)v2[1] - A[1], (double)v2[2] - A[2]};
  return bvh_loose(ab, ac);
}

// minimum and maximum of two float32 in the order of topo_enc (total: -0 below +0), so that a box is the same bytes whatever the order
// of its members
SH_HD float bvh_fmin(float a, float b) { return topo_enc(b) < topo_enc(a) ? b : a; }
SH_HD float bvh_fmax(float a, float b) { return topo_enc(b) > topo_enc(a) ? b : a; }

// the cell of a face along one axis: mn, mx its smallest and largest corner coordinate, lo, hi those of the tight faces of the mesh.
// s is twice the box centre and exact; ext > 0 fails for a flat mesh, whose cell is 0.
SH_HD int bvh_quant(float mn, float mx, float lo, float hi) {
  const double s = (double)mn + (double)mx, ext = 2.0 * ((double)hi - (double)lo);
  if (!(ext > 0.0)) return 0;
  const int q = (int)floor(((s - 2.0 * (double)lo) / ext) * 1024.0);
  return q < 1023 ? q : 1023;
}
// bit i of a 10-bit cell to bit 3 i
SH_HD unsigned bvh_spread(unsigned v) {
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
SH_HD unsigned bvh_code(int qx, int qy, int qz) { return bvh_spread((unsigned)qx) | (bvh_spread((unsigned)qy) << 1) | (bvh_spread((unsigned)qz) << 2); }
// the code of a tight face from its corners and the box (lo[3], hi[3]) of the tight faces
SH_HD unsigned bvh_face_code(const float* v0, const float* v1, const float* v2, const float* lo, const float* hi) {
  int q[3];
  for (int k = 0; k < 3; ++k) q[k] = bvh_quant(bvh_fmin(v0[k], bvh_fmin(v1[k], v2[k])), bvh_fmax(v0[k], bvh_fmax(v1[k], v2[k])), lo[k], hi[k]);
  return bvh_code(q[0], q[1], q[2]);
}
// the sort key: tight faces ascending by (code, id), the loose ones behind them ascending by id
SH_HD unsigned long long bvh_key(bool loose, unsigned code, int face) {
  return ((unsigned long long)(loose ? SH_BVH_LOOSE_CODE : code) << 32) | (unsigned long long)(unsigned)face;
}

// a box (lo[3], hi[3]) grown by a point, and by a box
SH_HD void bvh_box_point(float* bx, const float* v) {
  for (int k = 0; k < 3; ++k) { bx[k] = bvh_fmin(bx[k], v[k]); bx[3 + k] = bvh_fmax(bx[3 + k], v[k]); }
}
SH_HD void bvh_box_box(float* bx, const float* o) {
  for (int k = 0; k < 3; ++k) { bx[k] = bvh_fmin(bx[k], o[k]); bx[3 + k] = bvh_fmax(bx[3 + k], o[3 + k]); }
}

// THE PRUNING RULE (k_bvh.h states the argument): may the node with the float32 box bx be skipped by a point p whose best distance
// so far is best_r = sqrt(best d2) (1 + 2^-40), +inf without one?  near2: the squared distance from p to the widened box as computed.
SH_HD bool bvh_box_skip(const double* p, const float* bx, double best_r, double* near2_out) {
  double dn[3], df[3], m1 = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double lo = (double)bx[k], hi = (double)bx[3 + k];
    const double a = lo - p[k], b = p[k] - hi;
    dn[k] = fmax(fmax(a, b), 0.0);
    df[k] = fmax(fabs(a), fabs(b));
    m1 = m1 + fmax(fabs(lo), fabs(hi));
  }
  const double near2 = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2], far2 = (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2];
  const double thr = best_r + m1 * 0x1p-40;
  *near2_out = near2;
  return near2 > (thr * thr) * (1.0 + 0x1p-20) && far2 <= 1e8;
}

// d2 of entry i of "bvh.tri" (9 float32: the corners) to p: widened exactly as cp_face widens the mesh's vertices, so the same number
SH_HD double bvh_tri_d2(const double* p, const float* t) {
  const double A[3] = {(double)t[0], (double)t[1], (double)t[2]};
  const double ab[3] = {(double)t[3] - A[0], (double)t[4] - A[1], (double)t[5] - A[2]}, ac[3] = {(double)t[6] - A[0], (double)t[7] - A[1], (double)t[8] - A[2]};
  double u, w;
  int region;
  return closest_pt_tri(p, A, ab, ac, &u, &w, &region);
}

// THE DESCENT of one query point through the tree of one mesh (k_bvh.h k_cp_tree runs it with a stack in LDS, the host twin with an
// array): row the mesh's words of "bvh.off", bx its boxes, tr and ord its entries of "bvh.tri" and "bvh.order".  Pop a node word
// (level << 28 | node), test its box again -- the best may have fallen since it was pushed --; a leaf folds its entries into
// (*best, *best_f) under closest_key_less; an inner node pushes the children whose box survives, the nearest one last, so that it is
// descended first.  st.at(i) is word i of the stack: a walk that replaces a node by at most WIDTH children one level down never holds
// more than (levels - 1) (WIDTH - 1) + 1 <= SH_BVH_STACK.  COUNT: count[0] += the nodes popped, count[1] += the faces tested.
template <bool COUNT, typename Stack>
SH_HD void bvh_descend(const double* p, const int* row, const float* bx, const float* tr, const int* ord, Stack& st, double* best_io, int* best_f_io, long long* count) {
  const int T = row[0], levels = row[3];
  const int* lv = row + SH_BVH_OFF_LEVEL;
  double best = *best_io, best_r = sqrt(best) * (1.0 + 0x1p-40);
  int best_f = *best_f_io, sp = 0;
  if (levels > 0) st.at(sp++) = (unsigned)(levels - 1) << 28;
  while (sp > 0) {
    const unsigned e = st.at(--sp);
    const int k = (int)(e >> 28), j = (int)(e & 0x0fffffffu);
    double near2;
    if (COUNT) ++count[0];
    {
      const float* nb = bx + 6 * ((size_t)lv[k] + (size_t)j);
      const float bb[6] = {nb[0], nb[1], nb[2], nb[3], nb[4], nb[5]};
      if (bvh_box_skip(p, bb, best_r, &near2)) continue;
    }
    if (k == 0) {
      const int i0 = j * SH_BVH_LEAF, i1 = i0 + SH_BVH_LEAF < T ? i0 + SH_BVH_LEAF : T;
      for (int i = i0; i < i1; ++i) {
        const float* t = tr + 9 * (size_t)i;
        const float tt[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
        const double d2 = bvh_tri_d2(p, tt);
        const int f = ord[i];
        if (COUNT) ++count[1];
        if (closest_key_less(d2, f, best, best_f)) { best = d2; best_f = f; best_r = sqrt(d2) * (1.0 + 0x1p-40); }
      }
    } else {
      const int below = lv[k] - lv[k - 1];
      const int c0 = j * SH_BVH_WIDTH, c1 = c0 + SH_BVH_WIDTH < below ? c0 + SH_BVH_WIDTH : below;
      const float* ch = bx + 6 * (size_t)lv[k - 1];
      const unsigned tag = (unsigned)(k - 1) << 28;
      int nearest = -1;
      double nearest_d = 0.0;
      for (int c = c0; c < c1; ++c) {
        const float* nb = ch + 6 * (size_t)c;
        const float bb[6] = {nb[0], nb[1], nb[2], nb[3], nb[4], nb[5]};
        if (bvh_box_skip(p, bb, best_r, &near2)) continue;
        if (nearest < 0 || near2 < nearest_d) {
          if (nearest >= 0) st.at(sp++) = tag | (unsigned)nearest;
          nearest = c; nearest_d = near2;
        } else st.at(sp++) = tag | (unsigned)c;
      }
      if (nearest >= 0) st.at(sp++) = tag | (unsigned)nearest;
    }
  }
  *best_io = best; *best_f_io = best_f;
}

// ---- rays through the face hierarchy (include/shoulder_hip.h sh_ray_cast with SH_ACCEL_BVH, sh_ray_nearest; k_raytree.h) ----------------
// THE SKIP RULE OF A RAY (k_raytree.h states the argument): may the ray r (bvh_ray_set) skip the node with the float32 box bx?  tbest: the
// t of the best hit so far, +inf for a walk that wants every hit.  The half-line {o + s d, s >= 0} is held against the box grown on
// every side by
//     pad = 2^-8 |d| D E^2 + 2^-40 m1,
// D the distance from o to the box's far corner, E its diagonal, m1 the sum over the axes of the larger absolute bound.  Nothing is
// skipped when |d|^2 or D^2 is above 2^40 (or is NaN).  Every comparison that skips is written so that it is false for a NaN.
// *tn_out: the parameter at which the half-line enters the grown box, as computed (0 inside it; what the children are ordered by).
#define SH_BVH_RAY_GUARD2 0x1p40
// a ray as the skip rule reads it, formed once per ray: dd = d . d, dl = sqrt(dd), and the reciprocals of dl and of the components of d
struct BvhRay { double o[3], d[3], inv[3], dd, dl, inv_dl; };
SH_HD void bvh_ray_set(const double* o, const double* d, BvhRay* r) {
  for (int k = 0; k < 3; ++k) { r->o[k] = o[k]; r->d[k] = d[k]; r->inv[k] = 1.0 / d[k]; }
  r->dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  r->dl = sqrt(r->dd);
  r->inv_dl = 1.0 / r->dl;
}
SH_HD bool bvh_ray_box_skip(const BvhRay& r, const float* bx, double tbest, double* tn_out) {
  double lo[3], hi[3], df[3], ex[3], m1 = 0.0;
  for (int k = 0; k < 3; ++k) {
    lo[k] = (double)bx[k]; hi[k] = (double)bx[3 + k];
    df[k] = fmax(fabs(lo[k] - r.o[k]), fabs(r.o[k] - hi[k]));
    ex[k] = hi[k] - lo[k];
    m1 = m1 + fmax(fabs(lo[k]), fabs(hi[k]));
  }
  const double far2 = (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2], ext2 = (ex[0] * ex[0] + ex[1] * ex[1]) + ex[2] * ex[2];
  *tn_out = 0.0;
  if (!(r.dd <= SH_BVH_RAY_GUARD2 && far2 <= SH_BVH_RAY_GUARD2)) return false;
  const double pad = (0x1p-8 * r.dl) * (sqrt(far2) * ext2) + m1 * 0x1p-40;      // (finite: every factor is bounded)
  double tn = 0.0, tf = INFINITY;
  bool beside = false;
  for (int k = 0; k < 3; ++k) {
    const double l = lo[k] - pad, h = hi[k] + pad;
    if (r.d[k] == 0.0) {      // the ray keeps this coordinate: it is in the slab or it is not; no product, no quotient
      if (r.o[k] < l || r.o[k] > h) beside = true;
    } else if (fabs(r.inv[k]) < INFINITY) {      // a finite difference times a finite, non-zero reciprocal: +-inf at worst, never 0 * inf
      const double t1 = (l - r.o[k]) * r.inv[k], t2 = (h - r.o[k]) * r.inv[k];
      tn = fmax(tn, fmin(t1, t2));
      tf = fmin(tf, fmax(t1, t2));
    }                         // (a component so small that its reciprocal overflows: this axis decides nothing, which skips less)
  }
  *tn_out = tn;
  if (beside) return true;
  if (tn > tf + fabs(tf) * 0x1p-40) return true;      // (inf > inf, and anything against a NaN, is false)
  return (tn - pad * r.inv_dl) * (1.0 - 0x1p-40) > tbest;      // behind the best hit; false for tbest = +inf and for dl = 0
}

// THE DESCENT OF ONE RAY through the tree of one mesh (k_raytree.h runs it with a stack in LDS, the host twin with an array), the
// arguments as bvh_descend's.  Pop a node word (level << 28 | node); a walk that prunes by t tests its box again (the best may have
// fallen since it was pushed), the others have tested it when they pushed it.  A leaf runs ray_tri_hit on its entries of "bvh.tri", the
// corners widened as bvh_tri_d2 widens them with e1 = B - A and e2 = C - A taken first: t, side and the verdict are the bits ray_walk
// (k_rays.h) computes from the mesh.  Every hit goes to hit(t, face = ord[i], side); Hit::PRUNE says whether hit.bound() (the best t so
// far) may skip nodes.  An inner node pushes the children it may not skip, the one the ray enters first last.  The stack holds at most
// (levels - 1) (WIDTH - 1) + 1 <= SH_BVH_STACK words, as bvh_descend's.  COUNT: count[0] += the nodes popped, count[1] += the faces tested.
template <bool COUNT, typename Stack, typename Hit>
SH_HD void bvh_ray_descend(const double* o, const double* d, const int* row, const float* bx, const float* tr, const int* ord, Stack& st, Hit& hit, long long* count) {
  const int T = row[0], levels = row[3];
  const int* lv = row + SH_BVH_OFF_LEVEL;
  BvhRay ray;
  bvh_ray_set(o, d, &ray);
  int sp = 0;
  if (levels > 0) st.at(sp++) = (unsigned)(levels - 1) << 28;
  while (sp > 0) {
    const unsigned e = st.at(--sp);
    const int k = (int)(e >> 28), j = (int)(e & 0x0fffffffu);
    double tn;
    if (COUNT) ++count[0];
    if (Hit::PRUNE || k == levels - 1) {      // (the root is tested here in every walk)
      const float* nb = bx + 6 * ((size_t)lv[k] + (size_t)j);
      const float bb[6] = {nb[0], nb[1], nb[2], nb[3], nb[4], nb[5]};
      if (bvh_ray_box_skip(ray, bb, hit.bound(), &tn)) continue;
    }
    if (k == 0) {
      const int i0 = j * SH_BVH_LEAF, i1 = i0 + SH_BVH_LEAF < T ? i0 + SH_BVH_LEAF : T;
      for (int i = i0; i < i1; ++i) {
        const float* t = tr + 9 * (size_t)i;
        const double A[3] = {(double)t[0], (double)t[1], (double)t[2]};
        const double e1[3] = {(double)t[3] - A[0], (double)t[4] - A[1], (double)t[5] - A[2]}, e2[3] = {(double)t[6] - A[0], (double)t[7] - A[1], (double)t[8] - A[2]};
        double th = 0.0;
        int side = 0;
        if (COUNT) ++count[1];
        if (ray_tri_hit(o, d, A, e1, e2, &th, &side)) hit(th, ord[i], side);
      }
    } else {
      const int below = lv[k] - lv[k - 1];
      const int c0 = j * SH_BVH_WIDTH, c1 = c0 + SH_BVH_WIDTH < below ? c0 + SH_BVH_WIDTH : below;
      const float* ch = bx + 6 * (size_t)lv[k - 1];
      const unsigned tag = (unsigned)(k - 1) << 28;
      int first = -1;
      double first_t = 0.0;
      for (int c = c0; c < c1; ++c) {
        const float* nb = ch + 6 * (size_t)c;
        const float bb[6] = {nb[0], nb[1], nb[2], nb[3], nb[4], nb[5]};
        if (bvh_ray_box_skip(ray, bb, hit.bound(), &tn)) continue;
        if (first < 0 || tn < first_t) {
          if (first >= 0) st.at(sp++) = tag | (unsigned)first;
          first = c; first_t = tn;
        } else st.at(sp++) = tag | (unsigned)c;
      }
      if (first >= 0) st.at(sp++) = tag | (unsigned)first;
    }
  }
}

// the three readers of a descent: the count, the fill of a ray's segment of the pool (room: its length -- a write is guarded, as the
// brute fill's), the nearest hit under ray_key_less
struct RayHitCount {
  static constexpr bool PRUNE = false;
  int n = 0;
  SH_HD double bound() const { return INFINITY; }
  SH_HD void operator()(double, int, int) { ++n; }
};
struct RayHitNear {
  static constexpr bool PRUNE = true;
  double t = INFINITY;
  int face = -1, side = 0;
  SH_HD double bound() const { return t; }
  SH_HD void operator()(double th, int f, int s) { if (ray_key_less(th, f, t, face)) { t = th; face = f; side = s; } }
};

// ---- simplification of the resident batch by vertex clustering (include/shoulder_hip.h sh_mesh_simplify; k_simplify.h) ----------------
// float64, operation by operation in the written order (-ffp-contract=off), + - x / sqrt and floor only; restated by
// tests/simplify_oracle.py.  The placements and limits are the header's SH_SIMPLIFY_* (k_simplify.h holds them equal).
#define SH_SIMP_MEAN 0
#define SH_SIMP_QUADRIC 1
#define SH_SIMP_MAX_CELLS 1048576        // per axis
#define SH_SIMP_MAX_CLUSTERS 2097152     // per mesh
#define SH_SIMP_NO_KEY 0xffffffffffffffffull      // the key of a vertex that takes no part: above every cell (a key is below 2^60)
#define SH_SIMP_Q 10                     // the sums of a quadric: n0n0 n0n1 n0n2 n1n1 n1n2 n2n2 n0d n1d n2d dd

SH_HD bool simp_finite(double x) { return x - x == 0.0; }

// the cells per axis of the box [lo, hi] (float32, widened) at the cell h; false when an axis has more than SH_SIMP_MAX_CELLS (or the
// quotient is not a number)
SH_HD bool simp_grid(const float* lo, const float* hi, double h, long long* n /* 3 */) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double q = floor(((double)hi[k] - (double)lo[k]) / h);
    if (!(q >= 0.0 && q < (double)SH_SIMP_MAX_CELLS)) { ok = false; n[k] = 0; continue; }
    n[k] = (long long)q + 1;
  }
  return ok;
}
// the cell of the coordinate x on an axis of n cells that starts at lo
SH_HD long long simp_cell(float x, float lo, double h, long long n) {
  const long long i = (long long)floor(((double)x - (double)lo) / h);
  return i < n - 1 ? i : n - 1;
}
SH_HD unsigned long long simp_key(const long long* i, const long long* n) { return (unsigned long long)((i[2] * n[1] + i[1]) * n[0] + i[0]); }
SH_HD void simp_unkey(unsigned long long key, const long long* n, long long* i) {
  const unsigned long long nx = (unsigned long long)n[0], ny = (unsigned long long)n[1];
  i[0] = (long long)(key % nx); i[1] = (long long)((key / nx) % ny); i[2] = (long long)((key / nx) / ny);
}
// the centre of cell i on an axis
SH_HD double simp_center(long long i, float lo, double h) { return (double)lo + ((double)i + 0.5) * h; }

// the face with the widened corners A, B, C added to the ten sums q, relative to o: n = cross3(B - A, C - A), not normalised, d = -dot3(n, A - o)
SH_HD void simp_face_quadric(const double* A, const double* B, const double* C, const double* o, double* q /* SH_SIMP_Q */) {
  const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]}, t[3] = {A[0] - o[0], A[1] - o[1], A[2] - o[2]};
  double n[3];
  cross3(e1, e2, n);
  const double d = -dot3(n, t);
  q[0] = q[0] + n[0] * n[0]; q[1] = q[1] + n[0] * n[1]; q[2] = q[2] + n[0] * n[2]; q[3] = q[3] + n[1] * n[1]; q[4] = q[4] + n[1] * n[2];
  q[5] = q[5] + n[2] * n[2]; q[6] = q[6] + n[0] * d; q[7] = q[7] + n[1] * d; q[8] = q[8] + n[2] * d; q[9] = q[9] + d * d;
}

// The placement of a cluster from its quadric q, its mean m and its cell centre o: x, relative to o, solves (A + lambda I) x =
// lambda (m - o) - b, lambda = reg tr(A), by the 3 x 3 Cholesky factorisation written out.  false: the cluster takes its mean (tr 0.0 or
// not finite; a radicand <= 0.0 or not finite; an x that is not finite or leaves the clamped cell, |x_c| > 0.5 h clamp).
SH_HD bool simp_solve(const double* q, const double* m, const double* o, double h, double reg, double clamp, double* x /* 3 */) {
  const double tr = (q[0] + q[3]) + q[5];
  if (tr == 0.0 || !simp_finite(tr)) return false;
  const double lam = reg * tr;
  const double m00 = q[0] + lam, m11 = q[3] + lam, m22 = q[5] + lam;
  const double r0 = lam * (m[0] - o[0]) - q[6], r1 = lam * (m[1] - o[1]) - q[7], r2 = lam * (m[2] - o[2]) - q[8];
  if (!(m00 > 0.0) || !simp_finite(m00)) return false;
  const double l00 = sqrt(m00);
  const double l10 = q[1] / l00, l20 = q[2] / l00;
  const double p1 = m11 - l10 * l10;
  if (!(p1 > 0.0) || !simp_finite(p1)) return false;
  const double l11 = sqrt(p1);
  const double l21 = (q[4] - l20 * l10) / l11;
  const double p2 = (m22 - l20 * l20) - l21 * l21;
  if (!(p2 > 0.0) || !simp_finite(p2)) return false;
  const double l22 = sqrt(p2);
  const double y0 = r0 / l00;
  const double y1 = (r1 - l10 * y0) / l11;
  const double y2 = ((r2 - l20 * y0) - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = ((y0 - l10 * x[1]) - l20 * x[2]) / l00;
  const double lim = (0.5 * h) * clamp;
  for (int k = 0; k < 3; ++k)
    if (!simp_finite(x[k]) || fabs(x[k]) > lim) return false;
  return true;
}

// the three clusters of a face ascending -> s; false: two of them are equal (the face is collapsed)
SH_HD bool simp_triple(int a, int b, int c, int* s /* 3 */) {
  if (a == b || b == c || a == c) return false;
  int lo = a < b ? a : b, hi = a < b ? b : a;
  if (c < lo) { s[0] = c; s[1] = lo; s[2] = hi; }
  else if (c < hi) { s[0] = lo; s[1] = c; s[2] = hi; }
  else { s[0] = lo; s[1] = hi; s[2] = c; }
  return true;
}

// the distance a vertex moves: between the widened float32 positions x and p; 0.0 when it is not a number
SH_HD double simp_move(const float* x, const float* p) {
  const double d[3] = {(double)x[0] - (double)p[0], (double)x[1] - (double)p[1], (double)x[2] - (double)p[2]};
  const double r = sqrt(dot3(d, d));
  return r == r ? r : 0.0;
}

}  // namespace sh
