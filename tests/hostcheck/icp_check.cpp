// Test shim (NOT product): the registration arithmetic of shoulder_amd/csrc/sh_scalar.h (icp_pair_terms, sym4_jacobi, icp_horn_solve,
// chol6_solve, icp_plane_solve, icp_compose, icp_step -- the source k_icp.h runs on the device) and the argument checks and buffer
// plan of sh_query.h (precheck_register, icp_plan) on the host, for tests/test_icp_host.py.  ic_evaluate makes one evaluation as the
// kernels do: the points moved, paired against every face (closest_pt_tri under closest_key_less, as k_cp_walk / k_cp_join), the terms
// of each block of 256 put through the tree slot[i] += slot[i + h]; ic_register runs the whole loop.  Its own main() registers points
// onto a scalene box with both metrics and walks the failure cases, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static void face_of(const float* verts, const int* faces, int f, double* A, double* ab, double* ac) {
  const float *v0 = verts + 3 * (size_t)faces[3 * f], *v1 = verts + 3 * (size_t)faces[3 * f + 1], *v2 = verts + 3 * (size_t)faces[3 * f + 2];
  for (int k = 0; k < 3; ++k) { A[k] = (double)v0[k]; ab[k] = (double)v1[k] - A[k]; ac[k] = (double)v2[k] - A[k]; }
}

// k_cp_walk and k_cp_join for one point
static void closest_of(const float* verts, const int* faces, int nf, const double* p, sh_closest* out) {
  double best = INFINITY;
  int best_f = -1;
  for (int f = 0; f < nf; ++f) {
    double A[3], ab[3], ac[3], u, w;
    int region;
    face_of(verts, faces, f, A, ab, ac);
    const double d2 = sh::closest_pt_tri(p, A, ab, ac, &u, &w, &region);
    if (sh::closest_key_less(d2, f, best, best_f)) { best = d2; best_f = f; }
  }
  memset(out, 0, sizeof *out);
  if (best_f < 0) { out->face = -1; out->status = SH_ERR_GEOMETRY; return; }
  double A[3], ab[3], ac[3], u, w, q[3];
  int region;
  face_of(verts, faces, best_f, A, ab, ac);
  const double d2 = sh::closest_pt_tri(p, A, ab, ac, &u, &w, &region);
  sh::tri_point(A, ab, ac, u, w, q);
  const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  out->dist = sqrt(d2); out->point[0] = q[0]; out->point[1] = q[1]; out->point[2] = q[2];
  out->face = best_f; out->region = region; out->side = sh::closest_side(r, ab, ac); out->status = 0;
}

// the tree of one block: 256 slots, the missing ones +0.0
static double tree256(const double* vals, int n) {
  double slot[SH_ICP_BLOCK];
  for (int i = 0; i < SH_ICP_BLOCK; ++i) slot[i] = i < n ? vals[i] : 0.0;
  for (int h = SH_ICP_BLOCK / 2; h >= 1; h >>= 1)
    for (int i = 0; i < h; ++i) slot[i] += slot[i + h];
  return slot[0];
}

// n values: the block sums added in block order from 0.0
extern "C" void ic_tree(const double* vals, int n, double* out) {
  double tot = 0.0;
  for (int b0 = 0; b0 < n; b0 += SH_ICP_BLOCK) tot += tree256(vals + b0, n - b0 < SH_ICP_BLOCK ? n - b0 : SH_ICP_BLOCK);
  *out = tot;
}

extern "C" void ic_jacobi(double* A /* 16, in: the matrix, out: its diagonal holds the eigenvalues */, double* V /* 16 */) { sh::sym4_jacobi(A, V); }
extern "C" int ic_chol(const double* up, const double* b, double* x, double* min_pivot) { return sh::chol6_solve(up, b, x, min_pivot) ? 1 : 0; }

// rows (blocks x SH_ICP_TERMS) of one evaluation at Tst = (T, cbar, spare); phase 0 of k_icp_sum when metric < 0
static void rows_of(const float* verts, const int* faces, int nf, const double* points, int Q, const double* Tst, int metric, double reject, double* rows,
                    sh_closest* near_out) {
  const int blocks = (Q + SH_ICP_BLOCK - 1) / SH_ICP_BLOCK;
  std::vector<double> terms((size_t)Q * SH_ICP_TERMS, 0.0), col(SH_ICP_BLOCK);
  double c[3];
  sh::canal_map_point(Tst, Tst[16], Tst[17], Tst[18], c);
  for (int i = 0; i < Q; ++i) {
    double* t = &terms[(size_t)i * SH_ICP_TERMS];
    if (metric < 0) { t[0] = 1.0; t[2] = points[3 * i]; t[3] = points[3 * i + 1]; t[4] = points[3 * i + 2]; continue; }
    double pm[3], A[3], ab[3] = {0, 0, 0}, ac[3] = {0, 0, 0};
    sh::canal_map_point(Tst, points[3 * i], points[3 * i + 1], points[3 * i + 2], pm);
    sh_closest nr;
    closest_of(verts, faces, nf, pm, &nr);
    if (near_out) near_out[i] = nr;
    if (metric == SH_ICP_PLANE && nr.status == 0) face_of(verts, faces, nr.face, A, ab, ac);
    sh::icp_pair_terms(metric, pm, nr.point, nr.status, reject, ab, ac, c, t);
  }
  for (int blk = 0; blk < blocks; ++blk) {
    const int n = Q - blk * SH_ICP_BLOCK < SH_ICP_BLOCK ? Q - blk * SH_ICP_BLOCK : SH_ICP_BLOCK;
    for (int k = 0; k < SH_ICP_TERMS; ++k) {
      for (int i = 0; i < n; ++i) col[i] = terms[((size_t)blk * SH_ICP_BLOCK + i) * SH_ICP_TERMS + k];
      rows[(size_t)blk * SH_ICP_TERMS + k] = tree256(col.data(), n);
    }
  }
}
static void join_rows(const double* rows, int blocks, double* tot) {
  for (int k = 0; k < SH_ICP_TERMS; ++k) {
    double s = 0.0;
    for (int blk = 0; blk < blocks; ++blk) s += rows[(size_t)blk * SH_ICP_TERMS + k];
    tot[k] = s;
  }
}

extern "C" void ic_evaluate(const float* verts, const int* faces, int nf, const double* points, int Q, const double* Tst /* 20 */, int metric, double reject,
                            double* rows /* blocks x 32 */) {
  rows_of(verts, faces, nf, points, Q, Tst, metric, reject, rows, nullptr);
}

// the loop of sh_register_points for one humerus; near: Q records of the last evaluation (nullable)
extern "C" int ic_register(const float* verts, const int* faces, int nf, const double* points, int Q, const double* T0, const sh_icp_options* opt,
                           sh_registration* out, double* hist /* (max_iter + 1) x 2 */) {
  const int blocks = (Q + SH_ICP_BLOCK - 1) / SH_ICP_BLOCK, K = opt->max_iter;
  double Tst[20], tot[SH_ICP_TERMS];
  std::vector<double> rows((size_t)blocks * SH_ICP_TERMS);
  for (int i = 0; i < 20; ++i) Tst[i] = i < 16 ? (T0 ? T0[i] : (i % 5 == 0 ? 1.0 : 0.0)) : 0.0;
  memset(out, 0, sizeof *out);
  memset(hist, 0, sizeof(double) * 2 * (size_t)(K + 1));
  rows_of(verts, faces, nf, points, Q, Tst, -1, 0.0, rows.data(), nullptr);
  join_rows(rows.data(), blocks, tot);
  for (int i = 0; i < 3; ++i) Tst[16 + i] = tot[2 + i] / (double)Q;
  for (int k = 0; k <= K; ++k) {
    rows_of(verts, faces, nf, points, Q, Tst, opt->metric, opt->reject, rows.data(), nullptr);
    join_rows(rows.data(), blocks, tot);
    double rec[3] = {out->rms, out->rms_first, out->min_pivot};
    int irec[4];
    for (int i = 0; i < 16; ++i) out->T[i] = Tst[i];
    const int done = sh::icp_step(opt->metric, k, K, opt->tol, tot, Tst + 16, Tst, rec, irec, hist + 2 * k);
    out->rms = rec[0]; out->rms_first = rec[1]; out->min_pivot = rec[2];
    out->pairs = irec[0]; out->iterations = irec[1]; out->converged = irec[2]; out->status = irec[3];
    if (done) break;
  }
  return out->status;
}

// precheck_register against a context that is there (or not), holds B humeri and has n_pending runs in flight
extern "C" int ic_precheck(int ctx, const double* points, int Q, int per_humerus, const double* T0, const sh_icp_options* opt, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_register(points, Q, per_humerus, T0, opt, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st}).code;
}

extern "C" void ic_plan(int B, int Q, int per_humerus, long long maxF, int max_iter, size_t* out /* chunks, S, then the nine sizes in list order */) {
  const sh::IcpPlan p = sh::icp_plan(B, Q, per_humerus != 0, maxF, max_iter);
  size_t* o = out;
  *o++ = (size_t)p.chunks; *o++ = (size_t)p.S;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  ICP_BUFS(X)
#undef X
}

// stand-alone run (sanitizer build): recover a small rigid motion of points on a scalene box, both metrics; the failures
int main() {
  const float bv[24] = {0, 0, 0, 30, 0, 0, 0, 20, 0, 30, 20, 0, 0, 0, 10, 30, 0, 10, 0, 20, 10, 30, 20, 10};
  const int bf[36] = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  const double size[3] = {30, 20, 10};
  for (int Q : {6, 255, 257, 513}) {
    std::vector<double> truth(3 * (size_t)Q), pts(3 * (size_t)Q);
    unsigned long long seed = 12345;
    auto rnd = [&seed]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return 0.1 + 0.8 * (double)(seed >> 11) / 9007199254740992.0; };
    // a small rigid motion: the rotation of the quaternion (1, 0.01, 0.02, 0.03) normalised, and a shift
    double R[9];
    const double l = sqrt(1.0 + 0.0001 + 0.0004 + 0.0009);
    sh::quat_rot(1.0 / l, 0.01 / l, 0.02 / l, 0.03 / l, R);
    for (int i = 0; i < Q; ++i) {
      double p[3] = {rnd() * size[0], rnd() * size[1], rnd() * size[2]};
      p[(i % 6) / 2] = (i % 2) * size[(i % 6) / 2];
      for (int k = 0; k < 3; ++k) {
        truth[3 * i + k] = p[k];
        pts[3 * i + k] = ((R[3 * k] * p[0] + R[3 * k + 1] * p[1]) + R[3 * k + 2] * p[2]) + 0.1 * (k + 1);
      }
    }
    for (int metric : {SH_ICP_POINT, SH_ICP_PLANE}) {
      const sh_icp_options opt = {metric, metric == SH_ICP_PLANE ? 10 : 40, INFINITY, 0.0};
      sh_registration r;
      std::vector<double> hist(2 * (size_t)(opt.max_iter + 1));
      const int rc = ic_register(bv, bf, 12, pts.data(), Q, nullptr, &opt, &r, hist.data());
      const bool ok = rc == 0 && r.pairs == Q && r.iterations == opt.max_iter && r.rms <= r.rms_first && r.rms == hist[2 * opt.max_iter] &&
                      (metric == SH_ICP_POINT ? r.min_pivot == 1.0 : (r.min_pivot > 0.0 && r.min_pivot <= 1.0)) && (metric == SH_ICP_POINT || r.rms < 1e-9 || Q == 6);
      if (!ok) { printf("icp_check: box Q %d metric %d: rc %d pairs %d iterations %d rms %g first %g pivot %g\n", Q, metric, rc, r.pairs, r.iterations, r.rms, r.rms_first, r.min_pivot); return 1; }
    }
    // one face only under the plane metric: the system is exactly singular; five points: starved; everything rejected
    std::vector<double> flat(3 * (size_t)Q);
    for (int i = 0; i < Q; ++i) { flat[3 * i] = rnd() * 30; flat[3 * i + 1] = rnd() * 20; flat[3 * i + 2] = 10.5; }
    sh_registration r;
    double hist[2 * 4];
    sh_icp_options opt = {SH_ICP_PLANE, 3, INFINITY, 0.0};
    if (ic_register(bv, bf, 12, flat.data(), Q, nullptr, &opt, &r, hist) != SH_ERR_GEOMETRY || r.iterations != 0 || r.T[0] != 1.0 || r.T[3] != 0.0 || r.pairs != Q) {
      printf("icp_check: one face, Q %d: status %d iterations %d\n", Q, r.status, r.iterations); return 1;
    }
    if (ic_register(bv, bf, 12, pts.data(), Q < 5 ? Q : 5, nullptr, &opt, &r, hist) != SH_ERR_GEOMETRY || r.pairs != 5) { printf("icp_check: five points\n"); return 1; }
    opt.reject = 1e-30;
    if (ic_register(bv, bf, 12, pts.data(), Q, nullptr, &opt, &r, hist) != SH_ERR_GEOMETRY || r.pairs != 0 || r.rms != 0.0) { printf("icp_check: all rejected\n"); return 1; }
  }
  // the argument checks in their order
  const double pts[6] = {0, 0, 0, 1, 2, NAN};
  sh_icp_options opt = {SH_ICP_PLANE, 8, INFINITY, 0.0}, bad = {2, 8, 1.0, 0.0};
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, Tm[16], Ts[16], Tl[16];
  memcpy(Tm, T, sizeof T); memcpy(Ts, T, sizeof T); memcpy(Tl, T, sizeof T);
  Tm[0] = -1.0; Ts[1] = 1e-6; Tl[15] = 2.0;
  if (ic_precheck(1, pts, 1, 0, T, &opt, 1, 0) != SH_OK || ic_precheck(0, pts, 1, 0, T, &opt, 1, 0) != SH_ERR_ARG || ic_precheck(1, pts, 0, 0, T, &opt, 1, 0) != SH_ERR_ARG ||
      ic_precheck(1, pts, 1, 0, T, &bad, 0, 0) != SH_ERR_ARG || ic_precheck(1, pts, 1, 0, T, &opt, 0, 0) != SH_ERR_STATE || ic_precheck(1, pts, 1, 0, T, &opt, 1, 1) != SH_ERR_STATE ||
      ic_precheck(1, pts, 2, 0, T, &opt, 1, 0) != SH_ERR_ARG || ic_precheck(1, pts, 1, 0, Tm, &opt, 1, 0) != SH_ERR_ARG || ic_precheck(1, pts, 1, 0, Ts, &opt, 1, 0) != SH_ERR_ARG ||
      ic_precheck(1, pts, 1, 0, Tl, &opt, 1, 0) != SH_ERR_ARG) { printf("icp_check: precheck\n"); return 1; }
  printf("icp_check: ok\n");
  return 0;
}
