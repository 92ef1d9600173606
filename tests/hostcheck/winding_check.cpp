// Test shim (NOT product): the winding-number arithmetic of shoulder_amd/csrc/sh_scalar.h (solid_angle_terms, solid_angle_tri,
// winding_record, cp_split_range -- the source k_winding.h runs on the device) and the argument checks and the split of sh_query.h
// (precheck_winding, wn_splits, wn_plan) on the host, for tests/test_winding_host.py.  wc_mesh answers points against a mesh as the
// two kernels do: the blocks of 2048 faces dealt to S splits by cp_split_range, each block summed from 0 in face order, and the block
// sums either stored and added in block order by the join (S > 1) or added by the walk itself (S == 1).  Its own main() runs all of it
// on the cube of edge 2, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static void corners_of(const float* verts, const int* faces, int f, double* V) {
  for (int j = 0; j < 3; ++j) {
    const float* v = verts + 3 * (size_t)faces[3 * f + j];
    V[3 * j] = (double)v[0]; V[3 * j + 1] = (double)v[1]; V[3 * j + 2] = (double)v[2];
  }
}

extern "C" double wc_solid(const double* p, const double* tri /* 3 x 3 corners */, double* num, double* den) {
  sh::solid_angle_terms(p, tri, tri + 3, tri + 6, num, den);
  return sh::solid_angle_tri(p, tri, tri + 3, tri + 6);
}
extern "C" int wc_splits(long long groups, long long blocks) { return sh::wn_splits(groups, blocks); }
extern "C" void wc_split_range(int blocks, int S, int s, int* k0, int* k1) { sh::cp_split_range(blocks, S, s, k0, k1); }
extern "C" void wc_plan(int B, int Q, long long maxF, int* out /* kmax, chunks, S, stride */) {
  const sh::WnPlan pl = sh::wn_plan(B, Q, false, maxF);
  out[0] = pl.kmax; out[1] = pl.chunks; out[2] = pl.S; out[3] = pl.stride;
}

// k_wn_walk and k_wn_join for nq points and one mesh of float32 vertices
extern "C" void wc_mesh(const float* verts, const int* faces, int nf, const double* points, int nq, int S, sh_winding* out) {
  const int blocks = (nf + sh::AR_WN_BLOCK - 1) / sh::AR_WN_BLOCK;
  const int stride = S == 1 ? 1 : (blocks > 1 ? blocks : 1);
  std::vector<double> part((size_t)stride);
  for (int q = 0; q < nq; ++q) {
    const double* p = points + 3 * (size_t)q;
    for (int s = 0; s < S; ++s) {      // the workgroups of one chunk and humerus
      int k0, k1;
      sh::cp_split_range(blocks, S, s, &k0, &k1);
      double total = 0.0;
      for (int k = k0; k < k1; ++k) {
        double sum = 0.0;
        const int f1 = (k + 1) * sh::AR_WN_BLOCK < nf ? (k + 1) * sh::AR_WN_BLOCK : nf;
        for (int f = k * sh::AR_WN_BLOCK; f < f1; ++f) {
          double V[9];
          corners_of(verts, faces, f, V);
          sum += sh::solid_angle_tri(p, V, V + 3, V + 6);
        }
        if (S == 1) total += sum;
        else part[(size_t)k] = sum;
      }
      if (S == 1) part[0] = total;
    }
    double total;
    if (S == 1) total = part[0];
    else { total = 0.0; for (int k = 0; k < blocks; ++k) total += part[(size_t)k]; }
    int inside, status;
    sh::winding_record(total, &out[q].winding, &inside, &status, SH_ERR_GEOMETRY);
    out[q].inside = inside; out[q].status = status;
  }
}

// precheck_winding against a context that is there (or not), holds B humeri and has n_pending runs in flight
extern "C" int wc_precheck(int ctx, const double* points, int Q, int per_humerus, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_winding(points, Q, per_humerus, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st}).code;
}

// stand-alone run (sanitizer build): the cube of edge 2 about the origin -- closed, open, doubled, reversed -- and 3 000 copies of it
// in one mesh (two blocks), whose winding number at the centre is 3 000 whatever the split
int main() {
  const float cv[24] = {-1, -1, -1, 1, -1, -1, -1, 1, -1, 1, 1, -1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1};
  const int cf[36] = {0, 2, 3, 0, 3, 1, 0, 1, 5, 0, 5, 4, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5, 2, 6, 7, 2, 7, 3, 4, 5, 7, 4, 7, 6};
  const double centre[3] = {0, 0, 0}, outside[3] = {3, 1, 1}, on_face[3] = {0, 0.5, 1}, far[3] = {5.773502691896258e199, -5.773502691896258e199, 5.773502691896258e199}, axis[3] = {1e200, 0, 0};
  const double eps = 16 * 0x1p-53;
  sh_winding o;
  for (int f = 0; f < 12; ++f) {
    double V[9];
    corners_of(cv, cf, f, V);
    const double om = sh::solid_angle_tri(centre, V, V + 3, V + 6);
    if (fabs(om - 4.0 * M_PI / 12.0) > eps) { printf("winding_check: triangle %d subtends %.17g\n", f, om); return 1; }
  }
  wc_mesh(cv, cf, 12, centre, 1, 1, &o);
  if (fabs(o.winding - 1.0) > eps || o.inside != 1 || o.status != 0) { printf("winding_check: closed %.17g\n", o.winding); return 1; }
  wc_mesh(cv, cf, 10, centre, 1, 1, &o);
  if (fabs(o.winding - 5.0 / 6.0) > eps || o.inside != 1) { printf("winding_check: open %.17g\n", o.winding); return 1; }
  wc_mesh(cv, cf, 12, outside, 1, 1, &o);
  if (fabs(o.winding) > eps || o.inside != 0) { printf("winding_check: outside %.17g\n", o.winding); return 1; }
  wc_mesh(cv, cf, 12, on_face, 1, 1, &o);
  if (fabs(o.winding - 0.5) > eps) { printf("winding_check: on a face %.17g\n", o.winding); return 1; }
  wc_mesh(cv, cf, 12, far, 1, 1, &o);
  if (o.status != SH_ERR_GEOMETRY || o.winding != 0.0 || o.inside != 0) { printf("winding_check: far %d %.17g\n", o.status, o.winding); return 1; }
  wc_mesh(cv, cf, 12, axis, 1, 1, &o);      // one huge coordinate: num stays finite, den is +inf, every term is 0
  if (o.status != 0 || o.winding != 0.0 || o.inside != 0) { printf("winding_check: along an axis %d %.17g\n", o.status, o.winding); return 1; }
  int rf[36];
  for (int f = 0; f < 12; ++f) { rf[3 * f] = cf[3 * f + 2]; rf[3 * f + 1] = cf[3 * f + 1]; rf[3 * f + 2] = cf[3 * f]; }
  wc_mesh(cv, rf, 12, centre, 1, 1, &o);
  if (fabs(o.winding + 1.0) > eps || o.inside != 1) { printf("winding_check: reversed %.17g\n", o.winding); return 1; }
  const int N = 3000;
  std::vector<int> mf(36 * (size_t)N);
  for (int k = 0; k < N; ++k) memcpy(&mf[36 * (size_t)k], cf, sizeof cf);
  sh_winding first;
  for (int S : {1, 2, 5, 18}) {
    const double pts[6] = {0, 0, 0, 0.25, -0.5, 0.125};
    sh_winding two[2];
    wc_mesh(cv, mf.data(), 12 * N, pts, 2, S, two);
    if (fabs(two[0].winding - N) > 36.0 * N * 0x1p-53 * N || two[1].inside != 1) { printf("winding_check: %d cubes, S %d: %.17g\n", N, S, two[0].winding); return 1; }
    if (S == 1) first = two[1];
    else if (memcmp(&first, &two[1], sizeof first) != 0) { printf("winding_check: S %d changes bytes\n", S); return 1; }
  }
  if (sh::wn_splits(1, 1) != 1 || sh::wn_splits(1, 16) != 16 || sh::wn_splits(64, 16) != 16 || sh::wn_splits(64, 1016) != 16 || sh::wn_splits(4096, 1016) != 1 ||
      sh::wn_splits(1, 1016) != 1016) { printf("winding_check: splits\n"); return 1; }
  const double pts[6] = {0, 0, 0, 1, 2, NAN};
  if (wc_precheck(1, pts, 1, 0, 1, 0) != SH_OK || wc_precheck(1, pts, 2, 0, 1, 0) != SH_ERR_ARG || wc_precheck(1, pts, 0, 0, 1, 0) != SH_ERR_ARG ||
      wc_precheck(1, pts, 1, 0, 0, 0) != SH_ERR_STATE || wc_precheck(1, pts, 1, 0, 1, 1) != SH_ERR_STATE) { printf("winding_check: precheck\n"); return 1; }
  printf("winding_check: ok (the cube closed, open, reversed, from outside, on a face, from 1e200; %d cubes in one mesh)\n", N);
  return 0;
}
