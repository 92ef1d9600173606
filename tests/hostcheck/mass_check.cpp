// Test shim (NOT product): the mass-property arithmetic of shoulder_amd/csrc/sh_scalar.h (mass_face_terms, sym3_jacobi, mass_frame,
// mass_finish -- the source k_mass.h runs on the device) and, of sh_query.h, the argument checks of sh_mass_properties and
// sh_register_multistart, its pick rule, its subsample rule and its buffer plan, on the host, for tests/test_mass_host.py and
// tests/test_multistart_host.py.  mc_mass makes the record of one mesh as the kernels do: the terms of each block of 256 faces put
// through the tree slot[i] += slot[i + h], the block rows added in block order.  Its own main() measures a box, an open box and
// degenerate meshes and walks the checks, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(sizeof(sh_mass) == SH_MASS_DOUBLES * 8 + 16, "sh_mass: 48 doubles and four int32");

// the tree of one block: 256 slots, the missing ones +0.0
static double tree256(const double* vals, int n) {
  double slot[SH_MASS_BLOCK];
  for (int i = 0; i < SH_MASS_BLOCK; ++i) slot[i] = i < n ? vals[i] : 0.0;
  for (int h = SH_MASS_BLOCK / 2; h >= 1; h >>= 1)
    for (int i = 0; i < h; ++i) slot[i] += slot[i + h];
  return slot[0];
}

// k_mass_sum and k_mass_join for one mesh; rows: blocks x SH_MASS_TERMS (nullable)
extern "C" void mc_mass(const float* verts, int nv, const int* faces, int nf, sh_mass* out, double* rows) {
  const int blocks = (nf + SH_MASS_BLOCK - 1) / SH_MASS_BLOCK;
  double o[3] = {0.0, 0.0, 0.0}, tot[SH_MASS_TERMS];
  if (nv > 0) for (int k = 0; k < 3; ++k) o[k] = (double)verts[k];
  std::vector<double> terms((size_t)nf * SH_MASS_TERMS, 0.0), col(SH_MASS_BLOCK);
  for (int f = 0; f < nf; ++f) {
    double P[3][3];
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) P[j][k] = (double)verts[3 * (size_t)faces[3 * f + j] + k];
    sh::mass_face_terms(o, P[0], P[1], P[2], &terms[(size_t)f * SH_MASS_TERMS]);
  }
  for (int k = 0; k < SH_MASS_TERMS; ++k) tot[k] = 0.0;
  for (int blk = 0; blk < blocks; ++blk) {
    const int n = nf - blk * SH_MASS_BLOCK < SH_MASS_BLOCK ? nf - blk * SH_MASS_BLOCK : SH_MASS_BLOCK;
    for (int k = 0; k < SH_MASS_TERMS; ++k) {
      for (int i = 0; i < n; ++i) col[i] = terms[((size_t)blk * SH_MASS_BLOCK + i) * SH_MASS_TERMS + k];
      const double r = tree256(col.data(), n);
      if (rows) rows[(size_t)blk * SH_MASS_TERMS + k] = r;
      tot[k] += r;
    }
  }
  double rec[SH_MASS_DOUBLES];
  int irec[4];
  sh::mass_finish(tot, o, nf, rec, irec);
  memcpy(out, rec, sizeof rec);
  out->faces = irec[0]; out->degenerate = irec[1]; out->status = irec[2]; out->vstatus = irec[3];
}

extern "C" void mc_jacobi(double* A /* 9, in: the matrix, out: its diagonal holds the eigenvalues */, double* V /* 9 */) { sh::sym3_jacobi(A, V); }

extern "C" int mc_precheck_mass(int ctx, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_mass(sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st}).code;
}

// precheck_multistart; name_b / name_k: the humerus and the start the refusal must name (-1: do not look), returned as bit 16 when missing
extern "C" int mc_precheck_ms(int ctx, const double* points, int Q, int per_humerus, const double* T0s, int K, const sh_icp_options* coarse, int coarse_points,
                              int min_pairs, const sh_icp_options* fine, int B, int n_pending, char* text, int cap) {
  const sh::ArthroState st;
  const sh::ArthroError e = sh::precheck_multistart(points, Q, per_humerus, T0s, K, coarse, coarse_points, min_pairs, fine, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// the fold of k_ms_pick over n candidate records in ascending k -> the winner or -1
extern "C" int mc_pick(const sh_registration* cand, int n, int min_pairs) {
  int winner = -1;
  double best = 0.0;
  for (int k = 0; k < n; ++k)
    if (sh::ms_candidate_wins(cand[k].status, cand[k].pairs, cand[k].rms, min_pairs, winner, best)) { best = cand[k].rms; winner = k; }
  return winner;
}

extern "C" long long mc_coarse_index(int j, int Q, int Qc) { return sh::ms_coarse_index(j, Q, Qc); }

// out: Qc, blocks of the mass plan, the two mass sizes, the nine "icp.*" sizes of the multi-start plan, its five own sizes
extern "C" void mc_plan(int B, int Q, int per_humerus, long long maxF, int K, int coarse_points, int coarse_iter, int fine_iter, size_t* out) {
  const sh::MsPlan p = sh::ms_plan(B, Q, per_humerus != 0, maxF, K, coarse_points, coarse_iter, fine_iter);
  const sh::MassPlan m = sh::mass_plan(B, maxF);
  size_t* o = out;
  *o++ = (size_t)p.Qc; *o++ = (size_t)m.blocks;
#define X(f, name, T, elem) *o++ = m.bytes.f;
  MASS_BUFS(X)
#undef X
#define X(f, name, T, elem) *o++ = p.icp.f;
  ICP_BUFS(X)
#undef X
#define X(f, name, T, elem) *o++ = p.bytes.f;
  MS_BUFS(X)
#undef X
}

// stand-alone run (sanitizer build)
int main() {
  // the 30 x 20 x 10 box at integer CT coordinates: every product is an exact integer
  float bv[24];
  const int bf[36] = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  sh_mass r;
  double rows[SH_MASS_TERMS];
  mc_mass(bv, 8, bf, 12, &r, rows);
  if (r.status || r.vstatus || r.area != 2200.0 || r.volume != 6000.0 || r.closure != 0.0 || r.faces != 12 || r.degenerate != 0 ||
      fabs(r.center_mass[0] - 135.0) > 1e-12 || fabs(r.shell_axes[0]) != 1.0 || fabs(r.principal_axes[0]) != 1.0 || !(r.principal[0] < r.principal[1])) {
    printf("mass_check: box: status %d %d area %g volume %g closure %g\n", r.status, r.vstatus, r.area, r.volume, r.closure); return 1;
  }
  // the box without its top (faces 2 and 3): open, closure = cap area / area
  int open_f[30];
  memcpy(open_f, bf, 6 * sizeof(int)); memcpy(open_f + 6, bf + 12, 24 * sizeof(int));
  mc_mass(bv, 8, open_f, 10, &r, nullptr);
  if (r.status || r.area != 1600.0 || fabs(r.closure - 600.0 / 1600.0) > 1e-15) { printf("mass_check: open box: closure %g\n", r.closure); return 1; }
  // one face: a shell without a volume; a face of zero area alone: neither; no faces: neither
  const int one[3] = {0, 1, 2}, flat[3] = {0, 1, 1};
  mc_mass(bv, 8, one, 1, &r, nullptr);
  if (r.status != 0 || r.vstatus != SH_ERR_GEOMETRY || r.volume != 0.0 || r.area != 300.0) { printf("mass_check: one face\n"); return 1; }
  mc_mass(bv, 8, flat, 1, &r, nullptr);
  if (r.status != SH_ERR_GEOMETRY || r.vstatus != SH_ERR_GEOMETRY || r.degenerate != 1 || r.area != 0.0) { printf("mass_check: flat face\n"); return 1; }
  mc_mass(bv, 8, one, 0, &r, nullptr);
  if (r.status != SH_ERR_GEOMETRY || r.vstatus != SH_ERR_GEOMETRY || r.faces != 0) { printf("mass_check: no faces\n"); return 1; }
  // a mesh past one and two blocks: a fan of 513 faces about vertex 0
  std::vector<float> fv(3 * 515);
  std::vector<int> ff(3 * 513);
  for (int i = 0; i < 515; ++i) { fv[3 * i] = i == 0 ? 0.f : (float)cos(0.01 * i) * 40.f; fv[3 * i + 1] = i == 0 ? 0.f : (float)sin(0.01 * i) * 40.f; fv[3 * i + 2] = i == 0 ? 25.f : 0.f; }
  for (int i = 0; i < 513; ++i) { ff[3 * i] = 0; ff[3 * i + 1] = i + 1; ff[3 * i + 2] = i + 2; }
  std::vector<double> frows(3 * SH_MASS_TERMS);
  for (int nf : {255, 256, 257, 513}) {
    mc_mass(fv.data(), 515, ff.data(), nf, &r, frows.data());
    if (r.status || r.faces != nf || !(r.area > 0.0) || !(r.closure > 1e-3)) { printf("mass_check: fan %d: status %d area %g closure %g\n", nf, r.status, r.area, r.closure); return 1; }
  }
  // the checks of sh_mass_properties and sh_register_multistart in their order, and the pick rule
  if (mc_precheck_mass(0, 1, 0) != SH_ERR_ARG || mc_precheck_mass(1, 0, 0) != SH_ERR_STATE || mc_precheck_mass(1, 1, 1) != SH_ERR_STATE || mc_precheck_mass(1, 1, 0) != SH_OK) {
    printf("mass_check: precheck_mass\n"); return 1;
  }
  const double pts[6] = {0, 0, 0, 1, 2, NAN};
  const sh_icp_options opt = {SH_ICP_PLANE, 4, INFINITY, 0.0}, bad = {2, 4, 1.0, 0.0};
  double T[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, Tb[32];
  memcpy(Tb, T, sizeof T);
  Tb[16] = -1.0;
  char text[256];
  auto pre = [&](int ctx, const double* p, int Q, const double* T0s, int K, const sh_icp_options* co, int cp, int mp, const sh_icp_options* fi, int B, int pend) {
    return mc_precheck_ms(ctx, p, Q, 0, T0s, K, co, cp, mp, fi, B, pend, text, (int)sizeof text);
  };
  if (pre(1, pts, 1, T, 2, &opt, 0, 6, &opt, 1, 0) != SH_OK || pre(0, pts, 1, T, 2, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG || pre(1, pts, 1, nullptr, 2, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG ||
      pre(1, pts, 0, T, 2, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG || pre(1, pts, 1, T, 0, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG || pre(1, pts, 1, T, 65, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG ||
      pre(1, pts, 1, T, 2, &opt, -1, 6, &opt, 1, 0) != SH_ERR_ARG || pre(1, pts, 1, T, 2, &opt, 0, 5, &opt, 1, 0) != SH_ERR_ARG || pre(1, pts, 1, T, 2, &bad, 0, 6, &opt, 0, 0) != SH_ERR_ARG ||
      pre(1, pts, 1, T, 2, &opt, 0, 6, &bad, 0, 0) != SH_ERR_ARG || pre(1, pts, 1, T, 2, &opt, 0, 6, &opt, 0, 0) != SH_ERR_STATE || pre(1, pts, 1, T, 2, &opt, 0, 6, &opt, 1, 1) != SH_ERR_STATE ||
      pre(1, pts, 2, T, 2, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG || pre(1, pts, 1, Tb, 2, &opt, 0, 6, &opt, 1, 0) != SH_ERR_ARG || !strstr(text, "start 1 of humerus 0")) {
    printf("mass_check: precheck_multistart (%s)\n", text); return 1;
  }
  sh_registration cand[4];
  memset(cand, 0, sizeof cand);
  for (int k = 0; k < 4; ++k) { cand[k].pairs = 10; cand[k].rms = 2.0; }
  cand[2].rms = 1.0; cand[3].rms = 1.0;
  if (mc_pick(cand, 4, 6) != 2) { printf("mass_check: pick order\n"); return 1; }
  cand[2].status = SH_ERR_GEOMETRY; cand[3].pairs = 5;
  if (mc_pick(cand, 4, 6) != 0) { printf("mass_check: pick exclusions\n"); return 1; }
  if (mc_pick(cand, 4, 11) != -1) { printf("mass_check: no winner\n"); return 1; }
  printf("mass_check: ok\n");
  return 0;
}
