// Test shim (NOT product): the closest-point arithmetic of shoulder_amd/csrc/sh_scalar.h (closest_pt_tri, tri_point, closest_key_less,
// closest_side, cp_split_range -- the source k_closest.h runs on the device) and the argument checks and the face split of sh_query.h
// (precheck_closest, cp_splits) on the host, for tests/test_closest_host.py.  cc_mesh answers one point against a mesh as the two
// kernels do: the tiles of the mesh dealt to S splits by cp_split_range, each split folded into a partial with closest_key_less (the
// faces of a split walked backwards when asked: the order must not matter), the partials joined as k_cp_join joins them and the
// winner recomputed from its face alone.  Its own main() runs all of it on a tetrahedron and a tied pair of plates, so that the file
// can be built as a stand-alone program with -fsanitize=address,undefined.
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

extern "C" double cc_tri(const double* p, const double* tri /* 3 x 3 corners */, double* u, double* w, int* region) {
  const double ab[3] = {tri[3] - tri[0], tri[4] - tri[1], tri[5] - tri[2]}, ac[3] = {tri[6] - tri[0], tri[7] - tri[1], tri[8] - tri[2]};
  return sh::closest_pt_tri(p, tri, ab, ac, u, w, region);
}
extern "C" int cc_key_less(double d2a, int fa, double d2b, int fb) { return sh::closest_key_less(d2a, fa, d2b, fb) ? 1 : 0; }
extern "C" int cc_splits(long long groups, long long tiles) { return sh::cp_splits(groups, tiles); }
extern "C" void cc_split_range(int tiles, int S, int s, int* t0, int* t1) { sh::cp_split_range(tiles, S, s, t0, t1); }

// k_cp_walk and k_cp_join for one point and one mesh of float32 vertices
extern "C" void cc_mesh(const float* verts, const int* faces, int nf, const double* p, int S, int backwards, sh_closest* out) {
  const int tiles = (nf + sh::AR_CP_TILE - 1) / sh::AR_CP_TILE;
  std::vector<double> pd2((size_t)S, INFINITY);
  std::vector<int> pface((size_t)S, -1);
  for (int s = 0; s < S; ++s) {
    int t0, t1;
    sh::cp_split_range(tiles, S, s, &t0, &t1);
    const int f0 = t0 * sh::AR_CP_TILE, f1 = t1 * sh::AR_CP_TILE < nf ? t1 * sh::AR_CP_TILE : nf;
    for (int k = f0; k < f1; ++k) {
      const int f = backwards ? f1 - 1 - (k - f0) : k;
      double A[3], ab[3], ac[3], u, w;
      int region;
      face_of(verts, faces, f, A, ab, ac);
      const double d2 = sh::closest_pt_tri(p, A, ab, ac, &u, &w, &region);
      if (sh::closest_key_less(d2, f, pd2[s], pface[s])) { pd2[s] = d2; pface[s] = f; }
    }
  }
  double best = INFINITY;
  int best_f = -1;
  for (int s = 0; s < S; ++s)
    if (pface[s] >= 0 && sh::closest_key_less(pd2[s], pface[s], best, best_f)) { best = pd2[s]; best_f = pface[s]; }
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

// precheck_closest against a context that is there (or not), holds B humeri and has n_pending runs in flight
extern "C" int cc_precheck(int ctx, const double* points, int Q, int per_humerus, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_closest(points, Q, per_humerus, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st}).code;
}

// stand-alone run (sanitizer build): the tetrahedron (interior, edge, vertex, inside, on a face); two plates stored twice
int main() {
  const float tv[12] = {0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4};
  const int tf[12] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  struct Case { double p[3]; double dist; int face, region, side; double q[3]; };
  const Case cases[] = {
      {{1, 1, -2}, 2.0, 0, 0, 1, {1, 1, 0}},        // below the face z = 0: its interior
      {{2, -3, -4}, 5.0, 0, 3, 1, {2, 0, 0}},       // beside the edge y = z = 0: faces 0 and 1 tie, the smaller id wins (its edge CA)
      {{-2, -2, -1}, 3.0, 0, 4, 1, {0, 0, 0}},      // behind the vertex at the origin: three faces tie
      {{0.5, 0.5, 0.25}, 0.25, 0, 0, -1, {0.5, 0.5, 0}},      // inside the solid
      {{1, 1, 0}, 0.0, 0, 0, 1, {1, 1, 0}},         // on a face
  };
  for (const Case& c : cases)
    for (int S : {1, 3})
      for (int back : {0, 1}) {
        sh_closest o;
        cc_mesh(tv, tf, 4, c.p, S, back, &o);
        if (o.status != 0 || o.dist != c.dist || o.face != c.face || o.region != c.region || o.side != c.side || o.point[0] != c.q[0] || o.point[1] != c.q[1] ||
            o.point[2] != c.q[2]) {
          printf("closest_check: tetrahedron (%g %g %g): dist %g face %d region %d side %d\n", c.p[0], c.p[1], c.p[2], o.dist, o.face, o.region, o.side);
          return 1;
        }
      }
  // 300 plates z = k + 1, two triangles each, and the whole list stored a second time behind it: every face has a twin with a larger id
  const int P = 300;
  std::vector<float> pv(12 * (size_t)P);
  std::vector<int> pf(12 * (size_t)P);
  for (int k = 0; k < P; ++k) {
    const float z = (float)(k + 1), c[12] = {-1, -1, z, 1, -1, z, 1, 1, z, -1, 1, z};
    memcpy(&pv[12 * k], c, sizeof c);
    const int f[6] = {4 * k, 4 * k + 1, 4 * k + 2, 4 * k, 4 * k + 2, 4 * k + 3};
    memcpy(&pf[6 * k], f, sizeof f);
    memcpy(&pf[6 * (P + k)], f, sizeof f);
  }
  for (int S : {1, 2, 5})
    for (int back : {0, 1}) {
      sh_closest o;
      const double p[3] = {0.5, -0.25, 250.25};      // above the first triangle of plate 249 (z = 250): face 498 and its twin 1098
      cc_mesh(pv.data(), pf.data(), 4 * P, p, S, back, &o);
      if (o.face != 498 || o.dist != 0.25 || o.region != 0 || o.side != 1) { printf("closest_check: plates %d %g\n", o.face, o.dist); return 1; }
      const double e[3] = {0.25, 0.25, 0.5};         // below the diagonal of plate 0: faces 0, 1 and their twins tie on an edge
      cc_mesh(pv.data(), pf.data(), 4 * P, e, S, back, &o);
      if (o.face != 0 || o.dist != 0.5 || o.side != -1 || (o.region != 2 && o.region != 3)) { printf("closest_check: diagonal %d %g %d\n", o.face, o.dist, o.region); return 1; }
    }
  if (!sh::closest_key_less(1.0, 7, 1.0, 9) || sh::closest_key_less(1.0, 9, 1.0, 7) || sh::closest_key_less(NAN, 0, 1.0, 5) || !sh::closest_key_less(1.0, 5, NAN, 0) ||
      sh::closest_key_less(INFINITY, 0, NAN, 1) || sh::closest_key_less(NAN, 0, NAN, 1)) { printf("closest_check: key order\n"); return 1; }
  const double pts[6] = {0, 0, 0, 1, 2, NAN};
  if (cc_precheck(1, pts, 1, 0, 1, 0) != SH_OK || cc_precheck(1, pts, 2, 0, 1, 0) != SH_ERR_ARG || cc_precheck(1, pts, 0, 0, 1, 0) != SH_ERR_ARG ||
      cc_precheck(1, pts, 1, 0, 0, 0) != SH_ERR_STATE || cc_precheck(1, pts, 1, 0, 1, 1) != SH_ERR_STATE) { printf("closest_check: precheck\n"); return 1; }
  printf("closest_check: ok (tetrahedron %d cases, %d plates stored twice)\n", (int)(sizeof cases / sizeof cases[0]), P);
  return 0;
}
