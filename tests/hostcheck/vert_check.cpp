// Test shim (NOT product): the vertex-field rules of shoulder_amd/csrc/sh_scalar.h (vert_face, vert_gather, vert_smooth -- the source
// k_vert.h runs on the device) and, of sh_query.h, the argument checks of sh_vertex_fields and its buffer plan, on the host, for
// tests/test_vert_host.py.  vc_fields makes the buffers of one mesh as the kernels do: the face records and "vert.a2", the gather into
// the normals, the fields, the flags and the two raw planes, the rounds on four planes that are never re-initialised, the pack and the
// status.  Its own main() builds the incidence and the adjacency of a box, an open box, a fan and degenerate faces with the topo_*
// rules and walks them and the checks, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(SH_VERT_FIELDS == SH_VTX_FIELDS && SH_VERT_WEIGHT_ANGLE == SH_VTX_ANGLE && SH_VERT_USED == SH_VTX_USED && SH_VERT_BORDER == SH_VTX_BORDER &&
              SH_VERT_NONMANIFOLD == SH_VTX_NONMANIFOLD && SH_VERT_FLAT == SH_VTX_FLAT && sh::AR_VERT_FACE == SH_VTX_FACE, "the constants of sh_vertex_fields");

extern "C" void vc_fields(const float* verts, int nv, const int* faces, int nf, const int32_t* vrow /* nv + 1 */, const int32_t* vface /* 3 nf */,
                          const int32_t* adj /* 3 nf */, int weight, int smooth_rounds, double* frec /* 10 nf */, double* normals /* 3 nv */,
                          double* fields /* 8 nv */, int32_t* flags /* nv */, int32_t* status) {
  // k_vert_face
  std::vector<double> a2((size_t)nf + 1, 0.0);
  int state = 0;
  for (int f = 0; f < nf; ++f) {
    const int* fc = faces + 3 * (size_t)f;
    const bool deg = sh::topo_degenerate(fc, nv);
    double P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (!deg) sh::vert_corners(verts, fc, P);
    if (!sh::vert_face(P, deg, frec + SH_VTX_FACE * (size_t)f)) state = 1;
    a2[f] = frec[SH_VTX_FACE * (size_t)f + 3];
  }
  // k_vert_gather
  const size_t V = (size_t)nv;
  std::vector<double> plane(4 * V + 1, 0.0);
  for (int v = 0; v < nv; ++v) {
    double fl[5];
    sh::vert_gather(verts, faces, adj, frec, vface + vrow[v], vrow[v + 1] - vrow[v], v, weight, normals + 3 * (size_t)v, fl, flags + v);
    double* o = fields + SH_VTX_FIELDS * (size_t)v;
    for (int i = 0; i < 5; ++i) o[i] = fl[i];
    o[7] = 0.0;
    plane[v] = fl[3]; plane[V + v] = fl[4];
  }
  // k_vert_smooth, smooth_rounds times; k_vert_pack
  for (int r = 0; r < smooth_rounds; ++r) {
    const double* in = plane.data() + (size_t)(r & 1) * 2 * V;
    double* out = plane.data() + (size_t)((r + 1) & 1) * 2 * V;
    for (int v = 0; v < nv; ++v) sh::vert_smooth(faces, a2.data(), vface + vrow[v], vrow[v + 1] - vrow[v], in, in + V, out + v, out + V + v);
  }
  const double* fin = plane.data() + (size_t)(smooth_rounds & 1) * 2 * V;
  for (int v = 0; v < nv; ++v) { fields[SH_VTX_FIELDS * (size_t)v + 5] = fin[v]; fields[SH_VTX_FIELDS * (size_t)v + 6] = fin[V + v]; }
  *status = state ? 0 : SH_ERR_GEOMETRY;
}

// precheck_vertex_fields; the refusal's text to `text`
extern "C" int vc_precheck(int ctx, int weight, int smooth_rounds, int incidence, int B, int n_pending, char* text, int cap) {
  const sh::ArthroState st;
  const sh::ArthroError e = sh::precheck_vertex_fields(weight, smooth_rounds, incidence != 0, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: face blocks, vertex blocks, then the eight sizes of VERT_BUFS
extern "C" void vc_plan(int B, long long maxV, long long maxF, long long sumV, long long sumF, size_t* out) {
  const sh::VertPlan p = sh::vert_plan(B, maxV, maxF, sumV, sumF);
  size_t* o = out;
  *o++ = (size_t)p.fblocks; *o++ = (size_t)p.vblocks;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  VERT_BUFS(X)
#undef X
}

// ---- stand-alone run (sanitizer build) ----
struct Result {
  std::vector<double> face, normals, fields;
  std::vector<int32_t> flags;
  int32_t status;
};
// the incidence in ascending order and the adjacency by the topo_* rules, then vc_fields
static Result run(const std::vector<float>& v, const std::vector<int>& f, int weight, int rounds) {
  const int nv = (int)v.size() / 3, nf = (int)f.size() / 3;
  std::vector<int32_t> vrow((size_t)nv + 1, 0), vface(3 * (size_t)nf + 1, -1), adj(3 * (size_t)nf + 1, SH_TOPO_DEGENERATE);
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) ++vrow[f[3 * (size_t)i + k] + 1];
  for (int i = 0; i < nv; ++i) vrow[i + 1] += vrow[i];
  std::vector<int> cur(vrow.begin(), vrow.end());
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) vface[cur[f[3 * (size_t)i + k]]++] = i;
  for (int i = 0; i < nf; ++i) {
    if (sh::topo_degenerate(&f[3 * (size_t)i], nv)) continue;
    for (int e = 0; e < 3; ++e) {
      const int a = f[3 * (size_t)i + e];
      int owner, same;
      adj[3 * (size_t)i + e] = sh::topo_slot(f.data(), vface.data() + vrow[a], vrow[a + 1] - vrow[a], i, e, &owner, &same);
    }
  }
  Result r;
  r.face.resize(SH_VTX_FACE * (size_t)nf + 1); r.normals.resize(3 * (size_t)nv); r.fields.resize(SH_VTX_FIELDS * (size_t)nv); r.flags.resize((size_t)nv);
  vc_fields(v.data(), nv, f.data(), nf, vrow.data(), vface.data(), adj.data(), weight, rounds, r.face.data(), r.normals.data(), r.fields.data(), r.flags.data(), &r.status);
  return r;
}
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

int main() {
  const double PI = 3.141592653589793;
  std::vector<float> bv(24);
  const std::vector<int> bf = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  // the box: every defect pi / 2, the areas sum to its surface, Gauss-Bonnet gives 2, the normals point away from the centre
  for (int weight = 0; weight < 2; ++weight) {
    const Result r = run(bv, bf, weight, 3);
    double area = 0.0, defect = 0.0;
    for (int v = 0; v < 8; ++v) {
      const double* o = &r.fields[SH_VTX_FIELDS * (size_t)v];
      area += o[0]; defect += o[2];
      const double out = r.normals[3 * v] * ((v & 1) ? 1 : -1) + r.normals[3 * v + 1] * ((v & 2) ? 1 : -1) + r.normals[3 * v + 2] * ((v & 4) ? 1 : -1);
      const double len = sh::dot3(&r.normals[3 * v], &r.normals[3 * v]);
      if (!near(o[2], PI / 2, 1e-14) || !near(o[1], 3 * PI / 2, 1e-14) || r.flags[v] != SH_VERT_USED || !(out > 0.5) || !near(len, 1.0, 1e-14) || !(o[4] > 0.0) || o[7] != 0.0 ||
          !near(o[3], o[2] / o[0], 1e-15) || !(o[5] > 0.0) || !(o[6] > 0.0)) {
        printf("vert_check: box vertex %d (defect %.17g area %.17g flags %d)\n", v, o[2], o[0], r.flags[v]); return 1;
      }
    }
    if (r.status != 0 || !near(area, 2200.0, 1e-9) || !near(defect / (2 * PI), 2.0, 1e-14)) { printf("vert_check: box sums (%.17g %.17g)\n", area, defect); return 1; }
    if (r.face[3] != 600.0 || r.face[0] != 0.0 || r.face[2] != -600.0 || !near(r.face[4] + r.face[5] + r.face[6], PI, 1e-15)) { printf("vert_check: box face 0\n"); return 1; }
  }
  // without face 0: its three corners are border vertices and use pi
  {
    const std::vector<int> open(bf.begin() + 3, bf.end());
    const Result r = run(bv, open, 0, 0);
    int border = 0;
    for (int v = 0; v < 8; ++v) {
      const double* o = &r.fields[SH_VTX_FIELDS * (size_t)v];
      if (r.flags[v] & SH_VERT_BORDER) { ++border; if (!near(o[2], PI - o[1], 1e-15)) { printf("vert_check: border defect\n"); return 1; } }
      if (o[5] != o[3] || o[6] != o[4]) { printf("vert_check: no round, smoothed != raw\n"); return 1; }
    }
    if (border != 3 || !(r.flags[0] & SH_VERT_BORDER) || !(r.flags[1] & SH_VERT_BORDER) || !(r.flags[2] & SH_VERT_BORDER)) { printf("vert_check: open box (%d)\n", border); return 1; }
  }
  // a fan of 300 around vertex 0: one row of 300 faces
  {
    std::vector<float> av(3 * 302, 0.f);
    std::vector<int> af;
    for (int i = 0; i < 302; ++i) { av[3 * i] = (float)cos(0.02 * i) * (i ? 40.f : 0.f); av[3 * i + 1] = (float)sin(0.02 * i) * (i ? 40.f : 0.f); }
    av[2] = 25.f;
    for (int i = 1; i <= 300; ++i) { af.push_back(0); af.push_back(i); af.push_back(i + 1); }
    const Result r = run(av, af, 1, 2);
    if (r.status != 0 || r.flags[0] != (SH_VERT_USED | SH_VERT_BORDER) || !(r.fields[1] > 3.0) || !(r.normals[2] > 0.5)) { printf("vert_check: fan (%d %.17g)\n", r.flags[0], r.fields[1]); return 1; }
  }
  // degenerate faces around the box's; a face of zero area with distinct indices; only degenerate faces
  {
    std::vector<int> df = {0, 0, 1};
    df.insert(df.end(), bf.begin(), bf.end());
    df.insert(df.end(), {5, 7, 5});
    const Result plain = run(bv, bf, 0, 1), r = run(bv, df, 0, 1);
    if (memcmp(plain.fields.data(), r.fields.data(), plain.fields.size() * 8) != 0 || memcmp(plain.normals.data(), r.normals.data(), plain.normals.size() * 8) != 0 ||
        plain.flags != r.flags || r.face[3] != 0.0 || r.face[10 + 3] != 600.0) { printf("vert_check: degenerate faces take part\n"); return 1; }
    std::vector<float> fv = bv;
    fv.push_back(135.f); fv.push_back(-85.f); fv.push_back(410.f);
    std::vector<int> ff = bf;
    ff.insert(ff.end(), {0, 1, 8});
    const Result z = run(fv, ff, 0, 0);
    if (z.status != 0 || !(z.flags[0] & SH_VERT_FLAT) || !(z.flags[1] & SH_VERT_FLAT) || z.flags[8] != (SH_VERT_USED | SH_VERT_BORDER | SH_VERT_FLAT) || z.fields[8 * 8] != 0.0 ||
        z.fields[8 * 8 + 3] != 0.0 || z.normals[24] != 0.0 || z.face[10 * 12 + 3] != 0.0 || z.fields[0] != plain.fields[0]) { printf("vert_check: flat face (%d)\n", z.flags[8]); return 1; }
    const std::vector<int> only = {0, 1, 1, 2, 2, 3, 4, 5, 4, 6, 6, 6};
    const Result o = run(bv, only, 1, 2);
    bool zeros = o.status == SH_ERR_GEOMETRY;
    for (double x : o.fields) zeros = zeros && x == 0.0;
    for (double x : o.normals) zeros = zeros && x == 0.0;
    for (int x : o.flags) zeros = zeros && x == 0;
    if (!zeros) { printf("vert_check: only degenerate faces\n"); return 1; }
  }
  // the checks of sh_vertex_fields in their order, and the plan
  char text[256];
  auto pre = [&](int ctx, int weight, int rounds, int inc, int B, int pend) { return vc_precheck(ctx, weight, rounds, inc, B, pend, text, (int)sizeof text); };
  if (pre(1, 0, 0, 1, 1, 0) != SH_OK || pre(1, 1, 64, 1, 1, 0) != SH_OK || pre(0, 2, -1, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "no context") || pre(1, 2, 0, 0, 0, 0) != SH_ERR_ARG ||
      !strstr(text, "weight") || pre(1, -1, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, -1, 0, 0, 0) != SH_ERR_ARG || pre(1, 0, 65, 1, 1, 0) != SH_ERR_ARG ||
      pre(1, 0, 0, 0, 0, 0) != SH_ERR_STATE || pre(1, 0, 0, 0, 1, 1) != SH_ERR_STATE || !strstr(text, "in flight") || pre(1, 0, 0, 0, 1, 0) != SH_ERR_STATE ||
      !strstr(text, "sh_mesh_topology first")) {
    printf("vert_check: precheck_vertex_fields (%s)\n", text); return 1;
  }
  size_t plan[10];
  vc_plan(3, 300, 513, 900, 1200, plan);
  if (plan[0] != 3 || plan[1] != 2 || plan[2] != 96000 || plan[3] != 21600 || plan[4] != 57600 || plan[5] != 3600 || plan[6] != 12 || plan[7] != 9600 || plan[8] != 28800 ||
      plan[9] != 12) {
    printf("vert_check: plan\n"); return 1;
  }
  printf("vert_check: ok\n");
  return 0;
}
