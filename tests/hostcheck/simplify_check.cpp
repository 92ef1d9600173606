// Test shim (NOT product): the simplification rules of shoulder_amd/csrc/sh_scalar.h (simp_grid, simp_cell, simp_key, simp_unkey,
// simp_center, simp_face_quadric, simp_solve, simp_triple, simp_move -- the source k_simplify.h runs on the device) and, of sh_query.h,
// the argument checks of sh_mesh_simplify and its buffer plan, on the host, for tests/test_simplify_host.py.  sc_simplify makes the
// buffers of one mesh as the kernels do, on the incidence it is handed: the box of the used vertices as topo_enc words, the keys, a sort
// of the keys alone, the heads and their scan, the key and first place of every cluster, the bisection of every vertex, the second sort of
// (cluster << 32 | vertex), the vertex quadrics over the rows, the cluster sums over the member lists and the solve, the faces with the
// duplicate search through the rows of the smallest cluster's members, the two compactions and the record.  Its own main() walks a box
// at three cells, two sheets, a refused grid and the checks, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(sizeof(sh_simplify_options) == 24 && sizeof(sh_simplify_info) == 64, "the records of sh_mesh_simplify");
static_assert(SH_SIMPLIFY_QUADRIC == SH_SIMP_QUADRIC && SH_SIMPLIFY_MAX_CELLS == SH_SIMP_MAX_CELLS && SH_SIMPLIFY_MAX_CLUSTERS == SH_SIMP_MAX_CLUSTERS, "the modes of sh_mesh_simplify");

typedef unsigned long long u64;

extern "C" void sc_simplify(const float* verts, int nv, const int* faces, int nf, const int32_t* vrow /* nv + 1 */, const int32_t* vface, double h, int place, double reg,
                            double clamp, sh_simplify_info* info, float* overts /* 3 nv */, int32_t* ofaces /* 3 nf */, int32_t* map /* nv */, u64* key_out /* nv */,
                            int32_t* cid /* nv */, double* quad /* 10 nv */, float* pos /* 3 nv */) {
  memset(info, 0, sizeof *info);
  memset(overts, 0, (size_t)nv * 12); memset(ofaces, 0, (size_t)nf * 12); memset(quad, 0, (size_t)nv * SH_SIMP_Q * 8); memset(pos, 0, (size_t)nv * 12);
  info->cell = h;
  // k_simp_box
  unsigned box[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};
  int U = 0;
  for (int v = 0; v < nv; ++v) {
    if (vrow[v + 1] <= vrow[v]) continue;
    ++U;
    for (int k = 0; k < 3; ++k) {
      const unsigned e = sh::topo_enc(verts[3 * (size_t)v + k]);
      box[k] = e < box[k] ? e : box[k]; box[3 + k] = e > box[3 + k] ? e : box[3 + k];
    }
  }
  float lo[3], hi[3];
  for (int k = 0; k < 3; ++k) { lo[k] = sh::topo_dec(box[k]); hi[k] = sh::topo_dec(box[3 + k]); }
  long long n[3] = {0, 0, 0};
  const bool ok = U > 0 && sh::simp_grid(lo, hi, h, n);
  const bool grid_refused = U > 0 && !ok;
  // k_simp_key, the first sort, k_simp_heads, k_simp_scan, k_simp_ukey
  std::vector<u64> key((size_t)nv), sorted;
  for (int v = 0; v < nv; ++v) {
    u64 k = SH_SIMP_NO_KEY;
    if (ok && vrow[v + 1] > vrow[v]) {
      long long i[3];
      for (int a = 0; a < 3; ++a) i[a] = sh::simp_cell(verts[3 * (size_t)v + a], lo[a], h, n[a]);
      k = sh::simp_key(i, n);
    }
    key[v] = k;
    key_out[v] = k;
  }
  sorted = key;
  std::sort(sorted.begin(), sorted.end());
  std::vector<u64> ukey;
  std::vector<int> start;
  for (int i = 0; i < nv; ++i)
    if (sorted[i] != SH_SIMP_NO_KEY && (i == 0 || sorted[i - 1] != sorted[i])) { ukey.push_back(sorted[i]); start.push_back(i); }
  const int C = (int)ukey.size();
  const bool refused = grid_refused || C > SH_SIMP_MAX_CLUSTERS;
  // k_simp_assign, the second sort
  for (int v = 0; v < nv; ++v) {
    int c = -1;
    if (key[v] != SH_SIMP_NO_KEY && !refused) {
      int a = 0, b = C - 1;
      while (a < b) {
        const int mid = a + (b - a) / 2;
        if (ukey[mid] < key[v]) a = mid + 1; else b = mid;
      }
      c = a;
    }
    cid[v] = c;
    key[v] = c >= 0 ? ((u64)(unsigned)c << 32) | (u64)(unsigned)v : SH_SIMP_NO_KEY;
  }
  sorted = key;
  std::sort(sorted.begin(), sorted.end());
  auto members = [&](int c, int* i0, int* i1) { *i0 = start[c]; *i1 = c + 1 < C ? start[c + 1] : U; };
  auto corners = [&](int f, double* A, double* B, double* Cc) {
    for (int k = 0; k < 3; ++k) {
      A[k] = (double)verts[3 * (size_t)faces[3 * (size_t)f] + k]; B[k] = (double)verts[3 * (size_t)faces[3 * (size_t)f + 1] + k];
      Cc[k] = (double)verts[3 * (size_t)faces[3 * (size_t)f + 2] + k];
    }
  };
  // k_simp_quadric
  for (int v = 0; v < nv; ++v) {
    if (cid[v] < 0) continue;
    double o[3], q[SH_SIMP_Q] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < 3; ++a) o[a] = sh::simp_center(sh::simp_cell(verts[3 * (size_t)v + a], lo[a], h, n[a]), lo[a], h);
    for (int i = vrow[v]; i < vrow[v + 1]; ++i) {
      double A[3], B[3], Cc[3];
      corners(vface[i], A, B, Cc);
      sh::simp_face_quadric(A, B, Cc, o, q);
    }
    for (int k = 0; k < SH_SIMP_Q; ++k) quad[SH_SIMP_Q * (size_t)v + k] = q[k];
  }
  // k_simp_cluster
  int fallbacks = 0, largest = 0;
  for (int c = 0; c < C && !refused; ++c) {
    int i0, i1;
    members(c, &i0, &i1);
    double S[3] = {0, 0, 0}, q[SH_SIMP_Q] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = i0; i < i1; ++i) {
      const size_t v = (size_t)(unsigned)(sorted[i] & 0xffffffffull);
      for (int k = 0; k < 3; ++k) S[k] = S[k] + (double)verts[3 * v + k];
      for (int k = 0; k < SH_SIMP_Q; ++k) q[k] = q[k] + quad[SH_SIMP_Q * v + k];
    }
    const double count = (double)(i1 - i0);
    double m[3], o[3], x[3];
    long long ic[3];
    sh::simp_unkey(ukey[c], n, ic);
    for (int k = 0; k < 3; ++k) { m[k] = S[k] / count; o[k] = sh::simp_center(ic[k], lo[k], h); }
    bool solved = false;
    if (place == SH_SIMP_QUADRIC) {
      solved = sh::simp_solve(q, m, o, h, reg, clamp, x);
      if (!solved) ++fallbacks;
    }
    for (int k = 0; k < 3; ++k) pos[3 * (size_t)c + k] = solved ? (float)(o[k] + x[k]) : (float)m[k];
    largest = i1 - i0 > largest ? i1 - i0 : largest;
  }
  // k_simp_faces
  std::vector<int> keep((size_t)nf + 1, 0), named((size_t)nv + 1, 0);
  int collapsed = 0, duplicate = 0;
  for (int f = 0; f < nf && !refused; ++f) {
    const int* t = faces + 3 * (size_t)f;
    if (sh::topo_degenerate(t, nv)) continue;
    int s[3];
    if (!sh::simp_triple(cid[t[0]], cid[t[1]], cid[t[2]], s)) { ++collapsed; continue; }
    int i0 = 0, i1 = 0;
    for (int k = 0; k < 3; ++k) {
      int j0, j1;
      members(s[k], &j0, &j1);
      if (k == 0 || j1 - j0 < i1 - i0) { i0 = j0; i1 = j1; }
    }
    bool dup = false;
    for (int i = i0; i < i1 && !dup; ++i) {
      const size_t u = (size_t)(unsigned)(sorted[i] & 0xffffffffull);
      for (int j = vrow[u]; j < vrow[u + 1]; ++j) {
        const int g = vface[j];
        if (g >= f) break;
        const int* tg = faces + 3 * (size_t)g;
        int sg[3];
        if (sh::simp_triple(cid[tg[0]], cid[tg[1]], cid[tg[2]], sg) && sg[0] == s[0] && sg[1] == s[1] && sg[2] == s[2]) { dup = true; break; }
      }
    }
    if (dup) { ++duplicate; continue; }
    keep[f] = 1;
    for (int k = 0; k < 3; ++k) named[s[k]] = 1;
  }
  // the two scans, k_simp_emit
  std::vector<int> frank((size_t)nf + 1, 0), vrank((size_t)nv + 1, 0);
  int faces_out = 0, verts_out = 0;
  for (int f = 0; f < nf; ++f) { frank[f] = faces_out; faces_out += keep[f]; }
  for (int c = 0; c < nv; ++c) { vrank[c] = verts_out; verts_out += named[c]; }
  for (int f = 0; f < nf; ++f)
    if (keep[f])
      for (int k = 0; k < 3; ++k) ofaces[3 * (size_t)frank[f] + k] = vrank[cid[faces[3 * (size_t)f + k]]];
  for (int c = 0; c < (refused ? 0 : C); ++c)
    if (named[c])
      for (int k = 0; k < 3; ++k) overts[3 * (size_t)vrank[c] + k] = pos[3 * (size_t)c + k];
  double move = 0.0;
  for (int v = 0; v < nv; ++v) {
    const int c = cid[v];
    map[v] = c >= 0 && named[c] ? vrank[c] : -1;
    if (c >= 0) {
      const double d = sh::simp_move(verts + 3 * (size_t)v, pos + 3 * (size_t)c);
      move = d > move ? d : move;
    }
  }
  // k_simp_info
  info->status = refused ? SH_ERR_CAPACITY : faces_out == 0 ? SH_ERR_GEOMETRY : 0;
  info->verts_used = U; info->clusters = C; info->verts_out = verts_out; info->faces_out = faces_out; info->faces_collapsed = collapsed;
  info->faces_duplicate = duplicate; info->fallbacks = fallbacks; info->largest_cluster = largest; info->max_move = move;
}

// cells: B values, or null
extern "C" int sc_precheck(int ctx, int have_opt, int place, int reserved, double reg, double clamp, int have_cell, const double* cells, int incidence, int B, int n_pending,
                           char* text, int cap) {
  const sh::ArthroState st;
  const sh_simplify_options opt = {place, reserved, reg, clamp};
  const sh::ArthroError e = sh::precheck_simplify(have_opt ? &opt : nullptr, have_cell ? cells : nullptr, incidence != 0, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: blocks, vblocks, fblocks, the B + 1 segments, then the eighteen sizes of SIMPLIFY_BUFS -> the plan's code
extern "C" int sc_plan(int B, const long long* voff, const long long* foff, size_t* out) {
  long long maxV = 0, maxF = 0;
  for (int b = 0; b < B; ++b) {
    maxV = voff[b + 1] - voff[b] > maxV ? voff[b + 1] - voff[b] : maxV;
    maxF = foff[b + 1] - foff[b] > maxF ? foff[b + 1] - foff[b] : maxF;
  }
  sh::SimplifyPlan p;
  const sh::ArthroError e = sh::simplify_plan(B, maxV, maxF, voff, foff[B], &p);
  if (e.code) return e.code;
  size_t* o = out;
  *o++ = (size_t)p.blocks; *o++ = (size_t)p.vblocks; *o++ = (size_t)p.fblocks;
  for (unsigned x : p.seg) *o++ = (size_t)x;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  SIMPLIFY_BUFS(X)
#undef X
  return 0;
}

// the sizes of the two records, then the offsets of every field in the header's order: options (4), info (13)
extern "C" void sc_sizes(int* out) {
  int* o = out;
  *o++ = (int)sizeof(sh_simplify_options); *o++ = (int)sizeof(sh_simplify_info);
#define OFF(T, f) *o++ = (int)offsetof(T, f);
  OFF(sh_simplify_options, place) OFF(sh_simplify_options, reserved) OFF(sh_simplify_options, reg) OFF(sh_simplify_options, clamp)
  OFF(sh_simplify_info, status) OFF(sh_simplify_info, verts_used) OFF(sh_simplify_info, clusters) OFF(sh_simplify_info, verts_out) OFF(sh_simplify_info, faces_out)
  OFF(sh_simplify_info, faces_collapsed) OFF(sh_simplify_info, faces_duplicate) OFF(sh_simplify_info, fallbacks) OFF(sh_simplify_info, largest_cluster)
  OFF(sh_simplify_info, reserved) OFF(sh_simplify_info, cell) OFF(sh_simplify_info, max_move) OFF(sh_simplify_info, pad)
#undef OFF
}

// ---- stand-alone run (sanitizer build) ----
struct Result {
  sh_simplify_info info;
  std::vector<float> verts, pos;
  std::vector<int> faces, map, cid;
};

// the incidence rows of a mesh: the non-degenerate faces of every vertex, ascending
static void incidence(const std::vector<int>& f, int nv, std::vector<int>* vrow, std::vector<int>* vface) {
  const int nf = (int)f.size() / 3;
  vrow->assign((size_t)nv + 1, 0);
  vface->assign(3 * (size_t)nf + 1, -1);
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) ++(*vrow)[f[3 * (size_t)i + k] + 1];
  for (int v = 0; v < nv; ++v) (*vrow)[v + 1] += (*vrow)[v];
  std::vector<int> cur(vrow->begin(), vrow->end() - 1);
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) (*vface)[cur[f[3 * (size_t)i + k]]++] = i;
}

static Result run(const std::vector<float>& v, const std::vector<int>& f, double h, int place) {
  const int nv = (int)v.size() / 3, nf = (int)f.size() / 3;
  std::vector<int> vrow, vface;
  incidence(f, nv, &vrow, &vface);
  Result r;
  r.verts.resize(3 * (size_t)nv + 3); r.pos.resize(3 * (size_t)nv + 3); r.faces.resize(3 * (size_t)nf + 3); r.map.resize((size_t)nv + 1); r.cid.resize((size_t)nv + 1);
  std::vector<u64> key((size_t)nv + 1);
  std::vector<double> quad(SH_SIMP_Q * (size_t)nv + 1);
  sc_simplify(v.data(), nv, f.data(), nf, vrow.data(), vface.data(), h, place, 1e-3, 1.0, &r.info, r.verts.data(), r.faces.data(), r.map.data(), key.data(), r.cid.data(),
              quad.data(), r.pos.data());
  return r;
}

int main() {
  std::vector<float> bv(24);
  const std::vector<int> bf = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  // a cell below every edge: every vertex its own cluster, the faces renumbered in key order, nothing moves under the mean
  Result r = run(bv, bf, 5.0, SH_SIMPLIFY_MEAN);
  if (r.info.status || r.info.clusters != 8 || r.info.verts_out != 8 || r.info.faces_out != 12 || r.info.faces_collapsed || r.info.faces_duplicate || r.info.max_move != 0.0 ||
      r.info.largest_cluster != 1 || memcmp(r.verts.data(), bv.data(), 96) != 0 || memcmp(r.faces.data(), bf.data(), 144) != 0) {
    printf("simplify_check: box at 5 mm (clusters %d faces %d move %.17g)\n", r.info.clusters, r.info.faces_out, r.info.max_move); return 1;
  }
  // the quadric of a box corner is met at the corner itself: the three planes cross there
  r = run(bv, bf, 5.0, SH_SIMPLIFY_QUADRIC);
  if (r.info.status || r.info.faces_out != 12 || !(r.info.max_move < 1e-3)) { printf("simplify_check: box, quadric (move %.17g fallbacks %d)\n", r.info.max_move, r.info.fallbacks); return 1; }
  // a cell above the diagonal: one cluster, every face collapsed
  r = run(bv, bf, 100.0, SH_SIMPLIFY_QUADRIC);
  if (r.info.status != SH_ERR_GEOMETRY || r.info.clusters != 1 || r.info.faces_out || r.info.verts_out || r.info.faces_collapsed != 12 || r.info.largest_cluster != 8 || r.map[0] != -1) {
    printf("simplify_check: box at 100 mm (status %d)\n", r.info.status); return 1;
  }
  // a cell that gives more than 2^20 cells on an axis
  r = run(bv, bf, 1e-5, SH_SIMPLIFY_QUADRIC);
  if (r.info.status != SH_ERR_CAPACITY || r.info.verts_used != 8 || r.info.clusters || r.info.faces_out || r.map[7] != -1) { printf("simplify_check: refused grid (status %d)\n", r.info.status); return 1; }
  // two coincident copies of the box's faces on vertices half a millimetre apart: every second face is a duplicate, the smaller index stays
  std::vector<float> tv = bv;
  for (int i = 0; i < 8; ++i) { tv.push_back(bv[3 * i] + 0.5f); tv.push_back(bv[3 * i + 1]); tv.push_back(bv[3 * i + 2]); }
  std::vector<int> tf;
  for (int i = 0; i < 12; ++i) {
    for (int k = 0; k < 3; ++k) tf.push_back(bf[3 * i + k]);
    for (int k = 0; k < 3; ++k) tf.push_back(bf[3 * i + k] + 8);
  }
  r = run(tv, tf, 5.0, SH_SIMPLIFY_MEAN);
  if (r.info.status || r.info.clusters != 8 || r.info.faces_out != 12 || r.info.faces_duplicate != 12 || r.info.largest_cluster != 2 || memcmp(r.faces.data(), bf.data(), 144) != 0) {
    printf("simplify_check: doubled box (faces %d duplicates %d)\n", r.info.faces_out, r.info.faces_duplicate); return 1;
  }
  char text[256];
  const double good[2] = {2.0, 0.5}, zero[2] = {2.0, 0.0}, nan[2] = {NAN, 1.0};
  auto pre = [&](int ctx, int opt, int place, int reserved, double reg, double clamp, const double* cells, int inc, int B, int pend) {
    return sc_precheck(ctx, opt, place, reserved, reg, clamp, cells != nullptr, cells, inc, B, pend, text, (int)sizeof text);
  };
  if (pre(1, 1, 1, 0, 1e-3, 1.0, good, 1, 2, 0) != SH_OK || pre(0, 1, 1, 0, 1e-3, 1.0, good, 1, 2, 0) != SH_ERR_ARG || pre(1, 0, 1, 0, 1e-3, 1.0, good, 1, 2, 0) != SH_ERR_ARG ||
      pre(1, 1, 2, 0, 1e-3, 1.0, good, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "options") || pre(1, 1, 1, 1, 1e-3, 1.0, good, 1, 2, 0) != SH_ERR_ARG ||
      pre(1, 1, 1, 0, 1.5, 1.0, good, 1, 2, 0) != SH_ERR_ARG || pre(1, 1, 1, 0, 1e-3, 0.0, good, 1, 2, 0) != SH_ERR_ARG || pre(1, 1, 1, 0, 1e-3, 1.0, nullptr, 1, 2, 0) != SH_ERR_ARG ||
      pre(1, 1, 1, 0, 1e-3, 1.0, zero, 1, 2, 0) != SH_ERR_ARG || !strstr(text, "cell[1]") || pre(1, 1, 1, 0, 1e-3, 1.0, nan, 1, 2, 0) != SH_ERR_ARG || !strstr(text, "cell[0]") ||
      pre(1, 1, 1, 0, 1e-3, 1.0, good, 1, 0, 0) != SH_ERR_STATE || pre(1, 1, 1, 0, 1e-3, 1.0, good, 1, 2, 1) != SH_ERR_STATE || pre(1, 1, 1, 0, 1e-3, 1.0, good, 0, 2, 0) != SH_ERR_STATE ||
      !strstr(text, "sh_mesh_topology")) {
    printf("simplify_check: precheck_simplify (%s)\n", text); return 1;
  }
  printf("simplify_check: ok\n");
  return 0;
}
