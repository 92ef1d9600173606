// Test shim (NOT product): the topology rules of shoulder_amd/csrc/sh_scalar.h (topo_degenerate, topo_edge_slot, topo_slot, topo_round,
// topo_rounds, topo_enc / topo_dec -- the source k_topo.h runs on the device) and, of sh_query.h, the argument checks of sh_mesh_topology
// and its buffer plan, on the host, for tests/test_topo_host.py.  tc_topology makes the buffers of one mesh as the kernels do: counts,
// an exclusive scan, rows filled through a cursor IN REVERSE face order (the fill order is not defined) and put in order by rank, a walk
// of the shorter row per slot, Jacobi rounds on two arrays that are never re-initialised with a head word per round, the roots ranked
// in face order, the records summed and decoded.  Its own main() walks a box, two boxes, a fan, a strip, degenerate faces and the
// checks, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(sizeof(sh_topology) == 64 && sizeof(sh_shell) == 48 && sizeof(sh_topology_options) == 12, "the records of sh_mesh_topology");
static_assert(SH_ADJ_BORDER == SH_TOPO_BORDER && SH_ADJ_NONMANIFOLD == SH_TOPO_NONMANIFOLD && SH_ADJ_DEGENERATE == SH_TOPO_DEGENERATE, "the adjacency codes");

extern "C" void tc_topology(const float* verts, int nv, const int* faces, int nf, int max_shells, int max_rounds, int32_t* vrow /* nv + 1 */,
                            int32_t* vface /* 3 nf */, int32_t* adj /* 3 nf */, int32_t* label /* nf */, sh_topology* info, sh_shell* shells /* max_shells */) {
  // k_topo_count, k_topo_scan
  std::vector<int> cursor((size_t)nv + 1, 0), head(64, 0);
  int deg = 0, used = 0, maxv = 0;
  for (int f = 0; f < nf; ++f) {
    if (sh::topo_degenerate(faces + 3 * (size_t)f, nv)) { ++deg; continue; }
    for (int k = 0; k < 3; ++k) ++cursor[faces[3 * (size_t)f + k]];
  }
  int run = 0;
  for (int v = 0; v < nv; ++v) {
    const int c = cursor[v];
    vrow[v] = run; cursor[v] = run; run += c;
    used += c > 0 ? 1 : 0; maxv = c > maxv ? c : maxv;
  }
  vrow[nv] = run;
  head[0] = 1;
  // k_topo_fill (in reverse), k_topo_rows
  std::vector<int> tmp(3 * (size_t)nf + 1, -1);
  for (size_t i = 0; i < 3 * (size_t)nf; ++i) vface[i] = -1;
  for (int f = nf - 1; f >= 0; --f) {
    if (sh::topo_degenerate(faces + 3 * (size_t)f, nv)) continue;
    for (int k = 0; k < 3; ++k) tmp[cursor[faces[3 * (size_t)f + k]]++] = f;
  }
  for (int f = 0; f < nf; ++f) {
    if (sh::topo_degenerate(faces + 3 * (size_t)f, nv)) continue;
    for (int k = 0; k < 3; ++k) {
      const int s = vrow[faces[3 * (size_t)f + k]], e = vrow[faces[3 * (size_t)f + k] + 1];
      int rank = 0;
      for (int j = s; j < e; ++j) rank += tmp[j] < f ? 1 : 0;
      vface[s + rank] = f;
    }
  }
  // k_topo_adj
  int counts[4] = {0, 0, 0, 0};
  for (int f = 0; f < nf; ++f) {
    const int* fc = faces + 3 * (size_t)f;
    if (sh::topo_degenerate(fc, nv)) { adj[3 * (size_t)f] = adj[3 * (size_t)f + 1] = adj[3 * (size_t)f + 2] = SH_TOPO_DEGENERATE; continue; }
    for (int e = 0; e < 3; ++e) {
      const int a = fc[e], c = fc[e == 2 ? 0 : e + 1];
      const int na = vrow[a + 1] - vrow[a], nc = vrow[c + 1] - vrow[c];
      int owner, same;
      const int val = sh::topo_slot(faces, vface + vrow[nc < na ? c : a], nc < na ? nc : na, f, e, &owner, &same);
      adj[3 * (size_t)f + e] = val;
      if (owner) { counts[0] += 1; counts[1] += val == SH_TOPO_BORDER; counts[2] += val == SH_TOPO_NONMANIFOLD; counts[3] += same; }
    }
  }
  // k_topo_round, max_rounds times: two arrays, the one written still holds the round before the last
  std::vector<int> pa((size_t)nf), pb((size_t)nf);
  for (int f = 0; f < nf; ++f) pa[f] = pb[f] = f;
  for (int r = 0; r < max_rounds; ++r) {
    if (head[r] == 0) continue;
    const std::vector<int>& in = (r & 1) ? pb : pa;
    std::vector<int>& nxt = (r & 1) ? pa : pb;
    for (int u = 0; u < nf; ++u) {
      int self, hook;
      if (sh::topo_round(in.data(), adj + 3 * (size_t)u, u, &self, &hook)) head[r + 1] = 1;
      const int pu = in[u];
      if (nxt[u] > self) nxt[u] = self;
      if (hook < in[pu] && hook < nxt[pu]) nxt[pu] = hook;
    }
  }
  // k_topo_rank
  int full;
  const int rounds = sh::topo_rounds(head.data(), max_rounds, &full);
  const std::vector<int>& fin = (rounds & 1) ? pb : pa;
  std::vector<int> rank((size_t)nf, -1), cnt((size_t)nf + 1, 0);
  int n_shells = 0;
  if (!full)
    for (int f = 0; f < nf; ++f)
      if (adj[3 * (size_t)f] != SH_TOPO_DEGENERATE && fin[f] == f) rank[f] = n_shells++;
  std::vector<int32_t> rec((size_t)max_shells * 12, 0);
  for (int k = 0; k < max_shells && k < n_shells; ++k) rec[(size_t)k * 12 + 6] = rec[(size_t)k * 12 + 7] = rec[(size_t)k * 12 + 8] = -1;
  // k_topo_label
  for (int f = 0; f < nf; ++f) {
    const int* fc = faces + 3 * (size_t)f;
    const int lab = full || adj[3 * (size_t)f] == SH_TOPO_DEGENERATE ? -1 : rank[fin[f]];
    label[f] = lab;
    if (lab < 0) continue;
    ++cnt[lab];
    if (lab >= max_shells) continue;
    int32_t* r = &rec[(size_t)lab * 12];
    if (fin[f] == f) r[0] = f;
    r[1] += 1;
    for (int e = 0; e < 3; ++e) {
      const int v = adj[3 * (size_t)f + e];
      if (v == SH_TOPO_BORDER) r[2] += 1;
      else if (v == SH_TOPO_NONMANIFOLD) r[3] += 1;
      else if (v >= 0) {
        const int a = fc[e], c = fc[e == 2 ? 0 : e + 1];
        const int* g = faces + 3 * (size_t)v;
        const int ge = sh::topo_edge_slot(g, a, c);
        r[4] += 1;
        r[5] += ge >= 0 && g[ge] == a ? 1 : 0;
      }
    }
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) {
        const unsigned x = sh::topo_enc(verts[3 * (size_t)fc[j] + k]);
        unsigned* lo = (unsigned*)r + 6 + k;
        unsigned* hi = (unsigned*)r + 9 + k;
        if (x < *lo) *lo = x;
        if (x > *hi) *hi = x;
      }
  }
  // k_topo_finish
  int bc = 0, bk = -1;
  for (int k = 0; k < n_shells; ++k)
    if (cnt[k] > bc) { bc = cnt[k]; bk = k; }
  const int written = n_shells < max_shells ? n_shells : max_shells;
  for (int k = 0; k < written; ++k) {
    int32_t* r = &rec[(size_t)k * 12];
    r[4] /= 2; r[5] /= 2;
    for (int w = 6; w < 12; ++w) { const float x = sh::topo_dec((unsigned)r[w]); memcpy(r + w, &x, 4); }
  }
  memcpy(shells, rec.data(), (size_t)max_shells * sizeof(sh_shell));
  sh_topology t;
  t.status = full ? SH_ERR_CAPACITY : 0; t.rounds = rounds; t.faces_degenerate = deg; t.vertices_used = used;
  t.edges = counts[0]; t.border_edges = counts[1]; t.nonmanifold_edges = counts[2]; t.inconsistent_edges = counts[3];
  t.euler = used - counts[0] + (nf - deg); t.max_valence = maxv; t.n_shells = n_shells; t.shells_written = written;
  t.largest_shell = bk; t.largest_faces = bk >= 0 ? bc : 0;
  t.flags = (counts[1] == 0 && counts[2] == 0 && deg == 0 ? SH_TOPO_WATERTIGHT : 0) | (counts[3] == 0 ? SH_TOPO_CONSISTENT : 0);
  t.reserved = 0;
  *info = t;
}

// precheck_topology; the refusal's text to `text`
extern "C" int tc_precheck(int ctx, int have_opt, int max_shells, int max_rounds, int reserved, int B, int n_pending, char* text, int cap) {
  const sh::ArthroState st;
  const sh_topology_options opt = {max_shells, max_rounds, reserved};
  const sh::ArthroError e = sh::precheck_topology(have_opt ? &opt : nullptr, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: blocks, then the ten sizes of TOPO_BUFS
extern "C" void tc_plan(int B, int max_shells, long long maxF, long long sumV, long long sumF, size_t* out) {
  const sh::TopoPlan p = sh::topo_plan(B, max_shells, maxF, sumV, sumF);
  size_t* o = out;
  *o++ = (size_t)p.blocks;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  TOPO_BUFS(X)
#undef X
}

// ---- stand-alone run (sanitizer build) ----
struct Result {
  std::vector<int32_t> vrow, vface, adj, label;
  sh_topology info;
  std::vector<sh_shell> shells;
};
static Result run(const std::vector<float>& v, const std::vector<int>& f, int max_shells, int max_rounds) {
  const int nv = (int)v.size() / 3, nf = (int)f.size() / 3;
  Result r;
  r.vrow.resize((size_t)nv + 1); r.vface.resize(3 * (size_t)nf); r.adj.resize(3 * (size_t)nf); r.label.resize((size_t)nf); r.shells.resize((size_t)max_shells);
  tc_topology(v.data(), nv, f.data(), nf, max_shells, max_rounds, r.vrow.data(), r.vface.data(), r.adj.data(), r.label.data(), &r.info, r.shells.data());
  return r;
}
static bool is(const sh_topology& t, int faces_deg, int edges, int border, int same, int shells, int largest, int rounds) {
  return t.status == 0 && t.faces_degenerate == faces_deg && t.edges == edges && t.border_edges == border && t.inconsistent_edges == same && t.n_shells == shells &&
         t.largest_faces == largest && t.rounds == rounds;
}

int main() {
  std::vector<float> bv(24);
  const std::vector<int> bf = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  Result r = run(bv, bf, 4, 32);
  const sh_shell& s0 = r.shells[0];
  if (!is(r.info, 0, 18, 0, 0, 1, 12, 3) || r.info.euler != 2 || r.info.flags != 3 || r.info.vertices_used != 8 || s0.faces != 12 || s0.manifold_edges != 18 || s0.border_slots != 0 ||
      s0.lo[0] != 120.f || s0.hi[0] != 150.f || s0.lo[1] != -85.f || s0.hi[1] != -65.f || s0.lo[2] != 410.f || s0.hi[2] != 420.f || r.shells[1].faces != 0) {
    printf("topo_check: box (edges %d rounds %d shells %d)\n", r.info.edges, r.info.rounds, r.info.n_shells); return 1;
  }
  for (int f = 0; f < 12; ++f)
    for (int e = 0; e < 3; ++e) {      // adjacency is symmetric
      const int g = r.adj[3 * f + e];
      if (g < 0 || g > 11 || (r.adj[3 * g] != f && r.adj[3 * g + 1] != f && r.adj[3 * g + 2] != f)) { printf("topo_check: box adjacency\n"); return 1; }
    }
  // without face 0: three border edges; face 5 flipped: three edges run the same way
  std::vector<int> open(bf.begin() + 3, bf.end()), flip = bf;
  r = run(bv, open, 4, 32);
  if (!is(r.info, 0, 18, 3, 0, 1, 11, 4) || (r.info.flags & SH_TOPO_WATERTIGHT)) { printf("topo_check: open box\n"); return 1; }
  std::swap(flip[15], flip[16]);
  r = run(bv, flip, 4, 32);
  if (!is(r.info, 0, 18, 0, 3, 1, 12, 3) || r.info.flags != SH_TOPO_WATERTIGHT || r.shells[0].inconsistent_edges != 3) { printf("topo_check: flipped face\n"); return 1; }
  // two boxes; sharing only vertex 0; sharing the edge {0, 1}
  std::vector<float> v2 = bv;
  std::vector<int> f2 = bf;
  for (int i = 0; i < 24; ++i) v2.push_back(bv[i] + (i % 3 == 0 ? 100.f : 0.f));
  for (int x : bf) f2.push_back(x + 8);
  r = run(v2, f2, 1, 32);
  if (!is(r.info, 0, 36, 0, 0, 2, 12, 3) || r.info.shells_written != 1 || r.info.largest_shell != 0 || r.label[11] != 0 || r.label[12] != 1 || r.info.euler != 4) {
    printf("topo_check: two boxes\n"); return 1;
  }
  std::vector<int> fv = f2, fe = f2;
  for (int& x : fv) if (x == 8) x = 0;
  for (int& x : fe) if (x == 8 || x == 9) x -= 8;
  r = run(v2, fv, 4, 32);
  if (!is(r.info, 0, 36, 0, 0, 2, 12, 3) || r.info.vertices_used != 15) { printf("topo_check: boxes sharing a vertex\n"); return 1; }
  r = run(v2, fe, 4, 32);
  int slots = 0;
  for (int x : r.adj) slots += x == SH_ADJ_NONMANIFOLD;
  if (r.info.status || r.info.nonmanifold_edges != 1 || slots != 4 || r.info.n_shells != 2 || r.info.edges != 35 || r.shells[0].nonmanifold_slots != 2 || (r.info.flags & 1)) {
    printf("topo_check: boxes sharing an edge\n"); return 1;
  }
  // a fan of 300 around vertex 0; a strip of 600 in and out of rounds
  std::vector<float> av(3 * 302, 0.f);
  std::vector<int> af;
  for (int i = 0; i < 302; ++i) { av[3 * i] = (float)cos(0.02 * i) * (i ? 40.f : 0.f); av[3 * i + 1] = (float)sin(0.02 * i) * (i ? 40.f : 0.f); }
  for (int i = 1; i <= 300; ++i) { af.push_back(0); af.push_back(i); af.push_back(i + 1); }
  r = run(av, af, 4, 32);
  if (!is(r.info, 0, 601, 302, 0, 1, 300, 10) || r.info.max_valence != 300 || r.vrow[1] != 300) { printf("topo_check: fan (rounds %d)\n", r.info.rounds); return 1; }
  for (int i = 0; i < 300; ++i) if (r.vface[i] != i) { printf("topo_check: fan row\n"); return 1; }
  std::vector<float> sv(3 * 602, 0.f);
  std::vector<int> sf;
  for (int i = 0; i < 602; ++i) { sv[3 * i] = (float)(i / 2); sv[3 * i + 1] = (float)(i % 2); }
  for (int i = 0; i < 600; ++i) { sf.push_back((i & 1) ? i + 1 : i); sf.push_back((i & 1) ? i : i + 1); sf.push_back(i + 2); }
  r = run(sv, sf, 4, 32);
  if (!is(r.info, 0, 1201, 602, 0, 1, 600, 11)) { printf("topo_check: strip (rounds %d same %d)\n", r.info.rounds, r.info.inconsistent_edges); return 1; }
  const std::vector<int32_t> strip_adj = r.adj;
  r = run(sv, sf, 4, 4);
  bool none = r.info.status == SH_ERR_CAPACITY && r.info.rounds == 4 && r.info.n_shells == 0 && r.info.largest_shell == -1 && r.info.edges == 1201 && r.adj == strip_adj &&
              r.shells[0].faces == 0;
  for (int x : r.label) none = none && x == -1;
  if (!none) { printf("topo_check: strip out of rounds\n"); return 1; }
  // degenerate faces around a box face; only degenerate faces
  std::vector<int> df = {0, 0, 1};
  df.insert(df.end(), bf.begin(), bf.begin() + 18);
  df.insert(df.end(), {3, 3, 3});
  df.insert(df.end(), bf.begin() + 18, bf.end());
  df.insert(df.end(), {5, 7, 5});
  r = run(bv, df, 4, 32);
  if (!is(r.info, 3, 18, 0, 0, 1, 12, r.info.rounds) || r.label[0] != -1 || r.adj[0] != SH_ADJ_DEGENERATE || r.label[7] != -1 || r.label[14] != -1 || r.info.flags != SH_TOPO_CONSISTENT ||
      r.shells[0].first_face != 1 || r.vrow[8] != 36 || r.vface[36] != -1 || r.vface[44] != -1) {
    printf("topo_check: degenerate faces\n"); return 1;
  }
  const std::vector<int> only = {0, 1, 1, 2, 2, 3, 4, 5, 4, 6, 6, 6};
  r = run(bv, only, 4, 32);
  if (r.info.status || r.info.n_shells || r.info.faces_degenerate != 4 || r.info.edges || r.info.rounds != 1 || r.info.largest_shell != -1 || r.info.vertices_used ||
      r.info.flags != SH_TOPO_CONSISTENT) {
    printf("topo_check: only degenerate faces\n"); return 1;
  }
  // the order of -0 and +0, and the round trip of the encoding
  const float xs[6] = {-INFINITY, -1.5f, -0.f, 0.f, 1e-30f, INFINITY};
  for (int i = 0; i < 6; ++i) {
    const float back = sh::topo_dec(sh::topo_enc(xs[i]));
    if (memcmp(&back, xs + i, 4) != 0 || (i && !(sh::topo_enc(xs[i - 1]) < sh::topo_enc(xs[i])))) { printf("topo_check: encoding\n"); return 1; }
  }
  // the checks of sh_mesh_topology in their order
  char text[256];
  auto pre = [&](int ctx, int opt, int shells, int rounds, int reserved, int B, int pend) { return tc_precheck(ctx, opt, shells, rounds, reserved, B, pend, text, (int)sizeof text); };
  if (pre(1, 1, 64, 32, 0, 1, 0) != SH_OK || pre(0, 1, 64, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 0, 64, 32, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "must be given") ||
      pre(1, 1, 0, 32, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "options") || pre(1, 1, 65537, 32, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 65536, 1, 0, 1, 0) != SH_OK ||
      pre(1, 1, 64, 0, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 64, 33, 0, 1, 0) != SH_ERR_ARG || pre(1, 1, 64, 32, 1, 1, 0) != SH_ERR_ARG ||
      pre(1, 1, 64, 32, 0, 0, 0) != SH_ERR_STATE || pre(1, 1, 64, 32, 0, 1, 1) != SH_ERR_STATE) {
    printf("topo_check: precheck_topology (%s)\n", text); return 1;
  }
  size_t plan[11];
  tc_plan(3, 64, 513, 900, 1200, plan);
  if (plan[0] != 3 || plan[1] != 903 * 4 || plan[2] != 14400 || plan[3] != 14400 || plan[4] != 4800 || plan[5] != 192 || plan[6] != 3 * 64 * 48 || plan[7] != 3 * 64 * 4 ||
      plan[8] != 903 * 4 || plan[9] != 14400 || plan[10] != 9600) {
    printf("topo_check: plan\n"); return 1;
  }
  printf("topo_check: ok\n");
  return 0;
}
