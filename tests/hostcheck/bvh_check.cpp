// Test shim (NOT product): the face hierarchy of shoulder_amd/csrc/sh_scalar.h (bvh_* -- the source k_bvh.h runs on the device) and the
// kernel-free plan and checks of sh_query.h (bvh_plan, precheck_bvh, precheck_query_accel) on the host, for tests/test_bvh_host.py.
// bc_build makes the index of one mesh as the build kernels do, step by step: class (loose or tight, the box of the tight faces by
// topo_enc words), key, a sort of the unique keys, emit (order, loose list, corners, the row of "bvh.off", the record), the leaves'
// boxes, the levels above them.  bc_walk answers one point as k_cp_tree and k_cp_join do: bvh_descend -- the very function the kernel
// runs -- with a stack of SH_BVH_STACK words (an overrun is reported, not survived), the loose faces, the winner recomputed from its
// face alone.  Its own main() runs all of it, so that the file can be built as a stand-alone program with -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

extern "C" void bc_consts(int* out /* 6 */) {
  out[0] = SH_BVH_LEAF; out[1] = SH_BVH_WIDTH; out[2] = sh::SH_BVH_MAX_LEVELS; out[3] = sh::SH_BVH_STACK; out[4] = SH_BVH_OFF_WORDS; out[5] = SH_BVH_OFF_LEVEL;
}
extern "C" long long bc_max_faces() { return SH_BVH_MAX_FACES; }
extern "C" int bc_levels_of(long long tight) { return sh::bvh_levels_of(tight); }
extern "C" long long bc_nodes_of(long long tight) { return sh::bvh_nodes_of(tight); }
extern "C" void bc_off_row(int tight, int loose, int base, int* row) { sh::bvh_off_row(tight, loose, base, row); }
extern "C" int bc_loose(const float* tri /* 9 */) { return sh::bvh_face_loose(tri, tri + 3, tri + 6) ? 1 : 0; }
extern "C" unsigned bc_code(int qx, int qy, int qz) { return sh::bvh_code(qx, qy, qz); }
extern "C" int bc_quant(float mn, float mx, float lo, float hi) { return sh::bvh_quant(mn, mx, lo, hi); }
extern "C" int bc_box_skip(const double* p, const float* bx, double best_r) { double n2; return sh::bvh_box_skip(p, bx, best_r, &n2) ? 1 : 0; }

// the plan of a batch with the face offsets foff (B + 1): -> its refusal code, and fblocks, levels, leaf_blocks, nodes, the bytes of
// "bvh.box" / "bvh.tri" / "bvh.key" in out[0..6], the first node of every mesh in base (B + 1), the launches' workgroups per level in blocks
extern "C" int bc_plan(int B, const long long* foff, long long* out /* 7 */, int* base /* B + 1 */, int* blocks /* MAX_LEVELS */) {
  sh::BvhPlan p;
  const sh::ArthroError e = sh::bvh_plan(B, foff, &p);
  if (e.code) return e.code;
  out[0] = p.fblocks; out[1] = p.levels; out[2] = p.leaf_blocks; out[3] = p.base[(size_t)B];
  out[4] = (long long)p.bytes.bvh_box; out[5] = (long long)p.bytes.bvh_tri; out[6] = (long long)p.bytes.bvh_key;
  for (int b = 0; b <= B; ++b) base[b] = p.base[(size_t)b];
  for (int k = 0; k < sh::SH_BVH_MAX_LEVELS; ++k) blocks[k] = p.node_blocks[k];
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < sh::AR_BVH_HEAD; ++k)
      if (p.state0[(size_t)b * sh::AR_BVH_HEAD + k] != (k < 3 ? 0xffffffffu : 0u)) return -100;
  return SH_OK;
}
extern "C" int bc_precheck(int ctx, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_bvh(sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st}).code;
}
extern "C" int bc_precheck_accel(int ctx, int mode) { return sh::precheck_query_accel(ctx != 0, mode).code; }

// The index of one mesh of nf faces whose first node is `base`: order and loose nf int32 (tails -1), off SH_BVH_OFF_WORDS, box
// 6 x bvh_nodes_of(nf) float32 (the nodes the mesh has are written), tri 9 nf float32, one record.
extern "C" void bc_build(const float* verts, const int* faces, int nf, int base, int* order, int* loose, int* off, float* box, float* tri, sh_bvh_info* info) {
  auto corner = [&](int f, int c) { return verts + 3 * (size_t)faces[3 * (size_t)f + c]; };
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  int T = 0;
  std::vector<char> is_loose((size_t)nf);
  for (int f = 0; f < nf; ++f) {      // k_bvh_class
    is_loose[(size_t)f] = sh::bvh_face_loose(corner(f, 0), corner(f, 1), corner(f, 2));
    if (is_loose[(size_t)f]) continue;
    ++T;
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 3; ++k) { const unsigned e = sh::topo_enc(corner(f, c)[k]); lo[k] = std::min(lo[k], e); hi[k] = std::max(hi[k], e); }
  }
  const float flo[3] = {sh::topo_dec(lo[0]), sh::topo_dec(lo[1]), sh::topo_dec(lo[2])}, fhi[3] = {sh::topo_dec(hi[0]), sh::topo_dec(hi[1]), sh::topo_dec(hi[2])};
  std::vector<unsigned long long> key((size_t)nf);
  for (int f = 0; f < nf; ++f)      // k_bvh_key
    key[(size_t)f] = sh::bvh_key(is_loose[(size_t)f], is_loose[(size_t)f] ? 0u : sh::bvh_face_code(corner(f, 0), corner(f, 1), corner(f, 2), flo, fhi), f);
  std::sort(key.begin(), key.end());
  for (int i = 0; i < nf; ++i) {      // k_bvh_emit
    const int id = (int)(unsigned)(key[(size_t)i] & 0xffffffffull);
    if (i < T) {
      order[i] = id;
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) tri[9 * (size_t)i + 3 * c + k] = corner(id, c)[k];
    } else order[i] = -1;
    loose[i] = i < nf - T ? (int)(unsigned)(key[(size_t)(T + i)] & 0xffffffffull) : -1;
  }
  sh::bvh_off_row(T, nf - T, base, off);
  info->tight = off[0]; info->loose = off[1]; info->leaves = off[2]; info->levels = off[3]; info->nodes = off[4]; info->reserved = 0;
  for (int k = 0; k < 3; ++k) { info->lo[k] = T > 0 ? flo[k] : 0.0f; info->hi[k] = T > 0 ? fhi[k] : 0.0f; }
  const int* lv = off + SH_BVH_OFF_LEVEL;
  for (int j = 0; j < off[2]; ++j) {      // k_bvh_leaves
    const int i0 = j * SH_BVH_LEAF, i1 = std::min(i0 + SH_BVH_LEAF, T);
    float bx[6];
    for (int k = 0; k < 3; ++k) bx[k] = bx[3 + k] = tri[9 * (size_t)i0 + k];
    for (int i = i0; i < i1; ++i)
      for (int c = 0; c < 3; ++c) sh::bvh_box_point(bx, tri + 9 * (size_t)i + 3 * c);
    memcpy(box + 6 * (size_t)j, bx, sizeof bx);
  }
  for (int level = 1; level < off[3]; ++level) {      // k_bvh_level
    const int n = lv[level + 1] - lv[level], below = lv[level] - lv[level - 1];
    const float* ch = box + 6 * (size_t)lv[level - 1];
    for (int j = 0; j < n; ++j) {
      const int c0 = j * SH_BVH_WIDTH, c1 = std::min(c0 + SH_BVH_WIDTH, below);
      float bx[6];
      memcpy(bx, ch + 6 * (size_t)c0, sizeof bx);
      for (int c = c0 + 1; c < c1; ++c) sh::bvh_box_box(bx, ch + 6 * (size_t)c);
      memcpy(box + 6 * ((size_t)lv[level] + (size_t)j), bx, sizeof bx);
    }
  }
}

// a stack of SH_BVH_STACK words that remembers the deepest word touched; a word beyond it lands in a spare one and is reported
struct HostStack {
  unsigned w[sh::SH_BVH_STACK + 1];
  int deepest = 0;
  unsigned& at(int i) { deepest = std::max(deepest, i + 1); return w[i < sh::SH_BVH_STACK ? i : sh::SH_BVH_STACK]; }
};

// k_cp_tree and k_cp_join for one point and the index of one mesh (box: the mesh's own nodes); count: nodes popped, faces tested in the
// tree, loose faces tested, the deepest stack.  -> 0, or -1 when the stack went beyond SH_BVH_STACK
extern "C" int bc_walk(const float* verts, const int* faces, const int* order, const int* loose, const int* off, const float* box, const float* tri, const double* p,
                       sh_closest* out, long long* count /* 4 */) {
  auto face_of = [&](int f, double* A, double* ab, double* ac) {
    const float *v0 = verts + 3 * (size_t)faces[3 * (size_t)f], *v1 = verts + 3 * (size_t)faces[3 * (size_t)f + 1], *v2 = verts + 3 * (size_t)faces[3 * (size_t)f + 2];
    for (int k = 0; k < 3; ++k) { A[k] = (double)v0[k]; ab[k] = (double)v1[k] - A[k]; ac[k] = (double)v2[k] - A[k]; }
  };
  double best = INFINITY;
  int best_f = -1;
  HostStack st;
  count[0] = count[1] = count[2] = count[3] = 0;
  sh::bvh_descend<true>(p, off, box, tri, order, st, &best, &best_f, count);
  count[3] = st.deepest;
  for (int i = 0; i < off[1]; ++i) {
    const int f = loose[i];
    double A[3], ab[3], ac[3], u, w;
    int region;
    face_of(f, A, ab, ac);
    const double d2 = sh::closest_pt_tri(p, A, ab, ac, &u, &w, &region);
    ++count[2];
    if (sh::closest_key_less(d2, f, best, best_f)) { best = d2; best_f = f; }
  }
  memset(out, 0, sizeof *out);
  if (best_f < 0) { out->face = -1; out->status = SH_ERR_GEOMETRY; return st.deepest > sh::SH_BVH_STACK ? -1 : 0; }
  double A[3], ab[3], ac[3], u, w, q[3];
  int region;
  face_of(best_f, A, ab, ac);
  const double d2 = sh::closest_pt_tri(p, A, ab, ac, &u, &w, &region);
  sh::tri_point(A, ab, ac, u, w, q);
  const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  out->dist = sqrt(d2); out->point[0] = q[0]; out->point[1] = q[1]; out->point[2] = q[2];
  out->face = best_f; out->region = region; out->side = sh::closest_side(r, ab, ac); out->status = 0;
  return st.deepest > sh::SH_BVH_STACK ? -1 : 0;
}

// every face, no tree: the reference of main()
static void brute(const float* verts, const int* faces, int nf, const double* p, double* best, int* best_f) {
  *best = INFINITY; *best_f = -1;
  for (int f = 0; f < nf; ++f) {
    const float *v0 = verts + 3 * (size_t)faces[3 * f], *v1 = verts + 3 * (size_t)faces[3 * f + 1], *v2 = verts + 3 * (size_t)faces[3 * f + 2];
    double A[3], ab[3], ac[3], u, w;
    int region;
    for (int k = 0; k < 3; ++k) { A[k] = (double)v0[k]; ab[k] = (double)v1[k] - A[k]; ac[k] = (double)v2[k] - A[k]; }
    const double d2 = sh::closest_pt_tri(p, A, ab, ac, &u, &w, &region);
    if (sh::closest_key_less(d2, f, *best, *best_f)) { *best = d2; *best_f = f; }
  }
}

struct Index {
  std::vector<int> order, loose, off;
  std::vector<float> box, tri;
  sh_bvh_info info;
  Index(const std::vector<float>& v, const std::vector<int>& f) {
    const int nf = (int)(f.size() / 3);
    order.resize((size_t)nf); loose.resize((size_t)nf); off.resize(SH_BVH_OFF_WORDS); box.resize(6 * (size_t)sh::bvh_nodes_of(nf) + 6); tri.resize(9 * (size_t)nf);
    bc_build(v.data(), f.data(), nf, 0, order.data(), loose.data(), off.data(), box.data(), tri.data(), &info);
  }
};

// stand-alone run (sanitizer build): a tetrahedron, a grid of plates with slivers and point triangles between them stored twice, a
// mesh of loose faces alone; every point through the tree against every face without it
int main() {
  const std::vector<float> tv = {0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4};
  const std::vector<int> tf = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  {
    Index ix(tv, tf);
    if (ix.info.tight != 4 || ix.info.loose != 0 || ix.info.leaves != 1 || ix.info.levels != 1 || ix.info.nodes != 1) { printf("bvh_check: tetrahedron counts\n"); return 1; }
    const double pts[4][3] = {{1, 1, -2}, {2, -3, -4}, {-2, -2, -1}, {1e200, 0, 0}};
    const int faces[4] = {0, 0, 0, -1};
    for (int i = 0; i < 4; ++i) {
      sh_closest o; long long cnt[4];
      if (bc_walk(tv.data(), tf.data(), ix.order.data(), ix.loose.data(), ix.off.data(), ix.box.data(), ix.tri.data(), pts[i], &o, cnt) != 0 || o.face != faces[i] ||
          (i == 3) != (o.status == SH_ERR_GEOMETRY)) { printf("bvh_check: tetrahedron point %d: face %d status %d\n", i, o.face, o.status); return 1; }
    }
  }
  // 40 x 40 plates of two triangles at z = 0.25 (i + j), every seventh followed by a sliver and a point triangle; the list twice
  std::vector<float> pv;
  std::vector<int> pf;
  const int G = 40;
  for (int i = 0; i < G; ++i)
    for (int j = 0; j < G; ++j) {
      const float x = (float)i, y = (float)j, z = 0.25f * (float)(i + j);
      const int v0 = (int)(pv.size() / 3);
      const float c[12] = {x, y, z, x + 1, y, z, x + 1, y + 1, z, x, y + 1, z};
      pv.insert(pv.end(), c, c + 12);
      const int f[6] = {v0, v0 + 1, v0 + 2, v0, v0 + 2, v0 + 3};
      pf.insert(pf.end(), f, f + 6);
      if ((i * G + j) % 7 == 0) {
        const float s[3] = {x + 0.5f, y + 0.5f, z + 1e-4f};      // a sliver across the plate's diagonal and a point triangle
        pv.insert(pv.end(), s, s + 3);
        const int g[6] = {v0, v0 + 2, v0 + 4, v0 + 4, v0 + 4, v0 + 4};
        pf.insert(pf.end(), g, g + 6);
      }
    }
  const size_t once = pf.size();
  pf.insert(pf.end(), pf.begin(), pf.begin() + (long)once);
  {
    Index ix(pv, pf);
    const int nf = (int)(pf.size() / 3);
    if (ix.info.tight + ix.info.loose != nf || ix.info.loose < 2 * (G * G / 7) || ix.info.levels != sh::bvh_levels_of(ix.info.tight)) { printf("bvh_check: plates counts\n"); return 1; }
    for (int i = 1; i < ix.info.loose; ++i)
      if (ix.loose[(size_t)i - 1] >= ix.loose[(size_t)i]) { printf("bvh_check: the loose list does not ascend\n"); return 1; }
    unsigned long long seed = 1;
    long long deepest = 0, nodes = 0, tested = 0;
    const int Q = 400;
    for (int q = 0; q < Q; ++q) {
      double p[3];
      for (int k = 0; k < 3; ++k) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; p[k] = (double)(seed >> 40) / (double)(1 << 24) * (k == 2 ? 30.0 : 44.0) - 2.0; }
      if (q % 5 == 0) for (int k = 0; k < 3; ++k) p[k] = (double)pv[3 * (size_t)(q * 13 % (int)(pv.size() / 3)) + k];      // on a vertex: ties
      if (q == 7) p[0] = 2e4;
      sh_closest o; long long cnt[4];
      double best; int best_f;
      brute(pv.data(), pf.data(), nf, p, &best, &best_f);
      if (bc_walk(pv.data(), pf.data(), ix.order.data(), ix.loose.data(), ix.off.data(), ix.box.data(), ix.tri.data(), p, &o, cnt) != 0 || o.face != best_f ||
          o.dist != sqrt(best)) { printf("bvh_check: plates point %d: face %d (brute %d) dist %.17g (brute %.17g)\n", q, o.face, best_f, o.dist, sqrt(best)); return 1; }
      deepest = std::max(deepest, cnt[3]); nodes += cnt[0]; tested += cnt[1];
    }
    printf("bvh_check: plates: %d faces (%d loose), %d levels; per point %.1f nodes, %.1f faces, deepest stack %lld of %d\n", nf, ix.info.loose, ix.info.levels,
           (double)nodes / Q, (double)tested / Q, deepest, sh::SH_BVH_STACK);
  }
  {      // only loose faces: an empty tree
    const std::vector<float> lv = {0, 0, 0, 1, 0, 0, 2, 0, 0, 5, 5, 5};
    const std::vector<int> lf = {0, 1, 2, 3, 3, 3, 0, 2, 1, 1, 1, 2};
    Index ix(lv, lf);
    if (ix.info.tight != 0 || ix.info.loose != 4 || ix.info.levels != 0 || ix.info.nodes != 0 || ix.info.lo[0] != 0.0f) { printf("bvh_check: loose-only counts\n"); return 1; }
    const double p[3] = {1.5, 1.0, 0.0};
    sh_closest o; long long cnt[4];
    if (bc_walk(lv.data(), lf.data(), ix.order.data(), ix.loose.data(), ix.off.data(), ix.box.data(), ix.tri.data(), p, &o, cnt) != 0 || o.face != 0 || o.dist != 1.0 || cnt[2] != 4) {
      printf("bvh_check: loose-only walk: face %d dist %g\n", o.face, o.dist); return 1;
    }
  }
  {      // the plan: a ragged batch, and a mesh of the upload's maximum
    const long long foff[4] = {0, 4, 4 + 513, 4 + 513 + 32440};
    long long out[7]; int base[4], blocks[16];
    if (bc_plan(3, foff, out, base, blocks) != SH_OK || base[1] != sh::bvh_nodes_of(4) || base[2] != base[1] + sh::bvh_nodes_of(513) || out[1] != sh::bvh_levels_of(32440)) {
      printf("bvh_check: plan\n"); return 1;
    }
    const long long big[2] = {0, SH_BVH_MAX_FACES};
    if (bc_plan(1, big, out, base, blocks) != SH_OK || out[1] != sh::SH_BVH_MAX_LEVELS) { printf("bvh_check: plan at the maximum\n"); return 1; }
    const long long many[3] = {0, SH_BVH_MAX_FACES, 2 * SH_BVH_MAX_FACES};
    if (bc_plan(2, many, out, base, blocks) != SH_OK) { printf("bvh_check: plan of two maxima\n"); return 1; }
    const long long over[5] = {0, SH_BVH_MAX_FACES, 2 * SH_BVH_MAX_FACES, 3 * SH_BVH_MAX_FACES, 4 * SH_BVH_MAX_FACES};
    if (bc_plan(4, over, out, base, blocks) != SH_ERR_NOMEM) { printf("bvh_check: a batch of 2^31 faces is refused\n"); return 1; }
  }
  if (bc_precheck(0, 1, 0) != SH_ERR_ARG || bc_precheck(1, 0, 0) != SH_ERR_STATE || bc_precheck(1, 2, 1) != SH_ERR_STATE || bc_precheck(1, 2, 0) != SH_OK ||
      bc_precheck_accel(1, 2) != SH_ERR_ARG || bc_precheck_accel(0, 0) != SH_ERR_ARG || bc_precheck_accel(1, 1) != SH_OK) { printf("bvh_check: prechecks\n"); return 1; }
  printf("bvh_check: ok (LEAF %d, WIDTH %d, at most %d levels, stack %d)\n", SH_BVH_LEAF, SH_BVH_WIDTH, sh::SH_BVH_MAX_LEVELS, sh::SH_BVH_STACK);
  return 0;
}
