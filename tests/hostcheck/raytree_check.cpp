// Test shim (NOT product): the rays through the face hierarchy on the host, for tests/test_raytree_host.py.  rt_cast answers rays as
// k_ray_tree<false>, k_ray_tree<true> and k_ray_sort do -- sh_scalar.h bvh_ray_descend, the very function the kernels run, with a stack of
// SH_BVH_STACK words (an overrun is reported, not survived), the loose faces from the mesh, the pool ranked by (t, face); rt_brute is
// ray_check.cpp's statement of the walk over all faces (backwards into the pool); rt_near is k_ray_near.  The index comes from
// bvh_check.cpp, which this file includes with its main() renamed: one build, stated once.  Its own main() runs all of it, so that the
// file can be built as a stand-alone program with -fsanitize=address,undefined.
#define main bvh_check_main
#include "bvh_check.cpp"
#undef main

extern "C" int rt_box_skip(const double* o, const double* d, const float* bx, double tbest, double* tn) {
  sh::BvhRay r;
  sh::bvh_ray_set(o, d, &r);
  return sh::bvh_ray_box_skip(r, bx, tbest, tn) ? 1 : 0;
}

// k_ray_sort for one segment of n keys (ray_check.cpp rc_sort without a box frame)
static void rt_sort(const std::vector<double>& t, const std::vector<int>& face, const std::vector<int>& side, const double* o, const double* d, int cap, sh_ray_hit* out) {
  const int n = (int)t.size();
  for (int j = 0; j < n; ++j) {
    int rank = 0;
    for (int k = 0; k < n; ++k) rank += sh::ray_key_less(t[(size_t)k], face[(size_t)k], t[(size_t)j], face[(size_t)j]) ? 1 : 0;
    if (rank >= cap) continue;
    sh_ray_hit* h = out + rank;
    h->t = t[(size_t)j];
    for (int k = 0; k < 3; ++k) h->point[k] = o[k] + d[k] * t[(size_t)j];
    h->face = face[(size_t)j]; h->side = side[(size_t)j];
  }
  for (int s = n < cap ? n : cap; s < cap; ++s) { memset(out + s, 0, sizeof *out); out[s].face = -1; }
}

static void widen(const float* verts, const int* faces, int f, double* A, double* e1, double* e2) {
  const float *v0 = verts + 3 * (size_t)faces[3 * (size_t)f], *v1 = verts + 3 * (size_t)faces[3 * (size_t)f + 1], *v2 = verts + 3 * (size_t)faces[3 * (size_t)f + 2];
  for (int k = 0; k < 3; ++k) { A[k] = (double)v0[k]; e1[k] = (double)v1[k] - A[k]; e2[k] = (double)v2[k] - A[k]; }
}

struct Collect {
  static constexpr bool PRUNE = false;
  std::vector<double> t;
  std::vector<int> face, side;
  double bound() const { return INFINITY; }
  void operator()(double th, int f, int s) { t.push_back(th); face.push_back(f); side.push_back(s); }
};

// R rays (6 doubles each) over all faces of a mesh, no tree -> counts[R], hits[R][cap]
extern "C" void rt_brute(const float* verts, const int* faces, int nf, const double* rays, int R, int cap, sh_ray_hit* hits, int* counts) {
  for (int r = 0; r < R; ++r) {
    const double *o = rays + 6 * (size_t)r, *d = o + 3;
    Collect c;
    for (int f = nf - 1; f >= 0; --f) {
      double A[3], e1[3], e2[3], th;
      int s;
      widen(verts, faces, f, A, e1, e2);
      if (sh::ray_tri_hit(o, d, A, e1, e2, &th, &s)) c(th, f, s);
    }
    counts[r] = (int)c.t.size();
    rt_sort(c.t, c.face, c.side, o, d, cap, hits + (size_t)r * cap);
  }
}

// the same rays through the index of the mesh (box: the mesh's own nodes); count: nodes popped, faces tested in the tree, loose faces
// tested, the deepest stack, over all rays.  -> 0, or -1 when a stack went beyond SH_BVH_STACK, -2 when count and fill disagree
extern "C" int rt_cast(const float* verts, const int* faces, const int* order, const int* loose, const int* off, const float* box, const float* tri, const double* rays,
                       int R, int cap, sh_ray_hit* hits, int* counts, long long* count /* 4 */) {
  int rc = 0;
  count[0] = count[1] = count[2] = count[3] = 0;
  for (int r = 0; r < R; ++r) {
    const double *o = rays + 6 * (size_t)r, *d = o + 3;
    auto loose_faces = [&](auto& h) {
      for (int i = 0; i < off[1]; ++i) {
        double A[3], e1[3], e2[3], th;
        int s;
        widen(verts, faces, loose[i], A, e1, e2);
        if (sh::ray_tri_hit(o, d, A, e1, e2, &th, &s)) h(th, loose[i], s);
      }
    };
    HostStack st;
    sh::RayHitCount n;      // k_ray_tree<false>
    long long cnt[2] = {0, 0};
    sh::bvh_ray_descend<true>(o, d, off, box, tri, order, st, n, cnt);
    loose_faces(n);
    count[0] += cnt[0]; count[1] += cnt[1]; count[2] += off[1];
    counts[r] = n.n;
    Collect c;              // k_ray_tree<true>
    if (n.n > 0) {
      sh::bvh_ray_descend<false>(o, d, off, box, tri, order, st, c, nullptr);
      loose_faces(c);
    }
    if ((int)c.t.size() != n.n) rc = -2;
    count[3] = std::max(count[3], (long long)st.deepest);
    if (st.deepest > sh::SH_BVH_STACK) rc = -1;
    rt_sort(c.t, c.face, c.side, o, d, cap, hits + (size_t)r * cap);
  }
  return rc;
}

// k_ray_near: the least (t, face) of every ray, pruned by t; count as rt_cast's
extern "C" int rt_near(const float* verts, const int* faces, const int* order, const int* loose, const int* off, const float* box, const float* tri, const double* rays,
                       int R, sh_ray_hit* out, long long* count /* 4 */) {
  int rc = 0;
  count[0] = count[1] = count[2] = count[3] = 0;
  for (int r = 0; r < R; ++r) {
    const double *o = rays + 6 * (size_t)r, *d = o + 3;
    HostStack st;
    sh::RayHitNear h;
    long long cnt[2] = {0, 0};
    sh::bvh_ray_descend<true>(o, d, off, box, tri, order, st, h, cnt);
    for (int i = 0; i < off[1]; ++i) {
      double A[3], e1[3], e2[3], th;
      int s;
      widen(verts, faces, loose[i], A, e1, e2);
      if (sh::ray_tri_hit(o, d, A, e1, e2, &th, &s)) h(th, loose[i], s);
    }
    count[0] += cnt[0]; count[1] += cnt[1]; count[2] += off[1];
    count[3] = std::max(count[3], (long long)st.deepest);
    if (st.deepest > sh::SH_BVH_STACK) rc = -1;
    sh_ray_hit* q = out + r;
    memset(q, 0, sizeof *q);
    q->face = -1;
    if (h.face < 0) continue;
    q->t = h.t;
    for (int k = 0; k < 3; ++k) q->point[k] = o[k] + d[k] * h.t;
    q->face = h.face; q->side = h.side;
  }
  return rc;
}

// ray_plan: tmax, chunks, rays and the bytes of rays, counts, offs, cursor, hits, blockhit, near, status in out[0..10]
extern "C" void rt_plan(int B, int R, int per_humerus, int cap, long long maxF, int with_status, int tree, int near, long long* out /* 11 */) {
  const sh::RayPlan p = sh::ray_plan(B, R, per_humerus != 0, cap, maxF, with_status != 0, tree != 0, near != 0);
  out[0] = p.tmax; out[1] = p.chunks; out[2] = (long long)p.rays;
  out[3] = (long long)p.bytes.ray_rays; out[4] = (long long)p.bytes.ray_counts; out[5] = (long long)p.bytes.ray_offs; out[6] = (long long)p.bytes.ray_cursor;
  out[7] = (long long)p.bytes.ray_hits; out[8] = (long long)p.bytes.ray_blockhit; out[9] = (long long)p.near; out[10] = (long long)p.bytes.ray_status;
}

extern "C" int rt_precheck_nearest(const sh_ray* rays, int R, int per_humerus, int ctx, int B, int n_pending) {
  const sh::ArthroState st;
  return sh::precheck_ray_nearest(rays, R, per_humerus, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st}).code;
}

// every ray of `rays` through the tree against the walk over all faces, as bytes; the nearest against row 0
static int compare(const char* what, const std::vector<float>& v, const std::vector<int>& f, const std::vector<double>& rays, long long* total /* 4 */) {
  const int nf = (int)(f.size() / 3), R = (int)(rays.size() / 6), cap = 8;
  Index ix(v, f);
  std::vector<sh_ray_hit> a((size_t)R * cap), b((size_t)R * cap), n((size_t)R);
  std::vector<int> ca((size_t)R), cb((size_t)R);
  long long cnt[4];
  rt_brute(v.data(), f.data(), nf, rays.data(), R, cap, a.data(), ca.data());
  if (rt_cast(v.data(), f.data(), ix.order.data(), ix.loose.data(), ix.off.data(), ix.box.data(), ix.tri.data(), rays.data(), R, cap, b.data(), cb.data(), total) != 0) {
    printf("raytree_check: %s: the walk failed\n", what); return 1;
  }
  if (memcmp(ca.data(), cb.data(), (size_t)R * 4) != 0 || memcmp(a.data(), b.data(), (size_t)R * cap * sizeof(sh_ray_hit)) != 0) { printf("raytree_check: %s: tree != all faces\n", what); return 1; }
  if (rt_near(v.data(), f.data(), ix.order.data(), ix.loose.data(), ix.off.data(), ix.box.data(), ix.tri.data(), rays.data(), R, n.data(), cnt) != 0) {
    printf("raytree_check: %s: the nearest walk failed\n", what); return 1;
  }
  for (int r = 0; r < R; ++r)
    if (memcmp(&n[(size_t)r], &a[(size_t)r * cap], sizeof(sh_ray_hit)) != 0) { printf("raytree_check: %s: nearest of ray %d != row 0\n", what, r); return 1; }
  return 0;
}

// stand-alone run (sanitizer build): a tetrahedron, the plates of bvh_check.cpp (with loose faces), a mesh of loose faces alone, a flat sheet
int main() {
  long long cnt[4];
  unsigned long long seed = 7;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 40) / (double)(1 << 24); };
  {
    const std::vector<float> tv = {0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4};
    const std::vector<int> tf = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
    const std::vector<double> rays = {1, 1, -2, 0, 0, 1, 1, 1, 6, -1, -1, -2, 9, 9, -2, 0, 0, 1, 0, 0, -1, 0, 0, 1, 1, 1, 1e6, 0, 0, -1e-6};
    if (compare("tetrahedron", tv, tf, rays, cnt)) return 1;
  }
  std::vector<float> pv;
  std::vector<int> pf;
  const int G = 24;
  for (int i = 0; i < G; ++i)
    for (int j = 0; j < G; ++j) {
      const float x = (float)i, y = (float)j, z = 0.25f * (float)(i + j);
      const int v0 = (int)(pv.size() / 3);
      const float c[12] = {x, y, z, x + 1, y, z, x + 1, y + 1, z, x, y + 1, z};
      pv.insert(pv.end(), c, c + 12);
      const int f[6] = {v0, v0 + 1, v0 + 2, v0, v0 + 2, v0 + 3};
      pf.insert(pf.end(), f, f + 6);
      if ((i * G + j) % 7 == 0) {
        const float s[3] = {x + 0.5f, y + 0.5f, z + 1e-4f};
        pv.insert(pv.end(), s, s + 3);
        const int g[6] = {v0, v0 + 2, v0 + 4, v0 + 4, v0 + 4, v0 + 4};
        pf.insert(pf.end(), g, g + 6);
      }
    }
  {
    std::vector<double> rays;
    for (int q = 0; q < 300; ++q) {
      double r[6];
      for (int k = 0; k < 3; ++k) { r[k] = rnd() * 30.0 - 3.0; r[3 + k] = rnd() * 2.0 - 1.0; }
      if (q % 4 == 0) { r[3] = 0.0; r[4] = 0.0; r[5] = q % 8 == 0 ? -1.0 : 1.0; r[2] = q % 8 == 0 ? 40.0 : -5.0; }      // along z: through the stack of plates
      if (q % 9 == 0) { r[0] = (double)(q % G); r[3] = 0.0; }      // in a plane x = const that holds plate edges
      if (q == 5) for (int k = 0; k < 3; ++k) r[3 + k] *= 1e6;
      if (q == 6) for (int k = 0; k < 3; ++k) r[3 + k] *= 1e-6;
      if (q == 7) r[0] = 2e4;
      rays.insert(rays.end(), r, r + 6);
    }
    if (compare("plates", pv, pf, rays, cnt)) return 1;
    printf("raytree_check: plates: %d faces; per ray %.1f nodes, %.1f tree faces, %.1f loose faces, deepest stack %lld of %d\n", (int)(pf.size() / 3),
           (double)cnt[0] / 300, (double)cnt[1] / 300, (double)cnt[2] / 300, cnt[3], sh::SH_BVH_STACK);
  }
  {
    const std::vector<float> lv = {0, 0, 0, 1, 0, 0, 2, 0, 0, 5, 5, 5, 0, 1e-5f, 0};
    const std::vector<int> lf = {0, 1, 2, 3, 3, 3, 0, 2, 4, 1, 1, 2};
    const std::vector<double> rays = {1, 5e-6, -1, 0, 0, 1, 1, 1, -1, 0, 0, 1};
    if (compare("loose only", lv, lf, rays, cnt) || cnt[0] != 0 || cnt[2] != 8) { printf("raytree_check: loose only\n"); return 1; }
  }
  {      // a sheet in z = 2: boxes flat on an axis; rays in its plane, through it and beside it
    std::vector<float> sv;
    std::vector<int> sf;
    for (int i = 0; i <= 6; ++i)
      for (int j = 0; j <= 6; ++j) { const float c[3] = {(float)i, (float)j, 2.0f}; sv.insert(sv.end(), c, c + 3); }
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) { const int a = i * 7 + j, f[6] = {a, a + 7, a + 8, a, a + 8, a + 1}; sf.insert(sf.end(), f, f + 6); }
    const std::vector<double> rays = {-1, 3, 2, 1, 0, 0, 3.3, 2.2, -1, 0, 0, 1, 3, 3, 5, 0, 0, -1, 9, 9, 0, 0, 0, 1, -1, -1, 2, 1, 1, 0, 0.5, 0.5, 1, 1, 1, 0.25};
    if (compare("sheet", sv, sf, rays, cnt)) return 1;
  }
  long long out[11];
  rt_plan(3, 65, 0, 4, 520, 0, 1, 0, out);
  if (out[1] != 2 || out[8] != 0 || out[9] != 0 || out[4] != 3 * 65 * 4) { printf("raytree_check: plan\n"); return 1; }
  rt_plan(3, 65, 1, 1, 520, 0, 1, 1, out);
  if (out[1] != 2 || out[4] != 0 || out[7] != 0 || out[9] != 3 * 65 * 40 || out[3] != 3 * 65 * 48) { printf("raytree_check: plan of the nearest\n"); return 1; }
  sh_ray r[2] = {{{0, 0, 0}, {0, 0, 1}}, {{0, 0, 0}, {0, 0, 0}}};
  if (rt_precheck_nearest(r, 1, 0, 1, 1, 0) != SH_OK || rt_precheck_nearest(r, 2, 0, 1, 1, 0) != SH_ERR_ARG || rt_precheck_nearest(r, 0, 0, 1, 1, 0) != SH_ERR_ARG ||
      rt_precheck_nearest(r, 1, 0, 0, 1, 0) != SH_ERR_ARG || rt_precheck_nearest(r, 1, 0, 1, 0, 0) != SH_ERR_STATE || rt_precheck_nearest(r, 1, 0, 1, 1, 1) != SH_ERR_STATE) {
    printf("raytree_check: precheck\n"); return 1;
  }
  printf("raytree_check: ok\n");
  return 0;
}
