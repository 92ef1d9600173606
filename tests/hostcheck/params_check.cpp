// Test shim (NOT product): the host rules of the parameters (shoulder_amd/csrc/sh_params.h, and the layer table of sh_unet_plan.h) for
// tests/test_params_host.py.  Every checking call returns the code and *text (the fragment / refusal text, "" when accepted).
// main(): a stand-alone program over the same calls (for a sanitizer build).
#include "../../shoulder_amd/csrc/sh_params.h"
#include "../../shoulder_amd/csrc/sh_unet_plan.h"

#include <cstdio>
#include <cstring>

typedef unsigned long long u64;

static sh::ParamShape shape_of(int base, int depth, u64 F, u64 N, u64 T) {
  sh::ParamShape s;
  s.base = base; s.depth = depth; s.unet_floats = (size_t)F; s.nodes = (size_t)N; s.trees = (size_t)T;
  return s;
}
static int put_text(const std::string& all, char* out, int cap) {
  if ((int)all.size() + 1 > cap) return -100;
  memcpy(out, all.c_str(), all.size() + 1);
  return 0;
}

extern "C" {
// out: byte offsets of unet, feat, thr, ti, fi, lw, roots, then the total
void pc_layout(u64 F, u64 N, u64 T, u64* out) {
  const sh::ParamLayout L(shape_of(32, 1, F, N, T));
  const u64 v[8] = {L.unet, L.feat, L.thr, L.ti, L.fi, L.lw, L.roots, L.total};
  memcpy(out, v, sizeof v);
}
// out: the forest view's feat, thr, ti, fi, lw, roots of a block at address `block`
void pc_forest_view(u64 F, u64 N, u64 T, u64 block, u64* out) {
  const sh::ForestView v((const void*)(uintptr_t)block, sh::ParamLayout(shape_of(32, 1, F, N, T)));
  const u64 p[6] = {(u64)(uintptr_t)v.feat, (u64)(uintptr_t)v.thr, (u64)(uintptr_t)v.ti, (u64)(uintptr_t)v.fi, (u64)(uintptr_t)v.lw, (u64)(uintptr_t)v.roots};
  memcpy(out, p, sizeof p);
}
// a mirror of the shape: elements per section after resize, and what each() hands out (offset, bytes) per section -> out[7][3]
void pc_mirror(u64 F, u64 N, u64 T, u64* out) {
  const sh::ParamShape s = shape_of(32, 1, F, N, T);
  sh::ParamMirror m;
  m.resize(s);
  const u64 n[7] = {m.unet.size(), m.feat.size(), m.thr.size(), m.ti.size(), m.fi.size(), m.lw.size(), m.roots.size()};
  int k = 0;
  m.each(sh::ParamLayout(s), [&](void*, size_t off, size_t bytes) { out[3 * k] = n[k]; out[3 * k + 1] = off; out[3 * k + 2] = bytes; ++k; });
}
int pc_features() { return SH_RFC_FEATURES; }
int pc_forest_check(const int32_t* feat, const int32_t* ti, const int32_t* fi, int n_nodes, const int32_t* roots, int n_trees, const char** text) {
  const sh::ParamError e = sh::forest_check(feat, ti, fi, n_nodes, roots, n_trees);
  *text = e.text;
  return e.code;
}
void pc_default_params(sh_params* p) { *p = sh::default_run_params(); }
int pc_run_params(const sh_params* p, const char** text) {
  const sh::ParamError e = sh::run_params_check(*p);
  *text = e.text;
  return e.code;
}
// one line per layer of the table (by name, as the map holds it): name taps cin cout w_off b_off
int pc_layer_table(int base, int depth, char* out, int cap, long long* n_floats, const char** text) {
  static std::string refusal;
  sh::UnetLayers layers;
  size_t n = 0;
  const sh::UnetError e = sh::unet_layer_table(base, depth, &layers, &n);
  refusal = e.text;
  *text = refusal.c_str();
  *n_floats = (long long)n;
  std::string all;
  for (auto& kv : layers) {
    char b[160];
    snprintf(b, sizeof b, "%s %d %d %d %zu %zu\n", kv.first.c_str(), kv.second.taps, kv.second.cin, kv.second.cout, kv.second.w_off, kv.second.b_off);
    all += b;
  }
  const int rc = put_text(all, out, cap);
  return rc ? rc : e.code;
}
// the layer names in block order, one per line
int pc_layer_names(int depth, char* out, int cap) {
  std::string all;
  for (const std::string& n : sh::unet_layer_names(depth)) all += n + "\n";
  return put_text(all, out, cap);
}

// ParamState: events by number
enum { EV_UNET_LOADED, EV_RFC_LOADED, EV_BLOCK_EXPOSED, EV_BLOCK_LOST, EV_PACKED16, EV_PACKED_X3, EV_PACKTAB_UPLOADED, EV_FOREST_PACKED };
void* pc_state_new() { return new sh::ParamState(); }
void pc_state_free(void* h) { delete (sh::ParamState*)h; }
void pc_state_event(void* h, int ev, long long a, long long b, long long c) {
  sh::ParamState& s = *(sh::ParamState*)h;
  switch (ev) {
    case EV_UNET_LOADED: s.unet_loaded((int)a, (int)b, (size_t)c); break;
    case EV_RFC_LOADED: s.rfc_loaded((size_t)a, (size_t)b); break;
    case EV_BLOCK_EXPOSED: s.block_exposed(); break;
    case EV_BLOCK_LOST: s.block_lost(); break;
    case EV_PACKED16: s.packed16((int)a); break;
    case EV_PACKED_X3: s.packed_x3(); break;
    case EV_PACKTAB_UPLOADED: s.packtab_uploaded(); break;
    default: s.forest_packed(); break;
  }
}
// out: has_unet, has_rfc, base, depth, unet_floats, nodes, trees, need_pack16(0), need_pack16(1), need_pack_x3, need_packtab, need_forest_pack
void pc_state_queries(const void* h, long long* out) {
  const sh::ParamState& s = *(const sh::ParamState*)h;
  const sh::ParamShape& p = s.shape();
  const long long q[12] = {s.has_unet(), s.has_rfc(), p.base, p.depth, (long long)p.unet_floats, (long long)p.nodes, (long long)p.trees,
                           s.need_pack16(0), s.need_pack16(1), s.need_pack_x3(), s.need_packtab(), s.need_forest_pack()};
  memcpy(out, q, sizeof q);
}
int pc_same_shape(const void* a, const void* b) { return ((const sh::ParamState*)a)->same_shape(*(const sh::ParamState*)b); }
}

#define CHECK(cond) do { if (!(cond)) { printf("params_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  // layout, view, mirror: the shipped shape, an empty network, an empty forest, nothing at all
  const u64 shapes[4][3] = {{7759521, 32282, 40}, {0, 801, 1}, {100961, 0, 0}, {0, 0, 0}};
  for (auto& s : shapes) {
    u64 L[8], V[6], M[21];
    pc_layout(s[0], s[1], s[2], L);
    CHECK(L[0] == 0 && L[1] == 4 * s[0] && L[6] == 4 * s[0] + 20 * s[1] && L[7] == 4 * s[0] + 20 * s[1] + 4 * s[2]);
    pc_forest_view(s[0], s[1], s[2], 4096, V);
    for (int k = 0; k < 6; ++k) CHECK(V[k] == 4096 + 4 * s[0] + 4 * s[1] * k);
    pc_mirror(s[0], s[1], s[2], M);
    for (int k = 0; k < 7; ++k) CHECK(M[3 * k] == (k == 0 ? s[0] : k == 6 ? s[2] : s[1]) && M[3 * k + 1] == L[k] && M[3 * k + 2] == 4 * M[3 * k]);
  }
  // forest check: two complete trees of depth 3 (15 nodes each), then every fault
  const int n = 30;
  std::vector<int32_t> feat(n), ti(n), fi(n), roots = {0, 15};
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 15; ++i) {
      feat[15 * t + i] = (i + t) % pc_features();
      ti[15 * t + i] = i < 7 ? 15 * t + 2 * i + 1 : -1;
      fi[15 * t + i] = i < 7 ? 15 * t + 2 * i + 2 : -1;
    }
  const char* text = nullptr;
  auto check = [&](std::vector<int32_t> f, std::vector<int32_t> a, std::vector<int32_t> b, std::vector<int32_t> r) {
    return pc_forest_check(f.data(), a.data(), b.data(), n, r.data(), (int)r.size(), &text);
  };
  CHECK(check(feat, ti, fi, roots) == SH_OK && !*text);
  CHECK(pc_forest_check(nullptr, nullptr, nullptr, 0, nullptr, 0, &text) == SH_OK);
  auto with = [](std::vector<int32_t> v, int at, int32_t x) { v[at] = x; return v; };
  CHECK(check(with(feat, 3, -1), ti, fi, roots) == SH_ERR_ARG && !strcmp(text, "feature id out of range"));
  CHECK(check(with(feat, 29, pc_features()), ti, fi, roots) == SH_ERR_ARG && !strcmp(text, "feature id out of range"));
  CHECK(check(feat, with(ti, 9, 3), fi, roots) == SH_ERR_ARG && !strcmp(text, "bad child index"));
  CHECK(check(feat, ti, with(fi, 2, n), roots) == SH_ERR_ARG && !strcmp(text, "bad child index"));
  CHECK(check(feat, ti, fi, {0, -1}) == SH_ERR_ARG && !strcmp(text, "bad root"));
  CHECK(check(feat, ti, fi, {n, 15}) == SH_ERR_ARG && !strcmp(text, "bad root"));
  CHECK(check(feat, with(ti, 3, 0), fi, roots) == SH_ERR_ARG && strstr(text, "forest"));       // a cycle
  CHECK(check(feat, with(ti, 16, 1), fi, roots) == SH_ERR_ARG && strstr(text, "forest"));      // a shared subtree
  CHECK(check(feat, ti, fi, {0, 0}) == SH_ERR_ARG && strstr(text, "forest"));
  CHECK(check(with(feat, 20, 99), with(ti, 3, 0), fi, {0, -1}) == SH_ERR_ARG && !strcmp(text, "feature id out of range"));      // the earliest of three
  CHECK(check(feat, with(ti, 3, 0), fi, {0, -1}) == SH_ERR_ARG && !strcmp(text, "bad root"));
  // run parameters
  sh_params p;
  pc_default_params(&p);
  CHECK(pc_run_params(&p, &text) == SH_OK && p.groove_deg_window == 7.0 && p.unet_dtype == SH_UNET_F32 && p.bone_kind == SH_BONE_HUMERUS);
  sh_params q = p; q.canal_cutoff[1] = 1.5;
  CHECK(pc_run_params(&q, &text) == SH_ERR_ARG && !strcmp(text, "cut-off fractions must lie in [0, 1]"));
  q = p; q.groove_cutoff[0] = 0.3;
  CHECK(pc_run_params(&q, &text) == SH_ERR_ARG && !strcmp(text, "groove_cutoff must select 330 proximal rows"));
  q = p; q.canal_cutoff[0] = 0.75;
  CHECK(pc_run_params(&q, &text) == SH_ERR_ARG && !strcmp(text, "canal_cutoff selects fewer than 2 slices"));
  q = p; q.groove_deg_window = 181.0;
  CHECK(pc_run_params(&q, &text) == SH_ERR_ARG && strstr(text, "groove_deg_window"));
  q = p; q.unet_dtype = 4;
  CHECK(pc_run_params(&q, &text) == SH_ERR_ARG && strstr(text, "unet_dtype"));
  q = p; q.bone_kind = 2;
  CHECK(pc_run_params(&q, &text) == SH_ERR_ARG && strstr(text, "bone_kind"));
  // layer tables
  static char out[1 << 14];
  const int nets[5][2] = {{32, 1}, {32, 4}, {96, 2}, {256, 1}, {64, 6}};
  long long nf = 0;
  for (auto& net : nets) {
    CHECK(pc_layer_table(net[0], net[1], out, sizeof out, &nf, &text) == SH_OK && nf > 0);
    int lines = 0;
    for (const char* c = out; *c; ++c) lines += *c == '\n';
    CHECK(lines == 5 * net[1] + 3);
    CHECK(pc_layer_names(net[1], out, sizeof out) == 0);
  }
  CHECK(pc_layer_table(32, 4, out, sizeof out, &nf, &text) == SH_OK && nf == 7759521);
  const int bad[5][2] = {{16, 4}, {48, 4}, {SH_UNET_MAXBASE + 32, 1}, {32, 0}, {32, 7}};
  for (auto& net : bad) CHECK(pc_layer_table(net[0], net[1], out, sizeof out, &nf, &text) == SH_ERR_ARG && !*out && nf == 0 && !strcmp(text, SH_UNET_SHAPE_REFUSAL));
  // state: a seeded walk over the events; the invariants of every event hold after it
  void* h = pc_state_new();
  void* g = pc_state_new();
  long long s[12];
  pc_state_queries(h, s);
  const long long fresh[12] = {0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1};
  CHECK(!memcmp(s, fresh, sizeof s) && pc_same_shape(h, g));
  unsigned long long rng = 12345;
  for (int step = 0; step < 4000; ++step) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const int ev = (int)((rng >> 33) % 8), a = (int)((rng >> 40) % 2);
    pc_state_event(h, ev, ev == EV_UNET_LOADED ? 32 * (a + 1) : ev == EV_RFC_LOADED ? 801 + a : a, ev == EV_UNET_LOADED ? 1 + a : 1 + a, 1000 + a);
    pc_state_queries(h, s);
    if (ev == EV_UNET_LOADED) CHECK(s[0] == 1 && s[2] == 32 * (a + 1) && s[3] == 1 + a && s[4] == 1000 + a && s[10] == 1);
    if (ev == EV_RFC_LOADED) CHECK(s[1] == 1 && s[5] == 801 + a && s[6] == 1 + a && s[11] == 1);
    if (ev == EV_BLOCK_EXPOSED) CHECK(s[7] == 1 && s[8] == 1 && s[9] == 1 && s[11] == 1);
    if (ev == EV_BLOCK_LOST) CHECK(!memcmp(s, fresh, sizeof s));
    if (ev == EV_PACKED16) CHECK(s[7 + a] == 0 && s[8 - a] == 1);
    if (ev == EV_PACKED_X3) CHECK(s[9] == 0);
    if (ev == EV_PACKTAB_UPLOADED) CHECK(s[10] == 0);
    if (ev == EV_FOREST_PACKED) CHECK(s[11] == 0);
  }
  pc_state_event(h, EV_BLOCK_LOST, 0, 0, 0);
  pc_state_event(h, EV_UNET_LOADED, 32, 4, 7759521);
  CHECK(!pc_same_shape(h, g));
  pc_state_event(g, EV_UNET_LOADED, 32, 4, 7759521);
  pc_state_event(g, EV_PACKED16, 1, 0, 0);
  CHECK(pc_same_shape(h, g));
  pc_state_event(g, EV_RFC_LOADED, 801, 1, 0);
  CHECK(!pc_same_shape(h, g) && !pc_same_shape(g, h));
  pc_state_free(h);
  pc_state_free(g);
  printf("params_check OK (4 layouts, 13 forests, 7 parameter sets, 10 layer tables, 4000 events)\n");
  return 0;
}
