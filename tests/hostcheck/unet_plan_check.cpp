// Test shim (NOT product): the host decisions of the UNet runner (shoulder_amd/csrc/sh_unet_plan.h) for tests/test_unet_plan_host.py.
// The layer table is sh_load_unet's for (base, depth).  up_plan writes one line per step:
//   timer text kind ek t0 t1 t2 t3 gx gy gz block C0 C1 H W cout relu fuse src0 src1 dst pool layer layer2 tk_items tk_nwg tk_ngrp
// ("-" for an empty name).  Every call returns the error code and *text (null when accepted).
// -DUNET_PLAN_MAIN: a stand-alone program over the same calls (for a sanitizer build).
#include "../../shoulder_amd/csrc/sh_unet_plan.h"
#include <cstring>

static sh::UnetLayers layer_table(int base, int depth, size_t* n_floats) {      // (the product's: a refused shape gives an empty table)
  sh::UnetLayers layers;
  sh::unet_layer_table(base, depth, &layers, n_floats);
  return layers;
}

static std::string g_text;
static int give(const sh::UnetError& e, const char** text) {
  g_text = e.text;
  *text = e.code == SH_OK ? nullptr : g_text.c_str();
  return e.code;
}

extern "C" {
long long up_floats(int base, int depth) { size_t n; layer_table(base, depth, &n); return (long long)n; }
// the offset (floats) of a layer's weights in the block, -1: no such layer
long long up_w_off(int base, int depth, const char* layer) {
  size_t n;
  const sh::UnetLayers l = layer_table(base, depth, &n);
  auto it = l.find(layer);
  return it == l.end() ? -1 : (long long)it->second.w_off;
}
int up_plan(int base, int depth, int dtype, int reference, int H, int W, int nimg, int pgrid, int raw, char* out, int cap, const char** text) {
  size_t n;
  const sh::UnetLayers layers = layer_table(base, depth, &n);
  std::vector<sh::UnetStep> steps;
  const int rc = give(sh::unet_plan(layers, base, depth, dtype, reference != 0, H, W, nimg, pgrid, raw != 0, &steps), text);
  std::string all;
  if (rc == SH_OK)
    for (const sh::UnetStep& s : steps) {
      char b[400];
      snprintf(b, sizeof b, "%s %s %d %d %d %d %d %d %u %u %u %u %d %d %d %d %d %d %d %d %d %d %d %s %s %d %d %d\n", s.timer.c_str(), s.text().c_str(), s.kind, s.ek,
               s.t[0], s.t[1], s.t[2], s.t[3], s.grid[0], s.grid[1], s.grid[2], s.block, s.C0, s.C1, s.H, s.W, s.cout, s.relu, s.fuse, s.src0, s.src1, s.dst, s.pool,
               s.layer.empty() ? "-" : s.layer.c_str(), s.layer2.empty() ? "-" : s.layer2.c_str(), s.tk_items, s.tk_nwg, s.tk_ngrp);
      all += b;
    }
  if ((int)all.size() + 1 > cap) return -100;
  memcpy(out, all.c_str(), all.size() + 1);
  return rc;
}
int up_level0_fused(int dtype, int reference, int base, int depth, int H, int W) { return sh::plan_level0_fused(dtype, reference != 0, base, depth, H, W); }
int up_tickets(int total, int nwg, int ngrp, int* out, int cap) {
  const std::vector<int> t = sh::ticket_table(total, nwg, ngrp);
  if ((int)t.size() > cap) return -100;
  std::copy(t.begin(), t.end(), out);
  return (int)t.size();
}
// rows: first, w_off, T, Cin, Cout, pad per layer
int up_pack(int base, int depth, const float* host_w, long long* rows, int cap, int* nrows, long long* total, const char** text) {
  size_t n;
  const sh::UnetLayers layers = layer_table(base, depth, &n);
  std::vector<sh::PackRow> tab;
  const int rc = give(sh::pack_table(layers, &tab, total, host_w, host_w ? n : 0), text);
  if ((int)tab.size() > cap) return -100;
  *nrows = (int)tab.size();
  for (size_t i = 0; i < tab.size(); ++i) {
    const long long r[6] = {tab[i].first, tab[i].w_off, tab[i].T, tab[i].Cin, tab[i].Cout, tab[i].pad};
    std::copy(r, r + 6, rows + 6 * i);
  }
  return rc;
}
}

#ifdef UNET_PLAN_MAIN
int main() {
  static char out[1 << 16];
  const char* text = nullptr;
  const int nets[5][4] = {{32, 4, 256, 256}, {96, 2, 64, 64}, {160, 1, 32, 64}, {64, 3, 128, 256}, {256, 1, 32, 32}};
  const int sizes[3][2] = {{256, 256}, {256, 512}, {512, 512}}, nimgs[4] = {1, 5, 64, 200}, grids[2] = {256, 224};
  long plans = 0, steps = 0, tables = 0;
  std::vector<int> tab(1 << 18);
  for (int net = 0; net < 5; ++net)
    for (int sz = 0; sz < (net ? 1 : 3); ++sz)
      for (int dtype = 0; dtype < 4; ++dtype)
        for (int ref = 0; ref < 2; ++ref)
          for (int ni = 0; ni < 4; ++ni)
            for (int g = 0; g < 2; ++g)
              for (int raw = 0; raw < 2; ++raw) {
                const int H = net ? nets[net][2] : sizes[sz][0], W = net ? nets[net][3] : sizes[sz][1];
                if (up_plan(nets[net][0], nets[net][1], dtype, ref, H, W, nimgs[ni], grids[g], raw, out, sizeof out, &text) != SH_OK) { printf("plan failed: %s\n", text ? text : "?"); return 1; }
                ++plans;
                for (const char* p = out; *p; ++p) steps += *p == '\n';
                size_t n;
                const sh::UnetLayers layers = layer_table(nets[net][0], nets[net][1], &n);
                std::vector<sh::UnetStep> st;
                sh::unet_plan(layers, nets[net][0], nets[net][1], dtype, ref != 0, H, W, nimgs[ni], grids[g], raw != 0, &st);
                for (const sh::UnetStep& s : st)
                  if (s.tk_items) { if (up_tickets(s.tk_items, s.tk_nwg, s.tk_ngrp, tab.data(), (int)tab.size()) < 2) return 2; ++tables; }
              }
  const int edge[3][3] = {{5, 256, 1}, {1030, 224, 4}, {64, 256, 8}};
  for (auto& e : edge) if (up_tickets(e[0], e[1], e[2], tab.data(), (int)tab.size()) < 2) return 3;
  if (up_plan(32, 4, 1, 0, 250, 512, 1, 256, 0, out, sizeof out, &text) != SH_ERR_ARG || !text) return 4;
  std::vector<float> w((size_t)up_floats(32, 4), 0.5f);
  std::vector<long long> rows(6 * 64);
  int nrows = 0; long long total = 0;
  if (up_pack(32, 4, w.data(), rows.data(), 64, &nrows, &total, &text) != SH_OK || nrows != 21) return 5;
  const int packed = nrows;
  w[(size_t)up_w_off(32, 4, "dec1a") + 7] = -2000.0f;
  if (up_pack(32, 4, w.data(), rows.data(), 64, &nrows, &total, &text) != SH_ERR_ARG || !text || !strstr(text, "dec1a")) return 6;
  printf("unet_plan_check: %ld plans, %ld steps, %ld ticket tables, pack table %d rows: OK\n", plans, steps, tables, packed);
  return 0;
}
#endif
