// Test shim (NOT product): the host rules of the OBB stage (shoulder_amd/csrc/sh_obb_plan.h: hull_need, hull_fits, the two growth
// rules, hull_source and what follows from it, early_upload_ok, obb_plan) on the host, for tests/test_obb_plan_host.py.  Its own
// main() walks the boundary cases of the same calls, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include "../../shoulder_amd/csrc/sh_obb_plan.h"

#include <stdio.h>
#include <vector>
using namespace sh;

// ---- hull counts and the growth rules: capacities and needs as (v, f, e) --------------------------------------------------------------
extern "C" void oc_hull_need(const int* counts, int B, int* out) { const HullNeed n = hull_need(counts, B); out[0] = n.v; out[1] = n.f; out[2] = n.e; }
extern "C" int oc_hull_fits(const int* need, const int* cap) { return hull_fits(HullNeed{need[0], need[1], need[2]}, HullCap{cap[0], cap[1], cap[2]}) ? 1 : 0; }
extern "C" void oc_record_grown(const int* now, const int* need, int* out) {
  const HullCap g = hull_record_grown(HullCap{now[0], now[1], now[2]}, HullNeed{need[0], need[1], need[2]});
  out[0] = g.v; out[1] = g.f; out[2] = g.e;
}
extern "C" void oc_pitch_grown(const int* demand, int* out) {
  const HullCap g = hull_pitch_grown(HullNeed{demand[0], demand[1], demand[2]});
  out[0] = g.v; out[1] = g.f; out[2] = g.e;
}
extern "C" void oc_start_caps(int* out) { out[0] = SH_HV; out[1] = SH_HF; out[2] = SH_HE; out[3] = HD_SLOTS; out[4] = SH_OBB_TILE; }

// ---- where the hulls come from -> out: source, from_host, upload pending without / with an early upload, nfmax -----------------------------
extern "C" void oc_hull_source(int redo_nf, int device_now, int prepared_slot, int skip_nfmax, int slot_nf, int* out) {
  const HullSource s = hull_source(redo_nf, device_now != 0, prepared_slot);
  out[0] = (int)s; out[1] = hull_from_host(s); out[2] = hull_upload_pending(s, false); out[3] = hull_upload_pending(s, true);
  out[4] = hull_nfmax(s, redo_nf, skip_nfmax, HullNeed{1, slot_nf, 1});
}

// bytes: hull.hv, hull.normals, hull.edges, hull.nv, hull.nf, hull.ne
extern "C" int oc_early_upload_ok(int have_ev, int B, const int* cap, const unsigned long long* bytes) {
  const HullRecBytes z = {(size_t)bytes[0], (size_t)bytes[1], (size_t)bytes[2], (size_t)bytes[3], (size_t)bytes[4], (size_t)bytes[5]};
  return early_upload_ok(have_ev != 0, B, HullCap{cap[0], cap[1], cap[2]}, z) ? 1 : 0;
}

// ---- the launch plan -> out[19]: tier, TT, nemax, area2_grid, bnd_tiles, bounds_grid, ntiles, (mode, nt_pass, grid) x 2, nwg, silcap, four byte sizes
extern "C" void oc_obb_plan(int B, int nfmax, const int* cap, int sil_need, int nf_over, int prune, long long* out) {
  const ObbPlan p = obb_plan(B, nfmax, HullCap{cap[0], cap[1], cap[2]}, sil_need, nf_over != 0, prune != 0);
  const long long f[19] = {p.tier, p.TT, p.nemax, p.area2_grid, p.bnd_tiles, p.bounds_grid, p.ntiles,
                           p.pass[0].mode, p.pass[0].nt_pass, p.pass[0].grid, p.pass[1].mode, p.pass[1].nt_pass, p.pass[1].grid,
                           p.nwg, p.silcap, (long long)p.ws.fmask, (long long)p.ws.lists, (long long)p.ws.sxy, (long long)p.ws.area};
  for (int i = 0; i < 19; ++i) out[i] = f[i];
}

// ---- stand-alone run (sanitizer build): the boundary cases of every rule ---------------------------------------------------------------
#define CHECK(x) do { if (!(x)) { printf("obb_plan_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  const int start[3] = {SH_HV, SH_HF, SH_HE};
  int out[5];
  for (int B : {1, 3}) {      // the maximum in every place of every array; an all-zero block
    std::vector<int> cnt(3 * (size_t)B, 0);
    oc_hull_need(cnt.data(), B, out);
    CHECK(out[0] == 1 && out[1] == 1 && out[2] == 1);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < B; ++b) {
        std::vector<int> c2(3 * (size_t)B, 2);
        c2[(size_t)a * B + b] = 7;
        oc_hull_need(c2.data(), B, out);
        for (int k = 0; k < 3; ++k) CHECK(out[k] == (k == a ? 7 : 2));
      }
  }
  for (int k = 0; k < 3; ++k) {      // equality fits, one above does not; the record grows in that field alone and never shrinks
    int need[3] = {start[0], start[1], start[2]}, g[3];
    CHECK(oc_hull_fits(need, start) == 1);
    oc_record_grown(start, need, g);
    CHECK(g[0] == start[0] && g[1] == start[1] && g[2] == start[2]);
    need[k] += 1;
    CHECK(oc_hull_fits(need, start) == 0);
    oc_record_grown(start, need, g);
    for (int j = 0; j < 3; ++j) CHECK(j == k ? (g[j] > start[j] && g[j] % 1024 == 0) : g[j] == start[j]);
    const int small[3] = {1, 1, 1};
    oc_record_grown(g, small, out);
    CHECK(out[0] == g[0] && out[1] == g[1] && out[2] == g[2]);
  }
  { const int need[3] = {16385, 1, 1}; oc_record_grown(start, need, out); CHECK(out[0] == 19456); }      // (16 385 + 2 048 + 1 023) / 1024 * 1024
  { const int d[3] = {1, 40000, 1}; oc_pitch_grown(d, out); CHECK(out[0] == SH_HV && out[1] == 40960 && out[2] == SH_HE); }
  for (int redo = 0; redo < 2; ++redo)
    for (int dev = 0; dev < 2; ++dev)
      for (int prep = -1; prep < 2; ++prep) {
        oc_hull_source(redo ? 100 : 0, dev, prep, 5000, 2732, out);
        const int want = redo ? HULL_REDO : dev ? HULL_DEVICE : prep >= 0 ? HULL_PREPARED : HULL_FOREGROUND;
        CHECK(out[0] == want && out[4] == (redo ? 100 : dev ? 5000 : 2732));
      }
  {
    const unsigned long long need[6] = {64ull * SH_HV * 24, 64ull * SH_HF * 24, 64ull * SH_HE * 16, 256, 256, 256};
    CHECK(oc_early_upload_ok(1, 64, start, need) == 1 && oc_early_upload_ok(0, 64, start, need) == 0);
    for (int i = 0; i < 6; ++i) {
      unsigned long long z[6];
      for (int j = 0; j < 6; ++j) z[j] = need[j] - (j == i ? 1 : 0);
      CHECK(oc_early_upload_ok(1, 64, start, z) == 0);
    }
  }
  const int grown[3] = {20480, 40960, 61440};
  long long f[19];
  int n = 0;
  for (int nfmax : {1, 16, 17, 2732, 8192, 8193, 32768, 32769})
    for (int sil : {0, 512, 513, 2048, 2049})
      for (int over = 0; over < 2; ++over)
        for (int B : {1, 7, 8, 9, 64})
          for (int prune = 0; prune < 2; ++prune)
            for (const int* hc : {start, grown}) {
              oc_obb_plan(B, nfmax, hc, sil, over, prune, f);
              const bool ws = f[0] == OBB_TIER_WORKSPACE;
              CHECK(ws == (nfmax > 32768 || sil > 2048 || over));
              CHECK(f[11] * f[1] >= nfmax && f[8] * f[1] == SH_OBB_TILE);
              for (int g : {5, 9, 12}) CHECK(f[g] > 0 && ((ws && g != 5) ? (f[g] <= 256) : (f[g] % 8 == 0)));
              CHECK(ws ? (f[14] >= hc[0] + 64 && f[15] == 256ll * hc[1]) : (f[13] == 0 && f[14] == 0 && f[15] + f[16] + f[17] + f[18] == 0));
              ++n;
            }
  CHECK(n == 1600);
  printf("obb_plan_check OK (%d plans)\n", n);
  return 0;
}
