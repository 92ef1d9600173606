// Test shim (NOT product): the host decisions of the arthroplasty chain (shoulder_amd/csrc/sh_arthro.h) for tests/test_arthro_host.py.
// A precheck returns the error code and writes the text behind the entry point's name into `text` (empty when accepted).
// Facts of a call: ctx, B, n_pending, landmarks as ints and a Sim (an ArthroState with the batch generation a context would hold).
// A plan call writes, for every buffer of ARTHRO_BUFS in list order, its bytes (0: not ensured by that call) and its elem; ac_names
// gives the names in the same order.  -DARTHRO_CHECK_MAIN: a stand-alone program that runs one case of each group (for a sanitizer build).
#include "../../shoulder_amd/csrc/sh_arthro.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace sh;

struct Sim { ArthroState st; unsigned long long gen = 0; };
static ArthroFacts facts(int ctx, int B, int n_pending, int landmarks, const Sim* s) {
  if (!ctx) return ArthroFacts{false, 0, 0, 0, false, nullptr};
  return ArthroFacts{true, B, n_pending, s->gen, landmarks != 0, &s->st};
}
static int give(const ArthroError& e, char* text, int cap) { snprintf(text, (size_t)cap, "%s", e.text.c_str()); return e.code; }
static int dump(const ArthroBytes& z, unsigned long long* bytes, int* elems) {
  int i = 0;
#define X(f, name, T, elem) bytes[i] = z.f; elems[i] = elem; ++i;
  ARTHRO_BUFS(X)
#undef X
  return i;
}
static sh_resection a_rec; static sh_head_fit a_fit; static sh_seat a_seat; static sh_stem_fit a_stem; static sh_plan a_plan; static int a_int;      // "an output is there"

extern "C" {
int ac_names(const char** names) {
  int i = 0;
#define X(f, name, T, elem) names[i++] = name;
  ARTHRO_BUFS(X)
#undef X
  return i;
}
Sim* ac_new() { return new Sim; }
Sim* ac_clone(const Sim* s) { return new Sim(*s); }
void ac_free(Sim* s) { delete s; }
// events: 0 upload | 1 run submitted with mask a | 2 resection at level a with P = b, K = c | 3 a resection that fails between begin and end
// | 4 profile with L = a, A = b | 5 stems with K = a | 6 stems that fail between begin and end | 7 a profile that fails between begin and end
void ac_event(Sim* s, int ev, int a, int b, int c) {
  switch (ev) {
    case 0: ++s->gen; break;
    case 1: s->st.run_submitted((uint32_t)a, s->gen); break;
    case 2: s->st.resect_begin(); s->st.resect_end((ResectLevel)a, b, c, s->gen); break;
    case 3: s->st.resect_begin(); break;
    case 4: { s->st.profile_begin(); const sh_canal_grid g = {1.5, 0.25, a, b}; s->st.profile_end(g, s->gen); break; }
    case 5: s->st.stems_begin(); s->st.stems_end(a); break;
    case 6: s->st.stems_begin(); break;
    case 7: s->st.profile_begin(); break;
  }
}
// records (without the "landmarks" fact), resected, seated, profiled, stems current, P, K_h, K_s, grid L, grid A
void ac_query(const Sim* s, int* q) {
  q[0] = s->st.has_records(s->gen); q[1] = s->st.resected(s->gen); q[2] = s->st.seated(s->gen); q[3] = s->st.profiled(s->gen); q[4] = s->st.stems_current(s->gen);
  q[5] = s->st.P(); q[6] = s->st.Kh(); q[7] = s->st.Ks(); q[8] = s->st.grid().L; q[9] = s->st.grid().A;
}

int ac_pre_resect(int level, const double* planes, const double* offs, int P, int out, int fit_out, const double* heads, int K, int mode, int seat_out, int ctx, int B,
                  int n_pending, int landmarks, const Sim* s, char* text, int cap) {
  const ResectRequest q{"", (ResectLevel)level, planes, (const sh_cut_offset*)offs, P, out ? &a_rec : nullptr, fit_out ? &a_fit : nullptr, (const sh_implant_head*)heads,
                        K, mode, seat_out ? &a_seat : nullptr};
  return give(precheck_resect(q, facts(ctx, B, n_pending, landmarks, s)), text, cap);
}
int ac_pre_ring(int b, int p, int out, int cap_pts, int n_out, int ctx, int B, int n_pending, int landmarks, const Sim* s, char* text, int cap) {
  static double pts[3];
  return give(precheck_ring(b, p, out ? pts : nullptr, cap_pts, n_out ? &a_int : nullptr, facts(ctx, B, n_pending, landmarks, s)), text, cap);
}
int ac_pre_profile(const sh_canal_grid* g, const double* frames, int ctx, int B, int n_pending, int landmarks, const Sim* s, char* text, int cap) {
  return give(precheck_profile(g, frames, facts(ctx, B, n_pending, landmarks, s)), text, cap);
}
int ac_pre_stems(const double* stems, int K, int out, int ctx, int B, int n_pending, int landmarks, const Sim* s, char* text, int cap) {
  return give(precheck_stems((const sh_stem*)stems, K, out ? &a_stem : nullptr, facts(ctx, B, n_pending, landmarks, s)), text, cap);
}
int ac_pre_plan(const double* rule, const double* ref_planes, int N, int out, int ctx, int B, int n_pending, int landmarks, const Sim* s, char* text, int cap) {
  return give(precheck_plan((const sh_plan_rule*)rule, ref_planes, N, out ? &a_plan : nullptr, facts(ctx, B, n_pending, landmarks, s)), text, cap);
}

// pt: planes per pass, tmax
int ac_resect_plan(int B, int P, long long maxF, int level, int K, int from_offsets, int* pt, unsigned long long* bytes, int* elems) {
  const ResectPlan p = resect_plan(B, P, maxF, (ResectLevel)level, K, from_offsets != 0);
  pt[0] = p.pc; pt[1] = p.tmax;
  return dump(p.bytes, bytes, elems);
}
int ac_ring_tiles(long long nf) { return ring_tiles(nf); }
int ac_canal_plan(int B, int L, int A, long long maxF, unsigned long long* tr, unsigned long long* bytes, int* elems) {
  const CanalPlan p = canal_plan(B, L, A, maxF);
  tr[0] = (unsigned long long)p.tmax; tr[1] = p.rays;
  return dump(p.bytes, bytes, elems);
}
int ac_stem_bytes(int B, int P, int K, unsigned long long* bytes, int* elems) { return dump(stem_bytes(B, P, K), bytes, elems); }
int ac_plan_plan(int B, int P, int Kh, int Ks, int N, long long maxV, unsigned long long* tc, unsigned long long* bytes, int* elems) {
  const PlanPlan p = plan_plan(B, P, Kh, Ks, N, maxV);
  tc[0] = (unsigned long long)p.tmax; tc[1] = p.cuts;
  return dump(p.bytes, bytes, elems);
}
}

#ifdef ARTHRO_CHECK_MAIN
#define EXPECT(cond) do { if (!(cond)) { printf("arthro_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
int main() {
  char text[256];
  const char* names[64];
  unsigned long long bytes[64], two[2];
  int elems[64], pt[2], q[10];
  const int nb = ac_names(names);
  EXPECT(nb == 35 && !strcmp(names[0], "resect.planes") && !strcmp(names[nb - 1], "plan.out"));
  Sim* s = ac_new();
  ac_event(s, 0, 0, 0, 0);
  // checks: 4096 planes accepted, a NaN in the last one refused; a frame with determinant -1
  std::vector<double> planes(6 * 4096, 1.0);
  EXPECT(ac_pre_resect(0, planes.data(), nullptr, 4096, 1, 0, nullptr, 0, 0, 0, 1, 1, 0, 0, s, text, 256) == SH_OK && !text[0]);
  planes[6 * 4095 + 4] = NAN;
  EXPECT(ac_pre_resect(0, planes.data(), nullptr, 4096, 1, 0, nullptr, 0, 0, 0, 1, 1, 0, 0, s, text, 256) == SH_ERR_ARG && !strcmp(text, "zero normal or non-finite plane"));
  double frames[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1};
  const sh_canal_grid g = {1.0, 0.5, 1024, 256};
  EXPECT(ac_pre_profile(&g, frames, 1, 2, 0, 0, s, text, 256) == SH_ERR_ARG && !strcmp(text, "frame 1 is not a rigid CT -> frame matrix"));
  const double heads[4] = {6.0, 3.0, 5.0, 10.0};
  EXPECT(ac_pre_resect(2, planes.data(), nullptr, 1, 1, 1, heads, 2, 0, 1, 1, 1, 0, 0, s, text, 256) == SH_ERR_ARG && strstr(text, "bad catalogue"));
  // first-error order: a bad stem together with runs in flight; a bad rule together with a null context
  const double stems[3] = {2.0, -1.0, 1.0};
  EXPECT(ac_pre_stems(stems, 1, 1, 1, 1, 1, 0, s, text, 256) == SH_ERR_ARG && strstr(text, "finite and > 0"));
  double rule[12] = {0};
  rule[5] = -1.0;
  EXPECT(ac_pre_plan(rule, nullptr, 8, 1, 0, 0, 0, 0, nullptr, text, 256) == SH_ERR_ARG && strstr(text, "bad rule"));
  EXPECT(ac_pre_ring(0, 0, 0, 0, 1, 1, 1, 0, 0, s, text, 256) == SH_ERR_STATE && !strcmp(text, "no resection of the resident batch"));
  // pass plan
  EXPECT(ac_resect_plan(64, 65, 520, 2, 4, 0, pt, bytes, elems) == nb && pt[0] == 64 && pt[1] == 3 && bytes[0] == 64ull * 65 * 48 && bytes[8] == 0);
  EXPECT(ac_canal_plan(3, 64, 64, 520, two, bytes, elems) == nb && two[0] == 3 && two[1] == 3ull * 64 * 64 && bytes[0] == 0);
  EXPECT(ac_stem_bytes(3, 4, 8, bytes, elems) == nb && ac_plan_plan(3, 4, 4, 8, 8, 262, two, bytes, elems) == nb && two[0] == 2 && two[1] == 12);
  EXPECT(ac_ring_tiles(0) == 1 && ac_ring_tiles(257) == 2);
  // state: seated chain, then a failed stems call leaves no stems
  ac_event(s, 4, 64, 64, 0); ac_event(s, 2, 2, 4, 4); ac_event(s, 5, 8, 0, 0);
  ac_query(s, q);
  EXPECT(!q[0] && q[1] && q[2] && q[3] && q[4] && q[5] == 4 && q[6] == 4 && q[7] == 8 && q[8] == 64);
  ac_event(s, 6, 0, 0, 0);
  ac_query(s, q);
  EXPECT(q[2] && !q[4]);
  ac_free(s);
  printf("arthro_check: ok\n");
  return 0;
}
#endif
