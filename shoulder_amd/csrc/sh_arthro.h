// sh_arthro.h -- what the arthroplasty chain (batched resection -> head fit -> seats -> canal profile -> stems -> ranked plans) decides
// on the host: are the arguments acceptable, which refusal comes first, how a sweep is split into passes and how large every named
// buffer is, and what is valid against what (ArthroState).  No kernels, no HIP types: sh_ctx.h includes it, and so does a plain g++
// (tests/hostcheck/arthro_check.cpp).  An error is a code plus the text BEHIND the entry point's name: the caller puts
// "sh_resect_planes: " (or the name it was called under) in front.  The entry points themselves are sh_arthro_host.h.
// The queries of the resident batch (rays, closest points, winding numbers, registration, mass properties, surface samples, mesh topology, vertex fields, geodesics) are no links of the chain:
// sh_query.h, on top of this header and included at its end.  What both use is here: how a buffer list declares its structs (SH_BUF_LIST), the mesh buffers
// (MeshBufs), ArthroError with the shared refusal texts, ArthroFacts and the `resident` check.
#pragma once
#include "../../include/shoulder_hip.h"
#include "sh_common.h"      // det3_of4, SH_MAXSEG

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

namespace sh {

// ---- the named buffers of the chain, one statement each: X(field, "name", element type, elem) ------------------------------------
// The name is what sh_fetch / sh_buffer_info see, elem the element size they report.  The sizes (ArthroBytes, filled by the *_plan
// functions below), allocation and the typed view of a call (sh_ctx.h: ensure_bytes, view_of) all come from these lists.
// The element types of kernel headers are only named here (a view holds pointers to them): this header needs none of them complete.
struct ResectPart; struct PlanTop; struct PlanTerm;
#define ARTHRO_RESECT_BUFS(X)                                                                                                      \
  X(planes, "resect.planes", double, 8) X(status, "resect.status", int, 4) X(slab, "resect.slab", ResectPart, 8)                   \
  X(segcnt, "resect.segcnt", int, 4) X(segs, "resect.segs", int, 4) X(out, "resect.out", sh_resection, 8)                          \
  X(one, "resect.one", sh_resection, 8) X(ring, "resect.ring", double, 8) X(offs, "resect.offs", double, 8)                        \
  X(fit_slab, "resect.fit_slab", double, 8) X(fit_moments, "resect.fit_moments", double, 8) X(fit_ring, "resect.fit_ring", double, 8) \
  X(fit_out, "resect.fit_out", sh_head_fit, 8) X(seat_ring, "resect.seat_ring", double, 8)                                         \
  X(seat_heads, "resect.seat_heads", sh_implant_head, 8) X(seat_out, "resect.seat_out", sh_seat, 8)
#define ARTHRO_CANAL_BUFS(X)                                                                                                       \
  X(canal_near, "canal.near", double, 8) X(canal_far, "canal.far", double, 8) X(canal_levels, "canal.levels", sh_canal_level, 8)   \
  X(canal_frames, "canal.frames", double, 8) X(canal_status, "canal.status", int, 4) X(canal_dirs, "canal.dirs", double, 8)
#define ARTHRO_STEM_BUFS(X) X(stem_catalogue, "stem.catalogue", sh_stem, 8) X(stem_out, "stem.out", sh_stem_fit, 8)
#define ARTHRO_PLAN_BUFS(X)                                                                                                        \
  X(plan_ref_planes, "plan.ref_planes", double, 8) X(plan_compat, "plan.compat", unsigned long long, 8)                            \
  X(plan_ref_slab, "plan.ref_slab", PlanTop, 8) X(plan_ref, "plan.ref", sh_plan_ref, 8)                                            \
  X(plan_cut_terms, "plan.cut_terms", PlanTerm, 8) X(plan_head_terms, "plan.head_terms", PlanTerm, 8)                              \
  X(plan_stem_terms, "plan.stem_terms", PlanTerm, 8) X(plan_cut_vals, "plan.cut_vals", double, 8)                                  \
  X(plan_head_vals, "plan.head_vals", double, 8) X(plan_stem_vals, "plan.stem_vals", double, 8) X(plan_out, "plan.out", sh_plan, 8)
#define ARTHRO_BUFS(X) ARTHRO_RESECT_BUFS(X) ARTHRO_CANAL_BUFS(X) ARTHRO_STEM_BUFS(X) ARTHRO_PLAN_BUFS(X)
// what the chain reads and does not own (the mesh: upload / commit; the records of a run: alloc_batch): X(field, "name", type)
#define ARTHRO_INPUT_BUFS(X)                                                                                                       \
  X(verts, "verts", const float) X(faces, "faces", const int) X(voff, "voff", const long long) X(foff, "foff", const long long)    \
  X(lm, "landmarks", const sh_landmarks) /* null in the view without a run of the resident batch with the anatomic neck and the csys */

// One line per list declares its structs.  SH_BUF_LIST(Resect, ARTHRO_RESECT_BUFS) gives ResectBytes, the bytes of every buffer a call
// ensures (0: not this call's; every size of a call is > 0: B, P, K, L, A, N >= 1), and ResectBufs, the buffers as typed pointers (null:
// not there).  Every struct walks its own fields in list order: each(fn) calls fn(field, "field", "name"[, elem]).  What a call hands to
// its kernels is a view: the mesh's pointers and those of its lists in one struct (BufJoin).
#define SH_BUF_SIZE(f, name, T, ...) size_t f = 0;
#define SH_BUF_PTR(f, name, T, ...) T* f = nullptr;
#define SH_BUF_VISIT(f, name, T, ...) fn(f, #f, name, ##__VA_ARGS__);
#define SH_BUF_BYTES(Name, LIST) struct Name { LIST(SH_BUF_SIZE) template <typename F> void each(F&& fn) const { LIST(SH_BUF_VISIT) } };
#define SH_BUF_PTRS(Name, LIST) struct Name { LIST(SH_BUF_PTR) template <typename F> void each(F&& fn) { LIST(SH_BUF_VISIT) } };
#define SH_BUF_LIST(Name, LIST) SH_BUF_BYTES(Name##Bytes, LIST) SH_BUF_PTRS(Name##Bufs, LIST)
template <typename... Parts>
struct BufJoin : Parts... {      // several lists' structs as one: the fields of all, each() over all in order
  template <typename F> void each(F&& fn) { (Parts::each(fn), ...); }
  template <typename F> void each(F&& fn) const { (Parts::each(fn), ...); }
};
SH_BUF_PTRS(MeshBufs, ARTHRO_INPUT_BUFS)
SH_BUF_LIST(Resect, ARTHRO_RESECT_BUFS)
SH_BUF_LIST(Canal, ARTHRO_CANAL_BUFS)
SH_BUF_LIST(Stem, ARTHRO_STEM_BUFS)
SH_BUF_LIST(Plan, ARTHRO_PLAN_BUFS)
using ArthroBytes = BufJoin<ResectBytes, CanalBytes, StemBytes, PlanBytes>;
using ArthroView = BufJoin<MeshBufs, ResectBufs, CanalBufs, StemBufs, PlanBufs>;      // (sh_arthro_host.h arthro_view: group by group)

// what the kernel headers fix, restated (shoulder_hip.hip holds each against its header with a static_assert)
constexpr int AR_RS_TILE = 256, AR_HF_WORDS = 16, AR_RESECT_PART_BYTES = 32;      // SH_RS_TILE, SH_HF_WORDS, sizeof(ResectPart)
constexpr int AR_CANAL_TILE = 256, AR_PLAN_TILE = 256;                            // SH_CANAL_TILE, SH_PLAN_TILE
constexpr int AR_PLAN_TOP_BYTES = 16, AR_PLAN_TERM_BYTES = 16;                    // sizeof(PlanTop), sizeof(PlanTerm)

struct ArthroError { int code; std::string text; };      // code SH_OK: accepted (text empty)
inline ArthroError arthro_ok() { return {SH_OK, std::string()}; }
static const char* const AR_IN_FLIGHT = "runs are in flight (sh_collect them first)";
static const char* const AR_NO_MESHES = "no meshes uploaded";
static const char* const AR_NO_RESECTION = "no resection of the resident batch";

// what a call computes per cut: the record; the head fit beside it (the moment pass and the join that adds its slab and the ring's
// second moments); the seats of a catalogue on top (that join also stores the ring's in-plane coordinates of the pass)
enum ResectLevel { RS_RECORDS, RS_FIT, RS_SEAT };

struct ResectRequest {
  const char* fn;                    // the caller's name, for error texts
  ResectLevel level;
  const double* planes;              // B x P x (point, normal), or
  const sh_cut_offset* offs;         // P offsets, the same for every humerus (the one that is set is the source)
  int P;
  sh_resection* out;
  sh_head_fit* fit_out = nullptr;    // RS_FIT and up
  const sh_implant_head* heads = nullptr;      // RS_SEAT: the catalogue, its size, the centre mode and the records
  int K = 0, mode = 0;
  sh_seat* seat_out = nullptr;
};

// ---- the checks, each once --------------------------------------------------------------------------------------------------------
// n planes of (point, normal): the index of the first one that is not six finite doubles with a non-zero normal, or -1
inline long long first_bad_plane(const double* planes, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const double* pl = planes + 6 * i;
    bool fin = true;
    for (int k = 0; k < 6; ++k) fin = fin && std::isfinite(pl[k]);
    if (!fin || !((pl[3] * pl[3] + pl[4] * pl[4]) + pl[5] * pl[5] > 0.0)) return (long long)i;
  }
  return -1;
}

// every double of n structs T, which are nothing but doubles, passes `ok`
template <typename T, typename F>
inline bool all_doubles(const T* s, int n, F ok) {
  static_assert(sizeof(T) % sizeof(double) == 0 && alignof(T) == alignof(double), "a struct of doubles");
  const double* x = (const double*)s;
  for (size_t i = 0; i < (size_t)n * (sizeof(T) / sizeof(double)); ++i)
    if (!ok(x[i])) return false;
  return true;
}
static_assert(sizeof(sh_cut_offset) == 7 * sizeof(double), "sh_cut_offset is seven doubles");
static_assert(sizeof(sh_stem) == 3 * sizeof(double), "sh_stem is three doubles");
static_assert(sizeof(sh_plan_rule) == 12 * sizeof(double), "sh_plan_rule is twelve doubles");

inline bool cut_offsets_ok(const sh_cut_offset* offs, int P) { return all_doubles(offs, P, [](double x) { return std::isfinite(x); }); }

inline bool head_catalogue_ok(const sh_implant_head* heads, int K, int mode, const sh_seat* out) {
  if (!heads || !out || K < 1 || K > SH_SEAT_MAX_HEADS || (mode != SH_SEAT_CUT_CENTROID && mode != SH_SEAT_SPHERE_AXIS)) return false;
  for (int k = 0; k < K; ++k) {
    const double R = heads[k].radius, h = heads[k].thickness;
    if (!std::isfinite(R) || !std::isfinite(h) || !(h > 0.0) || !(h < 2.0 * R)) return false;
  }
  return true;
}

inline bool canal_grid_ok(const sh_canal_grid* g) {
  return g && std::isfinite(g->z0) && std::isfinite(g->dz) && g->dz > 0.0 && g->L >= 1 && g->L <= 1024 && g->A >= 3 && g->A <= 256;
}

// a rigid CT -> frame matrix: finite, last row 0 0 0 1, rotation rows orthonormal to 1e-9, determinant positive
inline bool rigid_frame_ok(const double* T) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T[i])) return false;
  if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double d = (T[4 * i] * T[4 * j] + T[4 * i + 1] * T[4 * j + 1]) + T[4 * i + 2] * T[4 * j + 2];
      if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-9)) return false;
    }
  return det3_of4(T) > 0.0;
}
inline int first_bad_frame(const double* frames, int B) {
  for (int b = 0; b < B; ++b)
    if (!rigid_frame_ok(frames + 16 * (size_t)b)) return b;
  return -1;
}

inline bool stem_catalogue_ok(const sh_stem* stems, int K) { return all_doubles(stems, K, [](double x) { return std::isfinite(x) && x > 0.0; }); }

inline bool plan_rule_ok(const sh_plan_rule* r) {
  if (!all_doubles(r, 1, [](double x) { return !std::isnan(x); })) return false;
  for (double w : {r->w_uncovered, r->w_overhang, r->w_cor, r->w_height, r->w_eccentricity, r->w_fill})
    if (!std::isfinite(w) || w < 0.0) return false;
  return r->margin >= 0.0;
}

// ---- the pass plan and the bytes of every buffer ------------------------------------------------------------------------------------
// Records: the slot ranges (4 KB per cut) and the slab (32 B per cut and tile) stay below 32 MB / 128 MB, so a pass takes at most
// 8 192 cuts; a sweep larger than that takes several passes over the mesh.  The pass a plane falls into does not change its record
// (the slab of a cut is its own).  Fit: the moment slab (128 B per cut and tile) has 128 MB of its own and a pass takes at most
// 4 096 cuts, so the planes per pass of a fitted sweep are at most the un-fitted ones -- which keep their split.  Seat: the ring
// coordinates of one pass (16 KB per cut; a fitted pass takes 4 096 / B planes but at least one, so max(B, 4 096) cuts: 64 MB up to
// B = 4 096 and the fitted split is kept), the catalogue and the B x P x K records, which have no limit of their own (SH_ERR_NOMEM
// when they do not fit).  "resect.slab" .. "resect.segs" are sized by the un-fitted split at every level.
struct ResectPlan { int pc, tmax; ArthroBytes bytes; };      // planes per pass, tiles per humerus in the slabs
inline long long tiles_of(long long n, int tile) { const long long t = (n + tile - 1) / tile; return t > 1 ? t : 1; }
inline ResectPlan resect_plan(int B, int P, long long maxF, ResectLevel level, int K, bool from_offsets) {
  auto clamp = [P](long long a, long long b) { const long long m = a < b ? a : b; return m < 1 ? 1 : (m < P ? m : P); };
  const long long tmax = tiles_of(maxF, AR_RS_TILE);
  const size_t n = (size_t)B * P;
  long long pc = clamp(8192 / B, (128LL << 20) / ((long long)AR_RESECT_PART_BYTES * B * tmax));
  ArthroBytes z;
  z.planes = n * 48; z.status = n * 4;
  z.slab = (size_t)B * pc * tmax * AR_RESECT_PART_BYTES; z.segcnt = (size_t)B * pc * 4; z.segs = (size_t)B * pc * SH_MAXSEG * 4;
  z.out = n * sizeof(sh_resection); z.one = sizeof(sh_resection); z.ring = (size_t)(SH_MAXSEG + 1) * 24;
  if (level >= RS_FIT) {
    pc = clamp(std::min<long long>(4096 / B, (128LL << 20) / (8LL * AR_HF_WORDS * B * tmax)), pc);
    z.fit_slab = (size_t)B * pc * tmax * AR_HF_WORDS * 8; z.fit_moments = n * 16 * 8; z.fit_ring = n * 8 * 8; z.fit_out = n * sizeof(sh_head_fit);
  }
  if (level == RS_SEAT) {
    z.seat_ring = (size_t)B * pc * 2 * SH_MAXSEG * 8; z.seat_heads = (size_t)K * sizeof(sh_implant_head); z.seat_out = n * K * sizeof(sh_seat);
  }
  if (from_offsets) z.offs = (size_t)P * sizeof(sh_cut_offset);
  return {(int)pc, (int)tmax, z};
}
// one cut of one humerus again (sh_resect_ring): its tiles
inline int ring_tiles(long long nf) { return (int)tiles_of(nf, AR_RS_TILE); }

struct CanalPlan { int tmax; size_t rays; ArthroBytes bytes; };      // face tiles per humerus, B x L x A
inline CanalPlan canal_plan(int B, int L, int A, long long maxF) {
  const size_t n = (size_t)B * L * A;
  ArthroBytes z;
  z.canal_near = n * 8; z.canal_far = n * 8; z.canal_levels = (size_t)B * L * sizeof(sh_canal_level);
  z.canal_frames = (size_t)B * 128; z.canal_status = (size_t)B * 4; z.canal_dirs = (size_t)A * 16;
  return {(int)tiles_of(maxF, AR_CANAL_TILE), n, z};
}

inline ArthroBytes stem_bytes(int B, int P, int K) {
  ArthroBytes z;
  z.stem_catalogue = (size_t)K * sizeof(sh_stem); z.stem_out = (size_t)B * P * K * sizeof(sh_stem_fit);
  return z;
}

struct PlanPlan { int tmax; size_t cuts; ArthroBytes bytes; };      // vertex tiles per humerus in "plan.ref_slab", B x P
inline PlanPlan plan_plan(int B, int P, int Kh, int Ks, int N, long long maxV) {
  const long long tmax = tiles_of(maxV, AR_PLAN_TILE);
  const size_t cuts = (size_t)B * P;
  ArthroBytes z;
  z.plan_ref_planes = (size_t)B * 48; z.plan_compat = (size_t)SH_SEAT_MAX_HEADS * 8;
  z.plan_ref_slab = (size_t)B * tmax * 2 * AR_PLAN_TOP_BYTES; z.plan_ref = (size_t)B * sizeof(sh_plan_ref);
  z.plan_cut_terms = cuts * AR_PLAN_TERM_BYTES; z.plan_head_terms = cuts * Kh * AR_PLAN_TERM_BYTES; z.plan_stem_terms = cuts * Ks * AR_PLAN_TERM_BYTES;
  z.plan_cut_vals = cuts * 8; z.plan_head_vals = cuts * Kh * 64; z.plan_stem_vals = cuts * Ks * 8;
  z.plan_out = (size_t)B * N * sizeof(sh_plan);
  return {(int)tmax, cuts, z};
}

// ---- what is valid against what -----------------------------------------------------------------------------------------------------
// One member of sh_ctx.  The resident batch is the context's (batch_gen: every upload / commit / store to "verts" takes a new one);
// the queries take it as an argument.  RULE: void first, commit on success -- a *_begin voids what the call is about to overwrite and
// everything fitted against it, the *_end behind the call's synchronisation commits; an early return between the two leaves the
// voided state.  A plan joins the seats and the stems of ONE resection and ONE profile: a resection voids the seats and the stems, a
// profile the stems.
class ArthroState {
 public:
  // events
  void run_submitted(uint32_t mask, unsigned long long batch_gen) { rec_mask_ = mask; rec_gen_ = batch_gen; }
  void resect_begin() { resect_gen_ = NONE; seated_ = false; stems_ = false; }
  void resect_end(ResectLevel level, int P, int K, unsigned long long batch_gen) {
    P_ = P; resect_gen_ = batch_gen;
    if (level == RS_SEAT) { seated_ = true; Kh_ = K; }
  }
  void profile_begin() { canal_gen_ = NONE; stems_ = false; }
  void profile_end(const sh_canal_grid& g, unsigned long long batch_gen) { grid_ = g; canal_gen_ = batch_gen; }
  void stems_begin() { stems_ = false; }      // (before "stem.out" can be resized or half rewritten: an early return leaves no stems for sh_resect_plan)
  void stems_end(int K) { stems_ = true; Ks_ = K; }
  // queries
  bool has_records(unsigned long long batch_gen) const {      // the last submitted run: this batch, with the anatomic neck and the csys
    const uint32_t need = SH_STAGE_ANP | SH_STAGE_CSYS;
    return rec_gen_ == batch_gen && (rec_mask_ & need) == need;
  }
  bool has_anp(unsigned long long batch_gen) const { return rec_gen_ == batch_gen && (rec_mask_ & SH_STAGE_ANP) != 0; }      // the last submitted run: this batch, with the anatomic neck
  bool resected(unsigned long long batch_gen) const { return resect_gen_ == batch_gen && P_ >= 1; }
  bool seated(unsigned long long batch_gen) const { return resected(batch_gen) && seated_; }
  bool profiled(unsigned long long batch_gen) const { return canal_gen_ == batch_gen; }
  bool stems_current(unsigned long long batch_gen) const { return profiled(batch_gen) && stems_; }      // against the last resection and the current profile
  int P() const { return P_; }            // planes per humerus of the last resection ("resect.planes": sh_resect_ring joins one of its cuts again)
  int Kh() const { return Kh_; }          // heads of the last seated resection
  int Ks() const { return Ks_; }          // stems of the last sh_resect_stems
  const sh_canal_grid& grid() const { return grid_; }      // of the last profile ("canal.*": sh_resect_stems reads them)

 private:
  static constexpr unsigned long long NONE = ~0ull;
  uint32_t rec_mask_ = 0;
  unsigned long long rec_gen_ = NONE, resect_gen_ = NONE, canal_gen_ = NONE;
  int P_ = 0, Kh_ = 0, Ks_ = 0;
  bool seated_ = false, stems_ = false;      // the seats are the last resection's; the stems the last resection's and the last profile's
  sh_canal_grid grid_ = {0.0, 0.0, 0, 0};
};

// ---- one ordered precheck per entry point: the first refusal, or SH_OK ------------------------------------------------------------------
struct ArthroFacts {
  bool ctx;                        // the context is there (false: everything below is zero)
  int B, n_pending;
  unsigned long long batch_gen;
  bool landmarks;                  // the "landmarks" buffer exists
  const ArthroState* st;
  bool records() const { return st->has_records(batch_gen) && landmarks; }
};
static const char* const AR_NEEDS_RUN = "needs a run of the resident batch with SH_STAGE_ANP and SH_STAGE_CSYS";

// a batch is resident and nothing of it is in flight: the two refusals that a call which only needs the mesh starts its state checks with
inline ArthroError resident(const ArthroFacts& f) {
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  return arthro_ok();
}

inline ArthroError precheck_resect(const ResectRequest& q, const ArthroFacts& f) {
  if (!f.ctx || (!q.offs && !q.planes) || !q.out || (q.level >= RS_FIT && !q.fit_out) || q.P < 1 || q.P > 4096) return {SH_ERR_ARG, "bad argument (P in 1..4096)"};
  if (q.level == RS_SEAT && !head_catalogue_ok(q.heads, q.K, q.mode, q.seat_out))
    return {SH_ERR_ARG, "bad catalogue (K in 1..64, 0 < thickness < 2 radius) or centre mode"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (q.offs) {
    if (!f.records()) return {SH_ERR_STATE, AR_NEEDS_RUN};
    if (!cut_offsets_ok(q.offs, q.P)) return {SH_ERR_ARG, "non-finite offset"};
  } else if (first_bad_plane(q.planes, (size_t)f.B * q.P) >= 0) {
    return {SH_ERR_ARG, "zero normal or non-finite plane"};
  }
  return arthro_ok();
}

inline ArthroError precheck_ring(int b, int p, const double* out, int cap, const int* n_out, const ArthroFacts& f) {
  if (!f.ctx || !n_out || cap < 0 || (cap > 0 && !out)) return {SH_ERR_ARG, "bad argument"};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  if (!f.st->resected(f.batch_gen)) return {SH_ERR_STATE, AR_NO_RESECTION};
  if (b < 0 || b >= f.B || p < 0 || p >= f.st->P()) return {SH_ERR_ARG, "index out of range"};
  return arthro_ok();
}

inline ArthroError precheck_profile(const sh_canal_grid* g, const double* frames, const ArthroFacts& f) {
  if (!f.ctx || !canal_grid_ok(g)) return {SH_ERR_ARG, "bad grid (finite z0, dz > 0, L in 1..1024, A in 3..256)"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (frames) {
    const int b = first_bad_frame(frames, f.B);
    if (b >= 0) return {SH_ERR_ARG, "frame " + std::to_string(b) + " is not a rigid CT -> frame matrix"};
  } else if (!f.records()) {
    return {SH_ERR_STATE, std::string("frames == NULL ") + AR_NEEDS_RUN};
  }
  return arthro_ok();
}

inline ArthroError precheck_stems(const sh_stem* stems, int K, const sh_stem_fit* out, const ArthroFacts& f) {
  if (!f.ctx || !stems || !out || K < 1 || K > SH_STEM_MAX) return {SH_ERR_ARG, "bad argument (K in 1..64)"};
  if (!stem_catalogue_ok(stems, K)) return {SH_ERR_ARG, "length, r_prox and r_tip of a stem must be finite and > 0"};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  if (f.B < 1 || !f.st->resected(f.batch_gen)) return {SH_ERR_STATE, AR_NO_RESECTION};
  if (!f.st->profiled(f.batch_gen)) return {SH_ERR_STATE, "no canal profile of the resident batch"};
  return arthro_ok();
}

// (the arguments that need no context come first here: a null context with a bad rule reports the rule)
inline ArthroError precheck_plan(const sh_plan_rule* rule, const double* ref_planes, int N, const sh_plan* out, const ArthroFacts& f) {
  if (!rule || !out || N < 1 || N > SH_PLAN_MAX) return {SH_ERR_ARG, "bad argument (N in 1..64)"};
  if (!plan_rule_ok(rule)) return {SH_ERR_ARG, "bad rule (no NaN, weights finite and >= 0, margin >= 0)"};
  if (!f.ctx) return {SH_ERR_ARG, std::string()};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  if (f.B < 1 || !f.st->seated(f.batch_gen))
    return {SH_ERR_STATE, "no seated resection of the resident batch (sh_resect_planes_seat / sh_resect_offsets_seat)"};
  if (!f.st->stems_current(f.batch_gen))
    return {SH_ERR_STATE, "no stems fitted against the last resection and the current canal profile (sh_resect_stems)"};
  if (!ref_planes && !f.records()) return {SH_ERR_STATE, std::string("ref_planes == NULL ") + AR_NEEDS_RUN};
  if (ref_planes) {
    const long long b = first_bad_plane(ref_planes, (size_t)f.B);
    if (b >= 0) return {SH_ERR_ARG, "reference plane " + std::to_string(b) + " has a zero normal or is not finite"};
  }
  return arthro_ok();
}

}  // namespace sh

// The host decisions come as one: a unit or a host test that includes this header has the queries' as well, as it had when they were
// written here (the include guard makes the order of the two headers free).
#include "sh_query.h"
