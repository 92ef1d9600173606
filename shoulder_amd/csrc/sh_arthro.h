// sh_arthro.h -- what the arthroplasty chain (batched resection -> head fit -> seats -> canal profile -> stems -> ranked plans) decides
// on the host: are the arguments acceptable, which refusal comes first, how a sweep is split into passes and how large every named
// buffer is, and what is valid against what (ArthroState).  No kernels, no HIP types: sh_ctx.h includes it, and so does a plain g++
// (tests/hostcheck/arthro_check.cpp).  An error is a code plus the text BEHIND the entry point's name: the caller puts
// "sh_resect_planes: " (or the name it was called under) in front.  The entry points themselves are sh_arthro_host.h.
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
// functions below), allocation and the typed view of a call (sh_arthro_host.h: arthro_ensure, ArthroView) all come from these lists.
// The element types of kernel headers (ResectPart, PlanTop, PlanTerm) are only named here: this header expands no type.
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
// the rays against the resident batch (sh_ray_cast / sh_anp_axis_hits) are not a link of the chain: buffers, sizes and view of their own
#define RAY_BUFS(X)                                                                                                                \
  X(ray_rays, "ray.rays", double, 8) X(ray_status, "ray.status", int, 4) X(ray_counts, "ray.counts", int, 4)                       \
  X(ray_offs, "ray.offs", unsigned long long, 8) X(ray_cursor, "ray.cursor", int, 4) X(ray_pool, "ray.pool", RayKey, 8)            \
  X(ray_hits, "ray.hits", sh_ray_hit, 8) X(ray_blockhit, "ray.blockhit", int, 4)
// the closest surface points (sh_closest_points) are no link of the chain either
#define CP_BUFS(X) X(cp_points, "cp.points", double, 8) X(cp_part, "cp.part", CpPart, 8) X(cp_out, "cp.out", sh_closest, 8)
// nor are the generalized winding numbers (sh_winding_numbers)
#define WN_BUFS(X) X(wn_points, "wn.points", double, 8) X(wn_part, "wn.part", double, 8) X(wn_out, "wn.out", sh_winding, 8)
// nor is the registration of point sets (sh_register_points): the walk runs on buffers of its own ("icp.cp_part", "icp.near")
#define ICP_BUFS(X)                                                                                                                \
  X(icp_points, "icp.points", double, 8) X(icp_moved, "icp.moved", double, 8) X(icp_cp_part, "icp.cp_part", CpPart, 8)             \
  X(icp_near, "icp.near", sh_closest, 8) X(icp_part, "icp.part", double, 8) X(icp_T, "icp.T", double, 8)                           \
  X(icp_hist, "icp.hist", double, 8) X(icp_flags, "icp.flags", int, 4) X(icp_out, "icp.out", sh_registration, 8)
// the mass properties (sh_mass_properties): the block rows and the records
#define MASS_BUFS(X) X(mass_part, "mass.part", double, 8) X(mass_out, "mass.out", sh_mass, 8)
// the multi-start registration (sh_register_multistart) runs the chain of sh_register_points on the "icp.*" buffers; these are its own
#define MS_BUFS(X)                                                                                                                 \
  X(ms_T0s, "ms.T0s", double, 8) X(ms_points, "ms.points", double, 8) X(ms_coarse, "ms.coarse", sh_registration, 8)                \
  X(ms_best, "ms.best", double, 8) X(ms_winner, "ms.winner", int, 4)
// what the chain reads and does not own (the mesh: upload / commit; the records of a run: alloc_batch): X(field, "name", type)
#define ARTHRO_INPUT_BUFS(X)                                                                                                       \
  X(verts, "verts", const float) X(faces, "faces", const int) X(voff, "voff", const long long) X(foff, "foff", const long long)    \
  X(lm, "landmarks", const sh_landmarks) /* null in the view without a run of the resident batch with the anatomic neck and the csys */

// bytes of every buffer a call ensures; 0: not this call's (every size of a call is > 0: B, P, K, L, A, N >= 1)
#define X(f, name, T, elem) size_t f = 0;
struct ArthroBytes { ARTHRO_BUFS(X) };
struct RayBytes { RAY_BUFS(X) };
struct CpBytes { CP_BUFS(X) };
struct WnBytes { WN_BUFS(X) };
struct IcpBytes { ICP_BUFS(X) };
struct MassBytes { MASS_BUFS(X) };
struct MsBytes { MS_BUFS(X) };
#undef X

// what the kernel headers fix, restated (shoulder_hip.hip holds each against its header with a static_assert)
constexpr int AR_RS_TILE = 256, AR_HF_WORDS = 16, AR_RESECT_PART_BYTES = 32;      // SH_RS_TILE, SH_HF_WORDS, sizeof(ResectPart)
constexpr int AR_CANAL_TILE = 256, AR_PLAN_TILE = 256;                            // SH_CANAL_TILE, SH_PLAN_TILE
constexpr int AR_PLAN_TOP_BYTES = 16, AR_PLAN_TERM_BYTES = 16;                    // sizeof(PlanTop), sizeof(PlanTerm)
constexpr int AR_RAY_TILE = 256, AR_RAY_CHUNK = 256, AR_RAY_KEY_BYTES = 16;       // SH_RAY_TILE, SH_RAY_CHUNK, sizeof(RayKey)
constexpr int AR_CP_TILE = 256, AR_CP_CHUNK = 256, AR_CP_PART_BYTES = 16;         // SH_CP_TILE, SH_CP_CHUNK, sizeof(CpPart)
constexpr int AR_CP_FILL = 1024;      // workgroups of k_cp_walk that fill the chip: four of 256 lanes on each of 256 compute units
constexpr int AR_WN_TILE = 256, AR_WN_CHUNK = 256, AR_WN_BLOCK = 2048;            // SH_WN_TILE, SH_WN_CHUNK, SH_WIND_BLOCK
constexpr int AR_WN_FILL = 1024;      // workgroups of k_wn_walk that fill the chip, as AR_CP_FILL
constexpr int AR_ICP_TERMS = 32, AR_ICP_TSTRIDE = 20;                             // SH_ICP_TERMS, SH_ICP_TSTRIDE
constexpr int AR_MASS_TERMS = 24;                                                 // SH_MASS_TERMS

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

// a rigid CT -> CT start of a registration: finite, last row exactly 0 0 0 1, |R^T R - I| <= 1e-9 in every entry (the columns: a shear
// of 1e-6 fails), determinant positive (a reflection fails)
inline bool rigid_start_ok(const double* T) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T[i])) return false;
  if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double d = (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j];
      if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-9)) return false;
    }
  return det3_of4(T) > 0.0;
}
inline bool icp_options_ok(const sh_icp_options* o) {
  return (o->metric == SH_ICP_POINT || o->metric == SH_ICP_PLANE) && o->max_iter >= 1 && o->max_iter <= SH_ICP_MAX_ITER && o->reject > 0.0 &&
         o->tol >= 0.0 && std::isfinite(o->tol);
}

inline bool stem_catalogue_ok(const sh_stem* stems, int K) { return all_doubles(stems, K, [](double x) { return std::isfinite(x) && x > 0.0; }); }

// n rays: the index of the first one that is not six finite doubles with a non-zero direction, or -1
inline long long first_bad_ray(const sh_ray* rays, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const sh_ray& r = rays[i];
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(r.origin[k]) && std::isfinite(r.dir[k]);
    if (!fin || (r.dir[0] == 0.0 && r.dir[1] == 0.0 && r.dir[2] == 0.0)) return (long long)i;
  }
  return -1;
}

// n points: the index of the first one with a coordinate that is not finite, or -1
inline long long first_bad_point(const double* pts, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(pts[3 * i]) || !std::isfinite(pts[3 * i + 1]) || !std::isfinite(pts[3 * i + 2])) return (long long)i;
  return -1;
}

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

// a cast of R rays per humerus with room for cap hits each: everything but the pool, which the counts size ("ray.pool", ray_pool_bytes)
struct RayPlan { int tmax, chunks; size_t rays; RayBytes bytes; };      // face tiles per humerus, ray chunks, B x R
inline RayPlan ray_plan(int B, int R, bool per_humerus, int cap, long long maxF, bool with_status) {
  const size_t n = (size_t)B * R;
  RayBytes z;
  z.ray_rays = (per_humerus ? n : (size_t)R) * sizeof(sh_ray); z.ray_counts = n * 4; z.ray_offs = (n + 1) * 8; z.ray_cursor = n * 4;
  z.ray_hits = n * cap * sizeof(sh_ray_hit);
  if (with_status) z.ray_status = (size_t)B * 4;
  const long long tmax = tiles_of(maxF, AR_RAY_TILE);
  const int chunks = (R + AR_RAY_CHUNK - 1) / AR_RAY_CHUNK;
  z.ray_blockhit = (size_t)tmax * B * chunks * 4;      // one word per workgroup of the walk
  return {(int)tmax, chunks, n, z};
}
inline size_t ray_pool_bytes(unsigned long long total) { return (size_t)(total > 0 ? total : 1) * AR_RAY_KEY_BYTES; }

// Closest points, Q per humerus.  The grid of k_cp_walk is (chunks of 256 points, B, S face splits): split s of a humerus with T tiles
// walks the tiles cp_split_range(T, S, s) (sh_scalar.h).  S is the host's choice and no knob: as many splits as bring the grid to
// AR_CP_FILL workgroups when B x chunks is small, never more than the tiles of the largest humerus, at least one.  A minimum under a
// total order does not depend on how its candidates are grouped, so S changes no result.
inline int cp_splits(long long groups /* B x chunks */, long long tiles /* of the largest humerus */) {
  const long long g = groups > 1 ? groups : 1, want = (AR_CP_FILL + g - 1) / g;
  const long long s = want < tiles ? want : tiles;
  return (int)(s > 1 ? s : 1);
}
struct CpPlan { int tmax, chunks, S; size_t points; CpBytes bytes; };      // face tiles of the largest humerus, point chunks, face splits, B x Q
inline CpPlan cp_plan(int B, int Q, bool per_humerus, long long maxF) {
  const size_t n = (size_t)B * Q;
  const long long tmax = tiles_of(maxF, AR_CP_TILE);
  const int chunks = (Q + AR_CP_CHUNK - 1) / AR_CP_CHUNK;
  const int S = cp_splits((long long)B * chunks, tmax);
  CpBytes z;
  z.cp_points = (per_humerus ? n : (size_t)Q) * 24; z.cp_part = n * S * AR_CP_PART_BYTES; z.cp_out = n * sizeof(sh_closest);
  return {(int)tmax, chunks, S, n, z};
}

// Winding numbers, Q per humerus.  The grid of k_wn_walk is (chunks of 256 points, B, S splits): split s of a humerus with K blocks of
// AR_WN_BLOCK faces walks the blocks cp_split_range(K, S, s) (sh_scalar.h) -- whole blocks, a split never cuts one, because the block
// sums are the fixed inner level of the summation tree.  S is the host's choice and no knob: as many splits as bring the grid to
// AR_WN_FILL workgroups when B x chunks is small, never more than the blocks of the largest humerus, at least one.  With S == 1 a
// workgroup owns all blocks of its humerus and adds the block sums itself, in block order ("wn.part" holds one total per point);
// with S > 1 "wn.part" holds the block sums (kmax per point) and k_wn_join adds them in the same order.  S changes no byte.
inline int wn_splits(long long groups /* B x chunks */, long long blocks /* of the largest humerus */) {
  const long long g = groups > 1 ? groups : 1, want = (AR_WN_FILL + g - 1) / g;
  const long long s = want < blocks ? want : blocks;
  return (int)(s > 1 ? s : 1);
}
struct WnPlan { int kmax, chunks, S, stride; size_t points; WnBytes bytes; };      // blocks of the largest humerus, point chunks, splits, doubles of "wn.part" per point, B x Q
inline WnPlan wn_plan(int B, int Q, bool per_humerus, long long maxF) {
  const size_t n = (size_t)B * Q;
  const long long kmax = tiles_of(maxF, AR_WN_BLOCK);
  const int chunks = (Q + AR_WN_CHUNK - 1) / AR_WN_CHUNK;
  const int S = wn_splits((long long)B * chunks, kmax);
  const int stride = S == 1 ? 1 : (int)kmax;
  WnBytes z;
  z.wn_points = (per_humerus ? n : (size_t)Q) * 24; z.wn_part = n * stride * sizeof(double); z.wn_out = n * sizeof(sh_winding);
  return {(int)kmax, chunks, S, stride, n, z};
}

// Registration, Q points per humerus.  The walk of an evaluation is the closest-point walk on the moved points, always per humerus:
// its chunks and its split S are cp_plan's, unchanged.  The sums take the points in blocks of SH_ICP_BLOCK = the walk's chunk, one
// row of AR_ICP_TERMS doubles per (humerus, block) in "icp.part"; "icp.T" holds the transform and the mean of the input points.
struct IcpPlan { int chunks, S; size_t points; IcpBytes bytes; };      // point chunks = blocks of the sums, face splits of the walk, B x Q
inline IcpPlan icp_plan(int B, int Q, bool per_humerus, long long maxF, int max_iter) {
  const CpPlan cp = cp_plan(B, Q, true, maxF);
  IcpBytes z;
  z.icp_points = (per_humerus ? cp.points : (size_t)Q) * 24; z.icp_moved = cp.points * 24; z.icp_cp_part = cp.bytes.cp_part; z.icp_near = cp.bytes.cp_out;
  z.icp_part = (size_t)B * cp.chunks * AR_ICP_TERMS * 8; z.icp_T = (size_t)B * AR_ICP_TSTRIDE * 8; z.icp_hist = (size_t)B * (max_iter + 1) * 16;
  z.icp_flags = (size_t)B * 4; z.icp_out = (size_t)B * sizeof(sh_registration);
  return {cp.chunks, cp.S, cp.points, z};
}

// Mass properties: one row of AR_MASS_TERMS doubles per (humerus, block of SH_MASS_BLOCK faces) in "mass.part", the blocks of the largest
// humerus for every humerus
struct MassPlan { int blocks; MassBytes bytes; };
inline MassPlan mass_plan(int B, long long maxF) {
  const long long blocks = tiles_of(maxF, SH_MASS_BLOCK);
  MassBytes z;
  z.mass_part = (size_t)B * blocks * AR_MASS_TERMS * 8; z.mass_out = (size_t)B * sizeof(sh_mass);
  return {(int)blocks, z};
}

// Multi-start registration: the coarse stage is sh_register_points on Qc points, the fine stage on all Q, both on the "icp.*" buffers,
// which take the larger of the two sizes field by field (the split of the walk, and so "icp.cp_part", may be larger for the fewer points).
inline int ms_coarse_count(int Q, int coarse_points) { return coarse_points == 0 || coarse_points > Q ? Q : coarse_points; }
inline long long ms_coarse_index(long long j, int Q, int Qc) { return j * Q / Qc; }      // point j of the coarse set
struct MsPlan { int Qc; IcpPlan coarse, fine; IcpBytes icp; MsBytes bytes; };
inline MsPlan ms_plan(int B, int Q, bool per_humerus, long long maxF, int K, int coarse_points, int coarse_iter, int fine_iter) {
  const int Qc = ms_coarse_count(Q, coarse_points);
  MsPlan p{Qc, icp_plan(B, Qc, per_humerus, maxF, coarse_iter), icp_plan(B, Q, per_humerus, maxF, fine_iter), IcpBytes(), MsBytes()};
#define X(f, name, T, elem) p.icp.f = std::max(p.coarse.bytes.f, p.fine.bytes.f);
  ICP_BUFS(X)
#undef X
  p.bytes.ms_T0s = (size_t)B * K * 128; p.bytes.ms_points = (per_humerus ? (size_t)B * Qc : (size_t)Qc) * 24;
  p.bytes.ms_coarse = (size_t)B * K * sizeof(sh_registration); p.bytes.ms_best = (size_t)B * 8; p.bytes.ms_winner = (size_t)B * 4;
  return p;
}

// The pick rule: does candidate k (its status, pairs and rms) replace the best so far (winner < 0: none yet)?  The candidates come in
// ascending k, so "strictly smaller rms" is the order (rms, k).  A candidate with a status, too few pairs or a NaN rms never wins.
SH_HD bool ms_candidate_wins(int status, int pairs, double rms, int min_pairs, int winner, double best_rms) {
  if (status != 0 || pairs < min_pairs || !(rms == rms)) return false;
  return winner < 0 || rms < best_rms;
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

inline ArthroError precheck_resect(const ResectRequest& q, const ArthroFacts& f) {
  if (!f.ctx || (!q.offs && !q.planes) || !q.out || (q.level >= RS_FIT && !q.fit_out) || q.P < 1 || q.P > 4096) return {SH_ERR_ARG, "bad argument (P in 1..4096)"};
  if (q.level == RS_SEAT && !head_catalogue_ok(q.heads, q.K, q.mode, q.seat_out))
    return {SH_ERR_ARG, "bad catalogue (K in 1..64, 0 < thickness < 2 radius) or centre mode"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
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
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
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

inline ArthroError precheck_ray_cast(const sh_ray* rays, int R, int per_humerus, int cap, const ArthroFacts& f) {
  if (!f.ctx || !rays || R < 1 || R > SH_RAY_MAX || cap < 1 || cap > SH_RAY_MAX_HITS) return {SH_ERR_ARG, "bad argument (R in 1..65536, cap in 1..1024)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  const long long i = first_bad_ray(rays, per_humerus ? (size_t)f.B * R : (size_t)R);
  if (i >= 0) return {SH_ERR_ARG, "ray " + std::to_string(i) + " has a non-finite number or a zero direction"};
  return arthro_ok();
}

inline ArthroError precheck_closest(const double* points, int Q, int per_humerus, const ArthroFacts& f) {
  if (!f.ctx || !points || Q < 1 || Q > SH_CLOSEST_MAX) return {SH_ERR_ARG, "bad argument (Q in 1..1048576)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  const long long i = first_bad_point(points, per_humerus ? (size_t)f.B * Q : (size_t)Q);
  if (i >= 0) return {SH_ERR_ARG, "point " + std::to_string(i) + " has a coordinate that is not finite"};
  return arthro_ok();
}

inline ArthroError precheck_winding(const double* points, int Q, int per_humerus, const ArthroFacts& f) {
  if (!f.ctx || !points || Q < 1 || Q > SH_WINDING_MAX) return {SH_ERR_ARG, "bad argument (Q in 1..1048576)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  const long long i = first_bad_point(points, per_humerus ? (size_t)f.B * Q : (size_t)Q);
  if (i >= 0) return {SH_ERR_ARG, "point " + std::to_string(i) + " has a coordinate that is not finite"};
  return arthro_ok();
}

inline ArthroError precheck_register(const double* points, int Q, int per_humerus, const double* T0, const sh_icp_options* opt, const ArthroFacts& f) {
  if (!f.ctx || !points || !opt) return {SH_ERR_ARG, "bad argument (context, points and options must be given)"};
  if (Q < 1 || Q > SH_CLOSEST_MAX) return {SH_ERR_ARG, "bad argument (Q in 1..1048576)"};
  if (!icp_options_ok(opt)) return {SH_ERR_ARG, "bad options (metric 0 or 1, max_iter in 1..64, reject > 0, tol >= 0 and finite)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  const long long i = first_bad_point(points, per_humerus ? (size_t)f.B * Q : (size_t)Q);
  if (i >= 0) return {SH_ERR_ARG, "point " + std::to_string(i) + " has a coordinate that is not finite"};
  if (T0)
    for (int b = 0; b < f.B; ++b)
      if (!rigid_start_ok(T0 + 16 * (size_t)b)) return {SH_ERR_ARG, "T0 of humerus " + std::to_string(b) + " is not a rigid matrix (last row 0 0 0 1, |R^T R - I| <= 1e-9, det > 0)"};
  return arthro_ok();
}

inline ArthroError precheck_mass(const ArthroFacts& f) {
  if (!f.ctx) return {SH_ERR_ARG, "bad argument (no context)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  return arthro_ok();
}

inline ArthroError precheck_multistart(const double* points, int Q, int per_humerus, const double* T0s, int K, const sh_icp_options* coarse,
                                       int coarse_points, int min_pairs, const sh_icp_options* fine, const ArthroFacts& f) {
  if (!f.ctx || !points || !T0s || !coarse || !fine) return {SH_ERR_ARG, "bad argument (context, points, T0s and both options must be given)"};
  if (Q < 1 || Q > SH_CLOSEST_MAX) return {SH_ERR_ARG, "bad argument (Q in 1..1048576)"};
  if (K < 1 || K > SH_MS_MAX_STARTS || coarse_points < 0 || min_pairs < 6) return {SH_ERR_ARG, "bad argument (K in 1..64, coarse_points >= 0, min_pairs >= 6)"};
  if (!icp_options_ok(coarse)) return {SH_ERR_ARG, "bad coarse options (metric 0 or 1, max_iter in 1..64, reject > 0, tol >= 0 and finite)"};
  if (!icp_options_ok(fine)) return {SH_ERR_ARG, "bad fine options (metric 0 or 1, max_iter in 1..64, reject > 0, tol >= 0 and finite)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  const long long i = first_bad_point(points, per_humerus ? (size_t)f.B * Q : (size_t)Q);
  if (i >= 0) return {SH_ERR_ARG, "point " + std::to_string(i) + " has a coordinate that is not finite"};
  for (int b = 0; b < f.B; ++b)
    for (int k = 0; k < K; ++k)
      if (!rigid_start_ok(T0s + 16 * ((size_t)b * K + k)))
        return {SH_ERR_ARG, "start " + std::to_string(k) + " of humerus " + std::to_string(b) + " is not a rigid matrix (last row 0 0 0 1, |R^T R - I| <= 1e-9, det > 0)"};
  return arthro_ok();
}

inline ArthroError precheck_anp_hits(int cap, const int32_t* status, const ArthroFacts& f) {
  if (!f.ctx || !status || cap < 1 || cap > SH_RAY_MAX_HITS) return {SH_ERR_ARG, "bad argument (cap in 1..1024)"};
  if (f.B < 1) return {SH_ERR_STATE, AR_NO_MESHES};
  if (f.n_pending != 0) return {SH_ERR_STATE, AR_IN_FLIGHT};
  if (!f.st->has_anp(f.batch_gen) || !f.landmarks) return {SH_ERR_STATE, "needs a collected run of the resident batch with SH_STAGE_ANP"};
  return arthro_ok();
}

}  // namespace sh
