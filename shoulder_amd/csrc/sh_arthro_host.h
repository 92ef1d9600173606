// sh_arthro_host.h -- the entry points of the arthroplasty chain: sh_resect_* (k_resect.h, k_headfit.h, k_seat.h), sh_canal_profile and
// sh_resect_stems (k_stem.h), sh_resect_plan (k_plan.h), the rays against the resident batch, sh_ray_cast / sh_anp_axis_hits (k_rays.h),
// its closest surface points, sh_closest_points (k_closest.h), its winding numbers, sh_winding_numbers (k_winding.h), the registration of point sets onto it, sh_register_points (k_icp.h) and sh_register_multistart (k_ms.h), and its mass
// properties, sh_mass_properties (k_mass.h).  Host code of shoulder_hip.hip, included there EXACTLY ONCE, behind the kernel
// headers and inside its extern "C" block.  A header and not a unit of its own: compiled in a unit that holds only the resection
// headers, the unchanged k_resect_faces takes 100 VGPRs instead of 92, four waves per SIMD instead of five, so the kernels
// stay in shoulder_hip.hip and the code that launches them with them.
// What the chain DECIDES is sh_arthro.h (checks, first refusal, pass plan, buffer sizes, ArthroState).  Every entry point here reads:
// precheck -> ensure -> view -> state begin -> enqueue -> copies back -> synchronise -> state end.
#pragma once

static_assert(AR_RS_TILE == SH_RS_TILE && AR_HF_WORDS == SH_HF_WORDS && AR_RESECT_PART_BYTES == sizeof(ResectPart), "sh_arthro.h: resection tile, moment words, slab entry");
static_assert(AR_CANAL_TILE == SH_CANAL_TILE && AR_PLAN_TILE == SH_PLAN_TILE && AR_PLAN_TOP_BYTES == sizeof(PlanTop) && AR_PLAN_TERM_BYTES == sizeof(PlanTerm),
              "sh_arthro.h: canal and plan tiles, PlanTop, PlanTerm");
static_assert(AR_RAY_TILE == SH_RAY_TILE && AR_RAY_CHUNK == SH_RAY_CHUNK && AR_RAY_KEY_BYTES == sizeof(RayKey), "sh_arthro.h: ray tile, ray chunk, RayKey");
static_assert(AR_CP_TILE == SH_CP_TILE && AR_CP_CHUNK == SH_CP_CHUNK && AR_CP_PART_BYTES == sizeof(CpPart), "sh_arthro.h: closest-point tile, chunk, CpPart");
static_assert(AR_WN_TILE == SH_WN_TILE && AR_WN_CHUNK == SH_WN_CHUNK && AR_WN_BLOCK == SH_WIND_BLOCK, "sh_arthro.h: winding tile, chunk, block");

// The named buffers of a call as typed pointers (ARTHRO_BUFS, ARTHRO_INPUT_BUFS), resolved once per call BEHIND the call's
// arthro_ensure (which may re-allocate them); a buffer that is not there is null.  No window offset: the chain works on the whole batch.
#define X(f, name, T, ...) T* f = nullptr;
struct ArthroView { ARTHRO_INPUT_BUFS(X) ARTHRO_BUFS(X) };
#undef X

static ArthroFacts arthro_facts(const sh_ctx* c) {
  if (!c) return ArthroFacts{false, 0, 0, 0, false, nullptr};
  return ArthroFacts{true, c->B, c->n_pending, c->batch_gen, c->bufs.find("landmarks") != c->bufs.end(), &c->arthro};
}

static int arthro_refuse(sh_ctx* c, const char* fn, const ArthroError& e) { return fail(c, e.code, std::string(fn) + ": " + e.text); }

// `groups`: which of the chain's own buffers the call touches (the inputs always); the others stay null and cost no lookup
enum : unsigned { AV_RESECT = 1, AV_CANAL = 2, AV_STEM = 4, AV_PLAN = 8 };
static ArthroView arthro_view(sh_ctx* c, unsigned groups) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  ArthroView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  ARTHRO_INPUT_BUFS(X)
  if (groups & AV_RESECT) { ARTHRO_RESECT_BUFS(X) }
  if (groups & AV_CANAL) { ARTHRO_CANAL_BUFS(X) }
  if (groups & AV_STEM) { ARTHRO_STEM_BUFS(X) }
  if (groups & AV_PLAN) { ARTHRO_PLAN_BUFS(X) }
#undef X
  if (!c->arthro.has_records(c->batch_gen)) v.lm = nullptr;
  return v;
}

// the buffers of a call at the sizes of its plan (0: not this call's), shared / scratch stride
static int arthro_ensure(sh_ctx* c, const ArthroBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  ARTHRO_BUFS(X)
#undef X
  return SH_OK;
}

struct ResectPass { int P, p0, pc, b0, nb, tmax; };      // planes [p0, p0 + pc) of humeri [b0, b0 + nb), tmax tiles per humerus in the slabs

// the join of a pass at a level; one / ring: the one-cut outputs of the records level (sh_resect_ring)
static int launch_join(sh_ctx* c, const ArthroView& v, ResectLevel level, const ResectPass& s, sh_resection* one = nullptr, double* ring = nullptr) {
  const dim3 grid((unsigned)(s.nb * s.pc)), block(SH_RS_JOIN_THREADS);
#define RJ_ARGS v.verts, v.faces, v.voff, v.foff, (const double*)v.planes, s.P, s.p0, s.pc, s.b0, s.tmax, (const int*)v.status, (const ResectPart*)v.slab, \
                (const int*)v.segcnt, (const int*)v.segs, v.out
  if (level == RS_SEAT) LAUNCH(c, "k_resect_join_seat", k_resect_join_seat, grid, block, RJ_ARGS, (const double*)v.fit_slab, v.fit_moments, v.fit_ring, v.seat_ring);
  else if (level == RS_FIT) LAUNCH(c, "k_resect_join_fit", k_resect_join_fit, grid, block, RJ_ARGS, (const double*)v.fit_slab, v.fit_moments, v.fit_ring);
  else LAUNCH(c, "k_resect_join", k_resect_join, grid, block, RJ_ARGS, one, ring);
#undef RJ_ARGS
  return SH_OK;
}

// the fits of planes [p0, p0 + pn) of every humerus from their moments, ring sums and records
static int launch_solve(sh_ctx* c, const ArthroView& v, int P, int p0, int pn) {
  const int n = c->B * pn;
  LAUNCH(c, "k_headfit_solve", k_headfit_solve, dim3((unsigned)((n + 63) / 64)), dim3(64), (const sh_resection*)v.out, (const int*)v.status,
         (const double*)v.fit_moments, (const double*)v.fit_ring, v.lm, P, p0, pn, n, v.fit_out);
  return SH_OK;
}

// face pass(es) and join of one pass
static int resect_pass(sh_ctx* c, const ArthroView& v, ResectLevel level, const ResectPass& s, sh_resection* one = nullptr, double* ring = nullptr) {
  HIPCHK(c, hipMemsetAsync(v.segcnt, 0, (size_t)s.nb * s.pc * 4, c->stream));
  const dim3 grid((unsigned)s.tmax, (unsigned)s.nb), block(SH_RS_TILE);
  LAUNCH(c, "k_resect_faces", k_resect_faces, grid, block, v.verts, v.faces, v.voff, v.foff, (const double*)v.planes, s.P, s.p0, s.pc, s.b0, s.tmax, v.slab,
         v.segcnt, v.segs);
  if (level >= RS_FIT)
    LAUNCH(c, "k_headfit_faces", k_headfit_faces, grid, block, v.verts, v.faces, v.voff, v.foff, (const double*)v.planes, s.P, s.p0, s.pc, s.b0, s.tmax,
           v.fit_slab);
  return launch_join(c, v, level, s, one, ring);
}

// ---- batched head resection: the six sh_resect_* entry points and the one pipeline behind them --------------------------------------
static int resect_run(sh_ctx* c, const ResectRequest& q) {
  if (const ArthroError e = precheck_resect(q, arthro_facts(c)); e.code) return arthro_refuse(c, q.fn, e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, P = q.P;
  const size_t n = (size_t)B * P;
  const ResectPlan plan = resect_plan(B, P, c->maxF, q.level, q.K, q.offs != nullptr);
  if (int rc = arthro_ensure(c, plan.bytes)) return rc;
  const ArthroView v = arthro_view(c, AV_RESECT);
  c->arthro.resect_begin();
  if (q.offs) {
    HIPCHK(c, hipMemcpyAsync(v.offs, q.offs, (size_t)P * 56, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_resect_make_planes", k_resect_make_planes, dim3((unsigned)B), dim3(64), v.lm, (const double*)v.offs, P, v.planes, v.status);
  } else {
    HIPCHK(c, hipMemcpyAsync(v.planes, q.planes, n * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(v.status, 0, n * 4, c->stream));
  }
  if (q.level >= RS_FIT) {      // (a cut whose humerus' record failed writes neither: zeros)
    HIPCHK(c, hipMemsetAsync(v.fit_moments, 0, n * 16 * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(v.fit_ring, 0, n * 8 * 8, c->stream));
  }
  if (q.level == RS_SEAT) HIPCHK(c, hipMemcpyAsync(v.seat_heads, q.heads, (size_t)q.K * sizeof(sh_implant_head), hipMemcpyHostToDevice, c->stream));
  for (int p0 = 0; p0 < P; p0 += plan.pc) {
    const int pn = std::min(plan.pc, P - p0);
    if (int rc = resect_pass(c, v, q.level, ResectPass{P, p0, pn, 0, B, plan.tmax})) return rc;
    if (q.level == RS_SEAT) {      // the ring coordinates are the pass': its fits and its seats before the next pass overwrites them
      if (int rc = launch_solve(c, v, P, p0, pn)) return rc;
      LAUNCH(c, "k_seat", k_seat, dim3((unsigned)(B * pn)), dim3(SH_SEAT_THREADS), (const sh_resection*)v.out, (const sh_head_fit*)v.fit_out,
             (const int*)v.status, (const double*)v.fit_moments, (const double*)v.seat_ring, v.lm, (const sh_implant_head*)v.seat_heads, q.K, q.mode, P, p0, pn,
             v.seat_out);
    }
  }
  HIPCHK(c, hipMemcpyAsync(q.out, v.out, n * sizeof(sh_resection), hipMemcpyDeviceToHost, c->stream));
  if (q.level >= RS_FIT) {
    if (int rc = q.level == RS_FIT ? launch_solve(c, v, P, 0, P) : SH_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(q.fit_out, v.fit_out, n * sizeof(sh_head_fit), hipMemcpyDeviceToHost, c->stream));
  }
  if (q.level == RS_SEAT) HIPCHK(c, hipMemcpyAsync(q.seat_out, v.seat_out, n * q.K * sizeof(sh_seat), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->arthro.resect_end(q.level, P, q.K, c->batch_gen);
  return SH_OK;
}

int sh_resect_planes(sh_ctx* c, const double* planes, int P, sh_resection* out) { return resect_run(c, ResectRequest{"sh_resect_planes", RS_RECORDS, planes, nullptr, P, out}); }
int sh_resect_offsets(sh_ctx* c, const sh_cut_offset* offs, int P, sh_resection* out) { return resect_run(c, ResectRequest{"sh_resect_offsets", RS_RECORDS, nullptr, offs, P, out}); }
int sh_resect_planes_fit(sh_ctx* c, const double* planes, int P, sh_resection* out, sh_head_fit* fit_out) {
  return resect_run(c, ResectRequest{"sh_resect_planes_fit", RS_FIT, planes, nullptr, P, out, fit_out});
}
int sh_resect_offsets_fit(sh_ctx* c, const sh_cut_offset* offs, int P, sh_resection* out, sh_head_fit* fit_out) {
  return resect_run(c, ResectRequest{"sh_resect_offsets_fit", RS_FIT, nullptr, offs, P, out, fit_out});
}
int sh_resect_planes_seat(sh_ctx* c, const double* planes, int P, const sh_implant_head* heads, int K, int center_mode, sh_resection* out,
                          sh_head_fit* fit_out, sh_seat* seat_out) {
  return resect_run(c, ResectRequest{"sh_resect_planes_seat", RS_SEAT, planes, nullptr, P, out, fit_out, heads, K, center_mode, seat_out});
}
int sh_resect_offsets_seat(sh_ctx* c, const sh_cut_offset* offs, int P, const sh_implant_head* heads, int K, int center_mode, sh_resection* out,
                           sh_head_fit* fit_out, sh_seat* seat_out) {
  return resect_run(c, ResectRequest{"sh_resect_offsets_seat", RS_SEAT, nullptr, offs, P, out, fit_out, heads, K, center_mode, seat_out});
}

// one cut of the last resection joined again for its ring (nothing is ensured: "resect.*" are that resection's; no state changes)
int sh_resect_ring(sh_ctx* c, int b, int p, double* out, int cap, int* n_out) {
  if (const ArthroError e = precheck_ring(b, p, out, cap, n_out, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_resect_ring", e);
  HIPCHK(c, hipSetDevice(c->device));
  const ArthroView v = arthro_view(c, AV_RESECT);
  const ResectPass one{c->arthro.P(), p, 1, b, 1, ring_tiles(c->h_foff[b + 1] - c->h_foff[b])};
  if (int rc = resect_pass(c, v, RS_RECORDS, one, v.one, v.ring)) return rc;
  sh_resection r;
  HIPCHK(c, hipMemcpyAsync(&r, v.one, sizeof r, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (r.status != 0 || r.n_loops < 1) { *n_out = 0; return SH_OK; }
  *n_out = r.n_ring + 1;
  if (!out || cap < r.n_ring + 1) return SH_OK;
  HIPCHK(c, hipMemcpy(out, v.ring, (size_t)(r.n_ring + 1) * 24, hipMemcpyDeviceToHost));
  return SH_OK;
}

// ---- canal profiles and stems below the cuts of the last resection (k_stem.h) ------------------------------------------------------
int sh_canal_profile(sh_ctx* c, const sh_canal_grid* g, const double* frames, double* near_out, double* far_out, sh_canal_level* levels_out) {
  if (const ArthroError e = precheck_profile(g, frames, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_canal_profile", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, L = g->L, A = g->A;
  const CanalPlan plan = canal_plan(B, L, A, c->maxF);
  const size_t n = plan.rays;
  if (int rc = arthro_ensure(c, plan.bytes)) return rc;
  const ArthroView v = arthro_view(c, AV_CANAL);
  c->arthro.profile_begin();
  const double two_pi = 2.0 * 3.14159265358979323846;
  std::vector<double> dirs(2 * (size_t)A);
  for (int a = 0; a < A; ++a) { const double t = (two_pi * (double)a) / (double)A; dirs[2 * a] = std::cos(t); dirs[2 * a + 1] = std::sin(t); }
  HIPCHK(c, hipMemcpyAsync(v.canal_dirs, dirs.data(), dirs.size() * 8, hipMemcpyHostToDevice, c->stream));
  if (frames) {
    HIPCHK(c, hipMemcpyAsync(v.canal_frames, frames, (size_t)B * 128, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(v.canal_status, 0, (size_t)B * 4, c->stream));
  } else {
    LAUNCH(c, "k_canal_frames", k_canal_frames, dim3((unsigned)((B + 63) / 64)), dim3(64), v.lm, B, v.canal_frames, v.canal_status);
  }
  LAUNCH(c, "k_canal_clear", k_canal_clear, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), (unsigned long long*)v.canal_near,
         (unsigned long long*)v.canal_far, (long long)n);
  LAUNCH(c, "k_canal_rays", k_canal_rays, dim3((unsigned)plan.tmax, (unsigned)B), dim3(SH_CANAL_TILE), v.verts, v.faces, v.voff, v.foff,
         (const double*)v.canal_frames, (const int*)v.canal_status, (const double*)v.canal_dirs, g->z0, g->dz, L, A, (unsigned long long*)v.canal_near,
         (unsigned long long*)v.canal_far);
  LAUNCH(c, "k_canal_levels", k_canal_levels, dim3((unsigned)(B * L)), dim3(64), (const double*)v.canal_near, (const double*)v.canal_far,
         (const int*)v.canal_status, (const double*)v.canal_dirs, 0.5 * std::sin(two_pi / (double)A), L, A, v.canal_levels);
  if (near_out) HIPCHK(c, hipMemcpyAsync(near_out, v.canal_near, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (far_out) HIPCHK(c, hipMemcpyAsync(far_out, v.canal_far, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (levels_out) HIPCHK(c, hipMemcpyAsync(levels_out, v.canal_levels, (size_t)B * L * sizeof(sh_canal_level), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->arthro.profile_end(*g, c->batch_gen);
  return SH_OK;
}

int sh_resect_stems(sh_ctx* c, const sh_stem* stems, int K, sh_stem_fit* out) {
  if (const ArthroError e = precheck_stems(stems, K, out, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_resect_stems", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, P = c->arthro.P();
  const size_t n = (size_t)B * P * K;
  c->arthro.stems_begin();      // in front of the ensure: "stem.out" may be resized
  if (int rc = arthro_ensure(c, stem_bytes(B, P, K))) return rc;
  const ArthroView v = arthro_view(c, AV_RESECT | AV_CANAL | AV_STEM);
  const sh_canal_grid& g = c->arthro.grid();
  HIPCHK(c, hipMemcpyAsync(v.stem_catalogue, stems, (size_t)K * sizeof(sh_stem), hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_stem_fit", k_stem_fit, dim3((unsigned)(B * P)), dim3(SH_STEM_THREADS), (const double*)v.planes, (const int*)v.status, (const sh_resection*)v.out,
         (const double*)v.canal_frames, (const int*)v.canal_status, (const double*)v.canal_near, (const sh_canal_level*)v.canal_levels,
         (const double*)v.canal_dirs, g.z0, g.dz, g.L, g.A, (const sh_stem*)v.stem_catalogue, K, P, v.stem_out);
  HIPCHK(c, hipMemcpyAsync(out, v.stem_out, n * sizeof(sh_stem_fit), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->arthro.stems_end(K);
  return SH_OK;
}

// ---- implant plans: the seats and the stems of the last resection joined and ranked (k_plan.h); reads the chain's state, changes none ----
int sh_resect_plan(sh_ctx* c, const sh_plan_rule* rule, const uint64_t* compat, const double* ref_planes, int N, sh_plan* out, sh_plan_ref* ref_out) {
  if (const ArthroError e = precheck_plan(rule, ref_planes, N, out, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_resect_plan", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, P = c->arthro.P(), Kh = c->arthro.Kh(), Ks = c->arthro.Ks();
  const PlanPlan plan = plan_plan(B, P, Kh, Ks, N, c->maxV);
  const int tmax = plan.tmax;
  if (int rc = arthro_ensure(c, plan.bytes)) return rc;
  const ArthroView v = arthro_view(c, AV_RESECT | AV_CANAL | AV_STEM | AV_PLAN);
  const double* d_rp = ref_planes ? v.plan_ref_planes : nullptr;      // the reference planes are the caller's or the records'
  const sh_landmarks* d_lm = ref_planes ? nullptr : v.lm;
  uint64_t words[SH_SEAT_MAX_HEADS];
  for (int k = 0; k < SH_SEAT_MAX_HEADS; ++k) words[k] = compat && k < Kh ? compat[k] : ~0ull;      // (pageable: the copy is staged before the call returns)
  HIPCHK(c, hipMemcpyAsync(v.plan_compat, words, sizeof words, hipMemcpyHostToDevice, c->stream));
  if (ref_planes) HIPCHK(c, hipMemcpyAsync(v.plan_ref_planes, ref_planes, (size_t)B * 48, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_plan_ref", k_plan_ref, dim3((unsigned)tmax, (unsigned)B), dim3(SH_PLAN_TILE), v.verts, v.voff, (const double*)v.canal_frames,
         (const int*)v.canal_status, d_lm, d_rp, rule->margin, tmax, v.plan_ref_slab);
  LAUNCH(c, "k_plan_ref_join", k_plan_ref_join, dim3((unsigned)B), dim3(64), v.verts, v.voff, (const int*)v.canal_status, d_lm, d_rp, tmax,
         (const PlanTop*)v.plan_ref_slab, v.plan_ref);
  LAUNCH(c, "k_plan_terms", k_plan_terms, dim3((unsigned)plan.cuts), dim3(SH_PLAN_TERM_THREADS), (const double*)v.planes, (const int*)v.status,
         (const sh_resection*)v.out, (const sh_head_fit*)v.fit_out, (const sh_seat*)v.seat_out, (const sh_implant_head*)v.seat_heads, Kh,
         (const sh_stem_fit*)v.stem_out, Ks, (const double*)v.canal_frames, (const sh_plan_ref*)v.plan_ref, *rule, P, v.plan_cut_terms, v.plan_head_terms,
         v.plan_stem_terms, v.plan_cut_vals, v.plan_head_vals, v.plan_stem_vals);
  LAUNCH(c, "k_plan_select", k_plan_select, dim3((unsigned)B), dim3(SH_PLAN_THREADS), (const PlanTerm*)v.plan_cut_terms, (const PlanTerm*)v.plan_head_terms,
         (const PlanTerm*)v.plan_stem_terms, (const double*)v.plan_cut_vals, (const double*)v.plan_head_vals, (const double*)v.plan_stem_vals,
         (const unsigned long long*)v.plan_compat, P, Kh, Ks, N, v.plan_ref, v.plan_out);
  HIPCHK(c, hipMemcpyAsync(out, v.plan_out, (size_t)B * N * sizeof(sh_plan), hipMemcpyDeviceToHost, c->stream));
  if (ref_out) HIPCHK(c, hipMemcpyAsync(ref_out, v.plan_ref, (size_t)B * sizeof(sh_plan_ref), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- rays against the resident batch, every hit (k_rays.h); reads the mesh (and, for the anatomic-neck rays, the last run), changes no state ----
#define X(f, name, T, ...) T* f = nullptr;
struct RayView { ARTHRO_INPUT_BUFS(X) RAY_BUFS(X) };
#undef X
static RayView ray_view(sh_ctx* c) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  RayView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  ARTHRO_INPUT_BUFS(X) RAY_BUFS(X)
#undef X
  return v;
}
static int ray_ensure(sh_ctx* c, const RayBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  RAY_BUFS(X)
#undef X
  return SH_OK;
}

// count -> scan -> the total to the host -> "ray.pool" -> fill -> sort -> copies back.  "ray.rays" (and "ray.status" with `box`) are filled
// by the caller on the stream; T_obb / hstatus: the box transforms and the humeri to leave out (sh_anp_axis_hits), or null.
static int ray_run(sh_ctx* c, const RayPlan& plan, int R, int per_humerus, int cap, const double* T_obb, const int* hstatus, sh_ray_hit* hits, int32_t* counts) {
  int rc;
  const int B = c->B;
  const size_t n = plan.rays;
  RayView v = ray_view(c);
  const bool box = T_obb != nullptr;
  HIPCHK(c, hipMemsetAsync(v.ray_counts, 0, n * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(v.ray_cursor, 0, n * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(v.ray_blockhit, 0, plan.bytes.ray_blockhit, c->stream));
  const dim3 grid((unsigned)plan.tmax, (unsigned)B, (unsigned)plan.chunks), block(SH_RAY_TILE);
  LAUNCH(c, "k_ray_count", box ? k_ray_count<true> : k_ray_count<false>, grid, block, v.verts, v.faces, v.voff, v.foff, T_obb, hstatus, (const double*)v.ray_rays, R,
         per_humerus, v.ray_counts, v.ray_blockhit);
  LAUNCH(c, "k_ray_scan", k_ray_scan, dim3(1), dim3(1024), (const int*)v.ray_counts, (long long)n, v.ray_offs);
  unsigned long long total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, v.ray_offs + n, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ENS_SHARED("ray.pool", ray_pool_bytes(total), 8);
  v = ray_view(c);
  LAUNCH(c, "k_ray_fill", box ? k_ray_fill<true> : k_ray_fill<false>, grid, block, v.verts, v.faces, v.voff, v.foff, T_obb, hstatus, (const double*)v.ray_rays, R,
         per_humerus, (const unsigned long long*)v.ray_offs, v.ray_cursor, v.ray_pool, v.ray_blockhit);
  LAUNCH(c, "k_ray_sort", box ? k_ray_sort<true> : k_ray_sort<false>, dim3((unsigned)n), dim3(64), (const double*)v.ray_rays, R, per_humerus,
         (const unsigned long long*)v.ray_offs, (const int*)v.ray_cursor, (const RayKey*)v.ray_pool, T_obb, cap, v.ray_hits);
  if (hits) HIPCHK(c, hipMemcpyAsync(hits, v.ray_hits, n * cap * sizeof(sh_ray_hit), hipMemcpyDeviceToHost, c->stream));
  if (counts) HIPCHK(c, hipMemcpyAsync(counts, v.ray_counts, n * 4, hipMemcpyDeviceToHost, c->stream));
  return SH_OK;
}

int sh_ray_cast(sh_ctx* c, const sh_ray* rays, int R, int per_humerus, int cap, sh_ray_hit* hits, int32_t* counts) {
  if (const ArthroError e = precheck_ray_cast(rays, R, per_humerus, cap, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_ray_cast", e);
  HIPCHK(c, hipSetDevice(c->device));
  const RayPlan plan = ray_plan(c->B, R, per_humerus != 0, cap, c->maxF, false);
  if (int rc = ray_ensure(c, plan.bytes)) return rc;
  const RayView v = ray_view(c);
  HIPCHK(c, hipMemcpyAsync(v.ray_rays, rays, plan.bytes.ray_rays, hipMemcpyHostToDevice, c->stream));
  if (int rc = ray_run(c, plan, R, per_humerus != 0, cap, nullptr, nullptr, hits, counts)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_anp_axis_hits(sh_ctx* c, int cap, sh_ray_hit* hits, int32_t* counts, int32_t* status) {
  if (const ArthroError e = precheck_anp_hits(cap, status, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_anp_axis_hits", e);
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  const double* plane = (const double*)at("anp.plane");
  const double* T_obb = (const double*)at("obb_transform");
  const sh_landmarks* lm = (const sh_landmarks*)at("landmarks");
  if (!plane || !T_obb || !lm) return fail(c, SH_ERR_STATE, "sh_anp_axis_hits: the buffers of the anatomic-neck stage are not there");
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  const RayPlan plan = ray_plan(B, 4, true, cap, c->maxF, true);
  if (int rc = ray_ensure(c, plan.bytes)) return rc;
  const RayView v = ray_view(c);
  LAUNCH(c, "k_ray_anp_rays", k_ray_anp_rays, dim3((unsigned)((B + 63) / 64)), dim3(64), lm, plane, B, v.ray_rays, v.ray_status);
  if (int rc = ray_run(c, plan, 4, 1, cap, T_obb, (const int*)v.ray_status, hits, counts)) return rc;
  HIPCHK(c, hipMemcpyAsync(status, v.ray_status, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- closest surface points of the resident batch (k_closest.h); reads the mesh, changes no state of the chain ----
#define X(f, name, T, ...) T* f = nullptr;
struct CpView { ARTHRO_INPUT_BUFS(X) CP_BUFS(X) };
#undef X
static CpView cp_view(sh_ctx* c) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  CpView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  ARTHRO_INPUT_BUFS(X) CP_BUFS(X)
#undef X
  return v;
}
static int cp_ensure(sh_ctx* c, const CpBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  CP_BUFS(X)
#undef X
  return SH_OK;
}

int sh_closest_points(sh_ctx* c, const double* points, int Q, int per_humerus, sh_closest* out) {
  if (const ArthroError e = precheck_closest(points, Q, per_humerus, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_closest_points", e);
  HIPCHK(c, hipSetDevice(c->device));
  const CpPlan plan = cp_plan(c->B, Q, per_humerus != 0, c->maxF);
  if (int rc = cp_ensure(c, plan.bytes)) return rc;
  const CpView v = cp_view(c);
  HIPCHK(c, hipMemcpyAsync(v.cp_points, points, plan.bytes.cp_points, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_cp_walk", k_cp_walk, dim3((unsigned)plan.chunks, (unsigned)c->B, (unsigned)plan.S), dim3(SH_CP_CHUNK), v.verts, v.faces, v.voff, v.foff,
         (const double*)v.cp_points, Q, per_humerus != 0 ? 1 : 0, plan.S, v.cp_part);
  LAUNCH(c, "k_cp_join", k_cp_join, dim3((unsigned)((plan.points + 255) / 256)), dim3(256), v.verts, v.faces, v.voff, v.foff, (const double*)v.cp_points, Q,
         per_humerus != 0 ? 1 : 0, plan.S, (const CpPart*)v.cp_part, (long long)plan.points, v.cp_out);
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.cp_out, plan.bytes.cp_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- generalized winding numbers of the resident batch (k_winding.h); reads the mesh, changes no state of the chain ----
#define X(f, name, T, ...) T* f = nullptr;
struct WnView { ARTHRO_INPUT_BUFS(X) WN_BUFS(X) };
#undef X
static WnView wn_view(sh_ctx* c) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  WnView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  ARTHRO_INPUT_BUFS(X) WN_BUFS(X)
#undef X
  return v;
}
static int wn_ensure(sh_ctx* c, const WnBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  WN_BUFS(X)
#undef X
  return SH_OK;
}

int sh_winding_numbers(sh_ctx* c, const double* points, int Q, int per_humerus, sh_winding* out) {
  if (const ArthroError e = precheck_winding(points, Q, per_humerus, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_winding_numbers", e);
  HIPCHK(c, hipSetDevice(c->device));
  const WnPlan plan = wn_plan(c->B, Q, per_humerus != 0, c->maxF);
  if (int rc = wn_ensure(c, plan.bytes)) return rc;
  const WnView v = wn_view(c);
  HIPCHK(c, hipMemcpyAsync(v.wn_points, points, plan.bytes.wn_points, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_wn_walk", k_wn_walk, dim3((unsigned)plan.chunks, (unsigned)c->B, (unsigned)plan.S), dim3(SH_WN_CHUNK), v.verts, v.faces, v.voff, v.foff,
         (const double*)v.wn_points, Q, per_humerus != 0 ? 1 : 0, plan.S, plan.stride, v.wn_part);
  LAUNCH(c, "k_wn_join", k_wn_join, dim3((unsigned)((plan.points + 255) / 256)), dim3(256), v.foff, Q, plan.S, plan.stride, (const double*)v.wn_part,
         (long long)plan.points, v.wn_out);
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.wn_out, plan.bytes.wn_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- rigid registration of point sets onto the resident batch (k_icp.h); reads the mesh, changes no state of the chain ----
static_assert(AR_ICP_TERMS == SH_ICP_TERMS && AR_ICP_TSTRIDE == SH_ICP_TSTRIDE, "sh_arthro.h: registration terms, stride of icp.T");
#define X(f, name, T, ...) T* f = nullptr;
struct IcpView { ARTHRO_INPUT_BUFS(X) ICP_BUFS(X) };
#undef X
static IcpView icp_view(sh_ctx* c) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  IcpView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  ARTHRO_INPUT_BUFS(X) ICP_BUFS(X)
#undef X
  return v;
}
static int icp_ensure(sh_ctx* c, const IcpBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  ICP_BUFS(X)
#undef X
  return SH_OK;
}

// The chain of one registration, enqueued on the context's stream: the mean of the input points (phase 0), then max_iter + 1 evaluations
// of move -> walk -> join -> sums -> step.  `pts` are the device points (Q, shared or per humerus); "icp.T", "icp.flags", "icp.out" and
// "icp.hist" are in place.  Both entry points below run exactly this.
static int icp_chain(sh_ctx* c, const IcpView& v, const double* pts, int Q, int per, const IcpPlan& plan, const sh_icp_options* opt) {
  const int B = c->B, K = opt->max_iter;
  const dim3 blocks((unsigned)plan.chunks, (unsigned)B), lanes(SH_ICP_BLOCK);
  // one pass over the blocks: phase 0 the mean of the input points, phase 1 evaluation k
  // (LAUNCH ends in HIPCHK(hipGetLastError()): a launch that fails returns SH_ERR_HIP from the lambda, which the callers pass on)
  auto sum_step = [&](int phase, int k) -> int {
    LAUNCH(c, "k_icp_sum", k_icp_sum, blocks, lanes, v.verts, v.faces, v.voff, v.foff, pts, (const double*)v.icp_moved,
           (const sh_closest*)v.icp_near, Q, per, phase, (int)opt->metric, opt->reject, (const double*)v.icp_T, (const int*)v.icp_flags, v.icp_part);
    LAUNCH(c, "k_icp_step", k_icp_step, dim3((unsigned)B), dim3(64), (const double*)v.icp_part, plan.chunks, Q, phase, (int)opt->metric, k, K, opt->tol,
           v.icp_T, v.icp_flags, v.icp_hist, v.icp_out);
    return SH_OK;
  };
  if (int rc = sum_step(0, 0)) return rc;
  for (int k = 0; k <= K; ++k) {
    LAUNCH(c, "k_icp_move", k_icp_move, blocks, lanes, pts, Q, per, (const double*)v.icp_T, (const int*)v.icp_flags, v.icp_moved);
    LAUNCH(c, "k_cp_walk", k_cp_walk, dim3((unsigned)plan.chunks, (unsigned)B, (unsigned)plan.S), dim3(SH_CP_CHUNK), v.verts, v.faces, v.voff, v.foff,
           (const double*)v.icp_moved, Q, 1, plan.S, v.icp_cp_part);
    LAUNCH(c, "k_cp_join", k_cp_join, dim3((unsigned)((plan.points + 255) / 256)), dim3(256), v.verts, v.faces, v.voff, v.foff, (const double*)v.icp_moved, Q, 1,
           plan.S, (const CpPart*)v.icp_cp_part, (long long)plan.points, v.icp_near);
    if (int rc = sum_step(1, k)) return rc;
  }
  return SH_OK;
}

int sh_register_points(sh_ctx* c, const double* points, int Q, int per_humerus, const double* T0, const sh_icp_options* opt, sh_registration* out,
                       double* history) {
  if (const ArthroError e = precheck_register(points, Q, per_humerus, T0, opt, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_register_points", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, per = per_humerus != 0 ? 1 : 0, K = opt->max_iter;
  const IcpPlan plan = icp_plan(B, Q, per != 0, c->maxF, K);
  if (int rc = icp_ensure(c, plan.bytes)) return rc;
  const IcpView v = icp_view(c);
  std::vector<double> start((size_t)B * SH_ICP_TSTRIDE, 0.0);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 16; ++i) start[(size_t)b * SH_ICP_TSTRIDE + i] = T0 ? T0[16 * (size_t)b + i] : (i % 5 == 0 ? 1.0 : 0.0);
  HIPCHK(c, hipMemcpyAsync(v.icp_T, start.data(), plan.bytes.icp_T, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.icp_points, points, plan.bytes.icp_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_flags, 0, plan.bytes.icp_flags, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_hist, 0, plan.bytes.icp_hist, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_out, 0, plan.bytes.icp_out, c->stream));
  if (int rc = icp_chain(c, v, (const double*)v.icp_points, Q, per, plan, opt)) return rc;
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.icp_out, plan.bytes.icp_out, hipMemcpyDeviceToHost, c->stream));
  if (history) HIPCHK(c, hipMemcpyAsync(history, v.icp_hist, plan.bytes.icp_hist, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- multi-start registration (k_ms.h around the chain above); reads the mesh, changes no state of the chain ----
#define X(f, name, T, ...) T* f = nullptr;
struct MsView { MS_BUFS(X) };
#undef X
static MsView ms_view(sh_ctx* c) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  MsView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  MS_BUFS(X)
#undef X
  return v;
}
static int ms_ensure(sh_ctx* c, const MsBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  MS_BUFS(X)
#undef X
  return SH_OK;
}

int sh_register_multistart(sh_ctx* c, const double* points, int Q, int per_humerus, const double* T0s, int K, const sh_icp_options* coarse,
                           int coarse_points, int min_pairs, const sh_icp_options* fine, sh_registration* out, sh_registration* coarse_out,
                           int32_t* winner) {
  if (const ArthroError e = precheck_multistart(points, Q, per_humerus, T0s, K, coarse, coarse_points, min_pairs, fine, arthro_facts(c)); e.code)
    return arthro_refuse(c, "sh_register_multistart", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, per = per_humerus != 0 ? 1 : 0;
  const MsPlan plan = ms_plan(B, Q, per != 0, c->maxF, K, coarse_points, coarse->max_iter, fine->max_iter);
  const int Qc = plan.Qc;
  if (int rc = icp_ensure(c, plan.icp)) return rc;
  if (int rc = ms_ensure(c, plan.bytes)) return rc;
  const IcpView v = icp_view(c);
  const MsView m = ms_view(c);
  const size_t sets = per ? (size_t)B : 1;
  std::vector<double> cpts(sets * Qc * 3);      // (pageable: the copy is staged before the call returns)
  for (size_t s = 0; s < sets; ++s)
    for (int j = 0; j < Qc; ++j) {
      const double* p = points + 3 * (s * Q + (size_t)ms_coarse_index(j, Q, Qc));
      double* q = &cpts[3 * (s * Qc + j)];
      q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
  HIPCHK(c, hipMemcpyAsync(m.ms_points, cpts.data(), plan.bytes.ms_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(m.ms_T0s, T0s, plan.bytes.ms_T0s, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.icp_points, points, plan.fine.bytes.icp_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_moved, 0, plan.icp.icp_moved, c->stream));      // (a humerus without a winner is walked, never moved, in the fine stage)
  HIPCHK(c, hipMemsetAsync(v.icp_hist, 0, plan.icp.icp_hist, c->stream));
  const dim3 per_b((unsigned)((B + 63) / 64)), wave(64);
  for (int k = 0; k < K; ++k) {
    LAUNCH(c, "k_ms_seed", k_ms_seed, per_b, wave, (const double*)m.ms_T0s, B, K, k, (const sh_registration*)m.ms_coarse, (const int*)m.ms_winner, v.icp_T,
           v.icp_flags, v.icp_out);
    if (int rc = icp_chain(c, v, (const double*)m.ms_points, Qc, per, plan.coarse, coarse)) return rc;
    LAUNCH(c, "k_ms_pick", k_ms_pick, per_b, wave, (const sh_registration*)v.icp_out, B, K, k, min_pairs, m.ms_coarse, m.ms_best, m.ms_winner);
  }
  HIPCHK(c, hipMemsetAsync(v.icp_hist, 0, plan.icp.icp_hist, c->stream));
  LAUNCH(c, "k_ms_seed", k_ms_seed, per_b, wave, (const double*)m.ms_T0s, B, K, -1, (const sh_registration*)m.ms_coarse, (const int*)m.ms_winner, v.icp_T,
         v.icp_flags, v.icp_out);
  if (int rc = icp_chain(c, v, (const double*)v.icp_points, Q, per, plan.fine, fine)) return rc;
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.icp_out, plan.fine.bytes.icp_out, hipMemcpyDeviceToHost, c->stream));
  if (coarse_out) HIPCHK(c, hipMemcpyAsync(coarse_out, m.ms_coarse, plan.bytes.ms_coarse, hipMemcpyDeviceToHost, c->stream));
  if (winner) HIPCHK(c, hipMemcpyAsync(winner, m.ms_winner, plan.bytes.ms_winner, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- mass properties of the resident batch (k_mass.h); reads the mesh, changes no state of the chain ----
static_assert(AR_MASS_TERMS == SH_MASS_TERMS, "sh_arthro.h: mass terms");
#define X(f, name, T, ...) T* f = nullptr;
struct MassView { ARTHRO_INPUT_BUFS(X) MASS_BUFS(X) };
#undef X
static MassView mass_view(sh_ctx* c) {
  auto at = [c](const char* name) { auto it = c->bufs.find(name); return it == c->bufs.end() ? nullptr : it->second.p; };
  MassView v;
#define X(f, name, T, ...) v.f = (T*)at(name);
  ARTHRO_INPUT_BUFS(X) MASS_BUFS(X)
#undef X
  return v;
}
static int mass_ensure(sh_ctx* c, const MassBytes& z) {
  int rc;
#define X(f, name, T, elem) if (z.f) ENS_SHARED(name, z.f, elem);
  MASS_BUFS(X)
#undef X
  return SH_OK;
}

int sh_mass_properties(sh_ctx* c, sh_mass* out) {
  if (const ArthroError e = precheck_mass(arthro_facts(c)); e.code) return arthro_refuse(c, "sh_mass_properties", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  const MassPlan plan = mass_plan(B, c->maxF);
  if (int rc = mass_ensure(c, plan.bytes)) return rc;
  const MassView v = mass_view(c);
  HIPCHK(c, hipMemsetAsync(v.mass_part, 0, plan.bytes.mass_part, c->stream));
  LAUNCH(c, "k_mass_sum", k_mass_sum, dim3((unsigned)plan.blocks, (unsigned)B), dim3(SH_MASS_BLOCK), v.verts, v.faces, v.voff, v.foff, v.mass_part);
  LAUNCH(c, "k_mass_join", k_mass_join, dim3((unsigned)B), dim3(64), v.verts, v.voff, v.foff, (const double*)v.mass_part, plan.blocks, v.mass_out);
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.mass_out, plan.bytes.mass_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}
