// sh_arthro_host.h -- the entry points of the arthroplasty chain: sh_resect_* (k_resect.h, k_headfit.h, k_seat.h), sh_canal_profile and
// sh_resect_stems (k_stem.h), sh_resect_plan (k_plan.h).  Host code of shoulder_hip.hip, included there EXACTLY ONCE, behind the kernel
// headers and inside its extern "C" block, with sh_query_host.h (the queries of the resident batch) right behind it.  Headers and not
// units of their own: compiled in a unit that holds only the resection headers, the unchanged k_resect_faces takes 100 VGPRs instead
// of 92, four waves per SIMD instead of five, so the kernels stay in shoulder_hip.hip and the code that launches them
// with them.
// What the chain DECIDES is sh_arthro.h (checks, first refusal, pass plan, buffer sizes, ArthroState).  Every entry point here reads:
// precheck -> ensure -> view -> state begin -> enqueue -> copies back -> synchronise -> state end.
#pragma once

static_assert(AR_RS_TILE == SH_RS_TILE && AR_HF_WORDS == SH_HF_WORDS && AR_RESECT_PART_BYTES == sizeof(ResectPart), "sh_arthro.h: resection tile, moment words, slab entry");
static_assert(AR_CANAL_TILE == SH_CANAL_TILE && AR_PLAN_TILE == SH_PLAN_TILE && AR_PLAN_TOP_BYTES == sizeof(PlanTop) && AR_PLAN_TERM_BYTES == sizeof(PlanTerm),
              "sh_arthro.h: canal and plan tiles, PlanTop, PlanTerm");

static ArthroFacts arthro_facts(const sh_ctx* c) {
  if (!c) return ArthroFacts{false, 0, 0, 0, false, nullptr};
  return ArthroFacts{true, c->B, c->n_pending, c->batch_gen, c->at("landmarks") != nullptr, &c->arthro};
}

static int arthro_refuse(sh_ctx* c, const char* fn, const ArthroError& e) { return fail(c, e.code, std::string(fn) + ": " + e.text); }

// The view of a call of the chain (sh_ctx.h view_of, behind the call's ensure_bytes), with its two rules.  `groups`: which of the
// chain's own lists the call touches (the mesh always); the others stay null and cost no lookup.  `lm` is null without a run of the
// resident batch with the anatomic neck and the csys.
enum : unsigned { AV_RESECT = 1, AV_CANAL = 2, AV_STEM = 4, AV_PLAN = 8 };
static ArthroView arthro_view(sh_ctx* c, unsigned groups) {
  ArthroView v;
  static_cast<MeshBufs&>(v) = view_of<MeshBufs>(c);
  if (groups & AV_RESECT) static_cast<ResectBufs&>(v) = view_of<ResectBufs>(c);
  if (groups & AV_CANAL) static_cast<CanalBufs&>(v) = view_of<CanalBufs>(c);
  if (groups & AV_STEM) static_cast<StemBufs&>(v) = view_of<StemBufs>(c);
  if (groups & AV_PLAN) static_cast<PlanBufs&>(v) = view_of<PlanBufs>(c);
  if (!c->arthro.has_records(c->batch_gen)) v.lm = nullptr;
  return v;
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
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
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
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
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
  if (int rc = ensure_bytes(c, stem_bytes(B, P, K))) return rc;
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
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
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
