// hull.hip -- the convex hulls of SH_STAGE_OBB: the device prefilter of the hull's points (k_hullpre.h), the host quickhull phase on the
// process-wide worker pool (sh_hull.h), the upload of its records, and the hull on the device (k_hull.h).  run_obb (shoulder_hip.hip)
// and the background threads of the overlap / staging paths call in here.
#include "sh_ctx.h"

#include "k_hullpre.h"
#include "k_hull.h"

using namespace sh;

// Scratch of the device hull (k_hull.h), ~1.6 MB per humerus, allocated on the first run that uses it.
static int alloc_hulld(sh_ctx* c) {
  const int B = c->B;
  int rc;
  ENS("hulld.fv", (size_t)B * HD_SLOTS * 3 * 4, 4);
  ENS("hulld.vis", (size_t)B * HD_KC * HD_VMAX * 4, 4);
  ENS("hulld.ev", (size_t)B * HD_KC * 3 * HD_VMAX * 2 * 4, 4);
  ENS("hulld.hor", (size_t)B * HD_KC * (HD_VMAX + 2) * 2 * 4, 4);
  ENS("hulld.newslot", (size_t)B * HD_SLOTS * 4, 4);
  ENS("hulld.freestack", (size_t)B * HD_SLOTS * 4, 4);
  ENS("hulld.tkeys", (size_t)B * HD_TBL * 8, 8);
  ENS("hulld.tvals", (size_t)B * HD_TBL * 4, 4);
  ENS("hulld.fail", (size_t)B * 4, 4);
  ENS("hulld.rounds", (size_t)B * 4, 4);
  ENS("hulld.skip", (size_t)B * 4, 4);
  if (c->skip_gen != c->batch_gen) {      // a new batch: the device hull takes every humerus again
    HIPCHK(c, hipMemsetAsync(c->bufs["hulld.skip"].p, 0, (size_t)B * 4, c->stream));
    c->skip_gen = c->batch_gen;
    c->batch.skip_list_cleared();
  }
  return SH_OK;
}

// The prefilter's buffers for B humeri with sumV vertices in all: the resident batch's (sfx "": [B][...] buffers with their window
// strides) or the staging side's (sfx ".s": no windows).
int sh::alloc_hullpre(sh_ctx* c, int B, long long sumV, const char* sfx) {
  const struct { const char* n; size_t per; int elem; } arr[] = {
      {"hullpre.ext", (size_t)SH_HP_NDIR * 4, 4}, {"hullpre.planes", (size_t)SH_HP_MAXPL * 4 * 8, 8}, {"hullpre.npl", 4, 4}, {"hullpre.nkept", 4, 4},
      {"hullpre.pval", (size_t)SH_HP_PARTS * SH_HP_NDIR * 8, 8}, {"hullpre.pidx", (size_t)SH_HP_PARTS * SH_HP_NDIR * 4, 4}, {"hullpre.pcnt", (size_t)SH_HP_PARTS * 4, 4},
      {"hullpre.poff", (size_t)SH_HP_PARTS * 8, 8}};
  const bool windows = sfx[0] == 0;
  int rc;
  for (const auto& a : arr) {
    const std::string nm = std::string(a.n) + sfx;
    if ((rc = ensure(c, nm.c_str(), (size_t)B * a.per, a.elem)) != SH_OK) return rc;
    c->bufs[nm].per_mesh = windows ? a.per : 0;
  }
  const std::string koff = std::string("hullpre.koff") + sfx, kept = std::string("hullpre.kept") + sfx;
  if ((rc = ensure(c, koff.c_str(), (size_t)(B + 1) * 8, 8)) != SH_OK) return rc;
  c->bufs[koff].per_mesh = windows ? (size_t)(B + 1) * 8 / (size_t)B : 0;
  if ((rc = ensure(c, kept.c_str(), (size_t)sumV * 12, 4)) != SH_OK) return rc;
  c->bufs[kept].per_mesh = windows ? (size_t)sumV * 12 / (size_t)B : 0;
  return SH_OK;
}

// The hull's input points.  Host-provided batch: the caller's vertices.  Device-generated batch: the prefilter
// (k_hullpre.h) drops the vertices strictly inside a 26-direction polytope on the device and only the rest comes back
// (39 % of a humerus, into pinned memory).  Callable from the background thread: no buffer-map access, no timers.
HullPre sh::hullpre_ptrs(sh_ctx* c, const char* sfx) {      // calling thread only (buffer map); sfx ".s": the staging side
  auto p = [&](const char* n) { return c->bufs[std::string(n) + sfx].p; };
  return HullPre{(const float*)p("verts"), (const long long*)p("voff"), (int*)p("hullpre.ext"), (double*)p("hullpre.planes"), (int*)p("hullpre.npl"), (float*)p("hullpre.kept"),
                 (int*)p("hullpre.nkept"), (long long*)p("hullpre.koff"), (double*)p("hullpre.pval"), (int*)p("hullpre.pidx"), (int*)p("hullpre.pcnt"), (long long*)p("hullpre.poff")};
}
// the five launches of the device prefilter (k_hullpre.h): survivors of all B humeri compacted into hp.kept at hp.koff
static void launch_prefilter(const HullPre& hp, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_hullpre_extremes, dim3(SH_HP_PARTS, B), dim3(256), 0, st, hp.verts, hp.voff, hp.pval, hp.pidx);
  hipLaunchKernelGGL(k_hullpre_polytope, dim3(B), dim3(256), 0, st, hp.verts, hp.voff, (const double*)hp.pval, (const int*)hp.pidx, hp.ext, hp.planes, hp.npl);
  hipLaunchKernelGGL(k_hullpre_filter<false>, dim3(SH_HP_PARTS, B), dim3(256), 0, st, hp.verts, hp.voff, (const double*)hp.planes, (const int*)hp.npl,
                     (const long long*)hp.poff, hp.kept, hp.pcnt);
  hipLaunchKernelGGL(k_hullpre_offsets, dim3(1), dim3(64), 0, st, (const int*)hp.pcnt, hp.koff, hp.poff, hp.nkept, B);
  hipLaunchKernelGGL(k_hullpre_filter<true>, dim3(SH_HP_PARTS, B), dim3(256), 0, st, hp.verts, hp.voff, (const double*)hp.planes, (const int*)hp.npl,
                     (const long long*)hp.poff, hp.kept, hp.pcnt);
}

// survivors of the device prefilter of a batch of B humeri (sumV vertices in all) -> pinned h_kept / h_koff, described by *out
hipError_t sh::fetch_prefiltered(const HullPre& hp, int B, long long sumV, long long* h_koff, float* h_kept, sh_ctx::HullPts* out, hipStream_t st) {
  hipError_t e;
  launch_prefilter(hp, B, st);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(h_koff, hp.koff, (size_t)(B + 1) * 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  const long long total = h_koff[B];
  if (total < 0 || total > sumV) return hipErrorUnknown;
  if (total > 0 && (e = hipMemcpyAsync(h_kept, hp.kept, (size_t)total * 12, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;      // one copy for the batch
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  out->off.resize(B); out->cnt.resize(B);
  for (int b = 0; b < B; ++b) { out->off[b] = h_koff[b]; out->cnt[b] = (int)(h_koff[b + 1] - h_koff[b]); }
  out->src = h_kept;
  return hipSuccess;
}

hipError_t sh::fetch_hull_points(sh_ctx* c, const HullPre& hp, hipStream_t st) {
  const int B = c->B;
  sh_ctx::HullPts& in = c->hull_in;
  in.cnt.resize(B);
  if (c->h_verts_valid) {
    in.off.assign(c->h_voff.begin(), c->h_voff.begin() + B);
    for (int b = 0; b < B; ++b) in.cnt[b] = (int)(c->h_voff[b + 1] - c->h_voff[b]);
    in.src = c->h_verts.data();
    return hipSuccess;
  }
  hipError_t e;
  if (!c->sw.hull_prefilter || !hp.kept) {
    c->h_verts.resize(3 * (size_t)c->sumV);
    if ((e = hipMemcpyAsync(c->h_verts.data(), hp.verts, c->sumV * 3 * 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    in.off.assign(c->h_voff.begin(), c->h_voff.begin() + B);
    for (int b = 0; b < B; ++b) in.cnt[b] = (int)(c->h_voff[b + 1] - c->h_voff[b]);
    in.src = c->h_verts.data();
    return hipSuccess;
  }
  return fetch_prefiltered(hp, B, c->sumV, c->h_koff, c->h_kept, &in, st);
}

// Process-wide worker pool of the host hull phase.  A job is a callable every participating thread runs to completion
// (the callable itself hands out mesh indices through an atomic counter); run() returns when all workers that picked
// the job up have left it.  Jobs of different contexts queue up FIFO and are served by the same threads.
class HullPool {
 public:
  static HullPool& instance() { static HullPool p; return p; }
  static unsigned thread_count() {
    unsigned nt = std::min(threads_per_local_rank(false), 32u);      // (affinity mask / LOCAL_WORLD_SIZE aware)
    if (const char* e = getenv("SHOULDER_HULL_THREADS")) { int v = atoi(e); if (v > 0) nt = (unsigned)v; }
    return nt;
  }
  void run(const std::function<void()>& fn, int items) {
    Job job;
    job.fn = fn;
    job.want = (int)std::min<unsigned>(std::max(1, items), (unsigned)workers_.size() + 1) - 1;      // helpers besides the caller
    if (job.want > 0) {
      { std::lock_guard<std::mutex> lk(mu_); queue_.push_back(&job); }
      cv_.notify_all();
    }
    fn();                                    // the caller takes part
    if (job.want > 0) {
      std::unique_lock<std::mutex> lk(mu_);
      // helpers that have not started yet are no longer needed (the counter inside fn is exhausted): withdraw the job
      auto it = std::find(queue_.begin(), queue_.end(), &job);
      if (it != queue_.end()) queue_.erase(it);
      done_cv_.wait(lk, [&] { return job.active == 0; });
    }
  }

 private:
  struct Job { std::function<void()> fn; int want = 0, taken = 0, active = 0; };
  HullPool() {
    const unsigned nt = thread_count();
    for (unsigned t = 1; t < nt; ++t) workers_.emplace_back([this] { loop(); });
  }
  ~HullPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || !queue_.empty(); });
      if (stop_) return;
      Job* j = queue_.front();
      ++j->taken; ++j->active;
      if (j->taken >= j->want) queue_.pop_front();
      lk.unlock();
      j->fn();
      lk.lock();
      if (--j->active == 0) done_cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  std::deque<Job*> queue_;
  std::vector<std::thread> workers_;
  bool stop_ = false;
};

// mesh.py:63-125.  Host: one quickhull per humerus on worker threads (sh_hull.h).  Device: candidate
// boxes for every hull face, pick + frame, end sections, circle fits, flip (k_obb.h).
// Host phase of the OBB stage for meshes [b0, b0 + B): one quickhull per humerus on worker threads into pinned slot
// `slot`.  Callable from the background thread: touches no error string, no timers; HIP errors come back as text.
// One hull phase at a time per process, the one a run is WAITING for first.  The pool is shared by the lanes of a process; two
// phases at once (a run's own and another lane's background preparation) interleaved on the same workers and both came late:
// measured at the start of a timed region, lanes idle -- the second lane's first hull phase took 12.8 ms instead of 5.1 beside
// the first lane's preparation of its NEXT step, the first UNet passes were 10-17 ms apart and 20 steps carried 0.5-0.8 ms each
// of it.  A background preparation now waits while a foreground phase is running or waiting, and one that is under way hands the
// pool over at the next hull boundary (its workers take no further humerus; it finishes the rest after the foreground phase).
struct HullPhaseGate {
  std::mutex m; std::condition_variable cv; bool busy = false; std::atomic<int> fg_waiting{0};
  void enter(bool background) {
    std::unique_lock<std::mutex> l(m);
    if (!background) ++fg_waiting;
    cv.wait(l, [&] { return !busy && (!background || fg_waiting.load() == 0); });
    if (!background) --fg_waiting;
    busy = true;
  }
  bool foreground_waits() const { return fg_waiting.load(std::memory_order_relaxed) > 0; }
  void leave() { { std::lock_guard<std::mutex> l(m); busy = false; } cv.notify_all(); }
  static HullPhaseGate& instance() { static HullPhaseGate g; return g; }
};

// One pinned slot for B humeri at `pitch` elements per humerus (what it held before is freed)
static int hull_stage_alloc(sh_ctx::HullStage& hs, int B, HullCap pitch, std::string* errtxt) {
  if (hs.hv) { (void)hipHostFree(hs.hv); (void)hipHostFree(hs.nr); (void)hipHostFree(hs.ed); (void)hipHostFree(hs.cnt); }
  hs.hv = nullptr; hs.cap = 0;
  hs.pv = pitch.v; hs.pf = pitch.f; hs.pe = pitch.e;
  HIPCHK_TXT(errtxt, hipHostMalloc((void**)&hs.hv, (size_t)B * hs.pv * 3 * 8));
  HIPCHK_TXT(errtxt, hipHostMalloc((void**)&hs.nr, (size_t)B * hs.pf * 3 * 8));
  HIPCHK_TXT(errtxt, hipHostMalloc((void**)&hs.ed, (size_t)B * hs.pe * 4 * 4));
  HIPCHK_TXT(errtxt, hipHostMalloc((void**)&hs.cnt, (size_t)B * 3 * 4));
  hs.cap = B;
  return SH_OK;
}

// The hull of one humerus: its float32 points widened into h.P, the quickhull (which has the retry / joggle logic) into h.H, the
// counts into h.n.  false: no hull.
bool sh::hull_of_points(const float* src, long long nv, HostHull& h) {
  h.P.assign(src, src + 3 * nv);
  if (!shhull::convex_hull(h.P.data(), (int)nv, h.H)) return false;
  h.n = {(int)h.H.vert_ids.size(), (int)h.H.tris.size() / 3, (int)h.H.edges.size() / 4};
  return true;
}
// the hull's vertices, in the order of the record
static void hull_gather(const HostHull& h, double* hv) {
  for (int i = 0; i < h.n.v; ++i)
    for (int k = 0; k < 3; ++k) hv[3 * (size_t)i + k] = h.P[3 * (size_t)h.H.vert_ids[i] + k];
}

int sh::hull_host_phase(sh_ctx* c, const sh_ctx::HullPts& in, int slot, int b0, int B, int* bad_mesh, double* ms, std::string* errtxt, bool background) {
  auto t0 = std::chrono::steady_clock::now();
  sh_ctx::HullStage& hs = c->hstage[slot];
  HullCap pitch = {hs.pv, hs.pf, hs.pe};
  bool grown = false;
  int rc;
again:
  if ((hs.cap < B || grown) && (rc = hull_stage_alloc(hs, B, pitch, errtxt)) != SH_OK) return rc;
  if (!hs.ev) HIPCHK_TXT(errtxt, hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));
  if (hs.used) HIPCHK_TXT(errtxt, hipEventSynchronize(hs.ev));     // the previous copies out of this slot are done
  // the other slot of the double buffer is allocated with the first one: pinning its 31 MB costs ~7 ms, and a context that had run
  // once (a warm-up step) paid that in its SECOND run -- the first timed step of a lane (round 3: 12 ms instead of 5 for that hull
  // phase, the first UNet passes of a 20-step region 14 ms apart)
  if (!c->hstage[slot ^ 1].hv && !grown && (rc = hull_stage_alloc(c->hstage[slot ^ 1], B, pitch, errtxt)) != SH_OK) return rc;
  double* hv = hs.hv; double* nr = hs.nr; int* ed = hs.ed; int* counts = hs.cnt;
  std::vector<int> status(B, 0);
  std::vector<int> demand(3 * (size_t)B, 0);      // [3][B] as the count block: of the humeri whose hull does not fit the staging pitch
  std::atomic<int> next(0);
  auto work = [&]() {
    HostHull h;
    for (;;) {
      if (background && HullPhaseGate::instance().foreground_waits()) break;      // a run is waiting for ITS hulls: hand the pool over
      int b = next.fetch_add(1);
      if (b >= B) break;
      counts[b] = counts[B + b] = counts[2 * B + b] = 0;
      if (!hull_of_points(in.src + 3 * in.off[b0 + b], in.cnt[b0 + b], h)) { status[b] = SH_ERR_GEOMETRY; continue; }
      if (!hull_fits(h.n, pitch)) { status[b] = 1; demand[b] = h.n.v; demand[B + b] = h.n.f; demand[2 * B + b] = h.n.e; continue; }      // the staging pitch is too small: see below
      hull_gather(h, hv + (size_t)b * hs.pv * 3);
      std::copy(h.H.normals.begin(), h.H.normals.end(), nr + (size_t)b * hs.pf * 3);
      std::copy(h.H.edges.begin(), h.H.edges.end(), ed + (size_t)b * hs.pe * 4);
      counts[b] = h.n.v; counts[B + b] = h.n.f; counts[2 * B + b] = h.n.e;
    }
  };
  // One pool of worker threads per process, started once and shared by every context (lane) of the process: the host's
  // hardware threads divided between the ranks of this node (torchrun exports LOCAL_WORLD_SIZE), at most 32 per process;
  // SHOULDER_HULL_THREADS overrides.  The calling thread works on its own batch too.  (Round 1 started up to 32 threads
  // per batch: a third of the 4.8 ms hull phase was thread start-up, and two lanes doubled the thread count.)
  do {
    HullPhaseGate::instance().enter(background);
    HullPool::instance().run(work, B);
    HullPhaseGate::instance().leave();
  } while (next.load() < B);      // (a background phase that handed the pool over: the remaining humeri)
  if (!grown && std::find(status.begin(), status.end(), 1) != status.end()) {
    // a hull larger than the staging pitch (a dense mesh): this slot gets the record capacity -- or, above it, what the largest hull
    // of the batch needs (the device record grows at the upload: grow_hull_records) -- and the phase runs again
    pitch = hull_pitch_grown(hull_need(demand.data(), B));
    grown = true;
    std::fill(status.begin(), status.end(), 0);
    next = 0;
    goto again;
  }
  *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int b = 0; b < B; ++b)
    if (status[b] != 0) { *bad_mesh = b0 + b; return status[b] == 1 ? SH_ERR_CAPACITY : status[b]; }      // (1 survives only if the re-sized staging still did not hold a hull)
  return SH_OK;
}

// Hull records of pinned slot `slot` -> device buffers on stream `st`: only the used head of every fixed-capacity record
// crosses PCIe (one strided copy per array).  `dst`: hull_rec() of the window (sh_ctx.h).
hipError_t sh::hull_upload(sh_ctx* c, int slot, int B, const HullRec& dst, hipStream_t st) {
  sh_ctx::HullStage& hs = c->hstage[slot];
  const int* counts = hs.cnt;
  const HullNeed n = hull_need(counts, B);
  if (!hull_fits(n, c->hcap)) return hipErrorInvalidValue;      // (the foreground grows the record first, a background thread leaves the upload to it)
  hipError_t e;
  if ((e = hipMemcpy2DAsync(dst.hv, (size_t)c->hcap.v * 24, hs.hv, (size_t)hs.pv * 24, (size_t)n.v * 24, B, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpy2DAsync(dst.normals, (size_t)c->hcap.f * 24, hs.nr, (size_t)hs.pf * 24, (size_t)n.f * 24, B, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpy2DAsync(dst.edges, (size_t)c->hcap.e * 16, hs.ed, (size_t)hs.pe * 16, (size_t)n.e * 16, B, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.nv, counts, (size_t)B * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.nf, counts + B, (size_t)B * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.ne, counts + 2 * B, (size_t)B * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipEventRecord(hs.ev, st)) != hipSuccess) return e;      // pinned slot is free again once these copies have run
  hs.used = true;
  return hipSuccess;
}
// ... and the record of ONE humerus (redo_given_up) -> `dst`, the record of that humerus as a window of one.  The sources are h's,
// pageable (hipMemcpyAsync stages them before it returns); the caller synchronises `st` before h goes out of scope all the same.
hipError_t sh::hull_upload_one(HostHull& h, const HullRec& dst, hipStream_t st) {
  h.hv.resize(3 * (size_t)h.n.v);
  hull_gather(h, h.hv.data());
  hipError_t e;
  if ((e = hipMemcpyAsync(dst.hv, h.hv.data(), h.hv.size() * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.normals, h.H.normals.data(), (size_t)h.n.f * 24, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.edges, h.H.edges.data(), (size_t)h.n.e * 16, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.nv, &h.n.v, 4, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(dst.nf, &h.n.f, 4, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  return hipMemcpyAsync(dst.ne, &h.n.e, 4, hipMemcpyHostToDevice, st);
}

// The hull on the device: prefilter -> round-based quickhull (k_hull.h), all on this context's stream; nothing comes to the host
// (the face count run_obb sizes its grids by is sh_obb_plan.h hull_nfmax).
int sh::run_device_hull(sh_ctx* c, int B) {
  { int arc = alloc_hulld(c); if (arc != SH_OK) return arc; }
  launch_prefilter(hullpre_ptrs(c), B, c->stream);
  HIPCHK(c, hipGetLastError());
  HullScratch hs{buf<int>(c, "hulld.fv"), buf<int>(c, "hulld.vis"), buf<int>(c, "hulld.ev"), buf<int>(c, "hulld.hor"), buf<int>(c, "hulld.newslot"),
                 buf<int>(c, "hulld.freestack"), buf<unsigned long long>(c, "hulld.tkeys"), buf<unsigned>(c, "hulld.tvals")};
  const HullRec h = hull_rec(c);
  LAUNCH(c, "k_hull_rounds", k_hull_rounds, dim3(B), dim3(HD_THREADS), (const float*)c->bufs["hullpre.kept"].p, (const long long*)c->bufs["hullpre.koff"].p, hs,
         h.hv, h.normals, h.edges, h.nv, h.nf, h.ne,
         buf<int>(c, "hulld.fail"), buf<int>(c, "hulld.rounds"), (const int*)buf<int>(c, "hulld.skip"), c->hcap);
  LAUNCH(c, "k_hull_flag", k_hull_flag, dim3((B + 63) / 64), dim3(64), buf<int>(c, "hulld.fail"), buf<int>(c, "err"), B);
  return SH_OK;
}
