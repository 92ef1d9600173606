// shoulder_hip.hip -- libshoulder_hip.so: context, buffers, C-ABI (include/shoulder_hip.h), meshes and the stage runner.  gfx950 only.
// The geometry kernels live in k_*.h next to this file; the UNet is unet.hip's, the collectives comm.hip's (sh_ctx.h: who owns what).
#include "sh_ctx.h"

#include "k_slices.h"
#include "k_ovf.h"
#include "k_open.h"
#include "k_stages.h"
#include "k_groove.h"
#include "k_anp.h"
#include "k_stl.h"
#include "k_clip.h"
#include "k_resect.h"
#include "k_headfit.h"
#include "k_seat.h"
#include "k_stem.h"
#include "k_plan.h"
#include "k_rays.h"
#include "k_closest.h"
#include "k_winding.h"
#include "k_icp.h"
#include "k_ms.h"
#include "k_mass.h"
#include "k_sample.h"
#include "k_topo.h"
#include "k_vert.h"
#include "k_geo.h"
#include "k_smooth.h"
#include "k_repair.h"
#include "k_simplify.h"
#include "k_bvh.h"
#include "k_raytree.h"
#include "k_te.h"
#include "k_obb.h"

#include <sched.h>

using namespace sh;

// Buffer clears of a run as ONE kernel launch per group of adjacent clears.  hipMemsetAsync costs the enqueuing thread ~60 us per
// call on this stack (rocprofv3 trace of bench.py: the five clears that open a step spread over 0.3 ms before its first kernel;
// ~17 per step = 1 ms of host time) -- a kernel launch costs ~5 us.
struct FillList { void* p[6]; unsigned long long n[6]; unsigned v[6]; };
__global__ void k_fill_list(FillList L) {
  unsigned* p = (unsigned*)L.p[blockIdx.y];
  const unsigned long long nw = L.n[blockIdx.y] >> 2;
  const unsigned v = L.v[blockIdx.y];
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < nw; i += (unsigned long long)gridDim.x * blockDim.x) p[i] = v;
}
int sh::fill_list(sh_ctx* c, std::initializer_list<FillEnt> ents) {
  FillList L{};
  int k = 0; size_t nmax = 0;
  for (const FillEnt& e : ents) {
    if (!e.p || e.bytes == 0) continue;
    if (k == 6 || (e.bytes & 3) || ((uintptr_t)e.p & 3)) return fail(c, SH_ERR_STATE, "fill_list: bad entry");
    L.p[k] = e.p; L.n[k] = e.bytes; L.v[k] = 0x01010101u * e.byte; ++k;
    nmax = std::max(nmax, e.bytes);
  }
  if (k == 0) return SH_OK;
  const unsigned gx = (unsigned)std::min<size_t>(512, std::max<size_t>(1, (nmax / 4 + 256 * 16 - 1) / (256 * 16)));
  LAUNCH(c, "fill", k_fill_list, dim3(gx, (unsigned)k), dim3(256), L);
  return SH_OK;
}

static void drain_timers(sh_ctx* c) {
  for (auto& t : c->pending) {
    float ms = 0;
    (void)hipEventSynchronize(std::get<2>(t));
    if (hipEventElapsedTime(&ms, std::get<1>(t), std::get<2>(t)) == hipSuccess) {
      KTimer& k = c->timers[std::get<0>(t)];
      k.ms += ms;
      k.n += 1;
    }
    (void)hipEventDestroy(std::get<1>(t));
    (void)hipEventDestroy(std::get<2>(t));
  }
  c->pending.clear();
}

static int join_prepared(sh_ctx* c) {
  if (!c->prep.key.active) return SH_OK;
  if (c->prep.th.joinable()) c->prep.th.join();
  c->prep.key.joined();
  if (c->timing) {
    KTimer& h = c->timers["host.hull"]; h.ms += c->prep.hull_ms; h.n += 1;
    if (c->prep.d2h_ms > 0) { KTimer& a = c->timers["host.verts_d2h"]; a.ms += c->prep.d2h_ms; a.n += 1; }
  }
  return c->prep.rc;      // a failed preparation is simply not used: the run repeats the host phase and reports the error itself
}

static void discard_staged(sh_ctx* c) {
  sh_ctx::StageSide& S = c->stg;
  if (!S.active) return;
  if (c->prep.key.staged) { (void)join_prepared(c); c->prep.key.staged_dropped(); }
  (void)hipEventSynchronize(S.ready_ev);      // nothing reads the pinned staging or writes the staging side any more
  S.active = false;
}

// ---------------------------------------------------------------------------------------------
extern "C" {

int sh_default_params(sh_params* p) {
  if (!p) return SH_ERR_ARG;
  *p = sh::default_run_params();
  return SH_OK;
}

}  // extern "C"

// "host" | "device" | "auto" (default).  auto: the host quickhull while this rank has enough usable hardware threads to itself -- 16 when it is
// the only rank of its host, 48 per rank otherwise -- (it
// is free for the GPU and hidden behind the previous step: at ~7 000 humeri/s a rank keeps ~14 cores busy with hulls), the device
// hull otherwise -- 8 ranks on a 256-thread host, a thin host, a rank pinned to a few cores (affinity mask), a cgroup CPU quota.
// Hardware threads this process may actually use: its affinity mask (taskset, a pinned rank, a container's cpuset) capped by a
// cgroup-v2 CPU quota where one is set (cpu.max "<quota> <period>") -- std::thread::hardware_concurrency() sees neither.
static unsigned usable_threads() {
  unsigned n = std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0) n = (unsigned)k; }
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0}; long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
      const long long quota = atoll(q);
      if (quota > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
    }
    fclose(f);
  }
  return n;
}

static unsigned affinity_threads() {
  unsigned n = std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0) n = (unsigned)k; }
  return n;
}

// `sustained`: count a CPU quota (it caps the AVERAGE cpu time -- what decides whether a rank can afford host hulls at all); the size
// of the worker pool goes by the affinity mask alone: a quota does not stop 32 threads from running a 4 ms burst side by side
// (measured under a 16-CPU quota: hull phase of a 64-batch 4.1 ms with 32 workers, 6.3 ms with 16).
unsigned sh::threads_per_local_rank(bool sustained) {
  unsigned hw = sustained ? usable_threads() : affinity_threads();
  if (const char* w = getenv("LOCAL_WORLD_SIZE")) { int v = atoi(w); if (v > 1) hw = std::max(1u, hw / (unsigned)v); }
  return hw;
}

static int hull_mode_from(const char* e) {
  if (e && (e[0] == 'h' || e[0] == '0')) return 0;
  if (e && (e[0] == 'd' || e[0] == '1')) return 1;
  // A rank keeps ~14 cores busy with hulls at ~7 000 humeri/s.  Several ranks on one host: host hull only with >= 48 threads per rank
  // (the ranks' pools and submitting threads must not fight for the cores).  A single rank: >= 16 usable threads are enough --
  // measured under a 16-CPU cgroup quota, B = 64, 20 steps: host hull 7 060 humeri/s (16 workers), device hull 6 720.
  const char* w = getenv("LOCAL_WORLD_SIZE");
  const bool alone = !(w && atoi(w) > 1);
  return threads_per_local_rank() >= (alone ? 16u : 48u) ? 0 : 1;
}

// A page-locked block of the context that holds `need` elements of `bytes_per` bytes: kept when it does, else freed and allocated
// anew with `extra` elements of headroom.  A failure leaves it empty.
template <typename T, typename N>
static int grow_pinned(sh_ctx* c, T** p, N* cap, size_t need, size_t bytes_per, size_t extra = 0) {
  if ((size_t)*cap >= need) return SH_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; *cap = 0;
  HIPCHK(c, hipHostMalloc((void**)p, (need + extra) * bytes_per));
  *cap = (N)(need + extra);
  return SH_OK;
}

// The n pieces of a copy dealt to SH_COPY_THREADS threads of their own (the caller is one; the hull pool's workers may all be inside
// another lane's hull phase): fn(k) copies piece k into page-locked memory and enqueues its H2D copy at once, so the PCIe transfer
// runs behind the memcpy instead of after it.  -> the last error of a piece.
#define SH_COPY_THREADS 4
template <typename F>
static hipError_t copy_pool(size_t n, F fn) {
  std::atomic<size_t> next(0);
  std::atomic<int> err((int)hipSuccess);
  auto work = [&]() {
    for (size_t k; (k = next.fetch_add(1)) < n;) {
      const hipError_t e = fn(k);
      if (e != hipSuccess) err.store((int)e);
    }
  };
  std::vector<std::thread> th;
  for (size_t t = 1; t < SH_COPY_THREADS && t < n; ++t) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return (hipError_t)err.load();
}

extern "C" {

int sh_set_hull_mode(sh_ctx* c, const char* mode) {
  if (!c || !mode) return SH_ERR_ARG;
  if (strcmp(mode, "host") && strcmp(mode, "device") && strcmp(mode, "auto")) return fail(c, SH_ERR_ARG, "sh_set_hull_mode: host | device | auto");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_set_hull_mode: runs are in flight");
  if (c->prep.key.active) { (void)join_prepared(c); c->prep.key.void_hulls(); }
  c->hull_mode = hull_mode_from(strcmp(mode, "auto") ? mode : nullptr);
  return SH_OK;
}

int sh_get_hull_mode(const sh_ctx* c) { return c ? c->hull_mode : SH_ERR_ARG; }
int sh_auto_hull_mode(void) { return hull_mode_from(nullptr); }

int sh_ctx_create(int device, void* hip_stream, sh_ctx** out) {
  if (!out) return SH_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SH_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return SH_ERR_HIP;
  sh_ctx* c = new (std::nothrow) sh_ctx();
  if (!c) return SH_ERR_NOMEM;
  c->device = device;
  c->hull_mode = hull_mode_from(getenv("SHOULDER_HULL"));
  c->unet.reference = getenv("SHOULDER_UNET_REFERENCE") && getenv("SHOULDER_UNET_REFERENCE")[0] == '1';
  {
    auto off = [](const char* n) { const char* e = getenv(n); return e && e[0] == '0'; };
    if (const char* e = getenv("SHOULDER_WINDOW")) { const int v = atoi(e); if (v > 0) c->sw.window = v; }
    c->sw.obb_prune = !off("SHOULDER_OBB_PRUNE");
    c->sw.slice_merge = !off("SHOULDER_SLICE_MERGE");
    c->sw.hull_prefilter = !off("SHOULDER_HULL_PREFILTER");
    c->sw.debug = getenv("SH_DEBUG") != nullptr;
  }
  sh_default_params(&c->params);
  if (hip_stream) c->stream = (hipStream_t)hip_stream;
  else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return SH_ERR_HIP; }
    c->own_stream = true;
  }
  *out = c;
  return SH_OK;
}

void sh_ctx_destroy(sh_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->prep.key.active && c->prep.th.joinable()) c->prep.th.join();
  (void)hipStreamSynchronize(c->stream);
  comm_forget(c);
  unet_turn_forget(c);
  if (c->unet.done_ev) (void)hipEventDestroy(c->unet.done_ev);
  drain_timers(c);
  if (c->stl_counted_ev) (void)hipEventDestroy(c->stl_counted_ev);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->side_stream) { (void)hipStreamSynchronize(c->side_stream); (void)hipStreamDestroy(c->side_stream); }
  if (c->side_fork_ev) (void)hipEventDestroy(c->side_fork_ev);
  if (c->side_join_ev) (void)hipEventDestroy(c->side_join_ev);
  if (c->stg.active) (void)hipEventSynchronize(c->stg.ready_ev);
  if (c->stg.h_src) (void)hipHostFree(c->stg.h_src);
  if (c->stg.h_flag) (void)hipHostFree(c->stg.h_flag);
  if (c->stg.h_kept) (void)hipHostFree(c->stg.h_kept);
  if (c->stg.h_koff) (void)hipHostFree(c->stg.h_koff);
  if (c->stg.ready_ev) (void)hipEventDestroy(c->stg.ready_ev);
  if (c->h_kept) (void)hipHostFree(c->h_kept);
  if (c->h_nkept) (void)hipHostFree(c->h_nkept);
  if (c->h_koff) (void)hipHostFree(c->h_koff);
  if (c->obb_done_ev) (void)hipEventDestroy(c->obb_done_ev);
  for (auto& tk : c->tickets) { if (tk.ev) (void)hipEventDestroy(tk.ev); if (tk.status) (void)hipHostFree(tk.status); }
  if (c->out_stream) (void)hipStreamDestroy(c->out_stream);
  for (auto& kv : c->bufs)
    if (kv.second.p) (void)hipFree(kv.second.p);
  for (auto& hs : c->hstage) {
    if (hs.hv) { (void)hipHostFree(hs.hv); (void)hipHostFree(hs.nr); (void)hipHostFree(hs.ed); (void)hipHostFree(hs.cnt); }
    if (hs.ev) (void)hipEventDestroy(hs.ev);
  }
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* sh_last_error(const sh_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int sh_set_params(sh_ctx* c, const sh_params* p) {
  if (!c || !p) return SH_ERR_ARG;
  const sh::ParamError e = sh::run_params_check(*p);
  if (e.code != SH_OK) return fail(c, e.code, e.text);
  if (c->prep.key.active && p->bone_kind != c->params.bone_kind) (void)join_prepared(c);
  c->params = *p;
  c->batch.params_set();
  return SH_OK;
}

int sh_get_params(const sh_ctx* c, sh_params* out) {
  if (!c || !out) return SH_ERR_ARG;
  *out = c->params;
  return SH_OK;
}

int sh_batch_size(const sh_ctx* c) { return c ? c->B : 0; }

// ---- the per-batch buffers of the stage runner: one statement each ---------------------------------------------------------------
// X(field, "name", element type, elements per humerus).  The name is what sh_fetch / sh_store / sh_buffer_info see.  Allocation
// (alloc_batch, alloc_prox, grow_hull_records: [B] x elements x sizeof(type), window stride = one humerus' bytes) and the typed view
// of a window (WinView, below) both come from these lists, so a kernel argument has the type its buffer was sized with.
// `c` is the context where a list is expanded (the hull record's and the end sections' capacities are its fields).
#define WIN_HULLCAP_BUFS(X) /* strided by c->hcap: grow_hull_records re-allocates exactly these */                                  \
  X(hull_hv, "hull.hv", double, (size_t)c->hcap.v * 3) X(hull_normals, "hull.normals", double, (size_t)c->hcap.f * 3)              \
  X(hull_edges, "hull.edges", int, (size_t)c->hcap.e * 4) X(obb_cand_vol, "obb.cand_vol", double, c->hcap.f)                       \
  X(obb_cand_edge, "obb.cand_edge", int, c->hcap.f) X(obb_area2, "obb.area2", double, c->hcap.f) X(obb_lb, "obb.lb", double, c->hcap.f) \
  X(obb_dir_list, "obb.dir_list", int, c->hcap.f) X(obb_seeded, "obb.seeded", unsigned char, c->hcap.f)
#define WIN_BATCH_BUFS(X)                                                                                                          \
  X(obb_transform, "obb_transform", double, 16) X(zb_enc, "zb_enc", unsigned long long, 2) X(z_bounds, "z_bounds", double, 2)      \
  X(z_length, "z_length", double, 1) X(err, "err", int, 1)                                                                         \
  X(open_stats, "open.stats", int, 2) /* chains bridged / dropped per humerus (sh_open_contour_stats) */                           \
  X(neck_z, "neck_z", double, 1) X(neck_index, "neck_index", int, 1)                                                               \
  X(canal_points_obb, "canal.points_obb", double, SH_CANAL_MAXPTS * 3) X(canal_axis_obb, "canal.axis_obb", double, 6)              \
  X(canal_axis_ct, "canal.axis_ct", double, 6) X(landmarks, "landmarks", sh_landmarks, 1)                                          \
  X(prox_ixy, "prox.ixy", double, (size_t)SH_NPROX * 2 * SH_MPROX) X(prox_itr_start, "prox.itr_start", double, (size_t)SH_NPROX * 2 * SH_MPROX) \
  X(prox_itr_centered_start, "prox.itr_centered_start", double, (size_t)SH_NPROX * 2 * SH_MPROX)                                   \
  /* groove */                                                                                                                     \
  X(groove_xraw, "groove.xraw", double, SH_GSLOTS * 9) X(groove_xs, "groove.xs", double, SH_GSLOTS * 9)                            \
  X(groove_ptheta, "groove.ptheta", double, SH_GSLOTS) X(groove_npk, "groove.npk", int, SH_GROOVE_NROWS)                           \
  X(groove_r0, "groove.r0", double, (size_t)SH_GROOVE_NROWS * SH_MPROX) X(groove_stats, "groove.stats", double, 18)                \
  X(groove_proba, "groove.proba", float, SH_GSLOTS) X(groove_slots, "groove.slots", int, SH_GSLOTS)                                \
  X(groove_nslot, "groove.nslot", int, 1) X(groove_bg_theta, "groove.bg_theta", double, 1)                                         \
  X(groove_local_idx, "groove.local_idx", int, SH_GROOVE_NROWS) X(groove_points_obb, "groove.points_obb", double, SH_GROOVE_NROWS * 3) \
  X(groove_points_ct, "groove.points_ct", double, SH_GROOVE_NROWS * 3) X(groove_axis_ct, "groove.axis_ct", double, 6)              \
  /* anatomic neck */                                                                                                              \
  X(anp_raw, "anp.raw", double, SH_IMG) X(anp_t01, "anp.t01", double, SH_ANP_ROWS * 2) X(anp_roll, "anp.roll", int, SH_ANP_ROWS)   \
  X(anp_maskbits, "anp.maskbits", unsigned long long, SH_ANP_ROWS * (SH_MPROX / 64)) X(anp_mm_enc, "anp.mm_enc", unsigned long long, 2) \
  X(metrics_partial, "metrics.partial", double, SH_SPH_PARTS * 14) X(anp_image, "anp.image", float, SH_IMG)                        \
  X(anp_logits, "anp.logits", float, SH_IMG) X(anp_points_obb, "anp.points_obb", double, SH_ANP_CAP * 3)                           \
  X(anp_counts, "anp.counts", int, 2) X(anp_rowcnt, "anp.rowcnt", int, SH_ANP_ROWS * 2) X(anp_ray_t, "anp.ray_t", unsigned long long, 4) \
  X(anp_plane, "anp.plane", double, 6) X(anp_axes_obb, "anp.axes_obb", double, 12)                                                 \
  /* trans-epicondylar */                                                                                                          \
  X(te_rects, "te.rects", double, SH_TE_NROWS * 7) X(te_axis_ct, "te.axis_ct", double, 6) X(te_ends_ct, "te.ends_ct", double, 6)   \
  X(te_row, "te.row", int, 1) X(flipped, "flipped", int, 1)                                                                        \
  /* oriented bounding box */                                                                                                      \
  WIN_HULLCAP_BUFS(X) X(hull_nv, "hull.nv", int, 1) X(hull_nf, "hull.nf", int, 1) X(hull_ne, "hull.ne", int, 1)                    \
  X(obb_best_enc, "obb.best_enc", unsigned long long, 1) X(obb_lbmin_enc, "obb.lbmin_enc", unsigned long long, 1)                  \
  X(obb_dir_count, "obb.dir_count", int, 1) X(obb_T_pre, "obb.T_pre", double, 16) X(obb_zb_pre, "obb.zb_pre", double, 2)           \
  X(obb_endpts, "obb.endpts", double, (size_t)2 * c->batch.caps().end * 2) X(obb_endcnt, "obb.endcnt", int, 2) X(obb_resid, "obb.resid", double, 2)
// the SH_BONE_PROXIMAL path's own (alloc_prox, on first use; null in the view of a context that never took it): the cut-off of the
// ProxObb area scan and the large Gram matrix of the neck change point
#define WIN_PROX_BUFS(X)                                                                                                           \
  X(pobb_cutoff, "pobb.cutoff", double, 2) X(pobb_cutoff_idx, "pobb.cutoff_idx", int, 2) X(neck_gram, "neck.gram", double, (size_t)SH_NFULL * SH_NFULL)
// not per humerus (window stride 0) or allocated elsewhere (the mesh: upload / commit; the demand block: ovf_pools): X(field, "name", type)
#define WIN_OTHER_BUFS(X)                                                                                                          \
  X(verts, "verts", float) X(faces, "faces", int) X(voff, "voff", long long) X(foff, "foff", long long)                            \
  X(verts_obb, "verts_obb", double) X(verts_csys, "verts_csys", double) X(slices_nlarge, "slices.nlarge", int)                     \
  X(ovf_ctr, "ovf.ctr", unsigned long long)

// The slice sets share one list of arrays: X(field, ".suffix", element type, elements per plane, which sets have it)
#define SLICE_SET_ARRAYS(X)                                                                                                        \
  X(zs, ".zs", double, 1, true) X(zeff, ".zeff", double, 1, true) X(seg_count, ".seg_count", int, 1, true)                         \
  X(segs, ".segs", Seg, SH_MAXSEG, true) X(centroids, ".centroids", double, 2, true) X(areas, ".areas", double, 1, true)           \
  X(nloops, ".nloops", int, 1, true) X(ring_n, ".ring_n", int, 1, true) X(ring, ".ring", double, (SH_MAXSEG + 1) * 2, s.ring)      \
  X(area_total, ".area_total", double, 1, s.total_area)
enum SetId { SET_FULL, SET_DISTAL, SET_PROX, SET_NECKC, SET_POBB, SET_COUNT };
struct SliceSetDef { const char* pfx; int N; bool ring /*keeps the largest loop's ring*/, total_area, prox_only /*allocated by alloc_prox*/; };
static const SliceSetDef SLICE_SETS[SET_COUNT] = {{"full", SH_NFULL, false, false, false}, {"distal", SH_NDIST, true, false, false},
                                                  {"prox", SH_NPROX, true, false, false}, {"neckc", 1, true, false, false},
                                                  {"pobb", SH_NPSCAN, false, true, true}};
#define X(f, sfx, T, n, has) T* f = nullptr;
struct SliceSetView { SLICE_SET_ARRAYS(X) };      // (an array the set does not have: null)
#undef X

// A window's buffers as typed pointers, the window offset applied as buf<T>() applies it (b0 * per_mesh).  RULE: resolved once, at
// the top of run_window (alloc_prox, the pools' first allocation and anything between runs -- sh_collect's regrowth, sh_commit_staged,
// alloc_batch -- lie in front of that), and resolved AGAIN behind the one thing that re-allocates its buffers inside a window:
// grow_hull_records (obb_hulls of run_obb does so; that is why they alone take the view non-const).  What is ensured where it is used stays out of
// the view and is resolved behind its ensure(): the overflow pools and plan arrays (ovf_pools / ovf_set), "obb.ws_*", "rfc.nodes";
// so does the device hull's scratch, which run_device_hull owns.  The view is the calling thread's; background threads get pointers by value.
#define X(f, name, T, ...) T* f = nullptr;
struct WinView {
  int B = 0;      // humeri in the window
  WIN_OTHER_BUFS(X) WIN_BATCH_BUFS(X) WIN_PROX_BUFS(X)
  SliceSetView set[SET_COUNT];
  HullRec hull() const { return {hull_hv, hull_normals, hull_edges, hull_nv, hull_nf, hull_ne}; }
};
#undef X
static WinView win_view(sh_ctx* c) {
  WinView v;
  v.B = c->Bwin;
#define X(f, name, T, ...) v.f = buf<T>(c, name);
  WIN_OTHER_BUFS(X) WIN_BATCH_BUFS(X) WIN_PROX_BUFS(X)
#undef X
  for (int i = 0; i < SET_COUNT; ++i) {
    const std::string p = SLICE_SETS[i].pfx;
#define X(f, sfx, T, n, has) v.set[i].f = buf<T>(c, (p + sfx).c_str());
    SLICE_SET_ARRAYS(X)
#undef X
  }
  return v;
}

// ---- meshes ------------------------------------------------------------------------------------
#define WIN_ENS(f, name, T, n) ENS_(name, (size_t)c->B * (size_t)(n) * sizeof(T), elem_of<T>(), (size_t)(n) * sizeof(T));
static int alloc_slice_set(sh_ctx* c, const SliceSetDef& s) {
  int rc;
  const std::string p = s.pfx;
#define X(f, sfx, T, n, has) if (has) WIN_ENS(f, (p + sfx).c_str(), T, (size_t)s.N * (n))
  SLICE_SET_ARRAYS(X)
#undef X
  return SH_OK;
}

static int alloc_batch(sh_ctx* c) {
  const int B = c->B;
  int rc;
  ENS_SHARED("verts_obb", c->sumV * 3 * 8, 8);        // ragged: indexed through voff
  ENS_SHARED("verts_csys", c->sumV * 3 * 8, 8);
  ENS_SHARED("slices.nlarge", 64, 4);
  c->bufs["voff"].per_mesh = 8;             // a window sees voff[b0 + b] (absolute vertex offsets) as voff[b]
  c->bufs["foff"].per_mesh = 8;
  c->b0 = 0; c->Bwin = B;
  WIN_BATCH_BUFS(WIN_ENS)
  for (const SliceSetDef& s : SLICE_SETS)
    if (!s.prox_only && (rc = alloc_slice_set(c, s)) != SH_OK) return rc;
  HIPCHK(c, hipMemsetAsync(buf<int>(c, "flipped"), 0, (size_t)B * 4, c->stream));
  if ((rc = alloc_hullpre(c, B, c->sumV, "")) != SH_OK) return rc;
  if ((rc = grow_pinned(c, &c->h_kept, &c->h_kept_cap, (size_t)c->sumV, 12)) != SH_OK) return rc;
  if ((rc = grow_pinned(c, &c->h_nkept, &c->h_nkept_cap, (size_t)B, 4)) != SH_OK) return rc;
  if ((rc = grow_pinned(c, &c->h_koff, &c->h_koff_cap, (size_t)B + 1, 8)) != SH_OK) return rc;
  c->batch.batch_resident();
  return SH_OK;
}

// Extra buffers of the SH_BONE_PROXIMAL path (allocated on first use): the ProxObb area scan and the large Gram matrix
// of the neck change point.
static int alloc_prox(sh_ctx* c) {
  int rc;
  for (const SliceSetDef& s : SLICE_SETS)
    if (s.prox_only && (rc = alloc_slice_set(c, s)) != SH_OK) return rc;
  WIN_PROX_BUFS(WIN_ENS)
  return SH_OK;
}

// ---- ingest: one STL scratch view, one parse chain, one commit (the decisions are sh_ingest.h's) ---------------------------------
// the eleven stl.* scratch buffers of a plan as typed device pointers, resolved once
struct StlView { unsigned char* raw; long long *file_off, *coff; float* corners; int2* table; int *slot, *vid, *fpos, *counts, *bsum, *nonfinite; };

static int stl_scratch(sh_ctx* c, int B, const StlPlan& p, StlView* v) {
  int rc;
  ENS_SHARED("stl.raw", (size_t)p.file_off[B], 1);
  ENS_SHARED("stl.file_off", (B + 1) * 8, 8);
  ENS_SHARED("stl.coff", (B + 1) * 8, 8);
  ENS_SHARED("stl.corners", (size_t)p.sumC * 12, 4);
  ENS_SHARED("stl.table", (size_t)B * p.tsize * 8, 4);
  ENS_SHARED("stl.slot", (size_t)p.sumC * 4, 4);
  ENS_SHARED("stl.vid", (size_t)p.sumC * 4, 4);
  ENS_SHARED("stl.fpos", (size_t)(p.sumC / 3) * 4, 4);
  ENS_SHARED("stl.counts", (size_t)B * 8, 4);
  ENS_SHARED("stl.bsum", stl_rank_scratch_ints(B, p.maxc) * 4, 4);
  ENS_SHARED("stl.nonfinite", (size_t)B * 4, 4);
  *v = StlView{(unsigned char*)c->at("stl.raw"), (long long*)c->at("stl.file_off"), (long long*)c->at("stl.coff"), (float*)c->at("stl.corners"), (int2*)c->at("stl.table"),
               (int*)c->at("stl.slot"), (int*)c->at("stl.vid"), (int*)c->at("stl.fpos"), (int*)c->at("stl.counts"), (int*)c->at("stl.bsum"), (int*)c->at("stl.nonfinite")};
  return SH_OK;
}

// A launch of the parse chain on stream `st`.  `timed` = the context whose stream `st` is (sh_upload_stl): the launch goes through
// LAUNCH_FN, so with timing on it is recorded under its name; null (the staged batch's thread, on the copy stream): a bare launch that
// touches nothing of the context -- `pending` belongs to the caller's thread -- and whose error the enqueueing function collects once.
#define STL_LAUNCH(name, kernel, grid, ...)                                                                          \
  do {                                                                                                               \
    if (timed) LAUNCH_FN(timed, name, hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, __VA_ARGS__));              \
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, __VA_ARGS__);                                            \
  } while (0)
static dim3 stl_corner_grid(int B, const StlPlan& p) { return dim3((unsigned)std::min<long long>((p.maxc + 255) / 256, 1024), (unsigned)B); }

// raw files -> corners -> hash table -> ranks: afterwards "stl.counts" holds the merged sizes and "stl.nonfinite" the NaN / inf words
static int stl_enqueue_parse(sh_ctx* timed, hipStream_t st, int B, const StlPlan& p, const StlView& v, std::string* et) {
  HIPCHK_TXT(et, hipMemsetAsync(v.nonfinite, 0, (size_t)B * 4, st));
  const dim3 gc = stl_corner_grid(B, p);
  STL_LAUNCH("k_stl_corners", k_stl_corners, gc, (const unsigned char*)v.raw, (const long long*)v.file_off, (const long long*)v.coff, v.corners, v.nonfinite);
  STL_LAUNCH("k_stl_table_init", k_stl_table_init, dim3(1024), v.table, (size_t)B * p.tsize);
  STL_LAUNCH("k_stl_hash", k_stl_hash, gc, (const float*)v.corners, (const long long*)v.coff, v.table, p.tsize, v.slot);
  stl_rank_launch(st, B, p.maxc, v.coff, v.table, p.tsize, v.slot, v.vid, v.fpos, v.counts, v.bsum);
  HIPCHK_TXT(et, hipGetLastError());
  return SH_OK;
}

// the merged meshes to their batch offsets (already on the device behind voff / foff)
static int stl_enqueue_emit(sh_ctx* timed, hipStream_t st, int B, const StlPlan& p, const StlView& v, const long long* voff, const long long* foff, float* verts, int* faces, std::string* et) {
  STL_LAUNCH("k_stl_emit", k_stl_emit, stl_corner_grid(B, p), (const float*)v.corners, (const long long*)v.coff, (const int2*)v.table, p.tsize, (const int*)v.slot,
             (const int*)v.vid, (const int*)v.fpos, voff, foff, verts, faces);
  HIPCHK_TXT(et, hipGetLastError());
  return SH_OK;
}
#undef STL_LAUNCH

// "ray.near" (sh_ray_nearest), "cp.out" (sh_closest_points), "wn.out" (sh_winding_numbers), "icp.out" and "icp.near" (sh_register_points), "mass.out" and "mass.part"
// (sh_mass_properties), "samp.*" (sh_sample_surface), "topo.*" (sh_mesh_topology), "vert.*" (sh_vertex_fields), "geo.*" (sh_geodesic), "smooth.*" (sh_smooth_vertices), "repair.*" (sh_mesh_repair), "simp.*" (sh_mesh_simplify: the list SIMPLIFY_BUFS of sh_query.h and the sorts' "simp.tmp"), "bvh.*" (sh_mesh_bvh) answer for the batch they were asked about: a new batch removes them
static void drop_closest(sh_ctx* c) {
  for (const char* name : {"ray.near", "cp.out", "wn.out", "icp.out", "icp.near", "mass.out", "mass.part", "samp.cdf", "samp.base", "samp.out", "samp.info", "samp.state",
                           "topo.vrow", "topo.vface", "topo.adj", "topo.label", "topo.info", "topo.shells", "topo.state", "topo.cursor", "topo.tmp", "topo.p",
                           "vert.face", "vert.normal", "vert.fields", "vert.flags", "vert.status", "vert.a2", "vert.plane", "vert.state",
                           "geo.face", "geo.dist", "geo.pred", "geo.source", "geo.info", "geo.opp", "geo.plane", "geo.jump", "geo.src", "geo.d0", "geo.state",
                           "smooth.nrow", "smooth.nbr", "smooth.w", "smooth.pos", "smooth.info", "smooth.plane", "smooth.pin", "smooth.mask", "smooth.part",
                           "repair.flip", "repair.faces", "repair.verts", "repair.info", "repair.shells", "repair.holes", "repair.off", "repair.par", "repair.work", "repair.edge",
                           "repair.term",
#define X(f, name, T, elem) name,
                           SIMPLIFY_BUFS(X)
#undef X
                           "simp.tmp",
                           "bvh.order", "bvh.loose", "bvh.off", "bvh.box", "bvh.tri", "bvh.info", "bvh.state", "bvh.base", "bvh.seg", "bvh.key", "bvh.sorted", "bvh.tmp"}) {
    auto it = c->bufs.find(name);
    if (it == c->bufs.end()) continue;
    if (it->second.p) (void)hipFree(it->second.p);
    c->bufs.erase(it);
  }
}

// Where the meshes of a batch that becomes resident are: host arrays to upload (sh_upload_meshes) | `fill` writes "verts" / "faces" on
// the context's stream once they and the offsets are in place (STL, synth) | `staged`: the ".s" side holds them, swap it in.
struct ResidentSource { const float* verts = nullptr; const int32_t* faces = nullptr; std::function<int()> fill; bool staged = false; };

// The commit of every way in.  voff / foff are swapped into the context.  A failure behind `c->B = 0` leaves "no meshes uploaded",
// never a half-committed batch; h_verts_valid only for host arrays (else the hull stage downloads the vertices).
static int make_resident(sh_ctx* c, int B, const MeshSizes& sz, std::vector<long long>& voff, std::vector<long long>& foff, const ResidentSource& src) {
  static const char* const names[4] = {"verts", "faces", "voff", "foff"};
  if (src.staged) for (const char* nm : names) std::swap(c->bufs[nm], c->bufs[std::string(nm) + ".s"]);      // (the staged batch's own thread keeps running)
  else { discard_staged(c); (void)join_prepared(c); }      // (sh_upload_stl dropped a staged batch already, before it took the stl.* scratch: nothing left to do for it here)
  ++c->batch_gen;      // hulls prepared for the previous batch are void
  drop_closest(c);
  c->B = 0;
  c->h_voff.swap(voff); c->h_foff.swap(foff);
  c->sumV = sz.sumV; c->sumF = sz.sumF; c->maxV = sz.maxV; c->maxF = sz.maxF;
  c->h_verts_valid = src.verts != nullptr;
  if (src.verts) c->h_verts.assign(src.verts, src.verts + 3 * sz.sumV);
  int rc;
  if (!src.staged) {
    const size_t nb[4] = {(size_t)sz.sumV * 12, (size_t)sz.sumF * 12, (size_t)(B + 1) * 8, (size_t)(B + 1) * 8};
    for (int k = 0; k < 4; ++k) if ((rc = ensure(c, names[k], nb[k], k < 2 ? 4 : 8)) != SH_OK) return rc;
    if (src.verts) {
      HIPCHK(c, hipMemcpyAsync(c->bufs["verts"].p, src.verts, nb[0], hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(c->bufs["faces"].p, src.faces, nb[1], hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->bufs["voff"].p, c->h_voff.data(), nb[2], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->bufs["foff"].p, c->h_foff.data(), nb[3], hipMemcpyHostToDevice, c->stream));
    if (src.fill && (rc = src.fill()) != SH_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  for (const char* nm : {"verts", "faces", "verts.s", "faces.s", "voff.s", "foff.s"}) { auto it = c->bufs.find(nm); if (it != c->bufs.end()) it->second.per_mesh = 0; }
  c->B = B;
  if ((rc = alloc_batch(c)) != SH_OK) c->B = 0;      // (voff / foff get their window stride there)
  return rc;
}

static int ingest_fail(sh_ctx* c, const char* entry, const IngestError& e) { return fail(c, e.code, std::string(entry) + ": " + e.text); }
static void offsets_out(const std::vector<long long>& off, int64_t* out) { if (out) std::copy(off.begin(), off.end(), out); }

int sh_upload_meshes(sh_ctx* c, const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int B) {
  if (!c || !verts || !faces || !v_off || !f_off || B <= 0) return fail(c, SH_ERR_ARG, "sh_upload_meshes: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  // Validate first, into locals: a rejected upload leaves the resident batch (B, offsets, device buffers) untouched.
  MeshSizes sz;
  const IngestError e = check_mesh_arrays(v_off, f_off, B, faces, verts, &sz);
  if (e.code != SH_OK) return ingest_fail(c, "sh_upload_meshes", e);
  std::vector<long long> voff(v_off, v_off + B + 1), foff(f_off, f_off + B + 1);
  ResidentSource src;
  src.verts = verts; src.faces = faces;
  return make_resident(c, B, sz, voff, foff, src);
}

// Binary STL files -> merged meshes, on the device (k_stl.h; replaces `trimesh.load_mesh(stl)` of mesh.py:22-27 incl. the
// vertex merge).  The host only checks the 84-byte headers and sums sizes.
int sh_upload_stl(sh_ctx* c, const void* const* files, const size_t* nbytes, int B, int64_t* v_off_out, int64_t* f_off_out) {
  if (!c || !files || !nbytes || B <= 0) return fail(c, SH_ERR_ARG, "sh_upload_stl: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  discard_staged(c);      // (a staged STL batch works in the same stl.* scratch)
  StlPlan plan;
  IngestError e = stl_plan(files, nbytes, B, &plan);
  if (e.code != SH_OK) return ingest_fail(c, "sh_upload_stl", e);
  StlView v;
  int rc;
  if ((rc = stl_scratch(c, B, plan, &v)) != SH_OK) return rc;
  for (int b = 0; b < B; ++b) HIPCHK(c, hipMemcpyAsync(v.raw + plan.file_off[b], files[b], nbytes[b], hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.file_off, plan.file_off.data(), (B + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.coff, plan.coff.data(), (B + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if ((rc = stl_enqueue_parse(c, c->stream, B, plan, v, &c->err)) != SH_OK) return rc;
  std::vector<int> counts(2 * B), nonfin(B);
  HIPCHK(c, hipMemcpyAsync(counts.data(), v.counts, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(nonfin.data(), v.nonfinite, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // Validate into locals: a rejected file set leaves the resident batch (B, offsets, "verts" / "faces") untouched -- only
  // the stl.* scratch buffers were written so far.
  std::vector<long long> voff, foff;
  MeshSizes sz;
  e = stl_counted(counts.data(), nonfin.data(), B, &voff, &foff, &sz);
  if (e.code != SH_OK) return ingest_fail(c, "sh_upload_stl", e);
  ResidentSource src;
  src.fill = [&]() -> int { return stl_enqueue_emit(c, c->stream, B, plan, v, (const long long*)c->bufs["voff"].p, (const long long*)c->bufs["foff"].p, (float*)c->bufs["verts"].p, (int*)c->bufs["faces"].p, &c->err); };
  if ((rc = make_resident(c, B, sz, voff, foff, src)) != SH_OK) return rc;
  offsets_out(c->h_voff, v_off_out); offsets_out(c->h_foff, f_off_out);
  return SH_OK;
}

int sh_synth_batch(sh_ctx* c, const double* T, int B) {
  if (!c || !T || B <= 0) return fail(c, SH_ERR_ARG, "sh_synth_batch: bad argument");
  if (c->B < 1) return fail(c, SH_ERR_STATE, "sh_synth_batch: upload a template mesh first");
  HIPCHK(c, hipSetDevice(c->device));
  const long long V = c->h_voff[1] - c->h_voff[0], F = c->h_foff[1] - c->h_foff[0];
  // keep the template aside
  int rc;
  if ((rc = ensure(c, "tmpl_verts", V * 3 * 4, 4)) != SH_OK) return rc;
  if ((rc = ensure(c, "tmpl_faces", F * 3 * 4, 4)) != SH_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(buf<float>(c, "tmpl_verts"), buf<float>(c, "verts") + 3 * c->h_voff[0], V * 3 * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(buf<int>(c, "tmpl_faces"), buf<int>(c, "faces") + 3 * c->h_foff[0], F * 3 * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<long long> voff(B + 1), foff(B + 1);
  for (int b = 0; b <= B; ++b) { voff[b] = V * b; foff[b] = F * b; }
  MeshSizes sz;
  sz.sumV = V * B; sz.sumF = F * B; sz.maxV = V; sz.maxF = F;
  ResidentSource src;
  src.fill = [&]() -> int {
    int rc;
    if ((rc = ensure(c, "synth_T", B * 16 * 8, 8)) != SH_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(buf<double>(c, "synth_T"), T, B * 16 * 8, hipMemcpyHostToDevice, c->stream));
    dim3 grid((unsigned)((V + 255) / 256), (unsigned)B);
    LAUNCH(c, "k_synth_batch", k_synth_batch, grid, dim3(256), buf<float>(c, "tmpl_verts"), buf<int>(c, "tmpl_faces"),
           (long long)V, (long long)F, buf<double>(c, "synth_T"), buf<float>(c, "verts"), buf<int>(c, "faces"));
    return SH_OK;
  };
  return make_resident(c, B, sz, voff, foff, src);
}

// ---- named buffers -----------------------------------------------------------------------------
int sh_buffer_info(sh_ctx* c, const char* name, size_t* nbytes, int* elem) {
  if (!c || !name) return SH_ERR_ARG;
  auto it = c->bufs.find(name);
  if (it == c->bufs.end()) return fail(c, SH_ERR_ARG, std::string("no buffer named ") + name);
  if (nbytes) *nbytes = it->second.bytes;
  if (elem) *elem = it->second.elem;
  return SH_OK;
}

int sh_buffer_device(sh_ctx* c, const char* name, void** dev_ptr, size_t* nbytes) {
  if (!c || !name || !dev_ptr) return SH_ERR_ARG;
  auto it = c->bufs.find(name);
  if (it == c->bufs.end() || !it->second.p) return fail(c, SH_ERR_ARG, std::string("no buffer named ") + name);
  *dev_ptr = it->second.p;
  if (nbytes) *nbytes = it->second.bytes;
  if (std::string(name) == "params") c->pstate.block_exposed();      // (the caller may write it)
  c->batch.buffer_touched(name, false);      // (... or a frame / an intermediate that moves the planes: the overflow tier runs again)
  return SH_OK;
}

int sh_fetch(sh_ctx* c, const char* name, void* host, size_t nbytes) {
  if (!c || !name || !host) return SH_ERR_ARG;
  auto it = c->bufs.find(name);
  if (it == c->bufs.end()) return fail(c, SH_ERR_ARG, std::string("no buffer named ") + name);
  if (nbytes > it->second.bytes) return fail(c, SH_ERR_ARG, std::string("sh_fetch: size exceeds buffer ") + name);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(host, it->second.p, nbytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_store(sh_ctx* c, const char* name, const void* host, size_t nbytes) {
  if (!c || !name || !host) return SH_ERR_ARG;
  auto it = c->bufs.find(name);
  if (it == c->bufs.end()) return fail(c, SH_ERR_ARG, std::string("no buffer named ") + name);
  if (nbytes > it->second.bytes) return fail(c, SH_ERR_ARG, std::string("sh_store: size exceeds buffer ") + name);
  HIPCHK(c, hipSetDevice(c->device));
  if (std::string(name) == "verts") { discard_staged(c); (void)join_prepared(c); ++c->batch_gen; c->h_verts_valid = false; drop_closest(c); }
  c->batch.buffer_touched(name, false);      // (an injected frame or intermediate moves the planes: the overflow tier runs again)
  if (std::string(name) == "params") c->pstate.block_exposed();
  HIPCHK(c, hipMemcpyAsync(it->second.p, host, nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch.buffer_touched(name, true);
  return SH_OK;
}

// ---- timing ------------------------------------------------------------------------------------
int sh_enable_timing(sh_ctx* c, int on) {
  if (!c) return SH_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  drain_timers(c);
  c->timing = on < 0 ? 0 : (on > 2 ? 1 : on);
  return SH_OK;
}

int sh_kernel_time_ms(sh_ctx* c, const char* kernel, double* avg_ms, int* launches) {
  if (!c) return SH_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  drain_timers(c);
  if (!kernel) { c->timers.clear(); return SH_OK; }
  auto it = c->timers.find(kernel);
  if (it == c->timers.end() || it->second.n == 0) { if (avg_ms) *avg_ms = 0; if (launches) *launches = 0; return SH_OK; }
  if (avg_ms) *avg_ms = it->second.ms / it->second.n;
  if (launches) *launches = it->second.n;
  return SH_OK;
}

// ---- affine --------------------------------------------------------------------------------------
int sh_affine_apply(sh_ctx* c, const double* T, const void* dev_in, void* dev_out, const int64_t* off, int B) {
  if (!c || !T || !dev_in || !dev_out || !off || B <= 0) return fail(c, SH_ERR_ARG, "sh_affine_apply: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, "aff_T", B * 16 * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "aff_off", (B + 1) * 8, 8)) != SH_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(buf<double>(c, "aff_T"), T, B * 16 * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(buf<long long>(c, "aff_off"), off, (B + 1) * 8, hipMemcpyHostToDevice, c->stream));
  long long mx = 0;
  for (int b = 0; b < B; ++b) mx = std::max<long long>(mx, off[b + 1] - off[b]);
  dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((mx + 255) / 256, 1024)), (unsigned)B);
  LAUNCH(c, "k_affine_f64", k_affine_f64, grid, dim3(256), buf<double>(c, "aff_T"), (const double*)dev_in, (double*)dev_out,
         buf<long long>(c, "aff_off"));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_transform_points(sh_ctx* c, const double* T, const double* in, int n, double* out) {
  if (!c || !T || !in || !out || n < 0) return fail(c, SH_ERR_ARG, "sh_transform_points: bad argument");
  if (n == 0) return SH_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, "tp_T", 16 * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "tp_io", (size_t)n * 3 * 8 * 2, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "tp_off", 2 * 8, 8)) != SH_OK) return rc;
  long long off[2] = {0, n};
  double* io = buf<double>(c, "tp_io");
  HIPCHK(c, hipMemcpyAsync(buf<double>(c, "tp_T"), T, 16 * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(buf<long long>(c, "tp_off"), off, 16, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(io, in, (size_t)n * 3 * 8, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_affine_f64", k_affine_f64, dim3((unsigned)std::min(1024, (n + 255) / 256), 1), dim3(256), buf<double>(c, "tp_T"), io, io + (size_t)n * 3,
         buf<long long>(c, "tp_off"));
  HIPCHK(c, hipMemcpyAsync(out, io + (size_t)n * 3, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// The closed largest loop of plane k of slice set `set` ("full" has none; "distal", "prox", "neckc") of humerus b after a run:
// n + 1 points (x, y) in the box frame, CCW, canonical start, first = last.  From the fixed slot range or, for a plane with more
// crossings than slots, from the overflow pool (k_ovf.h).  out == NULL or cap too small: *n_out = n + 1, nothing copied.
int sh_ring(sh_ctx* c, const char* set, int b, int k, double* out, int cap, int* n_out) {
  if (!c || !set || !n_out) return fail(c, SH_ERR_ARG, "sh_ring: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const std::string p = set;
  auto itn = c->bufs.find(p + ".ring_n");
  auto itr = c->bufs.find(p + ".ring");
  if (itn == c->bufs.end() || itr == c->bufs.end() || !itr->second.p) return fail(c, SH_ERR_ARG, "sh_ring: no such slice set with rings");
  const int N = (int)(itn->second.per_mesh / 4);
  if (b < 0 || b >= c->B || k < 0 || k >= N) return fail(c, SH_ERR_ARG, "sh_ring: index out of range");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t pl = (size_t)b * N + k;
  int n = 0;
  HIPCHK(c, hipMemcpy(&n, (const int*)itn->second.p + pl, 4, hipMemcpyDeviceToHost));
  *n_out = n + 1;
  if (!out || cap < n + 1) return SH_OK;
  long long roff = -1;
  if (const long long* d_roff = (const long long*)c->at((p + ".ovf_roff").c_str())) HIPCHK(c, hipMemcpy(&roff, d_roff + pl, 8, hipMemcpyDeviceToHost));
  const double* src = roff >= 0 ? (const double*)c->bufs["ovf.ring"].p + 2 * roff : (const double*)itr->second.p + pl * (SH_MAXSEG + 1) * 2;
  HIPCHK(c, hipMemcpy(out, src, (size_t)(n + 1) * 16, hipMemcpyDeviceToHost));
  return SH_OK;
}

int sh_section_plane(sh_ctx* c, int b, const double* origin, const double* normal, double* out_pts, int cap, int* n_out) {
  if (!c || !origin || !normal || !out_pts || !n_out || cap <= 0 || b < 0 || b >= c->B) return fail(c, SH_ERR_ARG, "sh_section_plane: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  double pl[6] = {origin[0], origin[1], origin[2], normal[0], normal[1], normal[2]};
  double nn = std::sqrt(pl[3] * pl[3] + pl[4] * pl[4] + pl[5] * pl[5]);
  if (!(nn > 0)) return fail(c, SH_ERR_ARG, "sh_section_plane: zero normal");
  for (int k = 3; k < 6; ++k) pl[k] /= nn;
  int rc;
  if ((rc = ensure(c, "sp_plane", 6 * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "sp_out", (size_t)cap * 3 * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "sp_cnt", 4, 4)) != SH_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(buf<double>(c, "sp_plane"), pl, 48, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(buf<int>(c, "sp_cnt"), 0, 4, c->stream));
  long long nf = c->h_foff[b + 1] - c->h_foff[b];
  LAUNCH(c, "k_section_points", k_section_points, dim3((unsigned)std::min<long long>((nf + 255) / 256, 1024)), dim3(256),
         buf<float>(c, "verts") + 3 * c->h_voff[b], buf<int>(c, "faces") + 3 * c->h_foff[b], nf, buf<double>(c, "sp_plane"), buf<double>(c, "sp_out"), cap,
         buf<int>(c, "sp_cnt"));
  int n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, buf<int>(c, "sp_cnt"), 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_out = n;
  if (n > cap) return fail(c, SH_ERR_CAPACITY, "sh_section_plane: more crossing points than capacity");
  HIPCHK(c, hipMemcpy(out_pts, buf<double>(c, "sp_out"), (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
  return SH_OK;
}

// Cut one mesh (host arrays, any coordinate system) with P planes and keep the side each normal points to
// (`Trimesh.slice_plane`, arthroplasty.py:80-87).  out_verts == nullptr: count only (counts[].n_verts = upper bound).
int sh_slice_mesh_planes(sh_ctx* c, const double* verts, int nv, const int32_t* faces, int nf, const double* origins, const double* normals, int P,
                         double* out_verts, int cap_v, int32_t* out_faces, int cap_f, int32_t* out_edges, int cap_e, int32_t* counts) {
  if (!c || !verts || !faces || !origins || !normals || !counts || nv < 1 || nf < 1 || P < 1 || P > 4096)
    return fail(c, SH_ERR_ARG, "sh_slice_mesh_planes: bad argument");
  if (out_verts && (!out_faces || cap_v < 1 || cap_f < 1 || (out_edges && cap_e < 1))) return fail(c, SH_ERR_ARG, "sh_slice_mesh_planes: bad output arguments");
  for (int i = 0; i < 3 * nf; ++i)
    if (faces[i] < 0 || faces[i] >= nv) return fail(c, SH_ERR_ARG, "sh_slice_mesh_planes: face index out of range");
  if ((long long)P * ((long long)nv + 2LL * nf) > (1LL << 30)) return fail(c, SH_ERR_CAPACITY, "sh_slice_mesh_planes: planes x mesh too large for one call");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> pl(6 * (size_t)P);
  for (int p = 0; p < P; ++p) {
    const double* n = normals + 3 * p;
    if (!((n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) > 0)) return fail(c, SH_ERR_ARG, "sh_slice_mesh_planes: zero normal");
    for (int k = 0; k < 3; ++k) { pl[6 * p + k] = origins[3 * p + k]; pl[6 * p + 3 + k] = n[k]; }      // the normal is used as given (trimesh does not normalise it)
  }
  void *d_v, *d_f, *d_pl, *d_sign, *d_cls, *d_fpos, *d_cnt;
  int rc;
  if ((rc = ensure(c, "clip.verts", (size_t)nv * 24, 8, &d_v)) || (rc = ensure(c, "clip.faces", (size_t)nf * 12, 4, &d_f)) ||
      (rc = ensure(c, "clip.planes", (size_t)P * 48, 8, &d_pl)) || (rc = ensure(c, "clip.sign", (size_t)P * nv, 1, &d_sign)) ||
      (rc = ensure(c, "clip.cls", (size_t)P * nf, 1, &d_cls)) || (rc = ensure(c, "clip.fpos", (size_t)P * nf * 4, 4, &d_fpos)) ||
      (rc = ensure(c, "clip.counts", (size_t)P * sizeof(ClipCounts), 4, &d_cnt)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(d_v, verts, (size_t)nv * 24, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_f, faces, (size_t)nf * 12, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_pl, pl.data(), (size_t)P * 48, hipMemcpyHostToDevice, c->stream));
  const unsigned gv = (unsigned)std::min(256, (nv + 255) / 256), gf = (unsigned)std::min(256, (nf + 255) / 256);
  LAUNCH(c, "k_clip_sign", k_clip_sign, dim3(gv, P), dim3(256), (const double*)d_v, nv, (const double*)d_pl, (signed char*)d_sign);
  LAUNCH(c, "k_clip_class", k_clip_class, dim3(P), dim3(SH_STL_SCAN_THREADS), (const double*)d_v, (const int*)d_f, nf, nv, (const double*)d_pl,
         (const signed char*)d_sign, (unsigned char*)d_cls, (int*)d_fpos, (ClipCounts*)d_cnt);
  std::vector<ClipCounts> cn(P);
  HIPCHK(c, hipMemcpyAsync(cn.data(), d_cnt, (size_t)P * sizeof(ClipCounts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  auto report = [&](bool upper) {
    for (int p = 0; p < P; ++p) { counts[3 * p] = upper ? cn[p].n_pre : cn[p].n_verts; counts[3 * p + 1] = cn[p].n_faces; counts[3 * p + 2] = cn[p].n_edges; }
  };
  if (!out_verts) { report(true); return SH_OK; }
  // per-plane offsets of the pre-merge arrays
  std::vector<long long> off(4 * (size_t)(P + 1) + (P + 1), 0);
  long long *new_off = off.data(), *face_off = new_off + (P + 1), *edge_off = face_off + (P + 1), *pre_off = edge_off + (P + 1), *tab_off = pre_off + (P + 1);
  for (int p = 0; p < P; ++p) {
    if (cn[p].n_faces > cap_f || (out_edges && cn[p].n_edges > cap_e)) { report(true); return fail(c, SH_ERR_CAPACITY, "sh_slice_mesh_planes: output capacity too small (counts hold the sizes needed)"); }
    new_off[p + 1] = new_off[p] + 2LL * (cn[p].n_quad + cn[p].n_tri);
    face_off[p + 1] = face_off[p] + cn[p].n_faces;
    edge_off[p + 1] = edge_off[p] + cn[p].n_edges;
    pre_off[p + 1] = pre_off[p] + cn[p].n_pre;
    long long ts = 1024;
    while (ts < 2LL * cn[p].n_pre) ts <<= 1;
    tab_off[p + 1] = tab_off[p] + ts;
  }
  void *d_off, *d_np, *d_pf, *d_pe, *d_ref, *d_keys, *d_tab, *d_slot, *d_vid, *d_ov, *d_of, *d_oe = nullptr;
  if ((rc = ensure(c, "clip.off", off.size() * 8, 8, &d_off)) || (rc = ensure(c, "clip.new_pts", (size_t)std::max(1LL, new_off[P]) * 24, 8, &d_np)) ||
      (rc = ensure(c, "clip.pre_faces", (size_t)std::max(1LL, face_off[P]) * 12, 4, &d_pf)) || (rc = ensure(c, "clip.pre_edges", (size_t)std::max(1LL, edge_off[P]) * 8, 4, &d_pe)) ||
      (rc = ensure(c, "clip.referenced", (size_t)pre_off[P], 1, &d_ref)) || (rc = ensure(c, "clip.keys", (size_t)pre_off[P] * 24, 8, &d_keys)) ||
      (rc = ensure(c, "clip.table", (size_t)tab_off[P] * 8, 8, &d_tab)) || (rc = ensure(c, "clip.slot", (size_t)pre_off[P] * 4, 4, &d_slot)) ||
      (rc = ensure(c, "clip.vid", (size_t)pre_off[P] * 4, 4, &d_vid)) || (rc = ensure(c, "clip.out_verts", (size_t)P * cap_v * 24, 8, &d_ov)) ||
      (rc = ensure(c, "clip.out_faces", (size_t)P * cap_f * 12, 4, &d_of)))
    return rc;
  if (out_edges && (rc = ensure(c, "clip.out_edges", (size_t)P * cap_e * 8, 4, &d_oe))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
  const long long *g_new = (const long long*)d_off, *g_face = g_new + (P + 1), *g_edge = g_face + (P + 1), *g_pre = g_edge + (P + 1), *g_tab = g_pre + (P + 1);
  HIPCHK(c, hipMemsetAsync(d_ref, 0, (size_t)pre_off[P], c->stream));
  LAUNCH(c, "k_stl_table_init", k_stl_table_init, dim3(256), dim3(256), (int2*)d_tab, (size_t)tab_off[P]);
  LAUNCH(c, "k_clip_emit", k_clip_emit, dim3(gf, P), dim3(256), (const double*)d_v, (const int*)d_f, nf, nv, (const double*)d_pl, (const signed char*)d_sign,
         (const unsigned char*)d_cls, (const int*)d_fpos, (const ClipCounts*)d_cnt, g_new, g_face, g_edge, (double*)d_np, (int*)d_pf, (int*)d_pe);
  LAUNCH(c, "k_clip_mark", k_clip_mark, dim3(gf, P), dim3(256), (const int*)d_pf, g_face, g_pre, (unsigned char*)d_ref);
  LAUNCH(c, "k_clip_hash", k_clip_hash, dim3(gv + gf, P), dim3(256), (const double*)d_v, nv, (const double*)d_np, g_new, g_pre, (const unsigned char*)d_ref,
         (long long*)d_keys, (int2*)d_tab, g_tab, (int*)d_slot);
  LAUNCH(c, "k_clip_rank", k_clip_rank, dim3(P), dim3(SH_STL_SCAN_THREADS), g_pre, (const unsigned char*)d_ref, (const int2*)d_tab, g_tab, (const int*)d_slot,
         (int*)d_vid, (ClipCounts*)d_cnt);
  HIPCHK(c, hipMemcpyAsync(cn.data(), d_cnt, (size_t)P * sizeof(ClipCounts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  report(false);
  for (int p = 0; p < P; ++p)
    if (cn[p].n_verts > cap_v) return fail(c, SH_ERR_CAPACITY, "sh_slice_mesh_planes: vertex capacity too small (counts hold the sizes needed)");
  LAUNCH(c, "k_clip_out", k_clip_out, dim3(gv + gf, P), dim3(256), (const double*)d_v, nv, (const double*)d_np, g_new, g_pre, (const unsigned char*)d_ref,
         (const int2*)d_tab, g_tab, (const int*)d_slot, (const int*)d_vid, (const int*)d_pf, g_face, (const int*)d_pe, g_edge, (double*)d_ov, cap_v, (int*)d_of,
         cap_f, (int*)d_oe, cap_e);
  for (int p = 0; p < P; ++p) {
    if (cn[p].n_verts) HIPCHK(c, hipMemcpyAsync(out_verts + 3 * (size_t)p * cap_v, (double*)d_ov + 3 * (size_t)p * cap_v, (size_t)cn[p].n_verts * 24, hipMemcpyDeviceToHost, c->stream));
    if (cn[p].n_faces) HIPCHK(c, hipMemcpyAsync(out_faces + 3 * (size_t)p * cap_f, (int*)d_of + 3 * (size_t)p * cap_f, (size_t)cn[p].n_faces * 12, hipMemcpyDeviceToHost, c->stream));
    if (out_edges && cn[p].n_edges) HIPCHK(c, hipMemcpyAsync(out_edges + 2 * (size_t)p * cap_e, (int*)d_oe + 2 * (size_t)p * cap_e, (size_t)cn[p].n_edges * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- the arthroplasty chain: sh_resect_*, sh_canal_profile, sh_resect_stems, sh_resect_plan (host code; the decisions are sh_arthro.h's) ----
#include "sh_arthro_host.h"
// ---- the queries of the resident batch: rays, closest points, winding numbers, registration, mass properties, surface samples, mesh topology, vertex fields, geodesics (the decisions are sh_query.h's) ----
#include "sh_query_host.h"

int sh_mesh_transformed(sh_ctx* c, int b, const double* T, double* out) {
  if (!c || !T || !out || b < 0 || b >= c->B) return fail(c, SH_ERR_ARG, "sh_mesh_transformed: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  long long V = c->h_voff[b + 1] - c->h_voff[b];
  int rc;
  if ((rc = ensure(c, "mt_T", 16 * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "mt_out", V * 3 * 8, 8)) != SH_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(buf<double>(c, "mt_T"), T, 16 * 8, hipMemcpyHostToDevice, c->stream));
  dim3 grid((unsigned)std::min<long long>((V + 255) / 256, 1024));
  LAUNCH(c, "k_affine_f32in", k_affine_f32in, grid, dim3(256), buf<double>(c, "mt_T"),
         buf<float>(c, "verts") + 3 * c->h_voff[b], buf<double>(c, "mt_out"), V);
  HIPCHK(c, hipMemcpyAsync(out, buf<double>(c, "mt_out"), V * 3 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- stage runner ----------------------------------------------------------------------------------
// ---- overflow planes of the slice layer (k_ovf.h) --------------------------------------------------------
static int ovf_pools(sh_ctx* c, OvfPools* P) {
  int rc;
  const DemandCaps& cap = c->batch.caps();
  if ((rc = ensure(c, "ovf.segs", cap.seg * sizeof(Seg), 1)) != SH_OK) return rc;
  if ((rc = ensure(c, "ovf.ring", cap.ring * 16, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "ovf.work", cap.work, 1)) != SH_OK) return rc;
  if ((rc = ensure(c, "ovf.ctr", SH_NCTR * 8, 8)) != SH_OK) return rc;      // the demand block of a run (sh_demand.h names its words)
  for (const char* n : {"ovf.segs", "ovf.ring", "ovf.work", "ovf.ctr"}) c->bufs[n].per_mesh = 0;
  P->segs = (Seg*)c->bufs["ovf.segs"].p; P->ring = (double*)c->bufs["ovf.ring"].p; P->work = (unsigned char*)c->bufs["ovf.work"].p;
  P->seg_cap = cap.seg; P->ring_cap = cap.ring; P->work_cap = cap.work;
  P->ctr = (unsigned long long*)c->bufs["ovf.ctr"].p;
  P->open_mode = c->open_mode;
  return SH_OK;
}
// the plan arrays of slice set `pfx` (N planes per humerus), window-relative like every [B][...] buffer
static int ovf_set(sh_ctx* c, const std::string& pfx, int N, OvfSet* S) {
  const size_t B = (size_t)c->B;
  int rc;
  struct A { const char* suffix; size_t elem; } arr[6] = {{".ovf_soff", 8}, {".ovf_roff", 8}, {".ovf_woff", 8}, {".ovf_fill", 4}, {".ovf_list", 4}, {".ovf_list2", 4}};
  for (const A& a : arr) {
    const std::string nm = pfx + a.suffix;
    const bool fresh = c->bufs.find(nm) == c->bufs.end() || c->bufs[nm].bytes < B * N * a.elem;
    if ((rc = ensure(c, nm.c_str(), B * N * a.elem, (int)a.elem)) != SH_OK) return rc;
    c->bufs[nm].per_mesh = (size_t)N * a.elem;
    if (fresh) HIPCHK(c, hipMemsetAsync(c->bufs[nm].p, 0xFF, B * N * a.elem, c->stream));      // "no overflow plane" until a plan says otherwise
  }
  if ((rc = ensure(c, (pfx + ".ovf_nlist").c_str(), 16, 4)) != SH_OK) return rc;
  c->bufs[pfx + ".ovf_nlist"].per_mesh = 0;
  S->soff = buf<long long>(c, (pfx + ".ovf_soff").c_str()); S->roff = buf<long long>(c, (pfx + ".ovf_roff").c_str());
  S->woff = buf<long long>(c, (pfx + ".ovf_woff").c_str()); S->fill = buf<int>(c, (pfx + ".ovf_fill").c_str());
  S->list = buf<int>(c, (pfx + ".ovf_list").c_str()); S->nlist = (int*)c->bufs[pfx + ".ovf_nlist"].p; S->list2 = buf<int>(c, (pfx + ".ovf_list2").c_str());
  return SH_OK;
}

// One or two slice sets through the set's launches together (k_slices.h SliceSets): plane heights (+ counter clears, bound decode),
// one pass over the mesh for their sections, one grid for their joins; the overflow tier and the resampling stay per set.
// (Planes per humerus, ring and total area: the set's, SLICE_SETS.)
struct SliceSpec { SetId id; int kind; bool resample; int select; bool decode_bounds; };
static int run_slice_sets(sh_ctx* c, const WinView& v, const SliceSpec* specs, int nspec) {
  const int B = v.B;
  if (nspec < 1 || nspec > 2) return fail(c, SH_ERR_STATE, "run_slice_sets: one or two sets");
  int ntot = 0;
  for (int i = 0; i < nspec; ++i) ntot += SLICE_SETS[specs[i].id].N;
  if (ntot > SH_EMIT_MAXN) return fail(c, SH_ERR_CAPACITY, "slice sets have more planes than k_slice_emit's LDS histogram");
  OvfPools OP; OvfSet OS[2];
  { int orc; if ((orc = ovf_pools(c, &OP)) != SH_OK) return orc; }
  const bool ovf_on = c->batch.tier_on(c->batch_gen);     // (known from an earlier run of this batch: no plane overflows)
  const bool bridge = c->open_mode != SH_OPEN_ERROR;
  SliceSets sets{};
  sets.n = nspec;
  sets.vobb = v.verts_obb; sets.voff = v.voff;
  sets.open = OpenCfg{c->open_mode, c->open_gap, c->open_mode ? v.open_stats : (int*)nullptr};
  for (int i = 0; i < nspec; ++i) {
    const SliceSpec& sp = specs[i];
    const SliceSetDef& def = SLICE_SETS[sp.id];
    const SliceSetView& a = v.set[sp.id];
    { int orc; if ((orc = ovf_set(c, def.pfx, def.N, &OS[i])) != SH_OK) return orc; }
    SliceSetDev& S = sets.s[i];
    S.N = def.N; S.kind = sp.kind; S.select = sp.select;
    S.zb = sp.kind == 4 ? v.obb_zb_pre : v.z_bounds;
    S.zs = a.zs; S.zeff = a.zeff; S.seg_count = a.seg_count; S.segs = a.segs;
    S.centroids = a.centroids; S.areas = a.areas; S.nloops = a.nloops; S.ring_n = a.ring_n;
    S.ring = a.ring; S.areas_total = a.area_total;      // (null where the set has none)
    S.nlarge = v.slices_nlarge + (sp.kind & 7);      // (one counter per kind of set)
    // planes with more than SH_MAXLOOPS loops: listed for the overflow tier's join (tier skipped: flagged, sh_collect runs again with it)
    S.many = ManyLoops{ovf_on ? OS[i].list2 : (int*)nullptr, ovf_on ? OS[i].nlist + 1 : (int*)nullptr, ovf_on ? (unsigned long long*)nullptr : OP.ctr + SH_CTR_TIER_MISSED};
    S.ovf_missed = ovf_on ? (unsigned long long*)nullptr : OP.ctr + SH_CTR_TIER_MISSED;
    // the plane-height launch also zeroes the set's crossing counters and its large-tier counter, resets the overflow tier's words
    // (segments / workspace used: per launch group, by its first set; ring points stay for the run) and, for the first set behind
    // k_transform_verts, decodes the z bounds (run_window)
    S.aux = PlaneAux{sp.decode_bounds ? (const unsigned long long*)v.zb_enc : (const unsigned long long*)nullptr, v.z_bounds, S.seg_count, S.nlarge,
                     ovf_on ? OS[i].nlist : (int*)nullptr, i == 0 ? OP.ctr : (unsigned long long*)nullptr};
  }
  LAUNCH(c, "k_make_planes", k_make_planes, dim3(B, nspec), dim3(256), sets, (const double*)v.neck_z, B);
  dim3 g((unsigned)std::min<long long>((c->maxF + 255) / 256, 4096), (unsigned)B);
  LAUNCH(c, "k_slice_emit", k_slice_emit, g, dim3(256), v.verts_obb, v.faces, v.voff, v.foff, sets);
  if (ovf_on)      // planes with more crossings than slots (k_ovf.h): plan their pool ranges, section them again into the segment pool
    for (int i = 0; i < nspec; ++i) {
      const SliceSetDev& S = sets.s[i];
      LAUNCH(c, "k_ovf_plan", k_ovf_plan, dim3((unsigned)((B * S.N + 255) / 256)), dim3(256), S.N, B * S.N, (const int*)S.seg_count, OP, OS[i], v.err);
      LAUNCH(c, "k_slice_emit_ovf", k_slice_emit_ovf, g, dim3(256), v.verts_obb, v.faces, v.voff, v.foff, (const double*)S.zeff, S.N, OP, OS[i]);
    }
  // two capacity tiers share the grid (k_slices.h): the planes of the other tier exit at once
  // (bridge mode: the joins with the open-contour code, k_open.h; the default mode's joins are built without it)
  LAUNCH(c, "k_slice_link", bridge ? k_slice_link<true> : k_slice_link<false>, dim3(B * ntot), dim3(SH_LINK_THREADS), sets, B, v.err);
  LAUNCH(c, "k_slice_link_large", bridge ? k_slice_link_large<true> : k_slice_link_large<false>, dim3(std::min(B * ntot, 512)), dim3(SH_LINK_THREADS), sets, B, v.err);
  for (int i = 0; i < nspec; ++i) {
    const SliceSpec& sp = specs[i];
    const SliceSetDev& S = sets.s[i];
    if (ovf_on) {
      LAUNCH(c, "k_ovf_plan_loops", k_ovf_plan_loops, dim3(16), dim3(256), S.N, (const int*)S.seg_count, (const Seg*)S.segs, OP, OS[i], v.err);
      LAUNCH(c, "k_slice_link_huge", bridge ? k_slice_link_huge<true> : k_slice_link_huge<false>, dim3(64), dim3(SH_HUGE_THREADS), S.N, (const int*)S.seg_count, OP, OS[i],
             S.centroids, S.areas, S.nloops, S.ring_n, SLICE_SETS[sp.id].ring ? 1 : 0, S.select, v.err, S.areas_total, (const double*)v.verts_obb, (const long long*)v.voff,
             (const double*)S.zeff, sets.open);
    }
    if (sp.resample) {
      RsWant want{c->keep_products ? 1 : 0, SH_ANP_ROW0, 0, 0};
      cutoff_range(SH_NPROX, c->params.groove_cutoff[0], c->params.groove_cutoff[1], &want.cs_lo, &want.cs_hi);
      if (c->b0 == 0) { c->rs_cs_lo = want.cs_lo; c->rs_cs_hi = want.cs_hi; c->rs_all = c->keep_products; c->rs_gen = c->batch_gen; }
#define RS_ROWS S.centroids, v.prox_ixy, v.prox_itr_start, v.prox_itr_centered_start      /* what every tier reads and writes */
      LAUNCH(c, "k_resample_polar", k_resample_polar, dim3(B * S.N), dim3(SH_RS_THREADS), S.N, SH_MPROX, S.ring_n, S.ring, RS_ROWS, (const long long*)OS[i].roff, want);
      LAUNCH(c, "k_resample_polar_large", k_resample_polar_large, dim3(std::min(B * S.N, 512)), dim3(SH_RS_THREADS), B * S.N, S.N, SH_MPROX, S.ring_n, S.ring, RS_ROWS,
             (const int*)S.nlarge, (const long long*)OS[i].roff, want);
      if (ovf_on) LAUNCH(c, "k_resample_polar_huge", k_resample_polar_huge, dim3(64), dim3(SH_RS_THREADS), S.N, SH_MPROX, (const int*)S.ring_n, OP, OS[i], RS_ROWS, want);
#undef RS_ROWS
    }
  }
  return SH_OK;
}
static int run_slice_set(sh_ctx* c, const WinView& v, const SliceSpec& sp) { return run_slice_sets(c, v, &sp, 1); }
// the five sets as the stages ask for them (kind, resampling, loop selection; decode: the first set behind k_transform_verts)
static SliceSpec spec_full(bool decode) { return {SET_FULL, 0, false, 0, decode}; }
static SliceSpec spec_distal(bool decode) { return {SET_DISTAL, 2, false, 0, decode}; }
static const SliceSpec SPEC_PROX = {SET_PROX, 1, true, 0, false}, SPEC_NECKC = {SET_NECKC, 3, false, 1, false}, SPEC_POBB = {SET_POBB, 4, false, 0, false};

// A hull above the record's capacity (a strictly convex surface keeps every vertex: 16 384 is not a bound of the reference's
// `convex_hull`, mesh.py:82): the hull record and the per-face arrays of the OBB stage are re-allocated at strides that hold it.
// Foreground only, nothing of this context in flight reads them afterwards (hipFree waits for the device).  A WinView resolved
// before this call is stale behind it.  (How far it grows: sh_obb_plan.h hull_record_grown.)
static int grow_hull_records(sh_ctx* c, HullNeed need) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->hcap = hull_record_grown(c->hcap, need);
  int rc;
  WIN_HULLCAP_BUFS(WIN_ENS)
  if (c->sw.debug) fprintf(stderr, "[sh] hull record grown to %d vertices / %d faces / %d edges per humerus\n", c->hcap.v, c->hcap.f, c->hcap.e);
  return SH_OK;
}

// mesh.py:63-125.  Host: convex hulls (hull_host_phase; already done by the background thread when `prepared_slot`
// >= 0).  Device: candidate boxes for every hull face, pick + frame, end sections, circle fits, flip (k_obb.h).
static bool device_hull_now(const sh_ctx* c) { return c->batch.device_hull(c->hull_mode, c->batch_gen); }

// What one window's stages tell each other; lives in run_window
struct WinState {
  bool bounds_cleared = false;      // run_obb's first fill of this window covered zb_enc / anp.mm_enc (stage_frame skips its own)
  bool side_pending = false;        // the side branch has been forked and not joined yet
  bool te_rows_done = false;        // run_te_rows has run (beside or in front of the chain)
};

// ---- the OBB stage: run_obb is its order; where the hulls come from, how the record grows and every number of the launches are
// sh_obb_plan.h's ----------------------------------------------------------------------------------------------------------------------
// The hull record of the window, on its way into hull.* behind this; *nfmax: the face count the launches are sized by.
// redo_nf > 0: a redo -- redo_given_up put the host quickhull's record of this window (of one humerus) into hull.*, with that many faces.
// `v` is resolved again when the hull record had to grow (the only re-allocation of a view's buffers inside a window).
static int obb_hulls(sh_ctx* c, WinView& v, int prepared_slot, int redo_nf, int* nfmax) {
  const int B = v.B;
  const HullSource src = hull_source(redo_nf, device_hull_now(c), prepared_slot);
  int slot = prepared_slot, rc;
  switch (src) {
    case HULL_REDO: case HULL_PREPARED: break;
    case HULL_DEVICE:
      if ((rc = run_device_hull(c, B)) != SH_OK) return rc;
      break;
    case HULL_FOREGROUND: {
      slot = c->hslot; c->hslot ^= 1;
      int bad = -1; double ms = 0; std::string et;
      rc = hull_host_phase(c, c->hull_in, slot, c->b0, B, &bad, &ms, &et);
      if (c->sw.debug) fprintf(stderr, "[sh] run_obb: foreground hull phase %.2f ms\n", ms);
      if (c->timing) { KTimer& h = c->timers["host.hull"]; h.ms += ms; h.n += 1; }
      if (rc == SH_ERR_HIP) { c->err = et; return rc; }
      if (rc != SH_OK) return fail(c, rc, hull_failed_text(bad, rc));
      break;
    }
  }
  HullNeed need = {1, 1, 1};
  if (hull_from_host(src)) {
    need = hull_need(c->hstage[slot].cnt, B);
    if (!hull_fits(need, c->hcap)) {      // (never with an early upload: the background threads upload only what fits)
      if ((rc = grow_hull_records(c, need)) != SH_OK) return rc;
      v = win_view(c);
    }
    if (hull_upload_pending(src, c->prep.uploaded)) HIPCHK(c, hull_upload(c, slot, B, v.hull(), c->stream));
  }
  *nfmax = hull_nfmax(src, redo_nf, c->batch.skip_nfmax(), need);
  return SH_OK;
}

// The workspace tier's buffers (k_obb.h ObbWs), ensured where the tier is used: X(field, "name", element type, element size as
// sh_buffer_info reports it).  obb_workspace: at the plan's sizes, no window stride (another tier: none of them) -> the kernel's argument.
#define OBB_WS_BUFS(X) X(fmask, "obb.ws_fmask", unsigned char, 1) X(lists, "obb.ws_lists", unsigned, 4) X(sxy, "obb.ws_sxy", double2, 8) X(area, "obb.ws_area", double, 8)
static int obb_workspace(sh_ctx* c, const ObbPlan& p, unsigned long long* need, ObbWs* ws) {
  *ws = ObbWs{};
  ws->need = need; ws->nwg = p.nwg; ws->silcap = p.silcap;
  if (p.tier != OBB_TIER_WORKSPACE) return SH_OK;
  int rc;
#define X(f, name, T, elem) ENS_SHARED(name, p.ws.f, elem);
  OBB_WS_BUFS(X)
#undef X
#define X(f, name, T, elem) ws->f = (T*)c->bufs[name].p;
  OBB_WS_BUFS(X)
#undef X
  return SH_OK;
}

// The clears of the stage, face areas and pruning bounds, then two passes of select + candidates: the seed tile, then the directions
// its best volume cannot exclude.  Every grid and size is the plan's.
static int obb_candidates(sh_ctx* c, const WinView& v, WinState* w, const ObbPlan& p) {
  const int B = v.B;
  const HullCap hc = c->hcap;
  FILL(c, {v.obb_best_enc, (size_t)B * 8, 0xFF} /*"no candidate volume yet"*/, {v.obb_lbmin_enc, (size_t)B * 8, 0xFF},
       {v.obb_area2, (size_t)B * hc.f * 8, 0}, {v.obb_endcnt, (size_t)B * 2 * 4, 0},
       {v.zb_enc, (size_t)B * 16, 0xFF} /*z bounds: "nothing seen yet"*/, {v.anp_mm_enc, (size_t)B * 16, 0xFF});
  w->bounds_cleared = true;
  LAUNCH(c, "k_obb_face_area2", k_obb_face_area2, dim3(p.area2_grid, (unsigned)B), dim3(256), v.hull_hv,
         v.hull_normals, v.hull_edges, (const int*)v.hull_ne, v.obb_area2, hc);
  LAUNCH(c, "k_obb_bounds", k_obb_bounds, dim3(p.bounds_grid), dim3(SH_OBB_BND_THREADS),
         v.hull_hv, (const int*)v.hull_nv, v.hull_normals, (const int*)v.hull_nf, v.obb_area2, v.obb_lb,
         v.obb_lbmin_enc, v.obb_cand_vol, v.obb_cand_edge, p.bnd_tiles, B, hc);
  const auto candidates = p.tier == OBB_TIER_WORKSPACE ? k_obb_candidates<SH_OBB_TILE_LARGE, 1, 0, 0, unsigned, true>
                          : p.tier == OBB_TIER_LARGE   ? k_obb_candidates<SH_OBB_TILE_LARGE, 1, SH_OBB_SIL_LARGE, SH_OBB_NF_LARGE, unsigned>
                                                       : k_obb_candidates<SH_OBB_TILE, SH_OBB_GROUP, SH_OBB_SIL_SMALL, SH_OBB_NF_SMALL, unsigned short>;
  ObbWs ws;
  if (int rc = obb_workspace(c, p, v.ovf_ctr + SH_CTR_SIL_NEED, &ws)) return rc;
  for (int pass = 0; pass < 2; ++pass) {
    const ObbPass& q = p.pass[pass];
    LAUNCH(c, "k_obb_select", k_obb_select, dim3(B), dim3(256), v.obb_lb, (const int*)v.hull_nf, v.obb_lbmin_enc,
           v.obb_best_enc, q.mode, v.obb_dir_list, v.obb_dir_count, v.obb_seeded, hc);
    LAUNCH(c, pass == 0 ? "k_obb_seed" : "k_obb_candidates", candidates, dim3(q.grid), dim3(SH_OBB_THREADS),
           v.hull_hv, v.hull_nv, v.hull_normals, v.hull_nf, v.hull_edges, v.hull_ne, v.obb_cand_vol,
           v.obb_cand_edge, v.err, v.obb_best_enc, v.obb_dir_list, v.obb_dir_count,
           q.nt_pass, B, c->sw.obb_prune ? 1 : 0, hc, ws);
  }
  return SH_OK;
}

// The smallest candidate -> the raw box frame; then the ProxObb scan of a proximal humerus, or the end sections, circle fits and flip
static int obb_frame(sh_ctx* c, const WinView& v, WinState* w) {
  const int B = v.B;
  LAUNCH(c, "k_obb_pick", k_obb_pick, dim3(B), dim3(256), v.hull_hv, v.hull_normals, (const int*)v.hull_nf, v.hull_edges,
         v.obb_cand_vol, v.obb_cand_edge, v.verts, v.voff, v.obb_T_pre, v.obb_zb_pre, v.err, c->hcap);
  if (!c->obb_done_ev) HIPCHK(c, hipEventCreateWithFlags(&c->obb_done_ev, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->obb_done_ev, c->stream));      // hull.* device buffers are free for the next run's records from here
  if (c->params.bone_kind == SH_BONE_PROXIMAL) {
    // mesh.py:134-192 ProxObb: 100 sections of the mesh in the raw box frame, head = largest area, canal range
    dim3 gv((unsigned)std::min<long long>((c->maxV + 255) / 256, 1024), (unsigned)B);
    LAUNCH(c, "k_transform_verts", k_transform_verts, gv, dim3(256), v.verts, v.voff, v.obb_T_pre, v.verts_obb, v.zb_enc);      // (zb_enc: cleared by the fill above; its values are not used here)
    w->bounds_cleared = false;      // ... and stage_frame clears it again for the box frame's pass
    int rc2;
    if ((rc2 = run_slice_set(c, v, SPEC_POBB)) != SH_OK) return rc2;
    LAUNCH(c, "k_prox_obb", k_prox_obb, dim3((B + 63) / 64), dim3(64), v.set[SET_POBB].area_total, v.set[SET_POBB].zs, v.obb_T_pre,
           v.obb_transform, v.flipped, v.pobb_cutoff, v.pobb_cutoff_idx, v.err, B);
    c->batch.frame_computed();
    return SH_OK;
  }
  dim3 g((unsigned)std::min<long long>((c->maxF + 255) / 256, 1024), (unsigned)B);
  const int end_cap = c->batch.caps().end;
  LAUNCH(c, "k_obb_end_points", k_obb_end_points, g, dim3(256), v.verts, v.faces, v.voff, v.foff, v.obb_T_pre, v.obb_zb_pre, v.obb_endpts, v.obb_endcnt, end_cap);
  LAUNCH(c, "k_obb_ends", k_obb_ends, dim3(B), dim3(128), v.obb_endpts, v.obb_endcnt, v.obb_T_pre, v.obb_resid, v.obb_transform, v.flipped, v.err, B, end_cap,
         v.ovf_ctr + SH_CTR_END_NEED);
  c->batch.frame_computed();
  return SH_OK;
}

static int run_obb(sh_ctx* c, WinView& v, WinState* w, int prepared_slot, int redo_nf) {
  int rc, nfmax = 1;
  c->batch.obb_begins(c->batch_gen);      // (a new batch: the small k_obb_candidates tier and the chosen hull mode again)
  if ((rc = obb_hulls(c, v, prepared_slot, redo_nf, &nfmax)) != SH_OK) return rc;
  const ObbPlan plan = obb_plan(v.B, nfmax, c->hcap, c->batch.caps().sil_need, c->batch.caps().nf_over, c->sw.obb_prune);
  if ((rc = obb_candidates(c, v, w, plan)) != SH_OK) return rc;
  return obb_frame(c, v, w);
}

// epicondyle.py:33-89, everything that needs the distal set only: the minimum-area rectangle of every distal slice in the cut (three
// capacity tiers) and the two ends of the widest one
static int run_te_rows(sh_ctx* c, const WinView& v) {
  const int B = v.B;
  const SliceSetView& distal = v.set[SET_DISTAL];
  OvfPools OP; OvfSet OS;
  { int orc; if ((orc = ovf_pools(c, &OP)) != SH_OK || (orc = ovf_set(c, "distal", SH_NDIST, &OS)) != SH_OK) return orc; }
  LAUNCH(c, "k_te_rows", k_te_rows<SH_SMALLSEG>, dim3(B * SH_TE_NROWS), dim3(64), distal.ring, distal.ring_n, v.te_rects, B, (const long long*)OS.roff);
  LAUNCH(c, "k_te_rows_large", k_te_rows<SH_MAXSEG>, dim3(B * SH_TE_NROWS), dim3(64), distal.ring, distal.ring_n, v.te_rects, B, (const long long*)OS.roff);
  if (c->batch.tier_on(c->batch_gen)) LAUNCH(c, "k_te_rows_huge", k_te_rows_huge, dim3(64), dim3(64), OP, OS, (const int*)distal.ring_n, v.te_rects);
  // epicondyle.py:39-89: the widest slice's end slivers, their centroids, the farthest pair (CT coordinates, piece order)
  LAUNCH(c, "k_te_ends", k_te_ends, dim3(B), dim3(64), distal.ring, distal.ring_n, v.te_rects, distal.zs, v.obb_transform, v.te_ends_ct, v.te_row, v.err, B, OP, OS);
  return SH_OK;
}

// ---- the stages of a window, in the order run_window calls them --------------------------------------------------------------------
// the box frame: verts_obb + z bounds (mesh.py:85-86)
static int stage_frame(sh_ctx* c, const WinView& v, uint32_t mask, const WinState& w) {
  const int B = v.B;
  // the encoded minima / maxima (z bounds of the box frame, the anatomic-neck image's range) start as all ones: one fill for both,
  // in run_obb's first fill when that stage runs (they were a launch each)
  if (!w.bounds_cleared && (mask & (SH_STAGE_OBB | SH_STAGE_FULL | SH_STAGE_ANP)))
    FILL(c, {v.zb_enc, (size_t)B * 16, 0xFF}, {v.anp_mm_enc, (size_t)B * 16, 0xFF});
  if (mask & (SH_STAGE_OBB | SH_STAGE_FULL)) {
    dim3 g((unsigned)std::min<long long>((c->maxV + 255) / 256, 1024), (unsigned)B);
    LAUNCH(c, "k_transform_verts", k_transform_verts, g, dim3(256), v.verts, v.voff, v.obb_transform, v.verts_obb, v.zb_enc);
    if (!(mask & SH_STAGE_FULL))      // (with the full set in the run its k_make_planes decodes them)
      LAUNCH(c, "k_decode_bounds", k_decode_bounds, dim3((2 * B + 63) / 64), dim3(64), v.zb_enc, v.z_bounds, B);
  }
  return SH_OK;
}

// the fork of the side branch: the side stream starts behind what the main stream has enqueued so far
static int fork_side(sh_ctx* c) {
  if (!c->side_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
  if (!c->side_fork_ev) { HIPCHK(c, hipEventCreateWithFlags(&c->side_fork_ev, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&c->side_join_ev, hipEventDisableTiming)); }
  HIPCHK(c, hipEventRecord(c->side_fork_ev, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->side_stream, c->side_fork_ev, 0));
  return SH_OK;
}

// the distal set (unless it went with the full set's launches: `merged`) and the trans-epicondylar rows that hang on it alone --
// on the side stream (`side`: forked here, joined by run_window) or in the chain
static int stage_distal(sh_ctx* c, const WinView& v, uint32_t mask, bool merged, bool side, WinState* w) {
  int rc;
  if (side && (rc = fork_side(c)) != SH_OK) return rc;
  {
    StreamScope on(c, side ? c->side_stream : c->stream);
    rc = merged ? SH_OK : run_slice_set(c, v, spec_distal(false));
    // In the chain, the trans-epicondylar rows run HERE, in front of the UNet pass instead of behind it: the same kernels on the same
    // stream, but the part of the step that follows the UNet -- what stands between the pass and the lane's next step -- is 0.3 ms
    // (0.6 ms beside the other lane's UNet) shorter: 8.00 -> 7.74 ms per step sustained, 8.48 -> 8.35 at 20 steps.
    const bool te_inline = !side && (mask & SH_STAGE_ANP);
    if (rc == SH_OK && (side || te_inline) && (mask & SH_STAGE_TE)) { rc = run_te_rows(c, v); w->te_rows_done = rc == SH_OK; }
  }
  if (side && rc == SH_OK) { HIPCHK(c, hipEventRecord(c->side_join_ev, c->side_stream)); w->side_pending = true; }
  return rc;
}

// surgical_neck.py:25-54: the change point of the full set's areas, then the contour at neck_z (loop whose vertex mean is nearest the
// origin) -- with the proximal set (which starts from neck_z as well) in the same launches when both stages run (`with_prox`)
static int stage_neck(sh_ctx* c, const WinView& v, bool with_prox) {
  const bool prox = c->params.bone_kind == SH_BONE_PROXIMAL;      // surgical_neck.py:25-28
  LAUNCH(c, "k_neck", prox ? k_neck<true> : k_neck<false>, dim3(v.B), dim3(64), v.set[SET_FULL].areas, v.set[SET_FULL].zs, v.neck_z, v.neck_index, v.B,
         prox ? 0.2 : 0.70, 0.99, prox ? v.neck_gram : (double*)nullptr);
  if (!with_prox) return run_slice_set(c, v, SPEC_NECKC);
  const SliceSpec sp[2] = {SPEC_NECKC, SPEC_PROX};
  return run_slice_sets(c, v, sp, 2);
}

static int stage_canal(sh_ctx* c, const WinView& v) {
  LAUNCH(c, "k_canal", k_canal, dim3(v.B), dim3(64), v.set[SET_FULL].centroids, v.set[SET_FULL].zs, v.z_bounds, v.obb_transform, c->params.canal_cutoff[0],
         c->params.canal_cutoff[1], c->params.bone_kind == SH_BONE_PROXIMAL ? v.pobb_cutoff : (const double*)nullptr,
         v.canal_points_obb, v.canal_axis_obb, v.canal_axis_ct, v.err);
  return SH_OK;
}

static int stage_groove(sh_ctx* c, const WinView& v, uint32_t mask) {
  const int B = v.B;
  int rc;
  if (!c->pstate.has_rfc()) return fail(c, SH_ERR_STATE, "sh_run: groove stage needs sh_load_rfc first");
  int ga, gb;
  cutoff_range(SH_NPROX, c->params.groove_cutoff[0], c->params.groove_cutoff[1], &ga, &gb);
  // the centred polar rows [ga, gb) come from the proximal set's resampling, which writes the rows of ITS run's cut-off range (RsWant)
  if (!(mask & SH_STAGE_PROXIMAL) && !(c->rs_gen == c->batch_gen && (c->rs_all || (ga >= c->rs_cs_lo && gb <= c->rs_cs_hi))))
    return fail(c, SH_ERR_STATE, "sh_run: SH_STAGE_GROOVE without SH_STAGE_PROXIMAL, and the proximal slices of this batch were not made for this groove_cutoff (run SH_STAGE_PROXIMAL again)");
  const ParamShape& ps = c->pstate.shape();
  const ForestView forest(buf<char>(c, "params"), ParamLayout(ps));
  const size_t N = ps.nodes;
  const double* prox_zs = v.set[SET_PROX].zs;
  LAUNCH(c, "k_groove_rows", k_groove_rows, dim3(B * SH_GROOVE_NROWS), dim3(64), v.prox_itr_centered_start, prox_zs, v.canal_axis_ct, ga, v.groove_xraw,
         v.groove_ptheta, v.groove_npk, v.groove_r0, v.err, B);
  LAUNCH(c, "k_groove_scale", k_groove_scale, dim3(B), dim3(256), v.groove_xraw, v.groove_npk, v.groove_stats, B, v.groove_slots, v.groove_nslot, v.groove_proba);
  if ((rc = ensure(c, "rfc.nodes", N * 16, 4)) != SH_OK) return rc;
  int4* nodes = (int4*)c->bufs["rfc.nodes"].p;
  if (c->pstate.need_forest_pack()) {      // once per parameter block (it was a launch of every step's chain: 5 us alone, ~50 us beside a UNet pass)
    LAUNCH(c, "k_rfc_pack", k_rfc_pack, dim3((unsigned)((N + 255) / 256)), dim3(256), forest.feat, forest.thr, forest.ti, forest.fi, forest.lw, nodes, (int)N);
    c->pstate.forest_packed();
  }
  LAUNCH(c, "k_groove_rfc", k_groove_rfc, dim3((unsigned)(B * ((SH_GSLOTS + 63) / 64))), dim3(64), v.groove_xraw, v.groove_slots, v.groove_nslot,
         v.groove_stats, nodes, forest.roots, (int)ps.trees, v.groove_xs, v.groove_proba, B);
  LAUNCH(c, "k_groove_tail", k_groove_tail, dim3(B), dim3(256), v.groove_ptheta, v.groove_proba, v.groove_bg_theta, v.err,
         v.prox_itr_centered_start, v.groove_r0, prox_zs, v.set[SET_PROX].centroids, ga, c->params.groove_deg_window,
         v.groove_local_idx, v.groove_points_obb, v.obb_transform, v.groove_axis_ct, v.groove_points_ct);
  return SH_OK;
}

static int stage_anp(sh_ctx* c, const WinView& v) {
  const int B = v.B;
  int rc;
  if (!c->pstate.has_unet()) return fail(c, SH_ERR_STATE, "sh_run: anatomic-neck stage needs sh_load_unet first");
  LAUNCH(c, "k_anp_rows", k_anp_rows, dim3(B * SH_ANP_ROWS), dim3(64), v.prox_itr_start, v.groove_bg_theta, v.anp_raw, v.anp_t01, v.anp_roll, B,
         v.anp_mm_enc);      // (+ the image's minimum / maximum: no second pass over it)
  // MinMaxScaler (anatomic_neck.py:56-58): the 16-bit network's first kernel applies it where it reads its patches (k_unet16_l0.h) --
  // no f32 image, 201 MB less traffic and a launch less per step; the other forms of the network and sh_set_keep_products get "anp.image"
  const bool scale_in_net = plan_level0_fused(c->params.unet_dtype, c->unet.reference, c->pstate.shape().base, c->pstate.shape().depth, SH_ANP_ROWS, SH_MPROX);
  if (!scale_in_net || c->keep_products) LAUNCH(c, "k_anp_scale", k_anp_scale, dim3(64, B), dim3(256), v.anp_raw, v.anp_mm_enc, v.anp_image);
  if ((rc = unet_turn_enter(c)) != SH_OK) return rc;
  rc = unet_dispatch(c, {v.anp_image, scale_in_net ? v.anp_raw : nullptr, scale_in_net ? v.anp_mm_enc : nullptr, v.anp_logits}, B, SH_ANP_ROWS, SH_MPROX);
  (void)unet_turn_leave(c);      // also after a failed pass: whatever was enqueued is what the next context waits for
  if (rc != SH_OK) return rc;
  const double* prox_zs = v.set[SET_PROX].zs;
  LAUNCH(c, "k_anp_edge_count", k_anp_edge_count, dim3(SH_ANP_ROWS / 8, B), dim3(512), v.anp_logits, v.anp_rowcnt, v.anp_maskbits);
  LAUNCH(c, "k_anp_edges", k_anp_edges, dim3(SH_ANP_ROWS / 8, B), dim3(512), v.anp_maskbits, v.anp_raw, v.anp_t01, v.anp_roll, prox_zs, v.anp_rowcnt,
         v.anp_points_obb, v.anp_counts, v.err);
  LAUNCH(c, "k_anp_plane", k_anp_plane, dim3(B), dim3(256), v.anp_points_obb, v.anp_counts, v.anp_plane, v.err, v.anp_ray_t);      // (+ "no hit yet" for the rays)
  LAUNCH(c, "k_rays_hit", k_rays_hit, dim3(SH_RAY_CHUNKS, B), dim3(256), v.verts_obb, v.faces, v.voff, v.foff, v.anp_plane, v.anp_ray_t);
  return SH_OK;
}

// metrics of bone_props.py (side, retroversion, neck-shaft angle, radius of curvature; the sphere's sums need the mask and the neck
// plane only), then ray points -> trans-epicondylar order -> record -> metrics: one launch, one workgroup per humerus (k_tail, k_te.h)
static int stage_tail(sh_ctx* c, const WinView& v, uint32_t mask) {
  const int B = v.B;
  const bool prox = c->params.bone_kind == SH_BONE_PROXIMAL;
  const uint32_t need = SH_STAGE_GROOVE | SH_STAGE_ANP | SH_STAGE_CSYS | (prox ? 0u : (uint32_t)SH_STAGE_TE);
  const bool metrics = (mask & need) == need;
  if (metrics)
    LAUNCH(c, "k_sphere_partial", k_sphere_partial, dim3(SH_SPH_PARTS, B), dim3(256), v.anp_maskbits, v.anp_raw, v.anp_t01, v.anp_roll, v.set[SET_PROX].zs,
           v.anp_plane, v.metrics_partial);
  PackArgs A{};
  A.lm = v.landmarks; A.T_obb = v.obb_transform; A.zb = v.z_bounds; A.neck_z = v.neck_z;
  A.neck_index = v.neck_index; A.flipped = v.flipped; A.canal_axis_ct = v.canal_axis_ct; A.te_axis_ct = v.te_axis_ct;
  A.groove_axis_ct = v.groove_axis_ct; A.bg_theta = v.groove_bg_theta; A.groove_pts_ct = v.groove_points_ct;
  A.plane = v.anp_plane; A.axes_obb = v.anp_axes_obb; A.anp_pts_obb = v.anp_points_obb; A.anp_counts = v.anp_counts;
  A.err = v.err; A.mask = mask; A.B = B; A.bone_kind = (int)c->params.bone_kind;
  A.canal_cut = prox ? v.pobb_cutoff : (const double*)nullptr;
  A.cc0 = c->params.canal_cutoff[0]; A.cc1 = c->params.canal_cutoff[1];
  A.ray_t = v.anp_ray_t; A.te_ends_ct = v.te_ends_ct; A.sphere_partial = v.metrics_partial; A.metrics = metrics ? 1 : 0;
  LAUNCH(c, "k_tail", k_tail, dim3(B), dim3(256), A);
  return SH_OK;
}

// bone.py:155: the mesh of every humerus in its own canal / trans-epicondylar (or canal / articular) frame
static int stage_apply(sh_ctx* c, const WinView& v) {
  dim3 g((unsigned)std::min<long long>((c->maxV + 255) / 256, 1024), (unsigned)v.B);
  LAUNCH(c, "k_apply_csys", k_apply_csys, g, dim3(256), v.landmarks, v.verts, v.voff, v.verts_csys);
  return SH_OK;
}

// All stages for the window [c->b0, c->b0 + c->Bwin) of the batch; everything is enqueued on the stream,
// nothing here waits for the device.  This function is the ORDER of the stages, which slice sets share their launches, the fork of
// the side branch and its join; what a stage launches is its function's.
static int run_window(sh_ctx* c, uint32_t mask, int prepared_slot, int redo_nf = 0) {
  auto has = [mask](uint32_t stages) { return (mask & stages) != 0; };
  int rc;
  WinView v = win_view(c);
  WinState w;
  if (has(SH_STAGE_OBB) && (rc = run_obb(c, v, &w, prepared_slot, redo_nf)) != SH_OK) return rc;
  if ((rc = stage_frame(c, v, mask, w)) != SH_OK) return rc;
  const bool transformed = has(SH_STAGE_OBB | SH_STAGE_FULL);
  // Slice sets that hang on the same inputs share their launches (run_slice_sets): full + distal behind the box frame, neck contour +
  // proximal behind neck_z -- 8 launches and two passes over the mesh less per step; same sections (SHOULDER_SLICE_MERGE=0: one
  // set per launch group, the A/B of tests/test_gpu_slices.py)
  const bool merge_env = c->sw.slice_merge;
  // The distal set and the first part of the trans-epicondylar stage (the rectangles of its rows, the ends of the widest one) need
  // nothing but the box frame.  Small batches (up to 16 humeri: one humerus gains 4 %, 6.01 -> 5.78 ms per run; at B = 64 two streams'
  // kernels just share the CUs and one lane LOSES 8 %): the whole branch runs on the side stream beside the full -> neck -> canal ->
  // proximal -> groove chain.  Larger batches: the distal set and the trans-epicondylar rows stay in the chain (DESIGN.md section 9:
  // the rows forked beside the lane's UNet pass, or run behind it, made the step slower).  Fork only when the overflow tier is known
  // to be idle for this batch (its pool counters are per set) and no per-launch timing is on.
  const bool can_fork = has(SH_STAGE_DISTAL) && !c->batch.tier_on(c->batch_gen) && c->timing != 1 && redo_nf == 0;
  const bool side = can_fork && v.B <= 16;
  const bool merge_fd = merge_env && has(SH_STAGE_FULL) && has(SH_STAGE_DISTAL) && !side;
  if (merge_fd) {
    // (both sets decode the z bounds themselves: their plane heights are made by ONE launch, the distal workgroups cannot wait for the
    //  full set's to write "z_bounds")
    const SliceSpec sp[2] = {spec_full(transformed), spec_distal(transformed)};
    if ((rc = run_slice_sets(c, v, sp, 2)) != SH_OK) return rc;
  } else if (has(SH_STAGE_FULL)) {
    if ((rc = run_slice_set(c, v, spec_full(transformed))) != SH_OK) return rc;
  }
  if (has(SH_STAGE_DISTAL) && (rc = stage_distal(c, v, mask, merge_fd, side, &w)) != SH_OK) return rc;
  const bool merge_np = merge_env && has(SH_STAGE_NECK) && has(SH_STAGE_PROXIMAL);
  if (has(SH_STAGE_NECK) && (rc = stage_neck(c, v, merge_np)) != SH_OK) return rc;
  if (has(SH_STAGE_CANAL) && (rc = stage_canal(c, v)) != SH_OK) return rc;
  if (has(SH_STAGE_PROXIMAL) && !merge_np && (rc = run_slice_set(c, v, SPEC_PROX)) != SH_OK) return rc;
  if (has(SH_STAGE_GROOVE) && (rc = stage_groove(c, v, mask)) != SH_OK) return rc;
  if (has(SH_STAGE_ANP) && (rc = stage_anp(c, v)) != SH_OK) return rc;
  // The join of the side branch (its rectangles and ends are done there), in ONE place: in front of the trans-epicondylar block and
  // of everything behind it.  (It used to stand a second time behind that block, for runs without SH_STAGE_TE; no launch lies between
  // the two positions then, so the stream order is the same.)
  if (w.side_pending) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_join_ev, 0)); w.side_pending = false; }
  if (has(SH_STAGE_TE) && !w.te_rows_done && (rc = run_te_rows(c, v)) != SH_OK) return rc;
  if ((rc = stage_tail(c, v, mask)) != SH_OK) return rc;
  if (has(SH_STAGE_APPLY) && (rc = stage_apply(c, v)) != SH_OK) return rc;
  return SH_OK;
}

// Humeri per window (sh_run.h SH_WINDOW).  Default: one window = the whole batch.  Measured on MI355X (bf16 UNet): B=256 as 4 windows of 64
// 2549 humeri/s vs 2744 as one window -- the kernels run ~15 % more efficiently on the larger launches, which is more
// than the hidden host hull (13 % of the step) buys back.  SHOULDER_WINDOW=<n> enables windows of n.

// ---- the background preparations of hulls (sh_ctx::Prepared; sh_run.h PreparedKey says who writes what) ----------------------------------
// the results of a new thread: nothing yet (the caller has just written the key)
static void prepared_reset(sh_ctx::Prepared& p) { p.rc = SH_OK; p.bad_mesh = -1; p.d2h_ms = p.hull_ms = 0; p.err.clear(); p.uploaded = false; }

// The tail of both threads: the host hulls of `pts` into the key's pinned slot, then (`can_upload`) the records to the device as soon as
// the running step no longer reads the hull.* buffers (after its k_obb_pick)
static void prepared_hulls(sh_ctx* c, const sh_ctx::HullPts& pts, const HullRec& dst, bool can_upload) {
  sh_ctx::Prepared& q = c->prep;
  const int slot = q.key.slot, B = q.key.B;
  q.rc = hull_host_phase(c, pts, slot, 0, B, &q.bad_mesh, &q.hull_ms, &q.err, true);
  if (q.rc == SH_OK && can_upload && hipStreamWaitEvent(c->copy_stream, c->obb_done_ev, 0) == hipSuccess && hull_upload(c, slot, B, dst, c->copy_stream) == hipSuccess &&
      hipStreamSynchronize(c->copy_stream) == hipSuccess)
    q.uploaded = true;
}

// overlap of the host hulls with the device work of the previous run
static void start_prepare(sh_ctx* c) {
  sh_ctx::Prepared& p = c->prep;
  p.key.begin_resident(c->hslot, c->B, c->batch_gen);
  prepared_reset(p);
  // device pointers are looked up here: the buffer map belongs to the calling thread
  const HullPre hp = hullpre_ptrs(c);
  const HullRec dst = hull_rec(c);
  const bool can_upload = early_upload_ok(c->obb_done_ev != nullptr, c->B, c->hcap, hull_rec_bytes(c));      // (the size half: always true here, sh_obb_plan.h)
  p.th = std::thread([c, hp, dst, can_upload]() {
    sh_ctx::Prepared& q = c->prep;
    if (hipSetDevice(c->device) != hipSuccess) { q.rc = SH_ERR_HIP; return; }
    if (!c->copy_stream && hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { q.rc = SH_ERR_HIP; return; }
    {      // the points of a device-generated batch come back for every run, on the copy stream, beside the kernels
      auto t0 = std::chrono::steady_clock::now();
      if (fetch_hull_points(c, hp, c->copy_stream) != hipSuccess) { q.rc = SH_ERR_HIP; return; }
      q.d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    prepared_hulls(c, c->hull_in, dst, can_upload);
  });
}

int sh_set_overlap(sh_ctx* c, int on) {
  if (!c) return SH_ERR_ARG;
  c->overlap = on != 0;      // hulls already in preparation stay usable by the next run
  return SH_OK;
}

int sh_set_unet_turns(sh_ctx* c, int on) {
  if (!c) return SH_ERR_ARG;
  c->unet.turn = on != 0;
  if (!c->unet.turn) unet_turn_forget(c);
  return SH_OK;
}

int sh_discard_prepared(sh_ctx* c) {
  if (!c) return SH_ERR_ARG;
  (void)join_prepared(c);
  c->prep.key.void_hulls();
  return SH_OK;
}

// ---- records on the wire ------------------------------------------------------------------------------------------------------
// A full record is 104 KB, 96 KB of it the padded anatomic-neck point list (4 096 rows; a humerus has ~1 000).  With
// sh_set_record_rows(R) the records a run hands out (`out` of sh_run / sh_submit: host memory or a gather's device send buffer)
// are PACKED: [the bytes of sh_landmarks in front of anp_points][its six trailing int32 fields][R rows of anp_points] -- the
// first min(n_anp, R) rows, zeros behind them; n_anp keeps the true count, sh_anp_points returns every row.

__global__ void __launch_bounds__(256)
k_wire_records(const sh_landmarks* __restrict__ lm, unsigned char* __restrict__ dst, int R, size_t rec) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* src = (const unsigned long long*)(lm + b);
  unsigned long long* d = (unsigned long long*)(dst + (size_t)b * rec);
  constexpr int HEAD = (int)(SH_REC_HEAD / 8), TAIL = (int)(SH_REC_TAIL / 8), PTS = (int)(sizeof(((sh_landmarks*)0)->anp_points) / 8);
  for (int i = tid; i < HEAD; i += 256) d[i] = src[i];
  for (int i = tid; i < TAIL; i += 256) d[HEAD + i] = src[HEAD + PTS + i];
  int n = lm[b].n_anp;
  n = n < 0 ? 0 : (n > R ? R : n);
  for (int i = tid; i < 3 * R; i += 256) d[HEAD + TAIL + i] = i < 3 * n ? src[HEAD + i] : 0ull;
}

}  // extern "C"

namespace sh {
// records [b0, b0 + n) of the run just enqueued -> dst (device memory, record b at dst + b * rec) on the context's stream
int emit_records(sh_ctx* c, void* dst, int b0, int n, int rows, size_t rec) {
  const sh_landmarks* src = (const sh_landmarks*)c->bufs["landmarks"].p + b0;
  if (rows <= 0) { HIPCHK(c, hipMemcpyAsync((char*)dst + (size_t)b0 * rec, src, (size_t)n * rec, hipMemcpyDeviceToDevice, c->stream)); return SH_OK; }
  LAUNCH(c, "k_wire_records", k_wire_records, dim3(n), dim3(256), src, (unsigned char*)dst + (size_t)b0 * rec, rows, rec);
  return SH_OK;
}
}  // namespace sh

extern "C" {

// every anatomic-neck point of humerus b (CT) of the last run: the rows a packed record cut off, or all of them
__global__ void k_anp_points_ct(const double* __restrict__ pts_obb, const double* __restrict__ T_obb, int b, int n, double* __restrict__ out) {
  double Ti[16];
  inv_transform(T_obb + 16 * b, Ti);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double* p = pts_obb + ((size_t)b * SH_ANP_CAP + i) * 3;
    xform_pt(Ti, p[0], p[1], p[2], out + 3 * (size_t)i);
  }
}

// ---- the staging side of the mesh slot: a stream of NEW batches at the resident rate -------------------------------------------
// The reference's unit of work is a new STL (mesh.py:22-27, bone.py:110-131).  sh_upload_* hands a batch over synchronously:
// host-side validation, pageable copies, a stream synchronize, and hulls that can only start once the run is submitted.  The
// staging calls below do the same hand-over beside a run of the resident batch:
//   sh_stage_meshes / sh_stage_stl   copy the caller's arrays / files through page-locked staging (worker threads) or straight
//                    from page-locked caller memory, enqueue the H2D copies, the validation (on the device) -- for STL files
//                    the parse / vertex-merge kernels of k_stl.h -- and the hull prefilter on the COPY stream, start the
//                    background hull thread, and return;
//   sh_commit_staged waits for the copies (long done when a run was in flight meanwhile), swaps the buffer entries of the two
//                    sides and makes the staged batch the resident one; the next sh_submit finds its hulls prepared.
// One batch can be staged at a time; commit needs the context idle (sh_collect first): the buffers that become the staging side
// are the ones the collected run read.  A rejected batch (bad index, NaN, not an STL) is reported by sh_commit_staged and leaves
// the resident batch untouched.  Records are identical to sh_upload_* + sh_run: same device buffers, same kernels.
// The caller's (pageable) memory -> page-locked staging -> device in 4 MiB pieces (copy_pool): 37 MB of arrays / 104 MB of files per batch.
static hipError_t staged_h2d(void* dev, void* pinned, const void* src, size_t n, hipStream_t st) {
  const size_t chunk = (size_t)4 << 20;
  return copy_pool((n + chunk - 1) / chunk, [=](size_t k) {
    const size_t o = k * chunk, m = std::min(chunk, n - o);
    memcpy((char*)pinned + o, (const char*)src + o, m);
    return hipMemcpyAsync((char*)dev + o, (char*)pinned + o, m, hipMemcpyHostToDevice, st);
  });
}

// where a caller's pointer lives: hipMemoryTypeHost (page-locked), hipMemoryTypeDevice; memory HIP does not know is neither
static bool pointer_is(const void* p, hipMemoryType where) {
  hipPointerAttribute_t at{};
  const bool is = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == where;
  (void)hipGetLastError();
  return is;
}

// The staging side for a batch of at most sumV_cap vertices / sumF_cap faces, `src_bytes` of page-locked staging for the caller's
// memory; the previous staged batch is dropped and the one background job of the context joined first.
static int stage_begin(sh_ctx* c, int B, long long sumV_cap, long long sumF_cap, size_t flag_ints, size_t src_bytes) {
  discard_staged(c);
  (void)join_prepared(c);      // one background job per context
  sh_ctx::StageSide& S = c->stg;
  int rc;
  if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (!S.ready_ev) HIPCHK(c, hipEventCreateWithFlags(&S.ready_ev, hipEventDisableTiming));
  if ((rc = grow_pinned(c, &S.h_flag, &S.h_flag_cap, flag_ints, 4)) != SH_OK) return rc;
  if ((rc = grow_pinned(c, &S.h_kept, &S.h_kept_cap, (size_t)sumV_cap, 12)) != SH_OK) return rc;
  if ((rc = grow_pinned(c, &S.h_koff, &S.h_koff_cap, (size_t)B + 1, 8)) != SH_OK) return rc;
  if ((rc = grow_pinned(c, &S.h_src, &S.h_src_cap, src_bytes, 1, src_bytes / 8)) != SH_OK) return rc;
  ENS_SHARED("verts.s", sumV_cap * 12, 4);
  ENS_SHARED("faces.s", sumF_cap * 12, 4);
  ENS_SHARED("voff.s", (size_t)(B + 1) * 8, 8);
  ENS_SHARED("foff.s", (size_t)(B + 1) * 8, 8);
  ENS_SHARED("stage.flag", 64, 4);
  if ((rc = alloc_hullpre(c, B, sumV_cap, ".s")) != SH_OK) return rc;
  return SH_OK;
}

// what the thread of a staged STL batch works from: the plan, the scratch view and the caller's files (read until the commit returns)
struct StlJob { StlPlan plan; StlView v; std::vector<const void*> files; std::vector<size_t> nbytes; std::vector<char> pinned; };

// The background thread of a staged batch: phase 0 (the caller's memory to the device, the first kernels), for STL files the sizes
// of the merged meshes -> offsets -> k_stl_emit, then hull points through the prefilter, host hulls into pinned slot `prep.key.slot`,
// records to the device as soon as the run in flight no longer reads hull.*.  `hulls` false (device hull): no hull work.
static int start_prepare_staged(sh_ctx* c, int B, std::shared_ptr<const StlJob> stl /*null: arrays*/, std::function<int(std::string*)> phase0) {
  sh_ctx::Prepared& p = c->prep;
  sh_ctx::StageSide& S = c->stg;
  const bool hulls = !device_hull_now(c);
  S.B = B;
  S.meta_ready = false; S.meta_rc = SH_OK; S.meta_err.clear();
  S.h_flag[0] = 0;
  HIPCHK(c, hipEventRecord(S.ready_ev, c->copy_stream));      // (recorded again by the thread behind the last copy / k_stl_emit; this one covers an early discard)
  S.active = true;
  p.key.begin_staged(c->hslot, S.B, c->batch_gen, hulls);
  prepared_reset(p);
  const HullPre hp = hullpre_ptrs(c, ".s");
  const HullRec dst = hull_rec_at(c, 0);      // (the whole batch's, whatever window the context stands at)
  struct Side { long long *voff, *foff; float* verts; int* faces; } side = {(long long*)c->bufs["voff.s"].p, (long long*)c->bufs["foff.s"].p, (float*)c->bufs["verts.s"].p, (int*)c->bufs["faces.s"].p};
  // early upload only into buffers that will not be re-allocated by the commit (alloc_batch grows them for a larger batch)
  const bool can_upload = early_upload_ok(c->obb_done_ev != nullptr, S.B, c->hcap, hull_rec_bytes(c));
  p.th = std::thread([c, hp, dst, side, can_upload, hulls, stl, B, phase0]() {
    sh_ctx::Prepared& q = c->prep;
    sh_ctx::StageSide& S = c->stg;
    auto meta = [&](int rc, const std::string& msg) {
      { std::lock_guard<std::mutex> lk(S.m); S.meta_rc = rc; if (rc != SH_OK) S.meta_err = msg; S.meta_ready = true; }
      S.cv.notify_all();
    };
    auto refuse = [&](int rc, const std::string& msg) { q.rc = rc; meta(rc, msg); };
    if (hipSetDevice(c->device) != hipSuccess) return refuse(SH_ERR_HIP, "hipSetDevice");
    const bool dbg = c->sw.debug;
    const auto tt0 = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tt0).count(); };
    double t_p0 = 0, t_meta = 0, t_pts = 0;
    {      // phase 0: the caller's memory -> page-locked staging, the copies and the first kernels enqueued (the staging call has returned)
      std::string et;
      const int rc0 = phase0(&et);
      if (rc0 != SH_OK) return refuse(rc0, et);
      if (!stl) meta(SH_OK, "");
      t_p0 = since();
    }
    if (stl) {
      if (hipEventSynchronize(c->stl_counted_ev) != hipSuccess) return refuse(SH_ERR_HIP, "sh_stage_stl: the parse kernels failed");
      MeshSizes sz;      // S.h_flag + 16: [2 B] merged vertices, faces per file, [B] non-finite words behind them
      const IngestError e = stl_counted(S.h_flag + 16, S.h_flag + 16 + 2 * B, B, &S.voff, &S.foff, &sz);
      if (e.code != SH_OK) return refuse(e.code, std::string("sh_stage_stl: ") + e.text);
      S.maxV = sz.maxV; S.maxF = sz.maxF; S.sumV = sz.sumV; S.sumF = sz.sumF;
      hipStream_t st = c->copy_stream;
      std::string et;
      if (hipMemcpyAsync(side.voff, S.voff.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
          hipMemcpyAsync(side.foff, S.foff.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
          stl_enqueue_emit(nullptr, st, B, stl->plan, stl->v, side.voff, side.foff, side.verts, side.faces, &et) != SH_OK || hipEventRecord(S.ready_ev, st) != hipSuccess)
        return refuse(SH_ERR_HIP, "sh_stage_stl: enqueueing the merge failed");
      meta(SH_OK, "");
      t_meta = since();
    }
    if (!hulls) return;
    {
      auto t0 = std::chrono::steady_clock::now();
      if (fetch_prefiltered(hp, B, S.sumV, S.h_koff, S.h_kept, &S.pts, c->copy_stream) != hipSuccess) { q.rc = SH_ERR_HIP; return; }
      q.d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    t_pts = since();
    if (!stl && S.h_flag[0] != 0) { q.rc = SH_ERR_ARG; return; }      // (the validation word came back in front of the survivors; the commit reports it)
    prepared_hulls(c, S.pts, dst, can_upload);
    if (dbg) fprintf(stderr, "[sh] staged batch: copies enqueued %.2f ms, sizes known %.2f, hull points back %.2f, hulls done and uploaded %.2f (hull phase %.2f)\n", t_p0, t_meta, t_pts, since(), q.hull_ms);
  });
  return SH_OK;
}

int sh_stage_meshes(sh_ctx* c, const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int B) {
  if (!c || !verts || !faces || !v_off || !f_off || B <= 0) return fail(c, SH_ERR_ARG, "sh_stage_meshes: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  MeshSizes sz;
  const IngestError e = check_mesh_arrays(v_off, f_off, B, nullptr, nullptr, &sz);      // (the elements are checked on the device)
  if (e.code != SH_OK) return ingest_fail(c, "sh_stage_meshes", e);
  // the caller's arrays -> page-locked memory (unless they are page-locked already) -> device, all by the background thread: the
  // caller keeps its arrays unchanged until sh_commit_staged has returned
  const size_t vb = (size_t)sz.sumV * 12, fb = (size_t)sz.sumF * 12, vpad = (vb + 255) & ~(size_t)255;
  const bool vpin = pointer_is(verts, hipMemoryTypeHost), fpin = pointer_is(faces, hipMemoryTypeHost);
  int rc;
  if ((rc = stage_begin(c, B, sz.sumV, sz.sumF, 64, (vpin ? 0 : vpad) + (fpin ? 0 : fb))) != SH_OK) return rc;
  sh_ctx::StageSide& S = c->stg;
  S.sumV = sz.sumV; S.sumF = sz.sumF; S.maxV = sz.maxV; S.maxF = sz.maxF; S.from_stl = false;
  S.voff.assign(v_off, v_off + B + 1); S.foff.assign(f_off, f_off + B + 1);
  void *dv = c->bufs["verts.s"].p, *df = c->bufs["faces.s"].p, *dvo = c->bufs["voff.s"].p, *dfo = c->bufs["foff.s"].p;
  int* flag = (int*)c->bufs["stage.flag"].p;
  const dim3 grid((unsigned)std::min<long long>((3 * std::max(sz.maxV, sz.maxF) + 255) / 256, 256), (unsigned)B);
  auto phase0 = [=](std::string* et) -> int {
    sh_ctx::StageSide& S = c->stg;
    hipStream_t st = c->copy_stream;
    if (vpin) HIPCHK_TXT(et, hipMemcpyAsync(dv, verts, vb, hipMemcpyHostToDevice, st));
    else HIPCHK_TXT(et, staged_h2d(dv, S.h_src, verts, vb, st));
    if (fpin) HIPCHK_TXT(et, hipMemcpyAsync(df, faces, fb, hipMemcpyHostToDevice, st));
    else HIPCHK_TXT(et, staged_h2d(df, (char*)S.h_src + (vpin ? 0 : vpad), faces, fb, st));
    HIPCHK_TXT(et, hipMemcpyAsync(dvo, S.voff.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK_TXT(et, hipMemcpyAsync(dfo, S.foff.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK_TXT(et, hipMemsetAsync(flag, 0, 4, st));
    hipLaunchKernelGGL(k_validate_meshes, grid, dim3(256), 0, st, (const float*)dv, (const int*)df, (const long long*)dvo, (const long long*)dfo, flag);
    HIPCHK_TXT(et, hipGetLastError());
    HIPCHK_TXT(et, hipMemcpyAsync(S.h_flag, flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK_TXT(et, hipEventRecord(S.ready_ev, st));
    return SH_OK;
  };
  return start_prepare_staged(c, B, nullptr, phase0);
}

int sh_stage_stl(sh_ctx* c, const void* const* files, const size_t* nbytes, int B) {
  if (!c || !files || !nbytes || B <= 0) return fail(c, SH_ERR_ARG, "sh_stage_stl: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  auto job = std::make_shared<StlJob>();
  StlPlan& plan = job->plan;
  const IngestError e = stl_plan(files, nbytes, B, &plan);
  if (e.code != SH_OK) return ingest_fail(c, "sh_stage_stl", e);
  // the merged meshes are at most as large as the corner lists: the staging side is sized by that bound, the true offsets are
  // made by the thread once the device has counted.  Page-locked staging: one image of the files (their starts 4-byte aligned) + the
  // two offset tables behind it
  const size_t tab_off = ((size_t)plan.file_off[B] + 255) & ~(size_t)255;
  int rc;
  if ((rc = stage_begin(c, B, plan.sumC, plan.sumC / 3, 16 + 3 * (size_t)B, tab_off + 2 * (size_t)(B + 1) * 8)) != SH_OK) return rc;
  if ((rc = stl_scratch(c, B, plan, &job->v)) != SH_OK) return rc;
  sh_ctx::StageSide& S = c->stg;
  long long* h_tabs = (long long*)((char*)S.h_src + tab_off);
  memcpy(h_tabs, plan.file_off.data(), (size_t)(B + 1) * 8);
  memcpy(h_tabs + B + 1, plan.coff.data(), (size_t)(B + 1) * 8);
  S.from_stl = true; S.sumV = S.sumF = S.maxV = S.maxF = 0;
  if (!c->stl_counted_ev) HIPCHK(c, hipEventCreateWithFlags(&c->stl_counted_ev, hipEventDisableTiming));
  // the files themselves are read by the background thread: the caller keeps them unchanged until sh_commit_staged has returned
  job->files.assign(files, files + B); job->nbytes.assign(nbytes, nbytes + B); job->pinned.resize(B);
  for (int b = 0; b < B; ++b) job->pinned[b] = pointer_is(files[b], hipMemoryTypeHost) ? 1 : 0;
  std::shared_ptr<const StlJob> a = job;
  auto phase0 = [c, a, h_tabs, B](std::string* et) -> int {
    sh_ctx::StageSide& S = c->stg;
    hipStream_t st = c->copy_stream;
    const StlView& v = a->v;
    // file by file: page-locked files go as they are, the others through the staging image; each file's H2D follows its memcpy at once
    HIPCHK_TXT(et, copy_pool((size_t)B, [&](size_t b) {
      char* img = (char*)S.h_src + a->plan.file_off[b];
      if (!a->pinned[b]) memcpy(img, a->files[b], a->nbytes[b]);
      const void* src = a->pinned[b] ? a->files[b] : img;
      return hipMemcpyAsync(v.raw + a->plan.file_off[b], src, a->nbytes[b], hipMemcpyHostToDevice, st);
    }));
    HIPCHK_TXT(et, hipMemcpyAsync(v.file_off, h_tabs, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK_TXT(et, hipMemcpyAsync(v.coff, h_tabs + B + 1, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    const int rc = stl_enqueue_parse(nullptr, st, B, a->plan, v, et);
    if (rc != SH_OK) return rc;
    HIPCHK_TXT(et, hipMemcpyAsync(S.h_flag + 16, v.counts, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_TXT(et, hipMemcpyAsync(S.h_flag + 16 + 2 * B, v.nonfinite, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK_TXT(et, hipEventRecord(c->stl_counted_ev, st));
    return SH_OK;
  };
  return start_prepare_staged(c, B, a, phase0);
}

int sh_commit_staged(sh_ctx* c, int64_t* v_off_out, int64_t* f_off_out) {
  if (!c) return SH_ERR_ARG;
  sh_ctx::StageSide& S = c->stg;
  if (!S.active) return fail(c, SH_ERR_STATE, "sh_commit_staged: no batch is staged");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_commit_staged: runs are in flight (sh_collect them first: they read the buffers that become the staging side)");
  HIPCHK(c, hipSetDevice(c->device));
  { std::unique_lock<std::mutex> lk(S.m); S.cv.wait(lk, [&] { return S.meta_ready; }); }
  if (S.meta_rc != SH_OK) { const int rc = S.meta_rc; const std::string msg = S.meta_err; discard_staged(c); return fail(c, rc, msg); }
  HIPCHK(c, hipEventSynchronize(S.ready_ev));
  if (!S.from_stl && S.h_flag[0] != 0) {
    const int f = S.h_flag[0];
    discard_staged(c);
    return fail(c, SH_ERR_ARG, (f & 1) ? "sh_stage_meshes: face index out of range" : "sh_stage_meshes: NaN / infinite vertex coordinate");
  }
  // a resident-overlap preparation cannot be under way (staging joined it); the staged batch's own thread keeps running
  offsets_out(S.voff, v_off_out); offsets_out(S.foff, f_off_out);
  MeshSizes sz;
  sz.sumV = S.sumV; sz.sumF = S.sumF; sz.maxV = S.maxV; sz.maxF = S.maxF;
  S.active = false;
  ResidentSource src;
  src.staged = true;
  return make_resident(c, S.B, sz, S.voff, S.foff, src);
}

int sh_staged(const sh_ctx* c) { return c ? (c->stg.active ? 1 : 0) : SH_ERR_ARG; }

// the status block of a run (sh_demand.h StatusBlock) from the live words, one launch
__global__ void k_stage_status(const int* __restrict__ err, const unsigned long long* __restrict__ ovf_ctr, const int* __restrict__ hull_fail /*or null*/, StatusBlock dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < dst.B) { dst.err()[i] = err[i]; dst.gave_up()[i] = hull_fail ? hull_fail[i] : 0; }
  if (i < SH_NCTR) dst.words()[i] = ovf_ctr[i];
}

// The device hull gave humeri up during the run of ticket `tk` (st.gave_up(); k_hull.h writes a unit tetrahedron for them, so
// everything queued behind ran on finite data and their records are void).  Each of them gets the host quickhull -- which
// has the retry / joggle logic -- its record goes into the device buffers where the device hull would have put it, and its
// stages run again as a window of one humerus.  All of it is enqueued on the context's stream: behind a second run that may
// be in flight (which finished with this batch's scratch buffers by then, and has parked its own results per ticket).
// hulld.skip[b] is set, so later runs of the resident batch get these humeri right the first time.
// *again: SH_RERUN_NONE when the records are complete, else why the whole batch has to run again (and with which capacities).
static int redo_given_up(sh_ctx* c, sh_ctx::Ticket& tk, const StatusBlock& st, const std::string& tslot, Verdict* again) {
  const int B = tk.B;
  if (std::none_of(st.gave_up(), st.gave_up() + B, [](int f) { return f != 0; })) return SH_OK;
  std::vector<float> hv32;
  HostHull hh;
  int rc = SH_OK;
  WindowScope whole(c, 0, B);      // (the copies below index the batch's buffers by humerus)
  for (int b = 0; b < B; ++b) {
    if (st.gave_up()[b] == 0) continue;
    const long long v0 = c->h_voff[b], nv = c->h_voff[b + 1] - v0;
    hv32.resize(3 * (size_t)nv);
    HIPCHK(c, hipMemcpyAsync(hv32.data(), (const float*)c->bufs["verts"].p + 3 * v0, (size_t)nv * 12, hipMemcpyDeviceToHost, c->out_stream));
    HIPCHK(c, hipStreamSynchronize(c->out_stream));
    if (!hull_of_points(hv32.data(), nv, hh)) return fail(c, SH_ERR_GEOMETRY, hull_failed_text(b, SH_ERR_GEOMETRY));
    const int fn = hh.n.f;
    if (!hull_fits(hh.n, c->hcap)) {
      // above the record: growing it here would drop the other humeri's records -- the batch runs again with its hulls from the
      // host (hull_host_phase sizes the staging, run_obb grows the record), and stays there while it is resident
      c->batch.hull_above_record();
      again->rerun = SH_RERUN_FORCE_HOST;
      return SH_OK;
    }
    const int one = 1;
    {
      WindowScope alone(c, b, 1);      // humerus b as a window of one: the hull record's rows, its status words and its stages
      HIPCHK(c, hull_upload_one(hh, hull_rec(c), c->stream));      // (pageable sources, as `one`: hipMemcpyAsync stages them before it returns)
      HIPCHK(c, hipMemcpyAsync(buf<int>(c, "hulld.skip"), &one, 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemsetAsync(buf<int>(c, "err"), 0, 4, c->stream));
      if (c->open_mode != SH_OPEN_ERROR) HIPCHK(c, hipMemsetAsync(buf<int>(c, "open.stats"), 0, 8, c->stream));      // (the void first pass counted too)
      HIPCHK(c, hipStreamSynchronize(c->stream));      // the sources above are locals
      c->batch.redo_used_faces(fn);
      rc = run_window(c, tk.mask, -1, fn);
    }
    if (rc != SH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    // the record and the status word of this humerus -> where the run's results were parked (or the caller's device buffer)
    if (void* dst = tk.host_out ? c->bufs["out.landmarks" + tslot].p : (void*)tk.out_arg) { int erc = emit_records(c, dst, b, 1, tk.rows, tk.rec); if (erc != SH_OK) return erc; }
    HIPCHK(c, hipMemcpyAsync((int*)c->bufs["out.err" + tslot].p + b, buf<int>(c, "err") + b, 4, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // The one-humerus windows above drew on the pools past sh_collect's check of the status block.  A dense humerus (the kind the device
  // hull gives up) may have asked for more than they hold (k_ovf_plan flagged it SH_ERR_CAPACITY_DEV), or its host hull for more than
  // the k_obb_candidates tier does: the live words get the same verdict, sh_collect raises the capacities and runs the whole batch
  // again (hulld.skip keeps the device hull off these humeri by then).
  unsigned long long ctr[SH_NCTR];
  HIPCHK(c, hipMemcpyAsync(ctr, c->bufs["ovf.ctr"].p, sizeof ctr, hipMemcpyDeviceToHost, c->out_stream));
  HIPCHK(c, hipStreamSynchronize(c->out_stream));
  *again = demand_verdict(ctr, c->batch.caps(), (tk.mask & SH_STAGE_OBB) != 0, tk.gen == c->batch_gen);
  if (again->rerun != SH_RERUN_NONE) return SH_OK;
  if (tk.host_out)
    HIPCHK(c, hipMemcpyAsync(tk.host_out, c->bufs["out.landmarks" + tslot].p, (size_t)B * tk.rec, hipMemcpyDeviceToHost, c->out_stream));
  HIPCHK(c, hipMemcpyAsync(tk.status, c->bufs["out.err" + tslot].p, (size_t)B * 4, hipMemcpyDeviceToHost, c->out_stream));
  HIPCHK(c, hipStreamSynchronize(c->out_stream));
  return SH_OK;
}

// the pinned status block of a ticket (StatusBlock: ONE device-to-host copy and one wait in sh_collect) and its event
static int ticket_setup(sh_ctx* c, sh_ctx::Ticket& tk, int B) {
  if (tk.cap < B) {
    if (tk.status) (void)hipHostFree(tk.status);
    tk.status = nullptr; tk.cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&tk.status, StatusBlock::bytes(B)));
    tk.cap = B;
  }
  if (!tk.ev) HIPCHK(c, hipEventCreateWithFlags(&tk.ev, hipEventDisableTiming));
  return SH_OK;
}

// A submit reads: precheck -> tickets and staging buffers -> clears -> prepared hand-over and plan (the plan needs the preparation's
// rc, which exists behind the join; the join stays behind the clears so that the device has them while the host waits) -> windows ->
// overlap -> park the results -> ticket.  The decisions are sh_run.h's.
int sh_submit(sh_ctx* c, uint32_t mask, sh_landmarks* out) {
  if (!c) return SH_ERR_ARG;
  // a refused submit enqueues nothing, allocates nothing and leaves "err", "ovf.ctr", "open.stats" and open_stats_run as they were
  RunFacts facts{c->B, c->n_pending, (int)c->params.bone_kind, c->hull_mode, c->sw.window, c->overlap, c->stg.active, c->batch_gen, c->hslot, &c->batch, c->prep.key, SH_OK};
  if (const RunError e = precheck_submit(mask, facts); e.code != SH_OK) return fail(c, e.code, e.text);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  // (`out` may also be device memory, e.g. the send buffer of a gather)
  const bool out_on_device = out && pointer_is(out, hipMemoryTypeDevice);
  sh_ctx::Ticket& tk = c->tickets[c->t_head];
  if (int e = ticket_setup(c, tk, B)) return e;
  // the other ticket's pinned block, event and device staging with the first one (else the context's SECOND run pays for them)
  if (sh_ctx::Ticket& to = c->tickets[c->t_head ^ 1]; !to.pending) {
    if (int e = ticket_setup(c, to, B)) return e;
    const std::string oslot = std::to_string(c->t_head ^ 1);
    if (int e = ensure(c, ("out.err" + oslot).c_str(), StatusBlock::bytes(B), 4)) return e;
    if (out && !out_on_device) { if (int e = ensure(c, ("out.landmarks" + oslot).c_str(), (size_t)B * rec_bytes_rows(c->rec_rows), 1)) return e; }
  }
  if (!c->out_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->out_stream, hipStreamNonBlocking));
  c->b0 = 0; c->Bwin = B;
  if (c->params.bone_kind == SH_BONE_PROXIMAL) { if (int e = alloc_prox(c)) return e; }
  { OvfPools OP; int orc = ovf_pools(c, &OP); if (orc != SH_OK) return orc; FILL(c, {buf<int>(c, "err"), (size_t)B * 4, 0}, {OP.ctr, SH_NCTR * 8, 0}); }      // overflow pools: empty, no demand recorded
  if (c->open_mode != SH_OPEN_ERROR) FILL(c, {buf<int>(c, "open.stats"), (size_t)B * 8, 0});      // (bridge mode only: the default run has no extra fill)
  c->open_stats_run = c->open_mode;
  // hulls prepared by the background thread during the previous run (sh_set_overlap)?  Windows: with the host hull in play the batch
  // can be walked in windows of SHOULDER_WINDOW humeri; all device work of a window is only enqueued, so the hulls of the next window
  // are computed while it runs (off by default; tests exercise small windows).
  facts.prep_rc = join_prepared(c);
  const RunPlan plan = run_plan(mask, facts);
  c->hslot = plan.next_hslot;
  if (plan.void_staged_hulls) c->prep.key.void_hulls();
  if (plan.fetch_points) {
    // the host hull needs its points (a device-generated batch: every run, a new batch is new data)
    auto t0 = std::chrono::steady_clock::now();
    HIPCHK(c, fetch_hull_points(c, hullpre_ptrs(c), c->stream));
    if (c->sw.debug) fprintf(stderr, "[sh] submit: hull points fetched after %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (c->timing && !c->h_verts_valid) { KTimer& a = c->timers["host.verts_d2h"]; a.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); a.n += 1; }
  }
  int rc = SH_OK, widx = 0;
  for (int b0 = 0; b0 < B && rc == SH_OK; b0 += plan.win, ++widx) {
    WindowScope w(c, b0, std::min(plan.win, B - b0));
    rc = run_window(c, mask, widx == 0 ? plan.prepared_slot : -1);
  }
  // everything of this run is enqueued: the host is free until the device is done -> hulls of the next run (of the whole batch again)
  if (rc == SH_OK && plan.start_overlap) start_prepare(c);
  c->batch.run_enqueued(mask);
  if (rc != SH_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  // Results.  A device-to-host copy enqueued HERE would sit in a DMA queue until the kernels of this run are done and hold
  // up every later copy behind it - the vertex read-back of the background hull thread above all, which then loses its
  // overlap with the device (measured: 14.3 -> 19.2 ms per step at B=64).  So the records and status words are parked in a
  // per-ticket device buffer (a 16 us device-to-device copy at the end of the run) and sh_collect copies them to the host
  // once the run has finished.  Device `out` (the send buffer of a gather) is written directly.
  const std::string tslot = std::to_string(c->t_head);
  void *lm_stage = nullptr, *err_stage = nullptr;
  if (int e = ensure(c, ("out.err" + tslot).c_str(), StatusBlock::bytes(B), 4, &err_stage)) return e;      // (the whole status block: the status words lead it)
  tk.host_out = nullptr;
  tk.rows = c->rec_rows; tk.rec = rec_bytes_rows(c->rec_rows);
  if (out_on_device) {
    if (int e = emit_records(c, out, 0, B, tk.rows, tk.rec)) return e;
  } else if (out) {
    if (int e = ensure(c, ("out.landmarks" + tslot).c_str(), (size_t)B * tk.rec, 1, &lm_stage)) return e;
    if (int e = emit_records(c, lm_stage, 0, B, tk.rows, tk.rec)) return e;
    tk.host_out = out;
  }
  // status words, what the run asked of the overflow pools (k_ovf.h: sh_collect grows them and runs again if it was more than they
  // hold) and which humeri the device hull gave up (its own word per humerus: the status word can be overwritten by a later stage)
  LAUNCH(c, "k_stage_status", k_stage_status, dim3((unsigned)((std::max(B, (int)SH_NCTR) + 255) / 256)), dim3(256), (const int*)buf<int>(c, "err"), (const unsigned long long*)c->bufs["ovf.ctr"].p,
         plan.dev_hull ? (const int*)buf<int>(c, "hulld.fail") : (const int*)nullptr, StatusBlock{(char*)err_stage, B});
  HIPCHK(c, hipEventRecord(tk.ev, c->stream));
  tk.B = B; tk.pending = true; tk.mask = mask; tk.out_arg = out; tk.dev_hull = plan.dev_hull; tk.gen = c->batch_gen;
  c->arthro.run_submitted(mask, c->batch_gen);
  c->t_head ^= 1; ++c->n_pending;
  return SH_OK;
}

int sh_collect(sh_ctx* c) {
  if (!c) return SH_ERR_ARG;
  if (c->n_pending == 0) return fail(c, SH_ERR_STATE, "sh_collect: nothing in flight");
  HIPCHK(c, hipSetDevice(c->device));
  sh_ctx::Ticket& tk = c->tickets[c->t_tail];
  const std::string tslot = std::to_string(c->t_tail);
  c->t_tail ^= 1; --c->n_pending; tk.pending = false;
  HIPCHK(c, hipEventSynchronize(tk.ev));
  if (tk.host_out)
    HIPCHK(c, hipMemcpyAsync(tk.host_out, buf<char>(c, ("out.landmarks" + tslot).c_str()), (size_t)tk.B * tk.rec, hipMemcpyDeviceToHost, c->out_stream));
  HIPCHK(c, hipMemcpyAsync(tk.status, buf<char>(c, ("out.err" + tslot).c_str()), StatusBlock::bytes(tk.B), hipMemcpyDeviceToHost, c->out_stream));      // status, demand block, give-up words
  HIPCHK(c, hipStreamSynchronize(c->out_stream));
  const StatusBlock st{tk.status, tk.B};
  const unsigned long long* w = st.words();
  c->batch.run_collected(w, tk.mask, (int)c->params.bone_kind, tk.gen, c->batch_gen);      // (may it vouch that the overflow tier is idle?)
  const DemandCaps& cap = c->batch.caps();
  if (c->sw.debug) fprintf(stderr, "[sh] collect: ovf need %llu %llu %llu cap %llu %llu %llu err0 %d\n", w[SH_CTR_SEG_NEED], w[SH_CTR_RING_NEED], w[SH_CTR_WORK_NEED], cap.seg, cap.ring, cap.work, st.err()[0]);
  // Are the records valid as far as capacity goes?  The status block's demand words first; then the humeri the device hull gave up
  // are done again alone, and their one-humerus windows may raise a demand of their own.
  Verdict v = demand_verdict(w, cap, (tk.mask & SH_STAGE_OBB) != 0, tk.gen == c->batch_gen);
  const bool redo = v.rerun == SH_RERUN_NONE && tk.dev_hull;
  if (redo) { if (int e = redo_given_up(c, tk, st, tslot, &v)) return e; }
  if (v.rerun != SH_RERUN_NONE) {
    // The records of this run are void: the whole batch again, with what it asked for -- here, synchronously, when nothing else is
    // in flight.
    c->batch.rerun_decided(v, redo);
    if (c->n_pending != 0) return fail(c, SH_ERR_CAPACITY, rerun_refusal_text(v.rerun));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool ends_grow = c->batch.rerun_granted(v);
    if (v.error) return fail(c, SH_ERR_CAPACITY, v.error);
    if (ends_grow) {
      const size_t eb = (size_t)c->B * 2 * cap.end * 2 * 8;
      if (int e = ensure(c, "obb.endpts", eb, 8)) return e;
      c->bufs["obb.endpts"].per_mesh = eb / (size_t)c->B;
    }
    if (int e = sh_submit(c, tk.mask, tk.out_arg)) return e;
    return sh_collect(c);
  }
  for (int b = 0; b < tk.B; ++b)
    if (st.err()[b] != 0) {
      char m[128];
      snprintf(m, sizeof m, "mesh %d: device stage error %d (capacity=-4, geometry=-5)", b, st.err()[b]);
      return fail(c, st.err()[b], m);
    }
  return SH_OK;
}

int sh_run(sh_ctx* c, uint32_t mask, sh_landmarks* out) {
  if (!c) return SH_ERR_ARG;
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_run: submitted runs are still in flight (sh_collect them first)");
  int rc = sh_submit(c, mask, out);
  if (rc != SH_OK) return rc;
  rc = sh_collect(c);
  if (rc == SH_OK) HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

// Page-locked host memory for result buffers the caller reuses from run to run (a fresh pageable buffer per run costs a
// page fault per 4 KB plus a staged copy: ~1 ms for the 6.8 MB of 64 landmark records).
int sh_host_alloc(sh_ctx* c, size_t nbytes, void** out) {
  if (!c || !out || nbytes == 0) return fail(c, SH_ERR_ARG, "sh_host_alloc: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostMalloc(out, nbytes));
  return SH_OK;
}

int sh_host_free(sh_ctx* c, void* p) {
  if (!c) return SH_ERR_ARG;
  if (p) HIPCHK(c, hipHostFree(p));
  return SH_OK;
}

int sh_set_keep_products(sh_ctx* c, int on) {
  if (!c) return SH_ERR_ARG;
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_set_keep_products: runs are in flight");
  c->keep_products = on != 0;
  return SH_OK;
}

// ---- open contours (k_open.h) ---------------------------------------------------------------------------
int sh_set_open_contours(sh_ctx* c, int mode, double max_gap) {
  if (!c) return SH_ERR_ARG;
  if (mode != SH_OPEN_ERROR && mode != SH_OPEN_BRIDGE) return fail(c, SH_ERR_ARG, "sh_set_open_contours: mode is SH_OPEN_ERROR or SH_OPEN_BRIDGE");
  if (!std::isfinite(max_gap) || max_gap < 0.0) return fail(c, SH_ERR_ARG, "sh_set_open_contours: max_gap must be finite and >= 0");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_set_open_contours: runs are in flight");
  c->open_mode = mode; c->open_gap = max_gap;
  return SH_OK;
}
int sh_get_open_contours(const sh_ctx* c, int* mode, double* max_gap) {
  if (!c) return SH_ERR_ARG;
  if (mode) *mode = c->open_mode;
  if (max_gap) *max_gap = c->open_gap;
  return SH_OK;
}
int sh_open_contour_stats(sh_ctx* c, int32_t* bridged, int32_t* dropped) {
  if (!c || !bridged || !dropped) return fail(c, SH_ERR_ARG, "sh_open_contour_stats: bad argument");
  if (c->B < 1) return fail(c, SH_ERR_STATE, "sh_open_contour_stats: no meshes uploaded");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_open_contour_stats: runs are in flight (sh_collect them first)");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int32_t> h((size_t)c->B * 2, 0);
  if (c->open_stats_run != SH_OPEN_ERROR) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h.data(), c->bufs["open.stats"].p, h.size() * 4, hipMemcpyDeviceToHost));
  }
  for (int b = 0; b < c->B; ++b) { bridged[b] = h[2 * (size_t)b]; dropped[b] = h[2 * (size_t)b + 1]; }
  return SH_OK;
}
int sh_mesh_open_edges(sh_ctx* c, int64_t* out) {
  if (!c || !out) return fail(c, SH_ERR_ARG, "sh_mesh_open_edges: bad argument");
  if (c->B < 1) return fail(c, SH_ERR_STATE, "sh_mesh_open_edges: no meshes uploaded");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_mesh_open_edges: runs are in flight (sh_collect them first)");
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  std::vector<long long> toff((size_t)B + 1, 0);      // per mesh a power of two >= 4 F_b slots (k_edge_insert)
  for (int b = 0; b < B; ++b) {
    const long long nf = c->h_foff[b + 1] - c->h_foff[b];
    long long t = 64;
    while (t < 4 * nf) t <<= 1;
    toff[b + 1] = toff[b] + t;
  }
  int rc;
  if ((rc = ensure(c, "open.ekeys", (size_t)toff[B] * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "open.euses", (size_t)toff[B] * 4, 4)) != SH_OK) return rc;
  if ((rc = ensure(c, "open.etoff", ((size_t)B + 1) * 8, 8)) != SH_OK) return rc;
  if ((rc = ensure(c, "open.ecount", (size_t)B * 8, 8)) != SH_OK) return rc;
  for (const char* n : {"open.ekeys", "open.euses", "open.etoff", "open.ecount"}) c->bufs[n].per_mesh = 0;
  unsigned long long* keys = (unsigned long long*)c->bufs["open.ekeys"].p;
  int* uses = (int*)c->bufs["open.euses"].p;
  long long* dtoff = (long long*)c->bufs["open.etoff"].p;
  unsigned long long* cnt = (unsigned long long*)c->bufs["open.ecount"].p;
  HIPCHK(c, hipMemcpyAsync(dtoff, toff.data(), toff.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(keys, 0xFF, (size_t)toff[B] * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(uses, 0, (size_t)toff[B] * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(cnt, 0, (size_t)B * 8, c->stream));
  WindowScope whole(c, 0, c->Bwin);      // (whole batch)
  LAUNCH(c, "k_edge_insert", k_edge_insert, dim3((unsigned)std::min<long long>((c->maxF + 255) / 256, 1024), (unsigned)B), dim3(256),
         (const int*)c->bufs["faces"].p, (const long long*)c->bufs["foff"].p, (const long long*)dtoff, keys, uses);
  long long tmax = 0;
  for (int b = 0; b < B; ++b) tmax = std::max(tmax, toff[b + 1] - toff[b]);
  LAUNCH(c, "k_edge_count_open", k_edge_count_open, dim3((unsigned)std::min<long long>((tmax + 255) / 256, 1024), (unsigned)B), dim3(256),
         (const long long*)dtoff, (const unsigned long long*)keys, (const int*)uses, cnt);
  std::vector<unsigned long long> h((size_t)B);
  HIPCHK(c, hipMemcpyAsync(h.data(), cnt, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < B; ++b) out[b] = (int64_t)h[b];
  for (const char* n : {"open.ekeys", "open.euses", "open.etoff", "open.ecount"}) {      // on demand: the tables (12 B per slot) do not stay
    auto it = c->bufs.find(n);
    if (it != c->bufs.end()) { if (it->second.p) (void)hipFree(it->second.p); c->bufs.erase(it); }
  }
  return SH_OK;
}

int sh_set_record_rows(sh_ctx* c, int anp_rows) {
  if (!c || anp_rows < 0 || anp_rows > SH_ANP_MAX_PTS) return fail(c, SH_ERR_ARG, "sh_set_record_rows: 0 (full records) .. 4096 rows");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_set_record_rows: runs are in flight");
  c->rec_rows = anp_rows;
  return SH_OK;
}

size_t sh_record_bytes(int anp_rows) { return rec_bytes_rows(anp_rows); }

int sh_anp_points(sh_ctx* c, int b, double* out, int cap, int* n_out) {
  if (!c || !n_out || b < 0 || b >= c->B || cap < 0 || (cap > 0 && !out)) return fail(c, SH_ERR_ARG, "sh_anp_points: bad argument");
  if (c->n_pending != 0) return fail(c, SH_ERR_STATE, "sh_anp_points: runs are in flight (sh_collect them first)");
  if (c->bufs.find("anp.counts") == c->bufs.end()) return fail(c, SH_ERR_STATE, "sh_anp_points: no run yet");
  HIPCHK(c, hipSetDevice(c->device));
  c->b0 = 0; c->Bwin = c->B;
  int cnt[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(cnt, buf<int>(c, "anp.counts") + 2 * b, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int n = std::min(cnt[0], (int)SH_ANP_CAP);
  *n_out = n;
  n = std::min(n, cap);
  if (n <= 0) return SH_OK;
  int rc = ensure(c, "anp.points_ct_one", (size_t)SH_ANP_CAP * 24, 8);
  if (rc != SH_OK) return rc;
  c->bufs["anp.points_ct_one"].per_mesh = 0;
  double* d = (double*)c->bufs["anp.points_ct_one"].p;
  LAUNCH(c, "k_anp_points_ct", k_anp_points_ct, dim3((unsigned)((n + 255) / 256)), dim3(256), (const double*)buf<double>(c, "anp.points_obb"), (const double*)buf<double>(c, "obb_transform"), b, n, d);
  HIPCHK(c, hipMemcpyAsync(out, d, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_landmarks_device(sh_ctx* c, void** p, size_t* n) {
  if (!c || !p || !n) return SH_ERR_ARG;
  *p = buf<void>(c, "landmarks");
  *n = (size_t)c->B * sizeof(sh_landmarks);
  return *p ? SH_OK : SH_ERR_STATE;
}

// ---- parameters (sh_params.h: the layout of the block, the forest check, ParamState) --------------------------------------------------
// every section between the block at `p` and a mirror laid out for it; `up`: host to device
static int copy_block(sh_ctx* c, char* p, ParamMirror& m, const ParamLayout& L, bool up) {
  hipError_t copied = hipSuccess;
  m.each(L, [&](void* host, size_t off, size_t n) {
    if (n && copied == hipSuccess) copied = up ? hipMemcpyAsync(p + off, host, n, hipMemcpyHostToDevice, c->stream) : hipMemcpyAsync(host, p + off, n, hipMemcpyDeviceToHost, c->stream);
  });
  HIPCHK(c, copied);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// the whole block again from the mirrors, at the loaded shape.  A failure leaves nothing loaded: the block may be gone (ensure frees
// it before it allocates), so neither half may stay "loaded" over it
static int upload_params(sh_ctx* c) {
  c->pstate.block_exposed();
  const ParamLayout L(c->pstate.shape());
  int rc = ensure(c, "params", L.total ? L.total : 16, 4);
  if (rc == SH_OK) rc = copy_block(c, buf<char>(c, "params"), c->mirror, L, true);
  if (rc != SH_OK) { c->pstate.block_lost(); c->mirror = ParamMirror(); c->ulayers.clear(); }
  return rc;
}

int sh_load_rfc(sh_ctx* c, const int32_t* feat, const float* thr, const int32_t* ti, const int32_t* fi, const float* lw, int n_nodes,
                const int32_t* roots, int n_trees) {
  if (!c || !feat || !thr || !ti || !fi || !lw || !roots || n_nodes <= 0 || n_trees <= 0) return fail(c, SH_ERR_ARG, "sh_load_rfc: bad argument");
  const ParamError e = forest_check(feat, ti, fi, n_nodes, roots, n_trees);
  if (e.code != SH_OK) return fail(c, e.code, std::string("sh_load_rfc: ") + e.text);
  HIPCHK(c, hipSetDevice(c->device));
  ParamMirror& m = c->mirror;
  m.feat.assign(feat, feat + n_nodes); m.thr.assign(thr, thr + n_nodes); m.ti.assign(ti, ti + n_nodes);
  m.fi.assign(fi, fi + n_nodes); m.lw.assign(lw, lw + n_nodes); m.roots.assign(roots, roots + n_trees);
  c->pstate.rfc_loaded(n_nodes, n_trees);
  return upload_params(c);
}

int sh_load_unet(sh_ctx* c, int base, int depth, const float* packed, size_t n_floats) {
  // The layer table is built aside and swapped in together with the parameters only after the size check: a rejected
  // call leaves the loaded network (table, host copy, device block) as it was.
  UnetLayers layers;
  size_t o = 0;
  if (!c || !packed || unet_layer_table(base, depth, &layers, &o).code != SH_OK) return fail(c, SH_ERR_ARG, SH_UNET_SHAPE_REFUSAL);
  HIPCHK(c, hipSetDevice(c->device));
  if (o != n_floats) {
    char m[160];
    snprintf(m, sizeof m, "sh_load_unet: expected %zu floats for base=%d depth=%d, got %zu", o, base, depth, n_floats);
    return fail(c, SH_ERR_ARG, m);
  }
  for (size_t i = 0; i < n_floats; ++i)
    if (!std::isfinite(packed[i])) return fail(c, SH_ERR_ARG, "sh_load_unet: NaN / infinite parameter");
  (void)hipStreamSynchronize(c->stream);      // no forward of the previous network is still reading the block
  c->ulayers.swap(layers);
  c->mirror.unet.assign(packed, packed + n_floats);
  c->pstate.unet_loaded(base, depth, n_floats);
  return upload_params(c);
}

int sh_param_block_commit(sh_ctx* c) {
  if (!c) return SH_ERR_ARG;
  c->pstate.block_exposed();
  auto it = c->bufs.find("params");
  if (it == c->bufs.end()) return fail(c, SH_ERR_STATE, "sh_param_block_commit: no parameters loaded");
  HIPCHK(c, hipSetDevice(c->device));
  const ParamShape& s = c->pstate.shape();
  ParamMirror m;
  m.resize(s);
  const int rc = copy_block(c, (char*)it->second.p, m, ParamLayout(s), false);
  if (rc != SH_OK) return rc;
  // the device walks the forest until it meets a leaf: what arrived must still be a forest over the same node count
  const ParamError e = forest_check(m.feat.data(), m.ti.data(), m.fi.data(), (int)s.nodes, m.roots.data(), (int)s.trees);
  if (e.code != SH_OK) return fail(c, e.code, std::string("sh_param_block_commit: ") + e.text + " in the device block");
  c->mirror = std::move(m);
  return SH_OK;
}

int sh_param_block(sh_ctx* c, void** p, size_t* n) {
  if (!c || !p || !n) return SH_ERR_ARG;
  c->pstate.block_exposed();      // the caller may write the block from here on (and confirms with sh_param_block_commit)
  auto it = c->bufs.find("params");
  if (it == c->bufs.end()) return fail(c, SH_ERR_STATE, "sh_param_block: no parameters loaded");
  *p = it->second.p;
  *n = ParamLayout(c->pstate.shape()).total;
  return SH_OK;
}

}  // extern "C"
