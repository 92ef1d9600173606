// sh_ctx.h -- what the host units of libshoulder_hip.so share: the context, the named-buffer helpers, the launch macros and the
// few functions that cross units.  No kernels here: every k_*.h is included by exactly one unit (-fno-gpu-rdc), the one whose
// host code launches it.
//   shoulder_hip.hip  context, C-ABI plumbing, meshes, the stage runner, submit / collect   (geometry kernels)
//                     -- its per-batch buffers are declared once (WIN_*_BUFS: name, element type, elements per humerus); allocation
//                     and the typed view of a window (WinView, resolved once per run_window) both come from that list
//                     -- the entry points of the arthroplasty chain are sh_arthro_host.h, those of the queries of the resident batch
//                     sh_query_host.h, each included by this unit once (headers, not units: the resection kernels keep their
//                     registers only in this unit); their buffers are declared once as well (sh_arthro.h ARTHRO_BUFS,
//                     sh_query.h RAY_BUFS ..: allocation from a plan's sizes, ensure_bytes, and the typed view of a call, view_of)
//   hull.hip          hull prefilter, host hull phase and its worker pool, device hull      (k_hullpre.h, k_hull.h)
//   unet.hip          the UNet runners, UNet turns, sh_unet_infer                          (k_unet*.h; unet16_pp.hip: k_unet16_pp.h)
//   comm.hip          the RCCL collectives
// Kernel-free and HIP-free beside it (a plain g++ compiles them for the host tests): sh_demand.h (a run's capacity demands and the
// verdict on them), sh_ingest.h (what mesh ingest checks and plans on the host before a batch becomes resident), sh_unet_plan.h (the
// steps of a UNet pass: kernel, grid, tensors and work tickets of every launch; the ticket and weight-packing tables), sh_arthro.h
// (the arthroplasty chain: its argument checks and which refusal comes first, the pass plan and the bytes of every resect.* / canal.* /
// stem.* / plan.* buffer, and ArthroState, the one record of what is valid against what), sh_query.h (the queries of the resident batch:
// rays, closest points, winding numbers, registration, mass properties, surface samples, mesh topology, vertex fields, geodesics -- their argument checks, plans and the bytes of their buffers),
// sh_run.h (the run: BatchState, the one record of what is known about the resident batch -- tier vouch, frame, capacities, OBB tier, hulls
// from the host; PreparedKey, the caller's half of the prepared-hull record; the refusals of sh_submit in their order and its plan),
// sh_obb_plan.h (the OBB stage: what hulls need of the record and of a pinned slot and how either grows, where a window's hulls come
// from, the early-upload rule, and the tier, grids and workspace bytes of the stage's launches), sh_params.h (the parameters: the layout
// of the block "params", the forest check, the checks of sh_set_params, ParamState: what is loaded, which packed copies are current).
#pragma once
#include "../../include/shoulder_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <vector>

#include "sh_demand.h"
#include "sh_hullcap.h"
#include "sh_hull.h"
#include "sh_ingest.h"
#include "sh_obb_plan.h"
#include "sh_params.h"
#include "sh_query.h"      // (and sh_arthro.h below it)
#include "sh_run.h"
#include "sh_unet_plan.h"

// ---------------------------------------------------------------------------------------------
struct Buf {
  void* p = nullptr;
  size_t bytes = 0;
  int elem = 1;
  size_t per_mesh = 0;     // bytes per humerus for [B][...] buffers (0: shared / ragged / scratch)
};

struct KTimer {
  double ms = 0;
  int n = 0;
};

struct sh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  sh_params params;
  int B = 0;
  long long sumV = 0, sumF = 0, maxV = 0, maxF = 0;
  std::vector<long long> h_voff, h_foff;
  std::map<std::string, Buf> bufs;
  // a named buffer's pointer, null when it is not there (inlined like the lambdas it replaces)
  __attribute__((always_inline)) void* at(const char* name) const { auto it = bufs.find(name); return it == bufs.end() ? nullptr : it->second.p; }
  // the parameters (sh_params.h): the host copy of every section of the block "params", what is loaded and which packed copies of
  // the block are current (ParamState: named events and queries), the loaded network's layers by name
  sh::ParamMirror mirror;
  sh::ParamState pstate;
  sh::UnetLayers ulayers;
  void* comm = nullptr;                      // sh_comm_init_all: this context's RCCL communicator (comm.hip), its rank and the group's size
  int comm_rank = -1, comm_n = 0;
  // sh_set_keep_products: every plane's resampled contour and polar rows leave k_resample_polar (k_slices.h, RsWant); off: the rows
  // the later stages read.  rs_*: what the last SH_STAGE_PROXIMAL run of the resident batch wrote (SH_STAGE_GROOVE checks it covers its rows)
  bool keep_products = false;
  int rs_cs_lo = 0, rs_cs_hi = 0;
  bool rs_all = false;
  unsigned long long rs_gen = ~0ull;
  int rec_rows = 0;                          // sh_set_record_rows: 0 = full sh_landmarks records, R > 0 = packed records with R anatomic-neck rows
  // hull of SH_STAGE_OBB: 1 = on the device (k_hull.h), 0 = host quickhull (sh_hull.h).  sh_set_hull_mode / SHOULDER_HULL=host|device|auto.
  // A humerus the device hull gives up (pinched horizon on nearly coplanar clouds, capacities) is re-done ALONE by sh_collect
  // (redo_given_up); `hulld.skip[b]` then keeps the device hull off it for as long as the batch stays resident (skip_gen == batch_gen).
  int hull_mode = 1;
  unsigned long long skip_gen = ~0ull;
  // What is known about the resident batch (sh_run.h BatchState: named events and queries): whether a run vouched that the overflow
  // tier of the slice layer (k_ovf.h) is idle for it, whether it has a frame, the capacities a run's demands are measured against and
  // sh_collect grows (pools, end sections, the k_obb_candidates tier), whether its hulls come from the host, the faces of redone hulls
  sh::BatchState batch;
  // sh_set_open_contours (k_open.h): SH_OPEN_ERROR / SH_OPEN_BRIDGE and the largest gap bridged (mm); open_stats_run: the mode of the
  // last sh_submit ("open.stats" is cleared, and counts, only in bridge mode)
  int open_mode = SH_OPEN_ERROR;
  double open_gap = SH_OPEN_GAP_DEFAULT;
  int open_stats_run = SH_OPEN_ERROR;
  sh::HullCap hcap = {SH_HV, SH_HF, SH_HE};      // per-humerus capacity (= stride) of the hull record and the per-face obb.* arrays; a batch with a larger
                                             // hull grows it (grow_hull_records) -- every kernel takes the strides as an argument
  std::vector<float> h_verts;                // host copy of the vertices (hull stage)
  bool h_verts_valid = false;
  // device-generated batches: the hull's points come back through the prefilter (k_hullpre.h) into pinned memory
  float* h_kept = nullptr; long long h_kept_cap = 0;
  int* h_nkept = nullptr; int h_nkept_cap = 0;
  struct HullPts { const float* src = nullptr;            // what hull_host_phase reads: h_verts.data() or the pinned survivors
                   std::vector<long long> off;            // first point of humerus b in src
                   std::vector<int> cnt; };               // points of humerus b in src
  HullPts hull_in;                           // ... of the resident batch
  long long* h_koff = nullptr; int h_koff_cap = 0;      // pinned: offsets of the survivors (B + 1)
  // The STAGING SIDE of the mesh slot (sh_stage_meshes / sh_stage_stl / sh_commit_staged): the next batch is copied into buffers of
  // its own ("verts.s", "faces.s", "voff.s", "foff.s") on the copy stream while a run of the resident batch executes, its hull
  // points come back through a prefilter scratch of its own ("hullpre.*.s") and its hulls are computed by the background thread
  // (`prep`, gen = batch_gen + 1) -- sh_commit_staged then only swaps the buffer entries and the next sh_submit finds its hulls.
  struct StageSide {
    bool active = false, from_stl = false;
    int B = 0; long long sumV = 0, sumF = 0, maxV = 0, maxF = 0;
    std::vector<long long> voff, foff;
    void* h_src = nullptr; size_t h_src_cap = 0;            // pinned staging of the caller's arrays / files
    int* h_flag = nullptr;                                  // pinned: validation word (+ STL: counts and non-finite words behind it)
    size_t h_flag_cap = 0;
    float* h_kept = nullptr; long long h_kept_cap = 0;      // pinned: prefilter survivors of the staged batch
    long long* h_koff = nullptr; int h_koff_cap = 0;
    HullPts pts;
    hipEvent_t ready_ev = nullptr;                          // everything the commit needs is on the device
    std::mutex m; std::condition_variable cv; bool meta_ready = true; int meta_rc = 0; std::string meta_err;      // STL: sizes known
  } stg;
  // Window of the batch the stage runner is working on: sh_run walks the batch in windows so that the
  // host hull of window k+1 overlaps the device work of window k.  buf<T>() applies the offset.  (What only one window needs to
  // know -- its typed buffer view, whether its bounds are cleared, whether its side branch is still to be joined -- is not here:
  // WinView / WinState of shoulder_hip.hip, locals of run_window.)
  int b0 = 0, Bwin = 0;
  struct HullStage { double* hv = nullptr; double* nr = nullptr; int* ed = nullptr; int* cnt = nullptr; int cap = 0; hipEvent_t ev = nullptr; bool used = false;
                     int pv = 4096, pf = 8192, pe = 12288; };      // per-humerus pitch of the pinned staging (elements): the usual hull fits the small
                                                                 // one; a batch with a larger hull re-allocates the slot at sh_obb_plan.h's
                                                                 // hull_pitch_grown: the record's start capacity or, above it, what the largest hull asks
  HullStage hstage[2];                       // pinned host staging, double buffered
  int hslot = 0;                             // slot the next hull goes to
  // Overlap (sh_set_overlap): while the device works on run k, a background thread computes the hulls run k+1 will
  // need (same resident batch -- invalidated by any upload) into the other pinned slot.  `key` is the caller's, the rest the thread's
  // results (sh_run.h PreparedKey states the threading rule).
  struct Prepared {
    std::thread th; sh::PreparedKey key;
    int rc = SH_OK, bad_mesh = -1; double d2h_ms = 0, hull_ms = 0; std::string err;
    bool uploaded = false;      // the hull records are already in the device buffers (copied by the background thread)
  } prep;
  hipEvent_t obb_done_ev = nullptr;      // recorded after the last kernel of a run that reads the hull.* device buffers
  // sh_submit / sh_collect: up to two runs in flight (the second one is enqueued while the first still executes)
  struct Ticket { hipEvent_t ev = nullptr; char* status = nullptr /*pinned sh::StatusBlock for `cap` humeri*/; int cap = 0, B = 0; bool pending = false; sh_landmarks* host_out = nullptr;
                  uint32_t mask = 0; sh_landmarks* out_arg = nullptr; bool dev_hull = false; unsigned long long gen = 0; size_t rec = sizeof(sh_landmarks); int rows = 0; };
  Ticket tickets[2];
  int t_head = 0, t_tail = 0, n_pending = 0;
  hipStream_t out_stream = nullptr;      // sh_collect copies the records / status words of a finished run to the host on this stream
  bool overlap = false;
  unsigned long long batch_gen = 0;
  // the arthroplasty chain (sh_arthro_host.h: sh_resect_*, sh_canal_profile, sh_resect_stems, sh_resect_plan): what is valid against
  // what -- the records of the last submitted run, the last resection with its seats, the last profile, the stems -- is this one
  // member's (sh_arthro.h ArthroState: named events and queries; batch_gen above stays the context's and is handed to the queries)
  sh::ArthroState arthro;
  int topo_shell_records = 0;                // the max_shells of the last sh_mesh_topology: the records per mesh of "topo.shells" (sh_mesh_repair reads them)
  int query_accel = SH_ACCEL_OFF;            // sh_set_query_accel: the closest-point step walks all faces (k_cp_walk) or descends "bvh.*" (k_cp_tree); same bytes
  hipStream_t copy_stream = nullptr;
  hipEvent_t stl_counted_ev = nullptr;      // sh_stage_stl: the device has counted the merged vertices / faces
  // side stream of the stage runner: the distal slice set and the rectangles of the trans-epicondylar stage hang on nothing but the
  // box frame, so they run beside the full -> neck -> proximal chain
  hipStream_t side_stream = nullptr;
  hipEvent_t side_fork_ev = nullptr, side_join_ev = nullptr;
  // Switches of equivalent paths (the A/B arms of tests/), read from the environment ONCE, when the context is created -- no launch
  // path consults the environment.  (Read elsewhere, process-wide: SHOULDER_HULL's default, SHOULDER_HULL_THREADS and
  // LOCAL_WORLD_SIZE for the hull pool, SHOULDER_RCCL_LIB.)
  struct Switches {
    int window = 0;            // SHOULDER_WINDOW=n: humeri per window of the host-hull walk (0: SH_WINDOW)
    bool obb_prune = true;     // SHOULDER_OBB_PRUNE=0: every hull-face direction is evaluated
    bool slice_merge = true;   // SHOULDER_SLICE_MERGE=0: one slice set per launch group
    bool hull_prefilter = true; // SHOULDER_HULL_PREFILTER=0: host hulls read every vertex back instead of the prefilter's survivors
    bool debug = false;        // SH_DEBUG: host-phase timings on stderr
  } sw;
  // the UNet runner's state (unet.hip)
  struct Unet {
    bool reference = false;          // SHOULDER_UNET_REFERENCE=1 at context creation: the 16-bit network layer by layer on the generic kernels
    bool turn = false;               // sh_set_unet_turns: UNet passes of the contexts of one device run one after another
    hipEvent_t done_ev = nullptr;    // ... recorded at the end of this context's pass
    int num_cus = 0;
    int ticket_next = 0;             // next free work counter of "unet16.tickets" (one per persistent launch of a forward pass)
    std::map<std::tuple<int, int, int>, std::pair<int, int>> tk_tabs;      // (items, workgroups, cout groups) -> (offset, tickets) in "unet16.tk_tab"
    int tk_tab_used = 0;
    bool zero_page_ready = false;    // "unet16.zero" is cleared
  } unet;
  // timing
  int timing = 0;      // 0 off, 1 every launch, 2 UNet layers only
  std::vector<std::tuple<std::string, hipEvent_t, hipEvent_t>> pending;
  std::map<std::string, KTimer> timers;
};

#define HIPCHK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
      return SH_ERR_HIP;                                                                    \
    }                                                                                       \
  } while (0)

// the same for code that has no context to write to (the background threads): the text goes to *errtxt
#define HIPCHK_TXT(errtxt, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { *(errtxt) = std::string(#call) + ": " + hipGetErrorString(e_); return SH_ERR_HIP; } } while (0)

// The window [b0, b0 + Bwin) for a scope; the previous one comes back when the scope is left (on its error returns too)
struct WindowScope {
  sh_ctx* c; int b0, Bwin;
  WindowScope(sh_ctx* c_, int nb0, int nBwin) : c(c_), b0(c_->b0), Bwin(c_->Bwin) { c->b0 = nb0; c->Bwin = nBwin; }
  ~WindowScope() { c->b0 = b0; c->Bwin = Bwin; }
  WindowScope(const WindowScope&) = delete; WindowScope& operator=(const WindowScope&) = delete;
};

// The stream the launches of a scope go to (the side branch of the stage runner); the context's own comes back like the window
struct StreamScope {
  sh_ctx* c; hipStream_t saved;
  StreamScope(sh_ctx* c_, hipStream_t s) : c(c_), saved(c_->stream) { c->stream = s; }
  ~StreamScope() { c->stream = saved; }
  StreamScope(const StreamScope&) = delete; StreamScope& operator=(const StreamScope&) = delete;
};

static inline int fail(sh_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

static inline int ensure(sh_ctx* c, const char* name, size_t bytes, int elem, void** out = nullptr) {
  Buf& b = c->bufs[name];
  if (b.bytes < bytes || b.p == nullptr) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    hipError_t e = hipMalloc(&b.p, bytes ? bytes : 16);
    if (e != hipSuccess) {
      c->err = std::string("hipMalloc(") + name + "): " + hipGetErrorString(e);
      b.bytes = 0;
      return SH_ERR_NOMEM;
    }
    b.bytes = bytes;
  }
  b.elem = elem;
  if (out) *out = b.p;
  return SH_OK;
}

template <typename T>
static inline T* buf(sh_ctx* c, const char* name) {
  auto it = c->bufs.find(name);
  if (it == c->bufs.end() || !it->second.p) return nullptr;
  return (T*)((char*)it->second.p + (size_t)c->b0 * it->second.per_mesh);
}

// The hull record of the current window (what the host hull uploads, the device hull writes and the OBB stage reads), resolved in
// one place.  Calling thread only (buffer map), and not across grow_hull_records / alloc_batch, which re-allocate it.
struct HullRec { double *hv, *normals; int *edges, *nv, *nf, *ne; };
static inline HullRec hull_rec_at(sh_ctx* c, int b0) {      // ... of the window that begins at humerus b0, wherever the context stands
  WindowScope from(c, b0, c->Bwin);
  return {buf<double>(c, "hull.hv"), buf<double>(c, "hull.normals"), buf<int>(c, "hull.edges"), buf<int>(c, "hull.nv"), buf<int>(c, "hull.nf"), buf<int>(c, "hull.ne")};
}
static inline HullRec hull_rec(sh_ctx* c) { return hull_rec_at(c, c->b0); }
// the bytes those six buffers hold (a missing one: 0), for sh_obb_plan.h early_upload_ok.  Calling thread only.
static inline sh::HullRecBytes hull_rec_bytes(sh_ctx* c) {
  auto z = [c](const char* n) { auto it = c->bufs.find(n); return it == c->bufs.end() || !it->second.p ? (size_t)0 : it->second.bytes; };
  return {z("hull.hv"), z("hull.normals"), z("hull.edges"), z("hull.nv"), z("hull.nf"), z("hull.ne")};
}
// One humerus on the host hull (hull.hip hull_of_points): its points widened, the quickhull, its counts; `hv`: the hull's vertices
// gathered for an upload of this humerus alone (hull_upload_one)
struct HostHull { std::vector<double> P, hv; shhull::Hull H; sh::HullNeed n; };
static inline std::string hull_failed_text(int mesh, int code) { char m[96]; snprintf(m, sizeof m, "mesh %d: convex hull failed (%d)", mesh, code); return m; }

// ensure() inside a function with `int rc`, and the buffer's window stride: ENS for [B][...] buffers (bytes / B per humerus),
// ENS_SHARED for shared / ragged / scratch ones (stride 0)
#define ENS_(name, bytes, elem, per_mesh_)                                          \
  do {                                                                              \
    if ((rc = ensure(c, name, (size_t)(bytes), elem)) != SH_OK) return rc;          \
    c->bufs[name].per_mesh = (per_mesh_);                                           \
  } while (0)
#define ENS(name, bytes, elem) ENS_(name, bytes, elem, (size_t)(bytes) / (size_t)c->B)
#define ENS_SHARED(name, bytes, elem) ENS_(name, bytes, elem, 0)
static inline int ensure_shared(sh_ctx* c, const char* name, size_t bytes, int elem) { int rc; ENS_SHARED(name, bytes, elem); return SH_OK; }

// The buffers of a list (sh_arthro.h SH_BUF_LIST) at the sizes of a call's plan, shared / scratch stride; 0: not this call's.
template <typename Bytes>
static inline int ensure_bytes(sh_ctx* c, const Bytes& z) {
  int rc = SH_OK;
  z.each([&](size_t bytes, const char*, const char* name, int elem) { if (bytes && rc == SH_OK) rc = ensure_shared(c, name, bytes, elem); });
  return rc;
}
// The named buffers of a list as typed pointers, no window offset; a buffer that is not there is null.  A VIEW IS RESOLVED BEHIND EVERY
// ENSURE THAT CAN RE-ALLOCATE ITS BUFFERS: once per call behind the call's ensure_bytes (a call that ensures two plans ensures their
// field-wise maximum first: sh_register_multistart), and again behind any later one (ray_run, where "ray.pool" is sized by the counts).
template <typename View>
static inline View view_of(const sh_ctx* c) {
  View v;
  v.each([c](auto*& p, const char*, const char* name, auto...) { p = static_cast<std::remove_reference_t<decltype(p)>>(c->at(name)); });
  return v;
}
// the element size sh_buffer_info reports for a buffer of T: records and segments count as bytes
template <typename T> constexpr int elem_of() { return sizeof(T) <= 8 ? (int)sizeof(T) : 1; }

// kernel launch with optional HIP-event timing on the ctx stream
// timing level 1: events around every launch; 2: around the UNet layers only ("unet.*": ~25 launches per run, so the
// measurement does not stretch the run it measures -- events around all ~150 launches cost ~0.7 ms per run at B = 64)
static inline bool timed_launch(const sh_ctx* c, const char* name) {
  return c->timing == 1 || (c->timing == 2 && name[0] == 'u' && name[1] == 'n' && name[2] == 'e' && name[3] == 't' && name[4] == '.');
}

// the bookkeeping around a launch: a kernel (LAUNCH) or a launcher function of another translation unit (unet16_pp.h)
#define LAUNCH_FN(ctx, name, call)                                                           \
  do {                                                                                      \
    hipEvent_t e0_ = nullptr, e1_ = nullptr;                                                \
    const bool timed_ = timed_launch(ctx, name);                                            \
    if (timed_) {                                                                           \
      (void)hipEventCreate(&e0_); (void)hipEventCreate(&e1_);                               \
      (void)hipEventRecord(e0_, (ctx)->stream);                                             \
    }                                                                                       \
    call;                                                                                   \
    if (timed_) {                                                                           \
      (void)hipEventRecord(e1_, (ctx)->stream);                                             \
      (ctx)->pending.emplace_back(name, e0_, e1_);                                          \
    }                                                                                       \
    HIPCHK(ctx, hipGetLastError());                                                         \
  } while (0)
#define LAUNCH(ctx, name, kernel, grid, block, ...) LAUNCH_FN(ctx, name, hipLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, __VA_ARGS__))

// records on the wire (shoulder_hip.hip): a full sh_landmarks, or packed with R anatomic-neck rows
#define SH_REC_HEAD offsetof(sh_landmarks, anp_points)
#define SH_REC_TAIL (sizeof(sh_landmarks) - SH_REC_HEAD - sizeof(((sh_landmarks*)0)->anp_points))
static inline size_t rec_bytes_rows(int rows) { return rows > 0 ? SH_REC_HEAD + SH_REC_TAIL + (size_t)rows * 24 : sizeof(sh_landmarks); }

// ---- functions that cross units ------------------------------------------------------------------------------------------------
struct HullPre { const float* verts; const long long* voff; int* ext; double* planes; int* npl; float* kept; int* nkept; long long* koff; double* pval; int* pidx; int* pcnt; long long* poff; };      // device pointers of the hull prefilter (hull.hip)
struct FillEnt { void* p; size_t bytes; unsigned char byte; };      // bytes: a multiple of 4, p 4-byte aligned
// a UNet pass reads `image` (f32, scaled) or, where its first kernel scales it itself (plan_level0_fused), `raw` with its encoded range `mm`
struct UnetIO { const float* image; const double* raw; const unsigned long long* mm; float* logits; };
namespace sh {
// shoulder_hip.hip
int fill_list(sh_ctx* c, std::initializer_list<FillEnt> ents);      // buffer clears of a run as one launch (k_fill_list)
int emit_records(sh_ctx* c, void* dst, int b0, int n, int rows, size_t rec);
unsigned threads_per_local_rank(bool sustained = true);
// hull.hip
HullPre hullpre_ptrs(sh_ctx* c, const char* sfx = "");      // calling thread only (buffer map); sfx ".s": the staging side
hipError_t fetch_prefiltered(const HullPre& hp, int B, long long sumV, long long* h_koff, float* h_kept, sh_ctx::HullPts* out, hipStream_t st);
hipError_t fetch_hull_points(sh_ctx* c, const HullPre& hp, hipStream_t st);
int hull_host_phase(sh_ctx* c, const sh_ctx::HullPts& in, int slot, int b0, int B, int* bad_mesh, double* ms, std::string* errtxt, bool background = false);
hipError_t hull_upload(sh_ctx* c, int slot, int B, const HullRec& dst, hipStream_t st);
bool hull_of_points(const float* src, long long nv, HostHull& h);
hipError_t hull_upload_one(HostHull& h, const HullRec& dst, hipStream_t st);
int run_device_hull(sh_ctx* c, int B);
int alloc_hullpre(sh_ctx* c, int B, long long sumV, const char* sfx);
// unet.hip
int unet_turn_enter(sh_ctx* c);
int unet_turn_leave(sh_ctx* c);
void unet_turn_forget(sh_ctx* c);
int unet_dispatch(sh_ctx* c, const UnetIO& io, int nimg, int H, int W);
// comm.hip
void comm_forget(sh_ctx* c);
}  // namespace sh

#define FILL(ctx, ...) do { int frc_ = sh::fill_list(ctx, {__VA_ARGS__}); if (frc_ != SH_OK) return frc_; } while (0)
