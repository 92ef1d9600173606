// sh_run.h -- the host rules of a run (sh_submit / sh_collect / redo_given_up and the background preparation of hulls): what is
// known about the resident batch, who owns the prepared-hull record, which submit is refused and what a submit does.  No kernels, no
// HIP types: shoulder_hip.hip acts on it, a plain g++ compiles it (tests/hostcheck/run_check.cpp).  Built on sh_demand.h.
#pragma once
#include "../../include/shoulder_hip.h"
#include "sh_demand.h"
#include "sh_hullcap.h"

#include <string.h>

namespace sh {

// May a collected run vouch that the overflow tier is idle for its batch?  Only one that asked nothing of the ring and segment pools,
// computed its own frame (a run on an injected frame says nothing about the planes of the next SH_STAGE_OBB, and the `pobb` set of a
// proximal humerus runs inside that stage), ran every slice stage its bone kind has, and ran on the batch that is still resident.
inline bool run_vouches(const unsigned long long* w, uint32_t mask, int bone_kind, bool same_batch) {
  const uint32_t slice_stages = SH_STAGE_FULL | SH_STAGE_DISTAL | SH_STAGE_NECK | SH_STAGE_PROXIMAL;
  const uint32_t all = bone_kind == SH_BONE_PROXIMAL ? (slice_stages & ~(uint32_t)SH_STAGE_DISTAL) : slice_stages;
  return w[SH_CTR_RING_NEED] == 0 && w[SH_CTR_SEG_NEED] == 0 && (mask & SH_STAGE_OBB) != 0 && (mask & slice_stages) == all && same_batch;
}

// ---- what is known about the resident batch ------------------------------------------------------------------------------------------
// One member of sh_ctx.  The batch generation stays the context's (every upload / commit / store to "verts" takes a new one) and is
// handed to the events and queries that need it.  The tier choices of the OBB stage and "hulls from the host" belong to the generation
// whose first OBB stage set them up (obb_begins: lazily, so a new batch keeps the old choice until then -- a staged batch decides
// whether its thread computes hulls by it).
class BatchState {
 public:
  // events, one per place that learns something
  void batch_resident() { frame_ = false; }                              // alloc_batch: no frame yet
  void params_set() { vouch_gen_ = NONE; }                               // the plane sets depend on the parameters
  // sh_buffer_device (the caller may write it) / sh_store: a frame or an intermediate can move the planes -- any name voids the vouch;
  // `stored`: the bytes are in place, "obb_transform" then is a frame
  void buffer_touched(const char* name, bool stored) {
    vouch_gen_ = NONE;
    if (stored && strcmp(name, "obb_transform") == 0) frame_ = true;
  }
  void obb_begins(unsigned long long gen) {                              // run_obb, in front of its first decision
    if (obb_gen_ == gen) return;
    obb_gen_ = gen; caps_.sil_need = 0; caps_.nf_over = false; force_host_ = false;
  }
  void frame_computed() { frame_ = true; }                               // run_obb: "obb_transform" is enqueued
  void run_enqueued(uint32_t mask) { if (mask & SH_STAGE_OBB) frame_ = true; }
  void run_collected(const unsigned long long* words, uint32_t mask, int bone_kind, unsigned long long run_gen, unsigned long long batch_gen) {
    if (run_vouches(words, mask, bone_kind, run_gen == batch_gen)) vouch_gen_ = batch_gen;
  }
  // the records are void and the batch runs again: the tier is on for it when a plane needed it while it was skipped, and behind a
  // redo (its hulls change)
  void rerun_decided(const Verdict& v, bool after_redo) { if (v.rerun == SH_RERUN_TIER || after_redo) vouch_gen_ = NONE; }
  // ... with what it asked for (nothing else is in flight).  -> "obb.endpts" has to grow to caps().end; a verdict with an error keeps the end sections
  bool rerun_granted(const Verdict& v) {
    caps_.seg = v.caps.seg; caps_.ring = v.caps.ring; caps_.work = v.caps.work; caps_.sil_need = v.caps.sil_need; caps_.nf_over = v.caps.nf_over;
    if (v.error || v.caps.end == caps_.end) return false;
    caps_.end = v.caps.end;
    return true;
  }
  void hull_above_record() { force_host_ = true; }                       // redo_given_up: the batch's hulls come from the host while it is resident
  void redo_used_faces(int nf) { if (nf > skip_nfmax_) skip_nfmax_ = nf; }
  void skip_list_cleared() { skip_nfmax_ = 0; }                          // the device hull's scratch, first use by a new batch: it takes every humerus again
  // queries
  bool tier_on(unsigned long long gen) const { return vouch_gen_ != gen; }      // the overflow tier's launches run (off: ~17 launches, ~60 us per step less)
  bool device_hull(int hull_mode, unsigned long long gen) const { return hull_mode == 1 && !(force_host_ && obb_gen_ == gen); }
  bool has_frame() const { return frame_; }
  const DemandCaps& caps() const { return caps_; }      // the pools (segments / ring points / bytes), points per end section, and the k_obb_candidates tier: the longest
                                                        // silhouette that overflowed one, "a hull had more faces than the tier masks"
  int skip_nfmax() const { return skip_nfmax_; }        // most hull faces among the humeri of this batch that are on the host hull (hulld.skip)

 private:
  static constexpr unsigned long long NONE = ~0ull;
  unsigned long long vouch_gen_ = NONE;      // a run of this generation planned no overflow plane in any set
  unsigned long long obb_gen_ = NONE;        // the generation caps_.sil_need, caps_.nf_over and force_host_ belong to
  DemandCaps caps_ = {1ull << 18, 1ull << 18, 32ull << 20, SH_ENDCAP, 0, false};
  bool force_host_ = false, frame_ = false;
  int skip_nfmax_ = 0;
};

// ---- the prepared-hull record: its key -------------------------------------------------------------------------------------------------
// THREADING RULE of sh_ctx::Prepared: the background thread writes the results (rc, bad_mesh, d2h_ms, hull_ms, err, uploaded) and the
// caller reads them only behind join_prepared; the caller writes this key, of which the thread reads only `slot` and `B`.
struct PreparedKey {
  static constexpr unsigned long long VOID = ~0ull;
  bool active = false;      // a thread is to be joined
  bool staged = false;      // it works for the STAGED batch
  int slot = 0, B = 0;      // the pinned slot the hulls go to, humeri
  unsigned long long gen = 0;         // the generation the hulls are for (staged: the one the batch gets at sh_commit_staged); read only behind a begin_*
  // events
  void begin_resident(int slot_, int B_, unsigned long long batch_gen) { active = true; staged = false; slot = slot_; B = B_; gen = batch_gen; }
  void begin_staged(int slot_, int B_, unsigned long long batch_gen, bool hulls) { active = true; staged = true; slot = slot_; B = B_; gen = hulls ? batch_gen + 1 : VOID; }
  void joined() { active = false; }
  void void_hulls() { gen = VOID; }
  void staged_dropped() { void_hulls(); staged = false; }
  // query: the run takes these hulls (`rc`: the preparation's, known behind the join)
  bool usable(bool obb, bool whole_batch_window, int rc, unsigned long long batch_gen, int B_) const {
    return obb && whole_batch_window && rc == SH_OK && gen == batch_gen && B == B_;
  }
};

// ---- a submit: the first refusal, then the plan ----------------------------------------------------------------------------------------
#define SH_WINDOW (1 << 30)      // humeri per window: the whole batch unless the switch asks for less
struct RunFacts {
  int B, n_pending, bone_kind, hull_mode;
  int window;                      // SHOULDER_WINDOW (0: SH_WINDOW)
  bool overlap, staged_active;     // sh_set_overlap; a batch is staged
  unsigned long long batch_gen;
  int hslot;                       // the pinned slot the next foreground hull goes to
  const BatchState* batch;
  PreparedKey prep;                // as it stood in front of the join
  int prep_rc;                     // what the join returned (SH_OK when nothing was under way)
};
struct RunError { int code; const char* text; };

inline RunError precheck_submit(uint32_t mask, const RunFacts& f) {
  const bool prox = f.bone_kind == SH_BONE_PROXIMAL;
  if (f.B < 1) return {SH_ERR_STATE, "sh_run: no meshes uploaded"};
  if (f.n_pending >= 2) return {SH_ERR_STATE, "sh_submit: two runs are in flight already (sh_collect first)"};
  if (prox && (mask & (SH_STAGE_DISTAL | SH_STAGE_TE))) return {SH_ERR_ARG, "sh_run: a proximal humerus has no distal / trans-epicondylar stage (bone.py:24-64)"};
  if ((mask & SH_STAGE_APPLY) && !(mask & SH_STAGE_CSYS)) return {SH_ERR_ARG, "sh_run: SH_STAGE_APPLY needs SH_STAGE_CSYS in the same run"};
  // a proximal humerus' frame is canal / articular (bone.py:53-62): k_pack builds it from the anatomic-neck axes of THIS run
  if (prox && (mask & SH_STAGE_CSYS) && !(mask & SH_STAGE_ANP))
    return {SH_ERR_ARG, "sh_run: SH_STAGE_CSYS of a proximal humerus needs SH_STAGE_ANP in the same run (canal / articular frame)"};
  if (!(mask & SH_STAGE_OBB) && !f.batch->has_frame()) return {SH_ERR_STATE, "sh_run: no OBB transform (run SH_STAGE_OBB or sh_store(\"obb_transform\"))"};
  return {SH_OK, ""};
}

struct RunPlan {
  bool dev_hull;            // the hulls of this run come from the device
  int win;                  // humeri per window: windows exist to overlap HOST hulls with device work, so only there and only for B > win
  int prepared_slot;        // the pinned slot whose prepared hulls the run takes, or -1
  int next_hslot;           // where the next foreground hull goes (prepared hulls keep their slot until the run has read them)
  bool void_staged_hulls;   // a run of the resident batch while hulls for the STAGED one wait: its own hull phase takes the same pinned slot and
                            // the same hull.* device buffers, so those are void (the staged batch stays; its first run computes them again)
  bool fetch_points;        // the foreground host hull needs its points
  bool start_overlap;       // everything enqueued: the hulls of the next run (of the whole batch again) on the background thread
};
inline RunPlan run_plan(uint32_t mask, const RunFacts& f) {
  const bool obb = (mask & SH_STAGE_OBB) != 0;
  const int wsize = f.window > 0 ? f.window : SH_WINDOW;
  RunPlan p;
  p.dev_hull = obb && f.batch->device_hull(f.hull_mode, f.batch_gen);
  p.win = (obb && f.B > wsize && !p.dev_hull) ? wsize : f.B;
  const bool usable = f.prep.active && f.prep.usable(obb, p.win == f.B, f.prep_rc, f.batch_gen, f.B);
  p.prepared_slot = (usable && !p.dev_hull) ? f.prep.slot : -1;
  p.next_hslot = usable ? (f.prep.slot ^ 1) : f.hslot;
  p.void_staged_hulls = obb && f.prep.staged && f.prep.gen != f.batch_gen;
  p.fetch_points = obb && p.prepared_slot < 0 && !p.dev_hull;
  p.start_overlap = f.overlap && obb && p.win == f.B && !p.dev_hull && !f.staged_active;
  return p;
}

// the records are void for `why` and a second run is in flight: sh_collect refuses with this
inline const char* rerun_refusal_text(Rerun why) {
  switch (why) {
    case SH_RERUN_TIER: return "a section needs the overflow tier while another run is in flight: collect it, then run the batch again (the tier is on by then)";
    case SH_RERUN_OBB_TIER: return "the OBB stage needs a larger tier while another run is in flight: collect it, then run the batch again (the tier is chosen by then)";
    case SH_RERUN_FORCE_HOST: return "a hull is above the device hull's record while another run is in flight: collect it, then run the batch again (its hulls come from the host by then)";
    default: return "slice overflow pools too small while another run is in flight: collect it, then run the batch again (the pools are grown by then)";
  }
}

}  // namespace sh
