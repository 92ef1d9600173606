// Test shim (NOT product): the host rules of a run (shoulder_amd/csrc/sh_run.h: precheck_submit, run_plan, BatchState, PreparedKey,
// run_vouches, rerun_refusal_text) on the host, for tests/test_run_plan_host.py.
#include "../../shoulder_amd/csrc/sh_run.h"
using namespace sh;
typedef unsigned long long u64;

// ---- BatchState: a handle, one function per event, one that reads every query -------------------------------------------------------------
extern "C" void* rc_batch_new() { return new BatchState(); }
extern "C" void rc_batch_free(void* h) { delete (BatchState*)h; }
extern "C" void rc_batch_resident(void* h) { ((BatchState*)h)->batch_resident(); }
extern "C" void rc_params_set(void* h) { ((BatchState*)h)->params_set(); }
extern "C" void rc_buffer_touched(void* h, const char* name, int stored) { ((BatchState*)h)->buffer_touched(name, stored != 0); }
extern "C" void rc_obb_begins(void* h, u64 gen) { ((BatchState*)h)->obb_begins(gen); }
extern "C" void rc_frame_computed(void* h) { ((BatchState*)h)->frame_computed(); }
extern "C" void rc_run_enqueued(void* h, unsigned mask) { ((BatchState*)h)->run_enqueued(mask); }
extern "C" void rc_run_collected(void* h, const u64* words, unsigned mask, int bone_kind, u64 run_gen, u64 batch_gen) {
  ((BatchState*)h)->run_collected(words, mask, bone_kind, run_gen, batch_gen);
}
// caps: seg, ring, work, end, sil_need, nf_over.  -> rerun_granted's answer, or -1 when only the decision was taken (others in flight)
extern "C" int rc_rerun(void* h, int why, const u64* caps, int error, int after_redo, int others_in_flight) {
  const Verdict v{(Rerun)why, DemandCaps{caps[0], caps[1], caps[2], (int)caps[3], (int)caps[4], caps[5] != 0}, error ? "error" : nullptr};
  ((BatchState*)h)->rerun_decided(v, after_redo != 0);
  if (others_in_flight) return -1;
  return ((BatchState*)h)->rerun_granted(v) ? 1 : 0;
}
extern "C" void rc_hull_above_record(void* h) { ((BatchState*)h)->hull_above_record(); }
extern "C" void rc_redo_used_faces(void* h, int nf) { ((BatchState*)h)->redo_used_faces(nf); }
extern "C" void rc_skip_list_cleared(void* h) { ((BatchState*)h)->skip_list_cleared(); }
// out: tier_on(gen), device_hull(0, gen), device_hull(1, gen), has_frame, skip_nfmax, then the six capacities
extern "C" void rc_batch_queries(const void* h, u64 gen, u64* out) {
  const BatchState& s = *(const BatchState*)h;
  const DemandCaps& c = s.caps();
  const u64 q[11] = {s.tier_on(gen), s.device_hull(0, gen), s.device_hull(1, gen), s.has_frame(), (u64)s.skip_nfmax(),
                     c.seg, c.ring, c.work, (u64)c.end, (u64)c.sil_need, c.nf_over};
  for (int i = 0; i < 11; ++i) out[i] = q[i];
}
extern "C" int rc_vouches(const u64* words, unsigned mask, int bone_kind, int same_batch) { return run_vouches(words, mask, bone_kind, same_batch != 0) ? 1 : 0; }
extern "C" const char* rc_refusal_text(int why) { return rerun_refusal_text((Rerun)why); }

// ---- PreparedKey: the key as five words (active, staged, slot, B, gen) in, an event, the key out -----------------------------------------
static PreparedKey key_of(const u64* k) { PreparedKey p; p.active = k[0] != 0; p.staged = k[1] != 0; p.slot = (int)k[2]; p.B = (int)k[3]; p.gen = k[4]; return p; }
// event: 0 begin_resident(slot, B, gen) | 1 begin_staged(slot, B, gen, hulls) | 2 joined | 3 void_hulls | 4 staged_dropped
extern "C" void rc_key_event(u64* k, int event, int slot, int B, u64 batch_gen, int hulls) {
  PreparedKey p = key_of(k);
  switch (event) {
    case 0: p.begin_resident(slot, B, batch_gen); break;
    case 1: p.begin_staged(slot, B, batch_gen, hulls != 0); break;
    case 2: p.joined(); break;
    case 3: p.void_hulls(); break;
    default: p.staged_dropped(); break;
  }
  k[0] = p.active; k[1] = p.staged; k[2] = (u64)p.slot; k[3] = (u64)p.B; k[4] = p.gen;
}
extern "C" void rc_key_fresh(u64* k) { const PreparedKey p; k[0] = p.active; k[1] = p.staged; k[2] = (u64)p.slot; k[3] = (u64)p.B; k[4] = p.gen; }
extern "C" int rc_key_usable(const u64* k, int obb, int whole, int rc, u64 batch_gen, int B) { return key_of(k).usable(obb != 0, whole != 0, rc, batch_gen, B) ? 1 : 0; }

// ---- a submit ------------------------------------------------------------------------------------------------------------------------------
// f: B, n_pending, bone_kind, hull_mode, window, overlap, staged_active, batch_gen, hslot, prep_rc; `batch`: a BatchState handle
static RunFacts facts_of(const long long* f, const void* batch, const u64* key) {
  return RunFacts{(int)f[0], (int)f[1], (int)f[2], (int)f[3], (int)f[4], f[5] != 0, f[6] != 0, (u64)f[7], (int)f[8], (const BatchState*)batch, key_of(key), (int)f[9]};
}
extern "C" int rc_precheck(unsigned mask, const long long* f, const void* batch, const u64* key, const char** text) {
  const RunError e = precheck_submit(mask, facts_of(f, batch, key));
  *text = e.text;
  return e.code;
}
// out: dev_hull, win, prepared_slot, next_hslot, void_staged_hulls, fetch_points, start_overlap
extern "C" void rc_plan(unsigned mask, const long long* f, const void* batch, const u64* key, long long* out) {
  const RunPlan p = run_plan(mask, facts_of(f, batch, key));
  out[0] = p.dev_hull; out[1] = p.win; out[2] = p.prepared_slot; out[3] = p.next_hslot; out[4] = p.void_staged_hulls; out[5] = p.fetch_points; out[6] = p.start_overlap;
}
