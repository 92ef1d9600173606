// sh_demand.h -- how a run tells the host "I needed more than you gave me", and what the host answers.  No kernels, no HIP types:
// the kernels and the host units include it, and so does a plain g++ (tests/hostcheck/demand_check.cpp).
#pragma once
#include "sh_common.h"
#include <stddef.h>

namespace sh {
// the words of the demand block "ovf.ctr" (SH_NCTR x u64): cleared by sh_submit, raised by the kernels of the run
enum DemandWord {
  SH_CTR_SEG_USED = 0, SH_CTR_RING_USED = 1, SH_CTR_WORK_USED = 2,      // k_ovf.h bump cursors of the pools: segments (per set), ring points (per run), workspace bytes (per set)
  SH_CTR_SEG_NEED = 3, SH_CTR_RING_NEED = 4, SH_CTR_WORK_NEED = 5,      // high-water marks of what the run would have taken from them
  SH_CTR_TIER_MISSED = 6,     // the overflow tier was skipped and a plane needed it (k_slice_link_large)
  SH_CTR_END_NEED = 7,        // most crossing points an end section of the box asked for (k_obb_ends)
  SH_CTR_SIL_NEED = 8,        // k_obb_candidates (ObbWs::need[0]): the longest silhouette, in edges, a direction had above its tier's lists
  SH_CTR_NF_OVER = 9,         // ... (ObbWs::need[1]): a hull had more faces than the tier's masks
  SH_NCTR = 16
};
static_assert(SH_CTR_NF_OVER == SH_CTR_SIL_NEED + 1, "ObbWs::need spans both k_obb_candidates words");

// the status words of a run as ONE block (device staging "out.err<slot>", pinned copy of the ticket; the layout follows the run's
// batch size): [err: B ints | pad to 8 | demand block: SH_NCTR x u64 | device hull's give-up words: B ints]
struct StatusBlock {
  char* base; int B;
  static SH_HD size_t words_off(int B) { return ((size_t)B * 4 + 7) & ~(size_t)7; }
  static SH_HD size_t bytes(int B) { return words_off(B) + SH_NCTR * 8 + (size_t)B * 4; }
  SH_HD int* err() const { return (int*)base; }
  SH_HD unsigned long long* words() const { return (unsigned long long*)(base + words_off(B)); }
  SH_HD int* gave_up() const { return (int*)(base + words_off(B) + SH_NCTR * 8); }
};

// what the demand words are measured against, and what a rerun raises (held by sh_run.h BatchState)
struct DemandCaps { unsigned long long seg, ring, work; int end; int sil_need; bool nf_over; };
// why the records of a run are void and the batch runs again: with the overflow tier on | on the k_obb_candidates tier that holds the
// silhouette / the faces | with larger pools / end sections | with its hulls from the host (redo_given_up: a hull above the device hull's record)
enum Rerun { SH_RERUN_NONE = 0, SH_RERUN_TIER, SH_RERUN_OBB_TIER, SH_RERUN_POOLS, SH_RERUN_FORCE_HOST };
// rerun != NONE: run the batch again with `caps`.  error != null (only with a reason): the demand cannot be met -- the caller still
// refuses / synchronises / takes `caps` as for the rerun, then fails with SH_ERR_CAPACITY and this text.
struct Verdict { Rerun rerun; DemandCaps caps; const char* error; };

inline unsigned long long demand_grown(unsigned long long cap, unsigned long long need) { const unsigned long long g = need + need / 4; return g > cap ? g : cap; }

// obb_stage: the run had SH_STAGE_OBB; same_batch: it ran on the batch that is resident now (else words 8 / 9 say nothing about it)
inline Verdict demand_verdict(const unsigned long long* w, const DemandCaps& cur, bool obb_stage, bool same_batch) {
  Verdict v{SH_RERUN_NONE, cur, nullptr};
  if (w[SH_CTR_TIER_MISSED] != 0) { v.rerun = SH_RERUN_TIER; return v; }
  const unsigned long long sil = w[SH_CTR_SIL_NEED], nf = w[SH_CTR_NF_OVER];
  if ((sil != 0 || nf != 0) && obb_stage && same_batch) {
    v.rerun = SH_RERUN_OBB_TIER;
    if ((int)sil <= cur.sil_need && !(nf != 0 && !cur.nf_over))      // (cannot happen: its lists hold what the last run asked for)
      v.error = "k_obb_candidates: silhouette demand did not shrink on the workspace tier";
    else {
      const int s = (int)(sil < (1ull << 30) ? sil : (1ull << 30));
      if (s > cur.sil_need) v.caps.sil_need = s;
      if (nf != 0) v.caps.nf_over = true;
    }
    return v;
  }
  const unsigned long long need_s = w[SH_CTR_SEG_NEED], need_r = w[SH_CTR_RING_NEED], need_w = w[SH_CTR_WORK_NEED], need_e = w[SH_CTR_END_NEED];
  if (need_s > cur.seg || need_r > cur.ring || need_w > cur.work || need_e > (unsigned long long)cur.end) {
    v.rerun = SH_RERUN_POOLS;      // grow to what the run asked for, with headroom
    v.caps.seg = demand_grown(cur.seg, need_s); v.caps.ring = demand_grown(cur.ring, need_r); v.caps.work = demand_grown(cur.work, need_w);
    if (need_e > (unsigned long long)cur.end) {      // an end section with more crossing points than "obb.endpts" holds (a very dense mesh)
      if (need_e > (1ull << 26)) v.error = "an end section has more than 2^26 crossing points";
      else v.caps.end = (int)demand_grown(0, need_e);
    }
  }
  return v;
}

}  // namespace sh
