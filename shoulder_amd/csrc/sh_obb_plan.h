// sh_obb_plan.h -- the host rules of the OBB stage (run_obb of shoulder_hip.hip, the host hull phase of hull.hip and the background
// preparation of hulls): what a batch's hulls need of the hull record and of a pinned slot, how either grows, where a window's hulls
// come from, when a background thread may upload them early, and every number of the stage's launches.  No kernels, no HIP types:
// the two units act on it, a plain g++ compiles it (tests/hostcheck/obb_plan_check.cpp).
#pragma once
#include "sh_hullcap.h"

#include <stddef.h>

namespace sh {

// ---- hull counts ---------------------------------------------------------------------------------------------------------------------
// The count block of a pinned slot is [3][B]: vertices, faces, edges of every humerus' hull.  One strided copy per array of the record
// takes the largest count of the batch as its width, so that is what has to fit.
struct HullNeed { int v, f, e; };
inline HullNeed hull_need(const int* counts /*[3][B]*/, int B) {
  HullNeed n = {1, 1, 1};      // (an empty hull still copies one element, and sizes one tile)
  for (int b = 0; b < B; ++b) {
    if (counts[b] > n.v) n.v = counts[b];
    if (counts[B + b] > n.f) n.f = counts[B + b];
    if (counts[2 * B + b] > n.e) n.e = counts[2 * B + b];
  }
  return n;
}
// THE fit test: of a batch's largest counts against the device record (sh_ctx::hcap), of one humerus' own counts against the pitch
// of the pinned slot it is written to (hull_host_phase) or against the record it is written to alone (redo_given_up)
inline bool hull_fits(HullNeed n, HullCap cap) { return n.v <= cap.v && n.f <= cap.f && n.e <= cap.e; }

// The two growth rules differ on purpose.
// The device record: only an exceeded field moves, with an eighth of headroom -- growing it waits for the device and re-allocates
// nine buffers, so the next slightly larger hull of the batch stream should not do it again.
inline HullCap hull_record_grown(HullCap now, HullNeed need) {
  auto up = [](int x) { return (x + x / 8 + 1023) / 1024 * 1024; };
  if (need.v > now.v) now.v = up(need.v);
  if (need.f > now.f) now.f = up(need.f);
  if (need.e > now.e) now.e = up(need.e);
  return now;
}
// The pitch of a pinned slot: at least the record's start capacity (the usual dense hull then fits for good), else exactly the largest
// demand of this batch -- page-locked memory is the scarcer kind, and the phase that found the demand runs again at once, so there is
// no later growth to save.
inline HullCap hull_pitch_grown(HullNeed demand) {
  auto up = [](int x) { return (x + 1023) / 1024 * 1024; };
  return {up(demand.v > SH_HV ? demand.v : SH_HV), up(demand.f > SH_HF ? demand.f : SH_HF), up(demand.e > SH_HE ? demand.e : SH_HE)};
}

// ---- where a window's hulls come from ---------------------------------------------------------------------------------------------------
enum HullSource {
  HULL_REDO,            // redo_given_up has put the record of this window (one humerus) into hull.*
  HULL_DEVICE,          // k_hull_rounds writes the record
  HULL_PREPARED,        // a background thread has made the hulls, in a pinned slot
  HULL_FOREGROUND       // the host hull phase runs now
};
inline HullSource hull_source(int redo_nf, bool device_hull_now, int prepared_slot) {
  if (redo_nf > 0) return HULL_REDO;
  if (device_hull_now) return HULL_DEVICE;
  return prepared_slot >= 0 ? HULL_PREPARED : HULL_FOREGROUND;
}
inline bool hull_from_host(HullSource s) { return s == HULL_PREPARED || s == HULL_FOREGROUND; }
// the pinned slot's records are still to be copied to the device (prep_uploaded: the background thread has done it)
inline bool hull_upload_pending(HullSource s, bool prep_uploaded) { return s == HULL_FOREGROUND || (s == HULL_PREPARED && !prep_uploaded); }
// The face count the stage sizes its grids by.  A redo: its one hull's.  The device hull: its face slots -- the counts stay on the
// device, the candidate kernel's tiles beyond a hull's faces return at once -- or more when a humerus kept on the host hull
// (hulld.skip) has more faces than that.  The host: the largest hull of the slot.
inline int hull_nfmax(HullSource s, int redo_nf, int skip_nfmax, HullNeed slot_need) {
  if (s == HULL_REDO) return redo_nf;
  if (s == HULL_DEVICE) return skip_nfmax > HD_SLOTS ? skip_nfmax : HD_SLOTS;
  return slot_need.f;
}

// ---- the early upload --------------------------------------------------------------------------------------------------------------------
// A background thread copies its hulls into hull.* as soon as the step in flight no longer reads them (obb_done_ev), but only when
// nothing re-allocates those buffers before the run that takes the hulls: every one of the six holds B humeri at the record's
// strides already.  The staged starter needs the test (sh_commit_staged's alloc_batch grows them for a larger batch).  For the
// resident starter the size half is always true: it runs behind a whole-batch window of the batch it prepares for, whose buffers
// alloc_batch sized for that B at hcap, and grow_hull_records, the one thing that changes hcap, re-ensures exactly the three
// strided by it in the same call; ensure() never shrinks.  A hull above the record is not uploaded at all (hull_upload refuses).
struct HullRecBytes { size_t hv, normals, edges, nv, nf, ne; };
inline bool early_upload_ok(bool have_obb_done_ev, int B, HullCap hc, const HullRecBytes& z) {
  const size_t nB = (size_t)B;
  return have_obb_done_ev && z.hv >= nB * hc.v * 24 && z.normals >= nB * hc.f * 24 && z.edges >= nB * hc.e * 16 && z.nv >= nB * 4 && z.nf >= nB * 4 && z.ne >= nB * 4;
}

// ---- the launches ------------------------------------------------------------------------------------------------------------------------
// Capacity tier of k_obb_candidates (k_obb.h): the small one unless a hull of this launch has more than SH_OBB_NF_SMALL faces or a
// direction of an earlier run of this batch had more than SH_OBB_SIL_SMALL silhouette edges; the workspace tier above
// SH_OBB_NF_LARGE faces / SH_OBB_SIL_LARGE edges, or when a run said a hull had more faces than its tier's masks.
enum ObbTier { OBB_TIER_SMALL, OBB_TIER_LARGE, OBB_TIER_WORKSPACE };
struct ObbWsBytes { size_t fmask, lists, sxy, area; };      // "obb.ws_*" (k_obb.h ObbWs)
struct ObbPass {
  int mode;             // k_obb_select's: 0 the seed tile, 1 the directions its best volume cannot exclude, 2 all the others (no pruning)
  int nt_pass;          // tiles per humerus
  unsigned grid;        // workgroups of the candidate launch
};
struct ObbPlan {
  ObbTier tier;
  int TT;               // faces per tile of the tier
  int nemax;            // edges of the largest hull
  unsigned area2_grid;  // k_obb_face_area2: x of (x, B)
  int bnd_tiles;
  unsigned bounds_grid;
  int ntiles;           // tiles of TT faces over the largest hull
  ObbPass pass[2];      // seed tile, then the survivors
  int nwg, silcap;      // the workspace tier's workgroups and list capacity (other tiers: 0)
  ObbWsBytes ws;        // ... and the bytes of its buffers (other tiers: 0)
};
inline ObbPlan obb_plan(int B, int nfmax, HullCap hc, int sil_need, bool nf_over, bool prune) {
  ObbPlan p = {};
  const unsigned rows8 = (unsigned)(((B + 7) / 8) * 8);      // (the XCD-aware order of the tiled kernels: humeri in chunks of 8)
  p.nemax = 3 * nfmax / 2 + 3;      // (a closed triangulated surface: 2 E = 3 F)
  p.area2_grid = (unsigned)(((p.nemax < hc.e ? p.nemax : hc.e) + 255) / 256);
  p.bnd_tiles = (nfmax + SH_OBB_BND_DIRS - 1) / SH_OBB_BND_DIRS;
  p.bounds_grid = (unsigned)p.bnd_tiles * rows8;
  const bool huge = nfmax > SH_OBB_NF_LARGE || sil_need > SH_OBB_SIL_LARGE || nf_over;
  const bool big = !huge && (nfmax > SH_OBB_NF_SMALL || sil_need > SH_OBB_SIL_SMALL);
  p.tier = huge ? OBB_TIER_WORKSPACE : big ? OBB_TIER_LARGE : OBB_TIER_SMALL;
  p.TT = (big || huge) ? SH_OBB_TILE_LARGE : SH_OBB_TILE;
  p.ntiles = (nfmax + p.TT - 1) / p.TT;
  if (huge) {
    p.nwg = 256;
    const int grown = sil_need + sil_need / 8;
    p.silcap = hc.v + 64 > grown ? hc.v + 64 : grown;      // (a silhouette is a cycle of the hull's graph; more only on degenerate input: then the demand is recorded)
    p.ws = {(size_t)p.nwg * hc.f, (size_t)p.nwg * 8 * p.silcap * 4, (size_t)p.nwg * p.silcap * 16, (size_t)p.nwg * p.silcap * 8};
  }
  for (int pass = 0; pass < 2; ++pass) {
    ObbPass& q = p.pass[pass];
    q.mode = (prune || pass == 0) ? pass : 2;      // SHOULDER_OBB_PRUNE=0: every direction is evaluated (same frames: tests/test_gpu_obb_prune.py)
    q.nt_pass = pass == 0 ? SH_OBB_TILE / p.TT : p.ntiles;      // (the seed pass: up to SH_OBB_TILE directions)
    q.grid = (unsigned)q.nt_pass * rows8;
    if (huge && q.grid > (unsigned)p.nwg) q.grid = (unsigned)p.nwg;      // (the workspace tier: its nwg workgroups walk the tiles)
  }
  return p;
}

}  // namespace sh
