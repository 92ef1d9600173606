// Test shim (NOT product): the capacity verdict sh_collect and redo_given_up ask for (shoulder_amd/csrc/sh_demand.h
// demand_verdict) on the host, for tests/test_rerun_verdict.py.  caps: seg, ring, work, end, sil_need, nf_over.
#include "../../shoulder_amd/csrc/sh_demand.h"
extern "C" int dc_verdict(const unsigned long long* words, const unsigned long long* caps, int obb_stage, int same_batch,
                          unsigned long long* caps_out, const char** error) {
  const sh::DemandCaps cur{caps[0], caps[1], caps[2], (int)caps[3], (int)caps[4], caps[5] != 0};
  const sh::Verdict v = sh::demand_verdict(words, cur, obb_stage != 0, same_batch != 0);
  caps_out[0] = v.caps.seg; caps_out[1] = v.caps.ring; caps_out[2] = v.caps.work;
  caps_out[3] = (unsigned long long)v.caps.end; caps_out[4] = (unsigned long long)v.caps.sil_need; caps_out[5] = v.caps.nf_over ? 1 : 0;
  *error = v.error;
  return (int)v.rerun;
}
