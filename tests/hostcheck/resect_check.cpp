// Test shim (NOT product): the plane bookkeeping of the batched resection (shoulder_amd/csrc/sh_scalar.h
// resect_plane_from_offsets, the source k_resect_make_planes runs on the device) on the host, for tests/test_resect_host.py.
#include "../../shoulder_amd/csrc/sh_scalar.h"
extern "C" int rc_plane_from_offsets(const double* T_anp, const double* p_ct, const double* n_ct, int side, const double* off7,
                                     double* out_p, double* out_n) {
  return sh::resect_plane_from_offsets(T_anp, p_ct, n_ct, side, off7, out_p, out_n) ? 0 : -1;
}
