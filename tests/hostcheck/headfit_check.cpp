// Test shim (NOT product): the two solves of the head fit (shoulder_amd/csrc/sh_scalar.h head_sphere_from_moments /
// ellipse_from_moments, the source k_headfit_solve runs on the device) on the host, for tests/test_headfit_host.py and the
// device-against-host check of tests/test_gpu_headfit.py.
#include "../../shoulder_amd/csrc/sh_scalar.h"
extern "C" int hf_sphere(const double* m16, double* c3, double* r, double* rms) { return sh::head_sphere_from_moments(m16, c3, r, rms) ? 0 : -5; }
extern "C" int hf_ellipse(const double* rm6, double* semi_major, double* semi_minor, double* dir2) {
  return sh::ellipse_from_moments(rm6, semi_major, semi_minor, dir2) ? 0 : -5;
}
