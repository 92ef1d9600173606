"""The host shim of the scalar stages (tests/hostcheck/hostcheck.cpp: sh_scalar.h instantiated by g++), built on first use and loaded
through ctypes.  Helper of test_host_scalar.py and test_row_cases_host.py; no test functions."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HC = os.path.join(ROOT, "tests", "hostcheck")
D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)


def dp(a):
    return a.ctypes.data_as(D)


def load_hostcheck():
    so = os.path.join(HC, "libhostcheck.so")
    src = os.path.join(HC, "hostcheck.cpp")
    hdrs = [os.path.join(ROOT, "shoulder_amd", "csrc", h) for h in ("sh_scalar.h", "sh_common.h", "sh_hull.h")] + [os.path.join(HC, "hull_rounds_ref.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hc_circle.restype = ctypes.c_double
    lib.hc_rfc.restype = ctypes.c_float
    lib.hc_interp.restype = ctypes.c_double
    lib.hc_linspace.restype = ctypes.c_double
    return lib


@pytest.fixture(scope="module")
def hc():
    return load_hostcheck()
