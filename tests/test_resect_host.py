"""Batched head resection (include/shoulder_hip.h sh_resect_*), the parts that need no GPU (record layout: test_abi_exports.py): the plane
bookkeeping the device runs (sh_scalar.h resect_plane_from_offsets) against oracle/osteotomy.py, argument checks."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import host_twin
from conftest import GOLDEN
from oracle.osteotomy import OracleOsteotomy
from shoulder_amd import _lib

FIELDS = [n for n, _ in _lib.CutOffset._fields_]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = host_twin.build_shim("resect", tmp_path_factory.mktemp("resect_check"))
    L.rc_plane_from_offsets.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    return L


def apply_offsets(O, off):
    """the calls a user makes for one sh_cut_offset, in its fixed order; a zero field is a call that is not made"""
    if off["retroversion_deg"]:
        O.offset_retroversion(off["retroversion_deg"])
    if off["neckshaft_deg"]:
        O.offest_neckshaft(off["neckshaft_deg"])
    for key, direction in (("depth_canal_mm", "canal"), ("depth_anp_mm", "anp"), ("depth_resection_mm", "resection")):
        if off[key]:
            O.offset_depth(off[key], direction)
    if off["anterior_mm"]:
        O.offset_anterior_posterior(off["anterior_mm"])
    if off["medial_mm"]:
        O.offset_medial_lateral(off["medial_mm"])
    return O


def offset_grid():
    vals = dict(retroversion_deg=(-10.0, 0.0, 7.5), neckshaft_deg=(0.0, 5.0), depth_canal_mm=(0.0, -6.0), depth_anp_mm=(0.0, 2.5),
                depth_resection_mm=(0.0, -1.5), anterior_mm=(0.0, 3.0), medial_mm=(0.0, -2.0))
    return [dict(zip(FIELDS, c)) for c in itertools.product(*[vals[f] for f in FIELDS])]


def test_plane_from_offsets_matches_the_oracle(shim):
    """The three recorded cases of osteotomy_golden.npz (both sides) x a grid in which every field is non-zero at least once and
    all at once, all zero included: the bounds test_osteotomy_golden.close holds the oracle itself to."""
    G = np.load(os.path.join(GOLDEN, "osteotomy_golden.npz"))
    grid = offset_grid()
    assert any(all(v != 0 for v in g.values()) for g in grid) and any(all(v == 0 for v in g.values()) for g in grid)
    sides = set()
    for c in range(3):
        T, p, n, side = (G[f"c{c}_{k}"] for k in ("T_anp", "point_ct", "normal_ct", "side"))
        side = str(side)
        sides.add(side)
        for off in grid:
            want_p, want_n = apply_offsets(OracleOsteotomy(T, p, n, side), off).plane(np.identity(4))
            o7 = np.array([off[f] for f in FIELDS])
            Tc, pc, nc = (np.ascontiguousarray(a, dtype=np.float64) for a in (T, p, n))
            gp, gn = np.zeros(3), np.zeros(3)
            assert shim.rc_plane_from_offsets(Tc.ctypes.data, pc.ctypes.data, nc.ctypes.data, 1 if side == "right" else 0,
                                              o7.ctypes.data, gp.ctypes.data, gn.ctypes.data) == 0
            np.testing.assert_allclose(gp, want_p, rtol=0, atol=1e-9)
            np.testing.assert_allclose(gn, want_n, rtol=0, atol=1e-12)
    assert sides == {"left", "right"}


def test_resection_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.load()
    buf = np.zeros(64)
    ptr = ctypes.c_void_p(buf.ctypes.data)
    n = ctypes.c_int()
    for P in (1, 0, -1, 4097):
        assert L.sh_resect_planes(None, ptr, P, ptr) == -1
        assert L.sh_resect_offsets(None, ptr, P, ptr) == -1
    assert L.sh_resect_ring(None, 0, 0, None, 0, ctypes.byref(n)) == -1
    for name in ("sh_resect_planes", "sh_resect_offsets", "sh_resect_ring"):
        assert name in _lib.EXPORTS


def test_engine_offsets_argument_forms():
    """resect(offsets=...) takes dicts or a structured array with sh_cut_offset's field names; the mirror keeps their order"""
    assert FIELDS == ["retroversion_deg", "neckshaft_deg", "depth_canal_mm", "depth_anp_mm", "depth_resection_mm", "anterior_mm", "medial_mm"]
    assert list(_lib.CUT_OFFSET_DTYPE.names) == FIELDS
