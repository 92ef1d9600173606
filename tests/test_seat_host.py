"""Seats of implant heads on a cut (include/shoulder_hip.h sh_seat), the parts that need no GPU (record layout: test_abi_exports.py): argument checks, the
seat arithmetic the device runs (sh_scalar.h seat_edge_term / seat_seg_dist2 / seat_winding_term / seat_surface_rms, host-compiled
with -ffp-contract=off through tests/hostcheck/seat_check.cpp) against closed forms, the NumPy statement and the N-gon clip of
tests/seat_oracle.py, and the arithmetic of best_seat.

Bounds.  Closed forms on the square: 1e-12 mm^2.  Covered area against the inscribed-N-gon clip: the clip's own deficit bound
pi rho^2 (1 - sin(2 pi / N) / (2 pi / N)), N = 4096.  surface_rms: 1e-6 mm, the project's landmark bound (tests/test_headfit_host.py)."""
import ctypes

import numpy as np
import pytest

import headfit_oracle as H
import seat_oracle as S
from shoulder_amd import _lib
from shoulder_amd.arthroplasty import best_seat

MM = 1e-6
SQUARE = (np.array([5.0, -5.0, -5.0, 5.0]), np.array([5.0, 5.0, -5.0, -5.0]))      # side 10 about its centre, counter-clockwise


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.build_shim(tmp_path_factory.mktemp("seat_check"))


@pytest.fixture(scope="module")
def fit_shim(tmp_path_factory):
    return H.build_shim(tmp_path_factory.mktemp("headfit_check_seat"))


@pytest.fixture(scope="module")
def humerus_cuts():
    return S.humerus_cuts()


def test_seat_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.load()
    buf = np.zeros(64 * 29)
    ptr = ctypes.c_void_p(buf.ctypes.data)
    good = np.tile([24.0, 18.0], (65, 1))

    def call(heads, K, mode):
        h = np.ascontiguousarray(heads, dtype=np.float64)
        return (L.sh_resect_planes_seat(None, ptr, 1, ctypes.c_void_p(h.ctypes.data), K, mode, ptr, ptr, ptr),
                L.sh_resect_offsets_seat(None, ptr, 1, ctypes.c_void_p(h.ctypes.data), K, mode, ptr, ptr, ptr))
    for heads, K, mode in ((good, 0, 0), (good, 65, 0), ([[24.0, 48.0]], 1, 0), ([[np.nan, 18.0]], 1, 0), (good, 1, 2), (good, 1, 0)):
        assert call(heads, K, mode) == (-1, -1)                                       # (the last: no context)
    assert "sh_resect_planes_seat" in _lib.EXPORTS and "sh_resect_offsets_seat" in _lib.EXPORTS


def test_square_closed_forms(shim):
    x, y = SQUARE
    for rho, want in ((3.0, np.pi * 9.0), (5.0, np.pi * 25.0), (6.0, np.pi * 36.0 - 4.0 * (36.0 * np.arccos(5.0 / 6.0) - 5.0 * np.sqrt(36.0 - 25.0))), (8.0, 100.0)):
        r = S.host_seat(shim, x, y, rho)
        print("rho", rho, "host", r["covered_area"] - want, "numpy", S.covered_area(x, y, rho) - want)
        assert abs(r["covered_area"] - want) <= 1e-12 and abs(S.covered_area(x, y, rho) - want) <= 1e-12
        assert r["rim_min"] == 5.0 and abs(r["rim_max"] - 5.0 * np.sqrt(2.0)) <= 1e-15 and r["winding"] == 1
        assert r["imin"] == 0 and r["imax"] == 0 and np.array_equal(r["near"], [0.0, 5.0]) and np.array_equal(r["far"], [5.0, 5.0])      # ties: the first in ring order
    # a tangent edge alone is a sector, not a chord: the quarter turn of the circle
    assert abs(shim.st_edge(5.0, -5.0, 5.0, 5.0, 25.0) - 0.5 * 25.0 * (np.pi / 2)) <= 1e-14
    # a degenerate edge and an edge through the centre
    assert shim.st_edge(1.0, 2.0, 1.0, 2.0, 9.0) == 0.0 and shim.st_edge(-1.0, 0.0, 1.0, 0.0, 9.0) == 0.0


def test_a_clockwise_ring_and_a_centre_outside(shim):
    x, y = SQUARE
    for rho in (3.0, 6.0, 8.0):
        assert S.host_seat(shim, x[::-1].copy(), y[::-1].copy(), rho)["covered_area"] == pytest.approx(S.host_seat(shim, x, y, rho)["covered_area"], abs=1e-12)
    assert S.host_seat(shim, x[::-1].copy(), y[::-1].copy(), 6.0)["winding"] == -1
    # the seat centre 9 to the right of the square's centre: outside it, the disk of radius 5.5 reaches 1.5 into the square (its chord
    # on the side x = -4 is 2 sqrt(5.5^2 - 16) = 7.55 long, inside the side's 10)
    xs = x - 9.0
    r = S.host_seat(shim, xs, y, 5.5)
    seg = 30.25 * np.arccos(4.0 / 5.5) - 4.0 * np.sqrt(30.25 - 16.0)                  # circular segment beyond the line x = -4
    clip = S.clip_area_ngon(xs, y, 5.5)
    print("outside:", r["covered_area"], seg, clip)
    assert r["winding"] == 0 and abs(r["covered_area"] - seg) <= 1e-12
    assert abs(r["covered_area"] - clip) <= S.ngon_bound(5.5)
    assert r["rim_min"] == 4.0 and np.array_equal(r["near"], [-4.0, 0.0]) and r["imin"] == 3
    assert abs(S.covered_area(xs, y, 5.5) - seg) <= 1e-12 and S.winding(xs, y) == 0


def test_numpy_statement_and_host_source_agree_on_a_ragged_ring(shim):
    rng = np.random.default_rng(11)
    t = np.sort(rng.uniform(0, 2 * np.pi, 301))
    r = 20.0 + 6.0 * np.sin(3 * t) + rng.uniform(-1.5, 1.5, len(t))
    x, y = r * np.cos(t) + 1.5, r * np.sin(t) - 2.0
    for rho in (10.0, 19.0, 24.0, 40.0):
        h = S.host_seat(shim, x, y, rho)
        rmin, near, imin, rmax, far, imax = S.rim(x, y)
        assert abs(h["covered_area"] - S.covered_area(x, y, rho)) <= 1e-9
        assert (h["imin"], h["imax"], h["winding"]) == (imin, imax, S.winding(x, y)) and abs(h["rim_min"] - rmin) <= 1e-12 and abs(h["rim_max"] - rmax) <= 1e-12
        if rho > rmin:      # (a disk wholly inside the ring falls short by EXACTLY the bound, whose 1 - sin t / t is itself rounded to 3e-10 of it)
            assert abs(h["covered_area"] - S.clip_area_ngon(x, y, rho)) <= S.ngon_bound(rho)
        else:
            assert abs(h["covered_area"] - np.pi * rho * rho) <= 1e-12


def test_humerus_cuts_against_the_ngon_clip(shim, humerus_cuts):
    for (o, n, O), factor in zip(humerus_cuts[2], (1.0, 1.15, 1.0, 1.15)):
        x, y = S.in_plane(O.ring[:-1], o, n)
        cx, cy = H.ring_sums(O.ring, o, n)[1:3] / (3.0 * H.ring_sums(O.ring, o, n)[0])
        x, y = x - cx, y - cy
        rho = factor * np.sqrt(O.ellipse[0] * O.ellipse[1])
        h = S.host_seat(shim, x, y, rho)
        clip = S.clip_area_ngon(x, y, rho)
        print("ring", len(x), "rho", rho, "covered", h["covered_area"], "clip deficit", h["covered_area"] - clip, "bound", S.ngon_bound(rho))
        assert abs(h["covered_area"] - clip) <= S.ngon_bound(rho)
        assert abs(h["covered_area"] - S.covered_area(x, y, rho)) <= 1e-9 and h["winding"] == 1
        assert h["covered_area"] <= min(abs(S.shoelace(x, y)), np.pi * rho * rho) + 1e-9


def test_surface_rms_from_moments(shim, fit_shim, humerus_cuts):
    for o, n, O in humerus_cuts[2]:
        rc, c, r, rms = H.host_sphere(fit_shim, O.moments)
        assert rc == 0
        got = S.host_rms(shim, O.moments, c, r)
        print("at the fitted sphere:", got, rms, O.rms)
        assert abs(got - rms) <= MM and abs(got - O.rms) <= MM
        un = n / np.linalg.norm(n)
        for c2, R2 in ((c + 1.5 * un, r), (c - np.array([2.0, -1.0, 0.5]), 0.9 * r), (O.q.mean(axis=0) + 3.0 * un, 1.2 * r)):
            got, want = S.host_rms(shim, O.moments, c2, R2), S.surface_rms_direct(O.q, O.w, c2, R2)
            print("elsewhere:", got, want, got - want)
            assert abs(got - want) <= MM
    assert S.host_rms(shim, np.zeros(16), np.zeros(3), 24.0) == 0.0


def test_best_seat_arithmetic():
    s = np.zeros(5, dtype=_lib.SEAT_DTYPE)
    s["coverage"], s["max_overhang"], s["status"] = [0.7, 0.95, 0.9, 0.99, 0.9], [0.0, 2.5, 1.0, 0.2, 0.5], [0, 0, 0, -5, 0]
    assert best_seat(s, 1.0) == 2 and best_seat(s, 3.0) == 1 and best_seat(s, 0.0) == 0 and best_seat(s, -1.0) is None
    assert best_seat([dict(coverage=0.5, max_overhang=0.0, status=-4)], 1.0) is None
    assert best_seat([{k: r[k] for k in ("coverage", "max_overhang", "status")} for r in s], 1.0) == 2
