"""Generalized winding numbers of the resident batch (include/shoulder_hip.h sh_winding_numbers), the parts that need no GPU (the
record layout: test_abi_exports.py): the ordered argument checks, the solid angle of the host-compiled statement
(-ffp-contract=off, tests/hostcheck/winding_check.cpp) against the NumPy statement of tests/winding_oracle.py, hand-worked values on the
cube of edge 2, the walk-and-join twin with any number of splits, the split formula, and the stand-alone sanitizer build of the twin.

Bounds.  num and den: bytes (the same operations in the same order).  omega: 4 ulp, for the two libraries' atan2.  A sum against the
oracle: winding_oracle.bound, (2 F + 16) 2^-53 max(1, A) with A the oracle's.  A sum against the same sum under another split: bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import winding_oracle as O
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

EPS = 2.0 ** -53
CENTRE, OUTSIDE, ON_FACE = (0.0, 0.0, 0.0), (3.0, 1.0, 1.0), (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("winding_check"))


@pytest.fixture(scope="module")
def humerus_mesh():
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def bits(x):
    return np.float64(x).tobytes()


def test_entry_point_checks_its_arguments_in_order_without_a_gpu(shim):
    assert _lib.WIND_BLOCK == O.BLOCK == 2048
    L = _lib.load()
    pts = np.zeros((4, 3))
    assert L.sh_winding_numbers(None, ctypes.c_void_p(pts.ctypes.data), 4, 0, None) == O.ARG      # (no context)
    assert "sh_winding_numbers" in _lib.EXPORTS
    pre = lambda p=pts, Q=4, per=0, B=2, pend=0, ctx=1: shim.wc_precheck(ctx, p.ctypes.data if p is not None else None, Q, per, B, pend)
    assert pre() == 0 and pre(Q=1) == 0
    assert pre(ctx=0) == O.ARG and pre(p=None) == O.ARG and pre(Q=0) == O.ARG and pre(Q=-1) == O.ARG and pre(Q=_lib.WINDING_MAX + 1) == O.ARG
    big = np.zeros((_lib.WINDING_MAX, 3))
    assert pre(p=big, Q=_lib.WINDING_MAX, B=1) == 0                                   # the largest Q is accepted
    assert pre(B=0) == O.STATE and pre(pend=1) == O.STATE
    for k, bad in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        p = pts.copy()
        p[3, k] = bad
        assert pre(p=p) == O.ARG and pre(p=p, Q=3) == 0, (k, bad)
    per = np.zeros((2, 2, 3))                                                          # per humerus: B x Q points are read
    assert pre(p=per, Q=2, per=1) == 0
    per[1, 1, 2] = np.nan
    assert pre(p=per, Q=2, per=1) == O.ARG and pre(p=per, Q=2, per=0) == 0
    # the order: the arguments that need no state, then the state, then the coordinates
    p = pts.copy()
    p[0, 0] = np.nan
    assert pre(p=p, Q=0, B=0) == O.ARG and pre(p=p, B=0) == O.STATE and pre(p=p, pend=1) == O.STATE and pre(p=p, B=0, pend=1) == O.STATE
    assert pre(p=p) == O.ARG


def random_pairs():
    """400 triangle / point pairs: 240 general ones with float32 corners, 80 slivers (one edge 1e-6 of the others), 80 with the point
    in the plane of the triangle up to rounding or exactly"""
    rng = np.random.default_rng(13)
    out = []
    for k in range(400):
        tri = rng.normal(size=(3, 3)).astype(np.float32).astype(np.float64)
        kind = "general"
        p = tri.T @ rng.dirichlet((1.0, 1.0, 1.0)) + rng.normal(size=3) * rng.choice([1e-3, 1.0, 30.0])
        if 240 <= k < 320:
            tri[2] = (tri[1] + 1e-6 * rng.normal(size=3)).astype(np.float32).astype(np.float64)
            kind = "sliver"
        elif k >= 320:
            kind = "coplanar"
            if k % 2:
                tri[:, 2] = 0.25                                                      # the plane z = 1/4, the point in it: num is an exact zero
                p = np.array([rng.normal(), rng.normal(), 0.25])
            else:
                p = tri.T @ rng.dirichlet((1.0, 1.0, 1.0)) * rng.choice([1.0, 3.0, -2.0])      # in the plane (or near it) as float64 rounds it
        out.append((kind, tri, p))
    return out


def test_solid_angle_twin_against_numpy_on_random_pairs(shim):
    worst, zeros = 0.0, 0
    for kind, tri, p in random_pairs():
        num, den, om = O.host_solid(shim, p, tri)
        n, d = O.solid_terms(tri[None, 0], tri[None, 1], tri[None, 2], p)
        assert bits(num) == bits(n[0]) and bits(den) == bits(d[0]), (kind, num, n[0], den, d[0])
        want = float(O.solid_angles(tri[None, 0], tri[None, 1], tri[None, 2], p)[0])
        ulp = np.spacing(abs(want)) if want != 0.0 else 0.0
        assert abs(om - want) <= 4.0 * ulp, (kind, om, want)
        worst = max(worst, abs(om - want) / ulp if ulp else 0.0)
        if num == 0.0:
            zeros += 1
            assert om == 0.0 and not np.signbit(om) and want == 0.0
        assert abs(om) <= 2.0 * np.pi
    print("solid angle, host twin against NumPy: largest difference", worst, "ulp; pairs with num == 0:", zeros)
    assert zeros >= 40                                                                 # the exact-zero rule was met
    # num == 0 with either sign of the zero, and whatever den is (behind the triangle's plane den < 0 would give +- 2 pi from atan2)
    tri = np.array([(1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 1.0, 0.0)])
    for p in ((0.0, 0.0, 0.0), (1.5, 0.25, 0.0), (-0.0, -0.0, -0.0)):
        num, den, om = O.host_solid(shim, p, tri)
        assert num == 0.0 and om == 0.0 and bits(om) == bits(0.0)
        assert O.solid_angles(tri[None, 0], tri[None, 1], tri[None, 2], np.array(p))[0] == 0.0
    num, den, om = O.host_solid(shim, (1.75, 0.25, 0.0), tri)                          # inside the triangle, in its plane: den < 0, num == 0
    assert num == 0.0 and den < 0.0 and om == 0.0


def test_hand_worked_values_on_the_cube(shim):
    v, f = O.cube()
    A, B, C = O.corners(v, f)
    om = O.solid_angles(A, B, C, np.array(CENTRE))
    host = [O.host_solid(shim, CENTRE, np.stack([A[k], B[k], C[k]]))[2] for k in range(12)]
    assert np.abs(om - 4.0 * np.pi / 12.0).max() <= 4 * EPS * 2 and np.abs(np.array(host) - 4.0 * np.pi / 12.0).max() <= 4 * EPS * 2      # every triangle: a twelfth of the sphere
    cases = [("closed", CENTRE, 1.0, 1), ("open", CENTRE, 5.0 / 6.0, 1), ("doubled", CENTRE, 2.0, 1), ("reversed", CENTRE, -1.0, 1),
             ("closed", OUTSIDE, 0.0, 0), ("closed", ON_FACE, 0.5, None), ("reversed", OUTSIDE, 0.0, 0), ("open", OUTSIDE, 0.0, 0)]
    for kind, p, w, inside in cases:
        v, f = O.cube(kind)
        want, absw = O.winding(v, f, [p])
        assert abs(want["winding"][0] - w) <= 16 * EPS * max(1.0, absw[0]), (kind, p, want["winding"][0])
        for S in (1, 2):
            got = O.host_mesh(shim, v, f, [p], S)
            assert got["status"][0] == 0 and abs(got["winding"][0] - w) <= 16 * EPS * max(1.0, absw[0]), (kind, p, S, got["winding"][0])
            if inside is not None:
                assert got["inside"][0] == want["inside"][0] == inside, (kind, p)
    # on the face z = 1 inside its triangle (4, 7, 6): both triangles of that side give an exact zero, the other ten give half the sphere
    om = O.solid_angles(*O.corners(*O.cube()), np.array(ON_FACE))
    assert om[10] == 0.0 and om[11] == 0.0 and np.all(om[:10] > 0.0)
    # from 1e200 mm along a diagonal the products of b x c overflow to inf - inf: the sum is NaN -- the status, zeros
    d = 1e200 / np.sqrt(3.0)
    for p in ((d, -d, d), (0.0, -1e200, 1e180), (-d, -d, -d)):
        want, absw = O.winding(*O.cube(), [p])
        got = O.host_mesh(shim, *O.cube(), [p])
        assert want["status"][0] == got["status"][0] == O.GEOMETRY and got.tobytes() == want.tobytes() and not got["winding"].any() and not got["inside"].any()


    # along one axis only the lengths overflow: num stays finite, den is +inf, atan2 gives 0 for every face -- w = 0 with status 0,
    # which is the right answer for a point that far outside
    for p in ((1e200, 0.0, 0.0), (0.0, 0.0, -1e200)):
        want, absw = O.winding(*O.cube(), [p])
        got = O.host_mesh(shim, *O.cube(), [p])
        assert want["status"][0] == 0 and got.tobytes() == want.tobytes() and got["winding"][0] == 0.0 and got["inside"][0] == 0


@pytest.mark.parametrize("F", [2047, 2048, 2049, 4097])
def test_walk_and_join_twin_against_the_oracle(shim, humerus_mesh, F):
    """the first F faces of humerus_left -- an open mesh: fractions -- at the block's edges; any number of splits gives the same bytes"""
    v, f = humerus_mesh
    f = np.ascontiguousarray(f[:F])
    rng = np.random.default_rng(F)
    used = v[np.unique(f)].astype(np.float64)
    pts = used[rng.integers(0, len(used), 24)] + rng.normal(size=(24, 3)) * rng.choice([0.5, 3.0, 20.0], size=(24, 1))
    want, absw = O.winding(v, f, pts)
    blocks = -(-F // O.BLOCK)
    first = O.host_mesh(shim, v, f, pts, 1)
    worst, lim = O.compare(first, want, absw, F)
    print("F =", F, "blocks", blocks, "max |twin - oracle|", worst, "bound", lim, "| winding in", float(want["winding"].min()), float(want["winding"].max()))
    assert np.all(np.abs(want["winding"]) < 1.0) and np.all(np.abs(want["winding"]) > 1e-6)      # an open patch: fractions, no integers
    for S in (2, 3, blocks, blocks + 2):                                               # more splits than blocks: the surplus ones are empty
        assert O.host_mesh(shim, v, f, pts, S).tobytes() == first.tobytes(), S


def test_the_split_formula(shim):
    fill = 1024
    for blocks, F in ((1, 2048), (16, 32440), (1016, 2080000)):
        assert -(-F // O.BLOCK) == blocks
        for groups in (1, 64, 4096):
            S = shim.wc_splits(groups, blocks)
            assert S == max(1, min(blocks, -(-fill // groups))) and 1 <= S <= blocks, (blocks, groups)
    assert [shim.wc_splits(g, 16) for g in (1, 64, 4096)] == [16, 16, 1] and [shim.wc_splits(g, 1016) for g in (1, 64, 4096)] == [1016, 16, 1]
    assert [shim.wc_splits(g, 1) for g in (1, 64, 4096)] == [1, 1, 1] and shim.wc_splits(0, 5) == 5 and shim.wc_splits(256, 16) == 4
    # the plan of a call: chunks of 256 points; "wn.part" holds one total per point when S == 1 and the block sums otherwise
    assert O.host_plan(shim, 1, 1, 32440) == (16, 1, 16, 16)
    assert O.host_plan(shim, 64, 1024, 32440) == (16, 4, 4, 16)
    assert O.host_plan(shim, 64, 4096, 32440) == (16, 16, 1, 1)
    assert O.host_plan(shim, 1, 257, 12) == (1, 2, 1, 1)
    # whole blocks, each exactly once, whatever the humerus' own block count is (a ragged batch: fewer blocks than S)
    for S in (1, 4, 16):
        for own in (1, 3, 16):
            seen = np.zeros(own, dtype=np.int32)
            for s in range(S):
                a, b = ctypes.c_int(-1), ctypes.c_int(-1)
                shim.wc_split_range(own, S, s, ctypes.addressof(a), ctypes.addressof(b))
                k0, k1 = a.value, b.value
                assert 0 <= k0 <= k1 <= own
                seen[k0:k1] += 1
            assert np.all(seen == 1), (S, own)


def test_the_twin_as_a_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "winding_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
