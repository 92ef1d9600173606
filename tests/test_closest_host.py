"""Closest surface points of the resident batch (include/shoulder_hip.h sh_closest_points), the parts that need no GPU (the record
layout: test_abi_exports.py): the ordered argument checks, the region rule on numbers worked by hand, the host twins
(closest_pt_tri, the key order, the walk-and-join of one mesh, host-compiled with -ffp-contract=off through
tests/hostcheck/closest_check.cpp) against the NumPy statement of tests/closest_oracle.py, and the face-split formula.

Bounds.  Hand-worked numbers are chosen exactly representable: equality.  Twins against the oracle: bytes (integers, and doubles that
the same operations in the same order produce)."""
import ctypes

import numpy as np
import pytest

import closest_oracle as O
import stem_oracle as SO
from shoulder_amd import _lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("closest_check"))


def bits(x):
    return np.float64(x).tobytes()


def test_entry_point_checks_its_arguments_in_order_without_a_gpu(shim):
    L = _lib.load()
    pts = np.zeros((4, 3))
    assert L.sh_closest_points(None, ctypes.c_void_p(pts.ctypes.data), 4, 0, None) == O.ARG      # (no context)
    assert "sh_closest_points" in _lib.EXPORTS
    pre = lambda p=pts, Q=4, per=0, B=2, pend=0, ctx=1: shim.cc_precheck(ctx, p.ctypes.data if p is not None else None, Q, per, B, pend)
    assert pre() == 0 and pre(Q=1) == 0
    assert pre(ctx=0) == O.ARG and pre(p=None) == O.ARG and pre(Q=0) == O.ARG and pre(Q=-1) == O.ARG and pre(Q=_lib.CLOSEST_MAX + 1) == O.ARG
    big = np.zeros((_lib.CLOSEST_MAX, 3))
    assert pre(p=big, Q=_lib.CLOSEST_MAX, B=1) == 0                                   # the largest Q is accepted
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


TRI = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)])                    # the unit right triangle in z = 0: A, B, C


def both(shim, p, tri=TRI):
    """the host twin and the oracle must agree in everything: u, w, d2 as bytes and the region"""
    h, o = O.host_tri(shim, p, tri), O.oracle_tri(p, tri)
    assert h[2] == o[2] and all(bits(a) == bits(b) for a, b in zip((h[0], h[1], h[3]), (o[0], o[1], o[3]))), (p, h, o)
    return h


def test_the_region_rule_on_numbers_worked_by_hand(shim):
    # one query in each of the seven regions: (u, w, region, d2)
    assert both(shim, (0.25, 0.25, 0.0)) == (0.25, 0.25, 0, 0.0)                        # interior, on the face
    assert both(shim, (0.25, 0.25, 2.0)) == (0.25, 0.25, 0, 4.0)                        # interior, above it
    assert both(shim, (0.5, -1.0, 0.0)) == (0.5, 0.0, 1, 1.0)                           # edge AB
    assert both(shim, (1.0, 1.0, 0.0)) == (0.5, 0.5, 2, 0.5)                            # edge BC
    assert both(shim, (-2.0, 0.5, 0.0)) == (0.0, 0.5, 3, 4.0)                           # edge CA
    assert both(shim, (-1.0, -1.0, 0.0)) == (0.0, 0.0, 4, 2.0)                          # vertex A
    assert both(shim, (2.0, -0.5, 0.0)) == (1.0, 0.0, 5, 1.25)                          # vertex B
    assert both(shim, (-0.5, 2.0, 0.0)) == (0.0, 1.0, 6, 1.25)                          # vertex C
    # exactly on the boundaries between regions: which branch of the fixed order takes them
    assert both(shim, (0.0, 0.0, 0.0))[:3] == (0.0, 0.0, 4)                             # the corner A itself: vertex A (d1 = d2 = 0)
    assert both(shim, (1.0, 0.0, 0.0))[:3] == (1.0, 0.0, 5)                             # B: vertex B (d3 = 0, d4 = -1 <= d3)
    assert both(shim, (0.0, 1.0, 0.0))[:3] == (0.0, 1.0, 6)                             # C: vertex C
    assert both(shim, (0.0, -1.0, 0.0))[:3] == (0.0, 0.0, 4)                            # on the line between vertex A and edge AB (d1 = 0): vertex A comes first
    assert both(shim, (-1.0, 0.0, 0.0))[:3] == (0.0, 0.0, 4)                            # ... between vertex A and edge CA (d2 = 0): vertex A
    assert both(shim, (1.0, -1.0, 0.0))[:3] == (1.0, 0.0, 5)                            # ... between edge AB and vertex B (d3 = 0): vertex B comes before the edge
    assert both(shim, (2.0, 1.0, 0.0))[:3] == (1.0, 0.0, 5)                             # ... between vertex B and edge BC (d4 = d3): vertex B
    assert both(shim, (-1.0, 1.0, 0.0))[:3] == (0.0, 1.0, 6)                            # ... between edge CA and vertex C (d6 = 0): vertex C comes before that edge
    assert both(shim, (1.0, 2.0, 0.0))[:3] == (0.0, 1.0, 6)                             # ... between vertex C and edge BC (d5 = d6): vertex C
    assert both(shim, (0.5, 0.0, 0.0))[:3] == (0.5, 0.0, 1)                             # on the edge AB (vc = 0): the edge, not the interior
    assert both(shim, (0.0, 0.5, 0.0))[:3] == (0.0, 0.5, 3)                             # on the edge CA (vb = 0)
    assert both(shim, (0.5, 0.5, 0.0))[:3] == (0.5, 0.5, 2)                             # on the edge BC (va = 0)
    assert both(shim, (0.5, 0.0, 3.0)) == (0.5, 0.0, 1, 9.0)                            # above the edge AB: still the edge
    # side, through the walk of a one-face mesh: above and below the plane, and in it
    v, f = TRI.astype(np.float32), np.array([(0, 1, 2)], dtype=np.int32)
    got = O.host_mesh(shim, v, f, [(0.25, 0.25, 2.0), (0.25, 0.25, -2.0), (0.25, 0.25, 0.0), (2.0, -0.5, 1.0), (2.0, -0.5, -1.0)])
    assert list(got["side"]) == [1, -1, 1, 1, -1] and list(got["region"]) == [0, 0, 0, 5, 5] and list(got["dist"]) == [2.0, 2.0, 0.0, 1.5, 1.5]
    assert got.tobytes() == O.closest(v, f, [(0.25, 0.25, 2.0), (0.25, 0.25, -2.0), (0.25, 0.25, 0.0), (2.0, -0.5, 1.0), (2.0, -0.5, -1.0)]).tobytes()


def random_pairs():
    """400 triangle / point pairs: 240 general ones with float32 corners, 80 slivers (one edge 1e-6 of the others), 80 collinear"""
    rng = np.random.default_rng(11)
    out = []
    for k in range(400):
        tri = rng.normal(size=(3, 3)).astype(np.float32).astype(np.float64)
        kind = "general"
        if 240 <= k < 320:
            tri[2] = (tri[1] + 1e-6 * rng.normal(size=3)).astype(np.float32).astype(np.float64) if k % 2 else tri[1] + 1e-6 * rng.normal(size=3)
            kind = "sliver"
        elif k >= 320:
            t = rng.uniform(-1.0, 2.0)
            tri[2] = tri[0] + t * (tri[1] - tri[0])                                   # on the line through A and B, as float64 rounds it
            kind = "collinear"
        p = tri.T @ rng.dirichlet((1.0, 1.0, 1.0)) + rng.normal(size=3) * rng.choice([0.0, 1e-3, 1.0])
        out.append((kind, tri, p))
    return out


def test_statement_twin_against_the_oracle_on_random_pairs(shim):
    regions, nonfinite = set(), 0
    for kind, tri, p in random_pairs():
        u, w, region, d2 = both(shim, p, tri)
        regions.add(region)
        if not np.isfinite(d2):
            nonfinite += 1
            assert kind == "collinear" and region == 0
            # such a candidate loses against any finite one, first or last
            assert shim.cc_key_less(d2, 0, 1e300, 5) == 0 and shim.cc_key_less(1e300, 5, d2, 0) == 1
    print("regions met:", sorted(regions), "candidates that are not finite:", nonfinite)
    assert regions == set(range(7))


def test_the_key_order(shim):
    less = shim.cc_key_less
    assert less(1.0, 3, 2.0, 1) == 1 and less(2.0, 1, 1.0, 3) == 0
    assert less(1.0, 3, 1.0, 7) == 1 and less(1.0, 7, 1.0, 3) == 0 and less(1.0, 3, 1.0, 3) == 0      # the smaller id; irreflexive
    assert less(0.0, 3, -0.0, 2) == 0 and less(-0.0, 2, 0.0, 3) == 1                                    # the zeros are one value
    for bad in (np.nan, np.inf, -np.inf):
        assert less(bad, 0, 1e308, 9) == 0 and less(1e308, 9, bad, 0) == 1 and less(bad, 0, bad, 1) == 0
    # two identical faces give the smaller id, and a collinear face in front or behind changes nothing
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5), (6, 6, 6), (7, 7, 7)], dtype=np.float32)
    p = [(0.25, 0.25, 1.0), (3.0, -1.0, 0.5)]
    for faces in ([(0, 1, 2), (0, 1, 2)], [(3, 4, 5), (0, 1, 2), (0, 1, 2)], [(0, 1, 2), (0, 1, 2), (3, 4, 5)]):
        f = np.array(faces, dtype=np.int32)
        want = O.closest(v, f, p)
        assert list(want["face"]) == [faces.index((0, 1, 2))] * 2
        for back in (False, True):
            assert O.host_mesh(shim, v, f, p, backwards=back).tobytes() == want.tobytes()


def test_a_candidate_that_is_not_finite_never_wins(shim):
    """Collinear triangles: exact ones (C = A + t (B - A) in small binary fractions) against points with all their bits.  Under the rule
    as written they end in a vertex or an edge branch, or in the interior branch with a quotient of rounding noise -- which is FINITE
    unless the three products sum to zero exactly (none did in 250 000 interior cases tried when this test was written).  So the twin
    is held to the oracle on them, bytes, whatever comes; and a d2 that is not finite is made where it certainly is: a point 1e200 mm
    away, whose squared distance overflows.  Alone such a candidate is the status, beside a finite one it loses, first or last."""
    rng = np.random.default_rng(5)
    interior = 0
    for _ in range(300):
        a, d = rng.integers(-256, 256, 3) / 64.0, rng.integers(1, 64, 3) / 64.0
        tri = np.stack([a, a + d, a + rng.choice([3.0, -3.0, 0.375, -0.625, 1.75]) * d])
        u, w, region, d2 = both(shim, np.round(rng.normal(size=3) * 4.0, 3), tri)
        interior += region == 0
    print("collinear triangles that reached the interior branch:", interior, "of 300")
    far = [(1e200, 0.0, 0.0), (1e200, -1e200, 1e180)]
    for p in far:
        u, w, region, d2 = both(shim, p)
        assert not np.isfinite(d2)
        assert shim.cc_key_less(d2, 0, 1e300, 5) == 0 and shim.cc_key_less(1e300, 5, d2, 0) == 1
    v = np.array([(0, 0, 0), (1, 0, 0), (3, 0, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=np.float32)      # a collinear face and a proper one
    line, both_faces = np.array([(0, 1, 2)], dtype=np.int32), np.array([(0, 1, 2), (3, 4, 5)], dtype=np.int32)
    alone = O.host_mesh(shim, v, line, far)
    assert np.all(alone["status"] == O.GEOMETRY) and np.all(alone["face"] == -1) and not alone["dist"].any() and not alone["point"].any()
    assert not alone["region"].any() and not alone["side"].any() and alone.tobytes() == O.closest(v, line, far).tobytes()
    near = [(2.0, 1.0, 0.0), (0.25, 0.25, 1.0), (-1.0, 0.0, 0.0)]                       # the collinear face is a segment: finite answers
    got = O.host_mesh(shim, v, line, near)
    assert np.all(got["status"] == 0) and list(got["dist"]) == [1.0, np.sqrt(0.0625 + 1.0), 1.0] and got.tobytes() == O.closest(v, line, near).tobytes()
    for f in (both_faces, both_faces[::-1].copy()):
        assert O.host_mesh(shim, v, f, near + far).tobytes() == O.closest(v, f, near + far).tobytes()


def test_walk_and_join_twin_against_the_oracle_on_small_meshes(shim):
    """the tetrahedron and the tilted 130-gon prism (520 faces, three tiles): any number of splits, either order of the walk -- bytes"""
    rng = np.random.default_rng(3)
    tv, tf = O.TETRA
    pts = [(1.0, 1.0, -2.0), (2.0, -3.0, -4.0), (-2.0, -2.0, -1.0), (0.5, 0.5, 0.25), (1.0, 1.0, 0.0), (4.0, 4.0, 4.0)]
    want = O.closest(tv, tf, pts)
    assert list(want["face"]) == [0, 0, 0, 0, 0, 3] and list(want["region"]) == [0, 3, 4, 0, 0, 0] and list(want["side"]) == [1, 1, 1, -1, 1, 1]
    assert list(want["dist"][:5]) == [2.0, 5.0, 3.0, 0.25, 0.0]
    for S, back in ((1, False), (1, True)):
        assert O.host_mesh(shim, tv, tf, pts, S, back).tobytes() == want.tobytes()
    pv, pf = SO.mesh_in_ct(SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75)), *SO.prism(130, 10.0, -4.0, 6.0, 0.1))
    pv = np.ascontiguousarray(pv, np.float32)
    pts = np.concatenate([rng.normal(size=(12, 3)) * 8.0, pv[rng.integers(0, len(pv), 6)].astype(np.float64)])
    want = O.closest(pv, pf, pts)
    assert (want["status"] == 0).all() and max(O.ties(pv, pf, p) for p in pts[12:]) >= 2      # a vertex is shared: exact ties
    for S in (1, 2, 3):
        for back in (False, True):
            assert O.host_mesh(shim, pv, pf, pts, S, back).tobytes() == want.tobytes(), (S, back)


@pytest.mark.parametrize("F", [1, 255, 256, 257, 32440])
def test_the_face_split_formula(shim, F):
    tiles = (F + 255) // 256
    for groups in (1, 64, 4096):
        S = shim.cc_splits(groups, tiles)
        assert 1 <= S <= tiles
        assert S == max(1, min(tiles, -(-1024 // groups)))                            # fills 1 024 workgroups, never more than the tiles
        # the splits cover every tile exactly once, whatever the humerus' own tile count is (a ragged batch: fewer tiles than S)
        for own in sorted({tiles, 1, max(1, tiles // 3)}):
            seen = np.zeros(own, dtype=np.int32)
            for s in range(S):
                t0, t1 = ctypes.c_int(-1), ctypes.c_int(-1)
                shim.cc_split_range(own, S, s, ctypes.addressof(t0), ctypes.addressof(t1))
                assert 0 <= t0.value <= t1.value <= own
                seen[t0.value:t1.value] += 1
            assert np.all(seen == 1), (F, groups, own)
    assert shim.cc_splits(1, 127) == 127 and shim.cc_splits(64, 127) == 16 and shim.cc_splits(4096, 127) == 1 and shim.cc_splits(0, 5) == 5
