"""Rays against the resident batch (include/shoulder_hip.h sh_ray_cast / sh_anp_axis_hits), the parts that need no GPU (the record
layout: test_abi_exports.py): the argument checks, the rule on numbers worked by hand, and the host twins (the
side-returning statement and the segment sort, host-compiled with -ffp-contract=off through tests/hostcheck/ray_check.cpp) against the
NumPy statement of tests/ray_oracle.py.

Bounds.  Hand-worked numbers are chosen exactly representable: equality.  Twins against the oracle: bytes (integers, and doubles that
the same operations in the same order produce)."""
import ctypes

import numpy as np
import pytest

import ray_oracle as O
import stem_oracle as SO
from shoulder_amd import _lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("ray_check"))


def test_ray_entry_points_check_their_arguments_without_a_gpu(shim):
    L = _lib.load()
    rays = np.zeros(4, dtype=_lib.RAY_DTYPE)
    rays["dir"] = (0.0, 0.0, 1.0)
    st = np.zeros(4, dtype=np.int32)
    p = ctypes.c_void_p(rays.ctypes.data)
    assert L.sh_ray_cast(None, p, 4, 0, 16, None, None) == O.ARG                      # (no context)
    assert L.sh_anp_axis_hits(None, 16, None, None, ctypes.c_void_p(st.ctypes.data)) == O.ARG
    assert "sh_ray_cast" in _lib.EXPORTS and "sh_anp_axis_hits" in _lib.EXPORTS
    # the ordered precheck itself against a context that is there (B = 2, idle)
    pre = lambda r=rays, R=4, per=0, cap=16, B=2, pend=0: shim.rc_precheck(r.ctypes.data if r is not None else None, R, per, cap, B, pend)
    assert pre() == 0 and pre(R=1) == 0 and pre(cap=1) == 0 and pre(cap=1024) == 0
    assert pre(cap=0) == O.ARG and pre(cap=1025) == O.ARG and pre(R=0) == O.ARG and pre(R=65537) == O.ARG and pre(r=None) == O.ARG
    assert pre(B=0) == O.STATE and pre(pend=1) == O.STATE
    for field, k, bad in (("origin", 1, np.nan), ("dir", 2, np.nan), ("origin", 0, np.inf), ("dir", 0, -np.inf)):
        r = rays.copy()
        r[field][3, k] = bad
        assert pre(r=r) == O.ARG and pre(r=r, R=3) == 0, (field, bad)
    r = rays.copy()
    r["dir"][2] = 0.0
    assert pre(r=r) == O.ARG
    r["dir"][2] = (0.0, -0.0, 5e-324)                                                 # a denormal direction is a direction
    assert pre(r=r) == 0
    per = np.zeros((2, 2), dtype=_lib.RAY_DTYPE)                                       # per humerus: B x R rays are read
    per["dir"] = (1.0, 0.0, 0.0)
    assert pre(r=per, R=2, per=1) == 0
    per["dir"][1, 1] = 0.0
    assert pre(r=per, R=2, per=1) == O.ARG and pre(r=per, R=2, per=0) == 0
    assert pre(cap=0, B=0) == O.ARG and pre(B=0, pend=1) == O.STATE                    # the argument comes first, then the state


TRI = np.array([(0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (0.0, 1.0, 2.0)])
UPZ = np.array([0.0, 0.0, 1.0])


def both(shim, o, d, tri):
    """the side-returning statement, which must agree with canal_ray_hit in verdict and t and with the oracle in everything"""
    (h, t, s), (h2, t2) = O.host_hit(shim, o, d, tri)
    assert h == h2 and (not h or np.float64(t).tobytes() == np.float64(t2).tobytes())
    ot, of, os_ = O.ray_hits(np.asarray(tri, np.float64), np.array([[0, 1, 2]]), o, d)
    assert len(ot) == h
    if h:
        assert np.float64(t).tobytes() == ot[0].tobytes() and s == os_[0]
    return (h, t, s) if h else (0, None, None)


def test_the_rule_on_numbers_worked_by_hand(shim):
    up, dn = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
    assert both(shim, (0.25, 0.25, 0.0), UPZ, TRI) == (1, 2.0, -1)                      # along the normal: it leaves
    assert both(shim, (0.25, 0.25, 0.0), UPZ, TRI[[0, 2, 1]]) == (1, 2.0, 1)            # the reversed triangle: it enters
    assert both(shim, (0.25, 0.25, 0.0), 2.0 * UPZ, TRI) == (1, 1.0, -1)                # t counts in units of |dir|
    assert both(shim, (0.25, 0.25, 4.0), -UPZ, TRI) == (1, 2.0, 1)
    # closed: the midpoints of the three edges and the three corners are hits
    for p in ((0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
        assert both(shim, (p[0], p[1], 0.0), UPZ, TRI)[:2] == (1, 2.0), p
    # one nextafter outside each edge is not
    assert both(shim, (0.5, dn(0.0), 0.0), UPZ, TRI)[0] == 0 and both(shim, (dn(0.0), 0.5, 0.0), UPZ, TRI)[0] == 0
    # the third edge is u + w <= 1 in float64: 0.5 + nextafter(0.5) rounds to 1.0 and is accepted by the rule as written, the first sum above 1 is not
    assert both(shim, (0.5, up(0.5), 0.0), UPZ, TRI)[0] == 1 and both(shim, (0.5, 0.5 + 2.0 ** -52, 0.0), UPZ, TRI)[0] == 0
    assert both(shim, (0.5 + 2.0 ** -52, 0.5, 0.0), UPZ, TRI)[0] == 0
    # an origin on the surface is not a hit (t > 1e-9), nor is one behind it; just in front of the bound is
    assert both(shim, (0.25, 0.25, 2.0), UPZ, TRI)[0] == 0 and both(shim, (0.25, 0.25, 3.0), UPZ, TRI)[0] == 0
    assert both(shim, (0.25, 0.25, 2.0 - 2.0 ** -29), UPZ, TRI) == (1, 2.0 ** -29, -1)    # 1.86e-9
    assert both(shim, (0.25, 0.25, 2.0 - 2.0 ** -30), UPZ, TRI)[0] == 0                  # 9.3e-10
    # parallel to the face, in its plane or beside it
    assert both(shim, (-1.0, 0.25, 2.0), (1.0, 0.0, 0.0), TRI)[0] == 0 and both(shim, (-1.0, 0.25, 1.0), (1.0, 0.0, 0.0), TRI)[0] == 0
    # |det| > 1e-12: a sliver of a direction across the face
    assert both(shim, (0.25, 0.25, 0.0), (1.0, 0.0, 1e-12), TRI)[0] == 0 and both(shim, (0.25, 0.25, 1.0), (0.0, 0.0, 2e-12), TRI)[0] == 1


def test_statement_twin_against_the_oracle_on_random_triangles(shim):
    rng = np.random.default_rng(5)
    n_hit = 0
    for _ in range(400):
        tri = rng.normal(size=(3, 3)).astype(np.float32).astype(np.float64)
        o = rng.normal(size=3) * 2.0
        target = tri.T @ rng.dirichlet((1.0, 1.0, 1.0)) if rng.random() < 0.7 else rng.normal(size=3)
        n_hit += both(shim, o, target - o, tri)[0]
    assert 150 < n_hit < 400


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_sort_twin_against_lexsort_with_exact_ties(shim, n):
    """t quantised to eight levels so that ties dominate; the keys arrive in a random order, as the device's slots do"""
    rng = np.random.default_rng(n)
    t = (rng.integers(1, 9, size=n) / 8.0).astype(np.float64)
    face = rng.permutation(4 * n)[:n].astype(np.int32)
    side = rng.choice(np.array([-1, 1], dtype=np.int32), size=n)
    o, d = rng.normal(size=3), rng.normal(size=3)
    order = np.lexsort((face, t))
    assert n == 1 or np.any(np.diff(t[order]) == 0)
    for cap in sorted({1, 8, n, n + 3, 1024}):
        got = O.host_sort(shim, t, face, side, o, d, cap)
        k = min(n, cap)
        want = np.zeros(cap, dtype=_lib.RAY_HIT_DTYPE)
        want["face"] = -1
        want["t"][:k], want["face"][:k], want["side"][:k] = t[order][:k], face[order][:k], side[order][:k]
        want["point"][:k] = o[None, :] + d[None, :] * t[order][:k, None]
        assert got.tobytes() == want.tobytes(), cap
    small = O.host_sort(shim, t, face, side, o, d, 8)                                  # a smaller cap is a byte prefix of a larger one
    assert O.host_sort(shim, t, face, side, o, d, 64)[:8].tobytes() == small.tobytes()


def test_cast_twin_against_the_oracle_on_small_meshes(shim):
    """tetrahedron (interior, vertex, edge, miss, origin on a face), the tilted 130-gon prism and the tube on a diameter, the plates
    with 40 hits and with 80 in tied pairs: t, face and side as bytes, the points too"""
    rng = np.random.default_rng(2)
    tv, tf = O.TETRA
    cases = [(tv, tf, (1.0, 1.0, -2.0), UPZ, 2), (tv, tf, (1.0, 1.0, 6.0), (-1.0, -1.0, -2.0), 3), (tv, tf, (2.0, -1.0, -1.0), (0.0, 1.0, 1.0), 3),
             (tv, tf, (9.0, 9.0, -2.0), UPZ, 0), (tv, tf, (1.0, 1.0, 0.0), UPZ, 1)]
    pv, pf = SO.mesh_in_ct(SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75)), *SO.prism(130, 10.0, -4.0, 6.0, 0.1))
    cases += [(pv, pf, rng.normal(size=3), rng.normal(size=3), None) for _ in range(8)]
    uv, uf = SO.tube(24, 4.0, 7.0, -5.0, 5.0, 0.05)
    cases += [(uv, uf, (-20.0, 0.3, 0.2), (1.0, 0.0, 0.0), 4)]
    qv, qf = O.plates(40)
    cases += [(qv, qf, (0.5, -0.25, 0.0), UPZ, 40), (qv, qf, (0.0, 0.0, 0.0), UPZ, 80), (qv, qf, (0.25, 0.25, 50.0), -UPZ, 80)]
    for v, f, o, d, want_n in cases:
        want, wn = O.cast(v, f, [o], [d], 128)
        got, n = O.host_cast(shim, v, f, o, d, 128)
        assert n == wn[0] and (want_n is None or n == want_n), (o, d, n)
        assert got.tobytes() == want[0].tobytes()
    got, n = O.host_cast(shim, uv, uf, (-20.0, 0.3, 0.2), (1.0, 0.0, 0.0), 8)
    assert list(got["side"][:4]) == [1, -1, 1, -1]                                     # in, out, in, out through the wall
    got, n = O.host_cast(shim, qv, qf, (0.0, 0.0, 0.0), UPZ, 128)
    assert np.array_equal(got["face"][:80], np.arange(80)) and np.array_equal(got["t"][:80], np.repeat(np.arange(1.0, 41.0), 2))
    got, n = O.host_cast(shim, tv, tf, (2.0, -1.0, -1.0), (0.0, 1.0, 1.0), 8)          # through the edge y = 0, z = 0: faces 0 and 1 at t = 1, then out
    assert list(got["face"][:3]) == [0, 1, 3] and list(got["t"][:3]) == [1.0, 1.0, 2.0] and list(got["side"][:3]) == [1, 1, -1]


def test_box_frame_twin_maps_corners_and_points(shim):
    """the box-frame loader: corners under T by xform_pt, the points back through inv_transform -- against the CT cast of the same mesh
    within 1e-9 mm (two rigid maps of numbers below 100), counts, faces and sides equal"""
    T = SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75))
    pv, pf = SO.prism(130, 10.0, -4.0, 6.0, 0.1)
    v32 = np.ascontiguousarray(pv, np.float32)
    rng = np.random.default_rng(4)
    for _ in range(6):
        o_ct, d_ct = rng.normal(size=3), rng.normal(size=3)
        o_box, d_box = T[:3, :3] @ o_ct + T[:3, 3], T[:3, :3] @ d_ct
        a, na = O.host_cast(shim, v32, pf, o_ct, d_ct, 16)
        b, nb = O.host_cast(shim, v32, pf, o_box, d_box, 16, T=T)
        assert na == nb and na >= 1 and np.array_equal(a["face"], b["face"]) and np.array_equal(a["side"], b["side"])
        assert np.abs(a["t"] - b["t"]).max() <= 1e-9 and np.abs(a["point"] - b["point"]).max() <= 1e-9
