"""Rays through the face hierarchy on the engine (include/shoulder_hip.h sh_ray_cast with SH_ACCEL_BVH, sh_ray_nearest; k_raytree.h),
the thickness on top of them and the facade.

Bounds.  Switch on against switch off, nearest against row 0, and the resident buffers against what the calls returned: bytes.  Against the
NumPy statements of tests/raytree_oracle.py (every ray against every face): faces equal, thickness and points within 1e-6 mm, the project's
bound."""
import os

import numpy as np
import pytest

import ray_oracle as O
import raytree_oracle as RT
import stem_oracle as SO
import shoulder_amd as shoulder
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.engine import THICKNESS_DTYPE, Engine, ShoulderHipError
from test_bvh_host import T_TILT, bone, f32, prism130, sheet

pytestmark = pytest.mark.gpu
MM = 1e-6


def tube24():
    return f32(SO.mesh_in_ct(T_TILT, *SO.tube(24, 4.0, 7.0, -5.0, 5.0, 0.05)))


def frame_rays(T, origins, directions):
    return SO.to_ct(T, origins), np.asarray(directions, np.float64) @ T[:3, :3]


@pytest.fixture
def accel(engine):
    """the engine with the switch off; off again afterwards"""
    engine.query_accel = "off"
    try:
        yield engine
    finally:
        engine.query_accel = "off"


def both(engine, o, d, cap):
    """ray_cast and ray_nearest with the switch off and on, everything compared as bytes -> the answer: hits, counts, nearest"""
    out = {}
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        hits, counts = engine.ray_cast(o, d, cap=cap)
        res_h = engine.fetch("ray.hits", _lib.RAY_HIT_DTYPE, hits.shape)
        res_c = engine.fetch("ray.counts", np.int32, counts.shape)
        assert res_h.tobytes() == hits.tobytes() and res_c.tobytes() == counts.tobytes(), mode
        near = engine.ray_nearest(o, d)
        assert engine.fetch("ray.near", _lib.RAY_HIT_DTYPE, near.shape).tobytes() == near.tobytes(), mode
        first = engine.ray_cast(o, d, cap=1)[0][..., 0]
        assert near.tobytes() == np.ascontiguousarray(first).tobytes() == np.ascontiguousarray(hits[..., 0]).tobytes(), mode
        out[mode] = (hits, counts, near)
    engine.query_accel = "off"
    (h0, c0, n0), (h1, c1, n1) = out["off"], out["bvh"]
    bad = np.argwhere(c0 != c1)
    assert len(bad) == 0, bad[:8]
    assert c0.tobytes() == c1.tobytes() and h0.tobytes() == h1.tobytes() and n0.tobytes() == n1.tobytes()
    miss = c0 == 0
    assert np.all(n0["face"][miss] == -1) and not n0["t"][miss].any() and not n0["point"][miss].any() and np.all(n0["face"][~miss] >= 0)
    return h0, c0, n0


def test_tetrahedron(accel):
    """the five rays of tests/test_gpu_rays.py test_tetrahedron: interior, vertex (three faces at one t), edge, miss, starting on a face"""
    engine = accel
    v, f = f32(O.TETRA)
    o = np.array([(1.0, 1.0, -2.0), (1.0, 1.0, 6.0), (2.0, -1.0, -1.0), (9.0, 9.0, -2.0), (1.0, 1.0, 0.0)])
    d = np.array([(0.0, 0.0, 1.0), (-1.0, -1.0, -2.0), (0.0, 1.0, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0)])
    engine.upload([(v, f)])
    hits, counts, near = both(engine, o, d, 8)
    assert list(counts[0]) == [2, 3, 3, 0, 1] and list(near[0]["face"]) == [0, 1, 0, -1, 3] and list(near[0]["t"]) == [2.0, 1.0, 1.0, 0.0, 2.0]


@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
def test_prism_across_chunk_edges(accel, R):
    """520 faces; R about the 64 rays of a tree chunk and the 256 of a brute one"""
    engine = accel
    v, f = prism130()
    rng = np.random.default_rng(R)
    o, d = frame_rays(T_TILT, rng.uniform(-6.0, 6.0, size=(R, 3)), rng.normal(size=(R, 3)))
    engine.upload([(v, f)])
    hits, counts, near = both(engine, o, d, 4)
    want, wn = O.cast(v, f, o, d, 4)
    assert np.array_equal(counts[0], wn) and np.array_equal(hits[0]["face"], want["face"]) and np.abs(hits[0]["t"] - want["t"]).max() <= MM


@pytest.mark.parametrize("cap", [1, 8])
def test_tube_on_a_diameter(accel, cap):
    """in, out, in, out: count 4 above cap 1 -- the prefix rule"""
    engine = accel
    v, f = tube24()
    o, d = frame_rays(T_TILT, [(-20.0, 0.3, 0.2), (0.0, 0.0, 0.0), (0.0, 0.0, 30.0)], [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
    engine.upload([(v, f)])
    hits, counts, near = both(engine, o, d, cap)
    assert list(counts[0]) == [4, 2, 0] and list(hits[0]["side"][0, :min(cap, 4)]) == [1, -1, 1, -1][:cap]


@pytest.mark.parametrize("per", [False, True])
def test_a_ragged_batch(accel, per):
    """tetrahedron, prism and humerus_left in one batch, with shared and with per-humerus rays"""
    engine = accel
    meshes = [f32(O.TETRA), prism130(), bone("humerus_left")]
    R = 70
    rays = [RT.random_rays(m[0], R, 20 + b) for b, m in enumerate(meshes)]
    o, d = (np.stack([r[k] for r in rays]) for k in (0, 1))
    if not per:
        o, d = np.concatenate([o[0, :20], o[1, :20], o[2, :30]]), np.concatenate([d[0, :20], d[1, :20], d[2, :30]])
    engine.upload(meshes)
    hits, counts, near = both(engine, o, d, 6)
    assert hits.shape == (3, R, 6) and all(counts[b].max() >= 1 for b in range(3))


@pytest.mark.parametrize("name", ["humerus_left", "proximal_left_cut"])
def test_bones_with_the_adversarial_rays(accel, name):
    """512 rays: the adversarial set of tests/raytree_oracle.py (vertices, edges, zero components, node box planes, grazing, long and
    short d, far origins, origins on faces) and random ones; proximal_left_cut has 61 loose faces"""
    engine = accel
    v, f = bone(name)
    engine.upload([(v, f)])
    engine.build_bvh()
    o, d, names = RT.rays_for(v, f, engine.bvh()[0], 512, seed=3)
    assert len(o) == 512 and names.count("random") == 512 - RT.N_ADVERSARIAL
    hits, counts, near = both(engine, o, d, 8)
    print(name, "rays with a hit", int((counts > 0).sum()), "most hits", int(counts.max()))
    assert (counts > 0).sum() > 100


def test_two_million_triangles(accel):
    """humerus_left subdivided three times (2 076 160 triangles, 9 408 loose), 256 rays, once"""
    from test_gpu_highres import subdivide
    engine = accel
    v, f = bone("humerus_left")
    v3, f3 = subdivide(*subdivide(*subdivide(v, f)))
    assert len(f3) == 2076160
    o, d = RT.random_rays(v3, 256, 5)
    try:
        engine.upload([(v3, f3)])
        hits, counts, near = both(engine, o, d, 8)
        assert (counts > 0).sum() > 20
    finally:
        engine.upload([(v, f)])                                                       # (the session's engine goes back to a small batch)


def test_refusals_of_ray_nearest(accel):
    """no context, no batch, a run in flight, R = 0, R above SH_RAY_MAX, a NaN, a zero direction: the codes of sh_ray_cast"""
    engine = accel
    o, d = np.zeros((2, 3)), np.array([(0.0, 0.0, 1.0), (1.0, 0.0, 0.0)])

    def refused(e, code, word, **kw):
        for fn in (e.ray_nearest, lambda **k: e.ray_cast(cap=1, **k)):
            with pytest.raises(ShoulderHipError) as ex:
                fn(**dict(dict(origins=o, directions=d), **kw))
            assert ex.value.code == code and word in str(ex.value), str(ex.value)
    rays = np.zeros(2, dtype=_lib.RAY_DTYPE)
    rays["dir"] = d
    assert engine.L.sh_ray_nearest(None, rays.ctypes.data, 2, 0, None) == -1 == engine.L.sh_ray_cast(None, rays.ctypes.data, 2, 0, 1, None, None)
    fresh = Engine(0)
    try:
        refused(fresh, -3, "no meshes")
    finally:
        fresh.close()
    v, f = bone("humerus_left")
    engine.reset_params()
    for mode in ("off", "bvh"):
        engine.upload([(v, f)])
        engine.query_accel = mode
        assert engine.ray_nearest(o, d).shape == (1, 2)
        refused(engine, -1, "R", origins=np.zeros((0, 3)), directions=np.zeros((0, 3)))
        big = np.zeros((_lib.RAY_MAX + 1, 3))
        refused(engine, -1, "R", origins=big, directions=big + (0.0, 0.0, 1.0))
        bad = d.copy()
        bad[1, 2] = np.nan
        refused(engine, -1, "ray 1", directions=bad)
        bad[1] = 0.0
        refused(engine, -1, "ray 1", directions=bad)
        engine.submit(_lib.STAGE_ALL, fetch=False)
        try:
            refused(engine, -3, "in flight")
        finally:
            engine.collect()


# ---- thickness ----------------------------------------------------------------------------------------------------------------------------
def face_points(v, f, faces):
    v64 = O.widen(v)
    A, B, C = v64[f[faces, 0]], v64[f[faces, 1]], v64[f[faces, 2]]
    return (A + B + C) / 3.0, np.cross(B - A, C - A)


def test_thickness_against_the_oracle_and_on_the_tube(accel):
    """Engine.thickness against raytree_oracle.thickness on the tube and the prism, switch off and on.  On the tube's outer wall (the
    centroids of its 48 outer side faces, normals outward) a ray is perpendicular to a side of the outer 24-gon (circumradius 7), at a
    lateral offset |s| <= 7 sin(pi/24) from the axis, and starts at the depth 7 cos(pi/24) along its own direction.  It ends on the
    inner 24-gon (circumradius 4), at a point whose distance r from the axis lies in [4 cos(pi/24), 4] and whose depth is
    sqrt(r^2 - s^2).  So the thickness lies in [7 cos(pi/24) - 4, 7 cos(pi/24) - sqrt(16 cos^2(pi/24) - 49 sin^2(pi/24))] =
    [2.940, 3.081] mm.  (The two polygons share their phase and a centroid lies a sixth of a side from the middle, so the value is
    in fact the distance of two parallel sides, 3 cos(pi/24) = 2.974.)"""
    engine = accel
    v, f = tube24()
    p, n = face_points(v, f, np.arange(48))
    engine.upload([(v, f), prism130()])
    pv, pf = prism130()
    pp, pn = face_points(pv, pf, np.arange(0, 520, 7))
    P, N = np.stack([np.concatenate([p, p[:27]]), pp]), np.stack([np.concatenate([n, n[:27]]), pn])
    got = {}
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        got[mode] = engine.thickness(P, N)
    assert got["off"].dtype == THICKNESS_DTYPE and got["off"].shape == (2, 75) and got["off"].tobytes() == got["bvh"].tobytes()
    for b, (mv, mf) in enumerate([(v, f), (pv, pf)]):
        th, pt, face = RT.thickness(mv, mf, P[b], N[b])
        assert np.array_equal(got["off"][b]["face"], face) and np.abs(got["off"][b]["thickness"] - th).max() <= MM and np.abs(got["off"][b]["point"] - pt).max() <= MM
    th = got["off"][0]["thickness"][:48]
    c24, s24 = np.cos(np.pi / 24), np.sin(np.pi / 24)
    lo, hi = 7.0 * c24 - 4.0, 7.0 * c24 - np.sqrt(16.0 * c24 * c24 - 49.0 * s24 * s24)
    print("tube wall", th.min(), th.max(), "bracket", lo, hi)
    assert np.all(th >= lo - MM) and np.all(th <= hi + MM) and np.all(got["off"][0]["face"][:48] >= 48)
    assert np.all(got["off"][1]["thickness"] > 0.0) and np.all(np.isfinite(got["off"][1]["thickness"]))
    shared = engine.thickness(p, n, offset=0.01)                                       # (N, 3) for all humeri, another offset
    assert shared.shape == (2, 48) and np.abs(shared[0]["thickness"] - th).max() <= MM
    with pytest.raises(ValueError):
        engine.thickness(p, np.zeros_like(n))
    with pytest.raises(ValueError):
        engine.thickness(p, np.where(np.arange(48)[:, None] == 3, np.nan, n))
    with pytest.raises(ValueError):
        engine.thickness(p, n[:5])


def test_a_ray_that_leaves_an_open_mesh(accel):
    """a flat sheet: nothing lies under it -- inf and face -1, with the switch off and on"""
    engine = accel
    v, f = sheet()
    p, n = face_points(v, f, np.arange(0, len(f), 5))
    engine.upload([(v, f)])
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        for sign in (1.0, -1.0):
            t = engine.thickness(p, sign * n)
            assert np.all(np.isinf(t["thickness"])) and np.all(t["thickness"] > 0) and np.all(t["face"] == -1) and not t["point"].any()


def test_the_facade(accel):
    """Humerus.thickness(sample=256) is finite and positive everywhere and the same bytes with accel="bvh" and without; with points it
    snaps them first; ray_first is the first location per ray of ray_hits"""
    engine = accel
    engine.reset_params()
    hum = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
    th, opp, face = hum.thickness(sample=256)
    th2, opp2, face2 = hum.thickness(sample=256, accel="bvh")
    assert engine.query_accel == "off"
    assert th.shape == (256,) and opp.shape == (256, 3) and face.shape == (256,)
    assert th.tobytes() == th2.tobytes() and opp.tobytes() == opp2.tobytes() and face.tobytes() == face2.tobytes()
    assert np.all(np.isfinite(th)) and np.all(th > 0.0) and np.all(face >= 0)
    print("humerus_left thickness: min", th.min(), "median", np.median(th), "max", th.max())
    pts, pf = hum.sample_surface(40, seed=3)
    ta, oa, fa = hum.thickness(points=pts + 0.01)
    tb, ob, fb = hum.thickness(points=pts + 0.01, accel="bvh")
    assert ta.tobytes() == tb.tobytes() and oa.tobytes() == ob.tobytes() and fa.tobytes() == fb.tobytes() and np.all(np.isfinite(ta))
    v, f = bone("humerus_left")
    want = RT.thickness(v, f, pts, face_points(v, f, pf)[1])
    tc, oc, fc = hum.thickness(points=pts)                                              # a sample snaps to itself, up to its rounding
    same = fc == want[2]
    assert same.mean() > 0.9 and np.abs(tc[same] - want[0][same]).max() <= 1e-3
    with pytest.raises(ValueError):
        hum.thickness()
    with pytest.raises(ValueError):
        hum.thickness(points=pts, sample=4)
    # ray_first against ray_hits
    c = v.astype(np.float64).mean(axis=0)
    d = np.random.default_rng(2).normal(size=(50, 3))
    o = np.concatenate([np.broadcast_to(c, (40, 3)), c - 500.0 * d[40:] / np.linalg.norm(d[40:], axis=1, keepdims=True)])      # from inside: one hit; from 500 mm outside through the middle: in and out
    for acc in (None, "bvh"):
        loc, ir, it = hum.ray_hits(o, d, accel=acc)
        l1, r1, t1 = hum.ray_first(o, d, accel=acc)
        firsts = np.concatenate([[True], ir[1:] != ir[:-1]])
        assert np.array_equal(r1, ir[firsts]) and np.array_equal(t1, it[firsts]) and l1.tobytes() == np.ascontiguousarray(loc[firsts]).tobytes()
        assert len(r1) >= 40 and len(loc) > len(l1)


def test_an_inward_wound_mesh(accel):
    """the thickness follows the winding: the prism with every face reversed has its normals inside, the rays leave it"""
    engine = accel
    v, f = prism130()
    r = np.ascontiguousarray(f[:, ::-1])
    p, n = face_points(v, r, np.arange(0, 520, 5))
    engine.upload([(v, r)])
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        t = engine.thickness(p, n)
        assert np.all(np.isinf(t["thickness"])) and np.all(t["face"] == -1)
