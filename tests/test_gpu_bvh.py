"""The face hierarchy of the resident batch (include/shoulder_hip.h sh_mesh_bvh, sh_set_query_accel; k_bvh.h) on the engine.

Bounds: none.  The index is compared as bytes with the NumPy statement of tests/bvh_oracle.py.  Every result with the switch on is
compared as bytes (`tobytes()`) with the same call with the switch off -- the brute-force walk of k_closest.h, which
tests/test_gpu_closest.py holds to the oracle --: no point is left out and no tolerance applies."""
import os

import numpy as np
import pytest

import bvh_oracle as B
import closest_oracle as O
import shoulder_amd as shoulder
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl
from test_bvh_host import bone, f32, prism130

pytestmark = pytest.mark.gpu
L_, W_ = B.LEAF, B.WIDTH
NAMES = ["humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped", "proximal_left_cut"]


@pytest.fixture(autouse=True)
def switch_off_afterwards(engine):
    yield
    engine.query_accel = "off"


def ragged():
    return [f32(O.TETRA), prism130(L_ * W_ + 1), bone("humerus_left")]


def both_modes(engine, pts):
    """closest_points with the switch off and on -> the records of the brute walk; the two calls and their "cp.out" are equal bytes"""
    engine.query_accel = "off"
    want = engine.closest_points(pts)
    want_out = engine.fetch("cp.out", _lib.CLOSEST_DTYPE, want.shape)
    engine.query_accel = "bvh"
    got = engine.closest_points(pts)
    got_out = engine.fetch("cp.out", _lib.CLOSEST_DTYPE, got.shape)
    engine.query_accel = "off"
    bad = np.argwhere((got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))).any(axis=-1))
    assert got.tobytes() == want.tobytes(), (len(bad), bad[:4], [(got[tuple(i)], want[tuple(i)]) for i in bad[:2]])
    assert got_out.tobytes() == want_out.tobytes() == want.tobytes()
    return want


def test_index_is_the_oracles_bytes_whatever_the_batch_order(engine):
    """a ragged batch (tetrahedron, prism of L W + 1 faces, humerus_left) and the same meshes in another order: order, loose list,
    offsets, boxes and corners of every mesh are the oracle's; only a mesh's first node depends on what stands before it"""
    meshes = ragged()
    seen = {}
    for perm in ([0, 1, 2], [2, 0, 1]):
        batch = [meshes[i] for i in perm]
        engine.upload(batch)
        info = engine.build_bvh()
        assert info.dtype == _lib.BVH_INFO_DTYPE and info.shape == (3,)
        got = engine.bvh()
        base = B.bases([len(m[1]) for m in batch])
        for b, i in enumerate(perm):
            want = B.build(*batch[b], base=base[b])
            assert B.same_index(got[b], want) is None, (perm, b, B.same_index(got[b], want))
            assert info[b].tobytes() == want["info"].tobytes()
            if i in seen:
                for k in ("order", "loose", "box", "tri"):
                    assert got[b][k].tobytes() == seen[i][k].tobytes(), k
                assert np.array_equal(np.delete(got[b]["off"], 5), np.delete(seen[i]["off"], 5))
            seen[i] = got[b]
        assert engine.fetch("bvh.info", _lib.BVH_INFO_DTYPE, (3,)).tobytes() == info.tobytes()
        F = sum(len(m[1]) for m in batch)
        order = engine.fetch("bvh.order", np.int32, (F,))
        assert (order == -1).sum() == int(info["loose"].sum())                          # the tails behind the tight faces
    assert [int(x) for x in seen[2]["off"][:2]] == [32431, 9] and seen[0]["off"][3] == 1 and seen[1]["off"][3] == 3


@pytest.mark.parametrize("name", NAMES)
def test_walk_bytes_one_bone(engine, name):
    """B = 1: the point classes of the host test (vertices, edge midpoints, inside, up to 50 mm outside, 2e4 mm away, 1e200) and every Q
    at a wave's edge"""
    v, f = bone(name)
    pts = B.point_classes(v, f, seed=21)
    engine.upload([(v, f)])
    want = both_modes(engine, pts)
    assert want.shape == (1, 512) and want["status"][0, -1] == B.GEOMETRY and not want["status"][0, :-1].any()
    shuffled = pts[np.random.default_rng(1).permutation(511)]
    for Q in (1, 63, 64, 65, 256, 257):
        both_modes(engine, shuffled[:Q])
    if name == "proximal_left_cut":
        assert int(engine.build_bvh()["loose"][0]) == 61


def test_walk_bytes_ragged_batch(engine):
    """B = 3, shared and per-humerus points, every Q"""
    meshes = ragged()
    engine.upload(meshes)
    per = np.stack([B.point_classes(v, f, seed=30 + b) for b, (v, f) in enumerate(meshes)])
    want = both_modes(engine, per)
    assert want.shape == (3, 512)
    both_modes(engine, per[2])                                                           # shared: the humerus' points against all three
    perm = np.random.default_rng(2).permutation(511)
    for Q in (1, 63, 64, 65, 256, 257):
        both_modes(engine, np.ascontiguousarray(per[:, perm[:Q]]))
        both_modes(engine, np.ascontiguousarray(per[1, perm[:Q]]))
    check = O.closest(*meshes[1], per[1])                                               # and the small one against the oracle without a tree
    assert want[1].tobytes() == check.tobytes()


def moved_points(v, n, seed):
    """n vertices of a bone turned 3 degrees about (1, 2, 3) through their centroid and shifted 2 mm"""
    rng = np.random.default_rng(seed)
    p = v[rng.choice(len(v), n, replace=False)].astype(np.float64)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(3.0)
    R = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    c = p.mean(axis=0)
    return (p - c) @ R.T + c + 2.0 * np.array([2.0, -1.0, 2.0]) / 3.0


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_registration_is_the_same_bytes(engine, metric):
    """sh_register_points, 6 iterations, 512 points of humerus_right moved 3 degrees and 2 mm: "icp.out" and "icp.near" with the switch
    on and off"""
    v, f = bone("humerus_right")
    pts = moved_points(v, 512, 7)
    engine.upload([(v, f)])
    res = {}
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        rec, hist = engine.register(pts, metric=metric, max_iter=6, history=True)
        res[mode] = (rec.tobytes(), hist.tobytes(), engine.fetch("icp.out", np.uint8).tobytes(), engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (1, 512)).tobytes())
        assert rec["status"][0] == 0 and rec["rms"][0] < rec["rms_first"][0]
    assert res["off"] == res["bvh"]


def test_multistart_is_the_same_bytes(engine):
    """register_multistart with 4 starts (the identity and three turns about the long axis)"""
    v, f = bone("humerus_right")
    pts = moved_points(v, 512, 8)
    c = pts.mean(axis=0)
    starts = []
    for deg in (0.0, 5.0, -5.0, 180.0):
        th = np.radians(deg)
        T = np.eye(4)
        T[:3, :3] = [[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]]
        T[:3, 3] = c - T[:3, :3] @ c
        starts.append(T)
    T0s = np.array(starts)[None]
    engine.upload([(v, f)])
    res = {}
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        out, cand, winner = engine.register_multistart(pts, T0s, coarse=dict(metric="plane", max_iter=3), coarse_points=128, min_pairs=64, fine=dict(metric="plane", max_iter=6))
        res[mode] = (out.tobytes(), cand.tobytes(), winner.tobytes(), engine.fetch("icp.out", np.uint8).tobytes(), engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (1, 512)).tobytes())
        assert out["status"][0] == 0 and winner[0] >= 0
    assert res["off"] == res["bvh"]


def test_state_and_arguments(engine):
    fresh = Engine(0)
    try:
        assert fresh.query_accel == "off"                                               # the default
        with pytest.raises(ShoulderHipError) as ex:
            fresh.build_bvh()                                                           # before an upload
        assert ex.value.code == B.STATE and "no meshes" in str(ex.value)
        assert fresh.L.sh_set_query_accel(fresh.h, 2) == B.ARG and fresh.L.sh_set_query_accel(fresh.h, -1) == B.ARG and fresh.query_accel == "off"
        assert fresh.L.sh_set_query_accel(None, 1) == B.ARG and fresh.L.sh_mesh_bvh(None, None) == B.ARG and fresh.L.sh_get_query_accel(None) == 0
        with pytest.raises(ValueError):
            fresh.query_accel = "fast"
    finally:
        fresh.close()
    v, f = bone("humerus_left")
    engine.reset_params()
    engine.upload([(v, f)])
    with pytest.raises(ShoulderHipError):
        engine.fetch("bvh.order", np.uint8)                                             # nothing is built by an upload
    pts = B.point_classes(v, f, n_each=20, far=1, seed=5)
    want = engine.closest_points(pts)
    with pytest.raises(ShoulderHipError):
        engine.fetch("bvh.order", np.uint8)                                             # ... nor by a query with the switch off
    # "cp.out", "topo.*" and a run's records keep their bytes across sh_mesh_bvh
    lm = engine.run(_lib.STAGE_ALL)
    engine.topology()
    names = ("landmarks", "cp.out", "topo.vrow", "topo.vface", "topo.adj", "topo.label", "topo.info", "verts", "faces", "verts_obb")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    info = engine.build_bvh()
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before
    assert (int(info["tight"][0]), int(info["loose"][0])) == (32431, 9)
    assert engine.build_bvh().tobytes() == info.tobytes()                               # built again: the same record
    # with a run in flight
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            engine.build_bvh()
        assert ex.value.code == B.STATE and "in flight" in str(ex.value)
    finally:
        engine.collect()
    # a new batch removes "bvh.*"; in BVH mode the first query rebuilds the index and still matches
    engine.query_accel = "bvh"
    assert engine.closest_points(pts).tobytes() == want.tobytes()
    engine.store("verts", engine.fetch("verts", np.float32))
    for n in ("bvh.order", "bvh.loose", "bvh.off", "bvh.box", "bvh.tri", "bvh.info"):
        with pytest.raises(ShoulderHipError):
            engine.fetch(n, np.uint8)
    assert engine.closest_points(pts).tobytes() == want.tobytes()
    assert engine.fetch("bvh.off", np.int32, (1, 32))[0, 0] == 32431
    v2, f2 = bone("humerus_right")
    engine.upload([(v2, f2)])
    with pytest.raises(ShoulderHipError):
        engine.fetch("bvh.order", np.uint8)
    assert engine.query_accel == "bvh"                                                  # the switch is the context's, not the batch's
    got = engine.closest_points(pts)
    assert engine.fetch("bvh.off", np.int32, (1, 32))[0, 0] == len(f2)
    engine.query_accel = "off"
    assert engine.closest_points(pts).tobytes() == got.tobytes()
    assert lm.shape == (1,)


def test_facade(engine):
    """Humerus.closest_point / surface_distance / signed_distance / register with accel="bvh": the same answers, and the engine's
    switch is what it was afterwards"""
    engine.reset_params()
    try:
        hum = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        mv = np.asarray(hum.mesh.vertices, np.float64)
        pts = mv[np.random.default_rng(4).choice(len(mv), 700, replace=False)] + (0.25, -0.5, 1.0)
        a, b = hum.closest_point(pts), hum.closest_point(pts, accel="bvh")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and engine.query_accel == "off"
        assert hum.surface_distance(pts) == hum.surface_distance(pts, accel="bvh")
        assert hum.signed_distance(pts[:100]).tobytes() == hum.signed_distance(pts[:100], accel="bvh").tobytes()
        M0, i0 = hum.register(pts, max_iter=4)
        M1, i1 = hum.register(pts, max_iter=4, accel="bvh")
        assert M0.tobytes() == M1.tobytes() and i0 == i1 and engine.query_accel == "off"
        engine.query_accel = "bvh"
        hum.closest_point(pts[:10], accel="off")
        assert engine.query_accel == "bvh"
        with pytest.raises(ValueError):
            hum.closest_point(pts[:10], accel="fast")
    finally:
        engine.query_accel = "off"
        engine.reset_params()


def test_two_million_triangles(engine):
    """the 2 076 160-triangle humerus of tests/test_gpu_highres.py, 256 points on and about it: the deepest tree in practice (eleven
    levels at LEAF = WIDTH = 4), the same bytes as the brute call"""
    from test_gpu_highres import subdivide
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    v3, f3 = subdivide(*subdivide(*subdivide(v, f)))
    assert len(f3) >= 2_000_000
    rng = np.random.default_rng(12)
    v64 = v3.astype(np.float64)
    fe = f3[rng.integers(0, len(f3), 64)]
    d = rng.normal(size=(96, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    c = v64.mean(axis=0)
    pts = np.concatenate([v64[rng.integers(0, len(v64), 64)], 0.5 * (v64[fe[:, 0]] + v64[fe[:, 1]]),
                          c + (v64[rng.integers(0, len(v64), 32)] - c) * rng.uniform(0.0, 0.9, size=(32, 1)),
                          v64[rng.integers(0, len(v64), 96)] + d * rng.uniform(0.0, 50.0, size=(96, 1))])
    assert pts.shape == (256, 3)
    try:
        engine.upload([(v3, f3)])
        want = both_modes(engine, pts)
        info = engine.fetch("bvh.info", _lib.BVH_INFO_DTYPE, (1,))[0]
        print("2.08 M triangles: tight", int(info["tight"]), "loose", int(info["loose"]), "levels", int(info["levels"]), "nodes", int(info["nodes"]))
        assert int(info["tight"]) + int(info["loose"]) == len(f3) and int(info["levels"]) == B.levels_of(int(info["tight"]))
        assert not want["status"].any() and want["dist"][0, :128].max() <= 1e-4          # on vertices and on edges
    finally:
        engine.upload([(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))])      # (the session's engine goes back to a small batch)
