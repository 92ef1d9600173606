"""Closest surface points of the resident batch (include/shoulder_hip.h sh_closest_points, k_closest.h) on the engine against the NumPy
statement of tests/closest_oracle.py: every point against every face, NO cull, the winner by np.lexsort((face, d2)).

Bounds.  Against the oracle: face, region, side and status equal, dist and point within 1e-9 mm (the same operations in the same
order: the largest difference is printed and 0.0 is expected).  Between runs, batches, point lists and face splits: bytes.  The small
shapes have integer or float32 coordinates, which the upload keeps exactly."""
import os

import numpy as np
import pytest

import closest_oracle as O
import stem_oracle as SO
import shoulder_amd as shoulder
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
TOL = 1e-9
T_TILT = SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75))                                 # CT -> frame, tilted and translated
NAMES = ["humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped"]
FAR = 1e200                                                                           # mm: a squared distance from here overflows


def f32(vf):
    return np.ascontiguousarray(vf[0], np.float32), np.ascontiguousarray(vf[1], np.int32)


def check(got, v, f, pts, want=None):
    """one humerus' records (Q,) against the oracle -> (the oracle's records, the largest difference)"""
    want = O.closest(v, f, pts) if want is None else want
    for k in ("face", "region", "side", "status"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k])[0][:8], got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])
    worst = max(float(np.abs(got["dist"] - want["dist"]).max()), float(np.abs(got["point"] - want["point"]).max()))
    assert worst <= TOL, worst
    return want, worst


def prism130():
    return f32(SO.mesh_in_ct(T_TILT, *SO.prism(130, 5.0, -2.5, 2.5, 0.011)))


@pytest.fixture(scope="module")
def humerus_mesh():
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def test_tetrahedron(engine):
    """1: below a face (its interior), beside an edge (two faces tie: the smaller id, its edge CA), behind a vertex (three tie), inside
    the solid, exactly on a face, and in front of the slanted face"""
    v, f = f32(O.TETRA)
    pts = np.array([(1.0, 1.0, -2.0), (2.0, -3.0, -4.0), (-2.0, -2.0, -1.0), (0.5, 0.5, 0.25), (1.0, 1.0, 0.0), (4.0, 4.0, 4.0)])
    engine.upload([(v, f)])
    got = engine.closest_points(pts)
    assert got.shape == (1, 6) and got.dtype == _lib.CLOSEST_DTYPE
    want, worst = check(got[0], v, f, pts)
    print("tetrahedron: max |gpu - oracle|", worst)
    g = got[0]
    assert list(g["dist"][:5]) == [2.0, 5.0, 3.0, 0.25, 0.0] and list(g["face"]) == [0, 0, 0, 0, 0, 3]
    assert list(g["region"]) == [0, 3, 4, 0, 0, 0] and list(g["side"]) == [1, 1, 1, -1, 1, 1] and not g["status"].any()
    assert np.array_equal(g["point"][:5], [(1.0, 1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.0), (1.0, 1.0, 0.0)])
    assert g.tobytes() == want.tobytes()
    assert engine.fetch("cp.out", _lib.CLOSEST_DTYPE, (1, 6)).tobytes() == got.tobytes()


@pytest.mark.parametrize("F", [255, 256, 257, 513])
def test_prism_across_tile_and_chunk_edges(engine, F):
    """2: the first F faces of the tilted 130-gon prism (one tile less a face, one tile, one tile and a face, two and a face); the first
    Q of 257 points about it for every Q at a wave's and a chunk's edge"""
    v, f = prism130()
    f = np.ascontiguousarray(f[:F])
    rng = np.random.default_rng(F)
    pts = SO.to_ct(T_TILT, rng.uniform(-7.0, 7.0, size=(257, 3)))
    pts[:16] = v[f[rng.integers(0, F, 16), rng.integers(0, 3, 16)]].astype(np.float64)      # on vertices: ties
    want = O.closest(v, f, pts)
    engine.upload([(v, f)])
    worst = 0.0
    for Q in (1, 63, 64, 65, 255, 256, 257):
        got = engine.closest_points(pts[:Q])
        assert got.shape == (1, Q)
        worst = max(worst, check(got[0], v, f, pts[:Q], want[:Q])[1])
    print("prism F =", F, "max |gpu - oracle|", worst, "regions", sorted(set(want["region"])))
    assert 0 in set(want["region"]) and set(want["region"]) & {1, 2, 3} and set(want["region"]) & {4, 5, 6}


def test_ties_go_to_the_smallest_face_id(engine):
    """3: one face stored twice under different ids (2 and 9, with eight others between), and a fan of eight faces round one vertex;
    queries exactly at the fan's vertex, above it, on a shared edge and above one, and over the twin faces"""
    ring = [(np.cos(k * np.pi / 4.0), np.sin(k * np.pi / 4.0), 0.0) for k in range(8)]
    v = np.array([(0.0, 0.0, 0.5)] + ring + [(10.0, 0.0, 0.0), (11.0, 0.0, 0.0), (10.0, 1.0, 0.0)], dtype=np.float32)
    fan = [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)]
    twin = (9, 10, 11)
    f = np.array(fan[:2] + [twin] + fan[2:] + [twin], dtype=np.int32)                   # ids: fan 0 1 . 3 4 5 6 7 8, twin 2 and 9
    edge_mid = 0.5 * (v[0].astype(np.float64) + v[4].astype(np.float64))                # on the edge apex - ring[3], shared by the fan faces 2 and 3: ids 3 and 4
    pts = np.array([v[0].astype(np.float64), (0.0, 0.0, 3.0), edge_mid, edge_mid + (0.0, 0.0, 0.25), (10.25, 0.25, 0.0), (10.25, 0.25, -2.0), (12.0, -1.0, 0.0),
                    v[5].astype(np.float64)])
    want = O.closest(v, f, pts)
    assert [O.ties(v, f, p) for p in pts[:2]] == [8, 8] and O.ties(v, f, pts[2]) == 2 and all(O.ties(v, f, p) == 2 for p in pts[4:7])
    engine.upload([(v, f)])
    got = engine.closest_points(pts)
    check(got[0], v, f, pts, want)
    assert list(got[0]["face"][:2]) == [0, 0] and got[0]["face"][2] == 3 and list(got[0]["face"][4:7]) == [2, 2, 2]
    assert list(got[0]["region"][:2]) == [4, 4] and got[0]["dist"][0] == 0.0 and got[0]["dist"][1] == 2.5 and got[0]["dist"][5] == 2.0
    assert got[0].tobytes() == want.tobytes()


def test_late_winner(engine):
    """4: two shells 400 mm apart in one mesh, the far one FIRST in face order; the queries sit beside the second, so the best shrinks
    only in the last tiles -- where a wrong cull bound or a wrong join of the splits shows.  Once alone (five tiles, five splits of one
    tile) and once as 512 copies (1 024 chunk-humerus pairs: one split walks all five tiles)"""
    v, f = prism130()
    shift = (SO.to_ct(T_TILT, [(400.0, 0.0, 0.0)]) - SO.to_ct(T_TILT, [(0.0, 0.0, 0.0)]))[0]
    v2 = (v.astype(np.float64) + shift).astype(np.float32)
    mv, mf = np.concatenate([v, v2]), np.concatenate([f, f + len(v)]).astype(np.int32)
    rng = np.random.default_rng(4)
    pts = v2[rng.integers(0, len(v2), 257)].astype(np.float64) + rng.normal(size=(257, 3)) * rng.choice([0.0, 0.01, 1.0, 8.0], size=(257, 1))
    pts[:8] = v.astype(np.float64)[:8] + (0.0, 0.0, 0.125)                              # and a few beside the first shell
    want = O.closest(mv, mf, pts)
    assert (want["face"][8:] >= len(f)).all() and (want["face"][:8] < len(f)).all()
    engine.upload([(mv, mf)])
    got = engine.closest_points(pts)
    _, worst = check(got[0], mv, mf, pts, want)
    engine.upload([(mv, mf)] * 512)
    many = engine.closest_points(pts)
    assert many.shape == (512, 257)
    for b in (0, 1, 255, 511):
        assert many[b].tobytes() == got[0].tobytes(), b
    assert np.all(many["face"] == got[0]["face"][None, :]) and np.all(many["dist"] == got[0]["dist"][None, :])
    print("late winner: max |gpu - oracle|", worst)


def mesh_points(v, Q, seed):
    """Q points about one mesh: half near its vertices (some exactly on them), half in its box blown up by a half"""
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    lo, hi = v64.min(axis=0), v64.max(axis=0)
    near = v64[rng.integers(0, len(v), Q // 2)] + rng.normal(size=(Q // 2, 3)) * rng.choice([0.0, 0.5, 3.0], size=(Q // 2, 1))
    box = 0.5 * (lo + hi) + rng.uniform(-1.0, 1.0, size=(Q - Q // 2, 3)) * (0.75 * (hi - lo) + 0.5)
    return np.concatenate([near, box])


def test_results_do_not_depend_on_the_batch_the_point_list_or_the_split(engine, humerus_mesh):
    """5: a ragged batch of the four fixture bones and the tetrahedron against every humerus alone, the batch permuted, shared against
    per-humerus points, a permuted and a shorter list, and one point asked alone (Q = 1: the faces in as many splits as fill the chip)
    against the same point inside Q = 300 (half as many) -- the sh_closest bytes are equal in all of these"""
    meshes = [f32(load_stl(os.path.join(BONES, n + ".stl"))) for n in NAMES] + [f32(O.TETRA)]
    Q = 65
    pts = np.stack([mesh_points(m[0], Q, 20 + b) for b, m in enumerate(meshes)])
    engine.upload(meshes)
    got = engine.closest_points(pts)
    assert got.shape == (5, Q) and not got["status"].any()
    assert engine.closest_points(pts).tobytes() == got.tobytes()
    check(got[4], meshes[4][0], meshes[4][1], pts[4])                                   # the small one against the oracle as well
    # shared points (the first humerus') against the same points handed over per humerus
    sh = engine.closest_points(pts[0])
    assert sh.tobytes() == engine.closest_points(np.broadcast_to(pts[0], pts.shape)).tobytes() and sh[0].tobytes() == got[0].tobytes()
    # a permuted list, a shorter one, one point alone, and that point inside a list of 300
    perm = np.random.default_rng(3).permutation(Q)
    assert engine.closest_points(np.ascontiguousarray(pts[:, perm])).tobytes() == np.ascontiguousarray(got[:, perm]).tobytes()
    assert engine.closest_points(np.ascontiguousarray(pts[:, 7:20])).tobytes() == np.ascontiguousarray(got[:, 7:20]).tobytes()
    one = engine.closest_points(np.ascontiguousarray(pts[:, 7:8]))
    assert one.tobytes() == np.ascontiguousarray(got[:, 7:8]).tobytes()
    long = np.concatenate([np.stack([mesh_points(m[0], 299, 40 + b) for b, m in enumerate(meshes)]), pts[:, 7:8]], axis=1)
    assert np.ascontiguousarray(engine.closest_points(long)[:, 299:]).tobytes() == one.tobytes()
    # the batch reversed, and every humerus alone
    engine.upload(meshes[::-1])
    assert np.ascontiguousarray(engine.closest_points(np.ascontiguousarray(pts[::-1]))[::-1]).tobytes() == got.tobytes()
    for b in range(5):
        engine.upload(meshes[b:b + 1])
        assert engine.closest_points(pts[b])[0].tobytes() == got[b].tobytes(), b


def test_humerus_left_160_points(engine, humerus_mesh):
    """6: 64 points 2 mm off random vertices, 32 exactly on vertices, 32 uniform in the box grown by 20 mm, 32 inside (a vertex moved
    3 mm against the normal of a face that holds it): against the oracle, and the distance against the independent formulation
    (plane projection with an inside test, else the nearest of the three edges) within 1e-9 mm.  The two formulations may choose
    another face among ties, so faces are compared with the operation-by-operation oracle only."""
    v, f = humerus_mesh
    v64 = O.widen(v)
    rng = np.random.default_rng(6)
    d = rng.normal(size=(64, 3))
    jit = v64[rng.integers(0, len(v), 64)] + 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    on = v64[rng.integers(0, len(v), 32)]
    lo, hi = v64.min(axis=0) - 20.0, v64.max(axis=0) + 20.0
    box = rng.uniform(lo, hi, size=(32, 3))
    fi = rng.integers(0, len(f), 32)
    n = np.cross(v64[f[fi, 1]] - v64[f[fi, 0]], v64[f[fi, 2]] - v64[f[fi, 0]])
    inside = v64[f[fi, 0]] - 3.0 * n / np.linalg.norm(n, axis=1, keepdims=True)
    pts = np.concatenate([jit, on, box, inside])
    engine.upload([(v, f)])
    got = engine.closest_points(pts)[0]
    want, worst = check(got, v, f, pts)
    tied = sum(O.ties(v, f, p) > 1 for p in pts)
    other = O.distance_independent(v, f, pts)
    print("humerus_left: max |gpu - oracle|", worst, "| points whose winning d2 is shared by several faces:", tied, "of 160 | max |dist - independent|",
          float(np.abs(got["dist"] - other).max()))
    assert np.abs(got["dist"] - other).max() <= TOL
    assert got["dist"][64:96].max() <= 1e-12 and np.all(got["region"][64:96] >= 4)      # on a vertex: distance zero, a vertex region
    assert np.all(got["dist"][:64] <= 2.0 + 1e-12) and np.all(got["dist"][128:] <= 3.0 + 1e-12)
    assert np.mean(got["side"][128:] == -1) > 0.5 and tied >= 32                        # inside: behind the winning face (its verdict: not a proof)


def test_a_humerus_without_a_finite_candidate(engine, humerus_mesh):
    """7: a humerus whose only faces are collinear triangles, between two proper neighbours.  Under the rule as written a collinear
    triangle is a segment with finite distances (its points end in a vertex or an edge branch, or in the interior branch with a quotient
    of rounding noise that is finite unless the three products cancel exactly: tests/test_closest_host.py), so near points are held to
    the oracle like any others.  Its status is reached where no face CAN give a finite d2: points 1e200 mm away, whose squared distance
    overflows -- status SH_ERR_GEOMETRY, face -1, zeros.  The neighbours in the batch are untouched."""
    line = (np.array([(0, 0, 0), (1, 0, 0), (3, 0, 0), (0, 1, 2), (0, 2, 4), (0, -3, -6), (1, 1, 1)], dtype=np.float32),
            np.array([(0, 1, 2), (3, 4, 5), (2, 0, 1), (6, 6, 6)], dtype=np.int32))      # three collinear faces and a point face
    tet, pr = f32(O.TETRA), prism130()
    near = np.array([(2.0, 1.0, 0.0), (0.25, 0.25, 1.0), (-1.0, 0.0, 0.0), (0.0, 1.5, 3.0)])
    far = np.array([(FAR, 0.0, 0.0), (FAR, -FAR, 1e180), (0.0, 0.0, -FAR), (-FAR, FAR, FAR)])
    pts = np.stack([near, far, near])
    engine.upload([tet, line, pr])
    got = engine.closest_points(pts)
    bad = got[1]
    assert np.all(bad["status"] == O.GEOMETRY) and np.all(bad["face"] == -1)
    assert not bad["dist"].any() and not bad["point"].any() and not bad["region"].any() and not bad["side"].any()
    assert bad.tobytes() == O.closest(*line, far).tobytes()
    check(got[0], *tet, near)
    check(got[2], *pr, near)
    for b, m in ((0, tet), (2, pr)):                                                   # ... what they give alone
        engine.upload([m])
        assert engine.closest_points(near)[0].tobytes() == got[b].tobytes()
    engine.upload([tet, line, pr])
    again = engine.closest_points(near)                                                # shared near points: the segment answers, the point face too
    want = check(again[1], *line, near)[0]
    assert not again["status"].any() and again[1].tobytes() == want.tobytes() and again[1]["dist"][0] == 1.0 and again[1]["dist"][3] == 0.0
    everyone = engine.closest_points(far)                                              # shared far points: every humerus has the status
    assert np.all(everyone["status"] == O.GEOMETRY) and np.all(everyone["face"] == -1) and not everyone["dist"].any()


def test_state_and_arguments(engine, humerus_mesh):
    """8"""
    pts = np.array([(0.0, 0.0, 0.0), (1.0, 2.0, 3.0)])

    def refused(e, code, word, **kw):
        with pytest.raises(ShoulderHipError) as ex:
            e.closest_points(**dict(dict(points=pts), **kw))
        assert ex.value.code == code and word in str(ex.value), str(ex.value)
    fresh = Engine(0)
    try:
        refused(fresh, -3, "no meshes")                                               # without a batch
    finally:
        fresh.close()
    v, f = humerus_mesh
    engine.reset_params()
    engine.upload([(v, f)])
    assert engine.closest_points(pts).shape == (1, 2)                                 # a batch is enough: no run
    refused(engine, -1, "Q", points=np.zeros((0, 3)))
    bad = pts.copy()
    bad[1, 2] = np.nan
    refused(engine, -1, "point 1", points=bad)
    bad[1, 2], bad[0, 0] = 3.0, -np.inf
    refused(engine, -1, "point 0", points=bad)
    with pytest.raises(ValueError):
        engine.closest_points(np.zeros((2, 2, 3)))                                    # (B, Q, 3) with another B
    # the records of a run and the buffers of the chain are the same bytes before and after, and the chain goes on
    lm = engine.run(_lib.STAGE_ALL).copy()
    rec, fit, seat = engine.resect(offsets=[dict(), dict(depth_canal_mm=-4.0)], fit=True, heads=[(24.0, 18.0), (22.0, 16.0)])
    engine.canal_profile(40.0, 4.0, 8, 16)
    stems = engine.resect_stems([(100.0, 6.0, 3.5)])
    c = v.astype(np.float64).mean(axis=0)
    hits, counts = engine.ray_cast(c[None] + np.zeros((3, 1)), np.eye(3), cap=4)
    names = ("landmarks", "resect.out", "resect.fit_out", "resect.seat_out", "stem.out", "canal.near", "canal.levels", "ray.hits", "ray.counts", "anp.ray_t", "verts_obb")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    got = engine.closest_points(v[:300].astype(np.float64) + (0.0, 0.0, 0.5))
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before
    assert not got["status"].any() and got["dist"].max() <= 0.5
    assert engine.resect_stems([(100.0, 6.0, 3.5)]).tobytes() == stems.tobytes()     # the chain's state is what it was
    plans, refs = engine.plan(4, dict(w_uncovered=10.0, w_overhang=1.0, w_height=0.25, w_eccentricity=2.0, w_fill=3.0, fill_target=0.5))
    assert plans.shape == (1, 4) and refs["status"][0] == 0
    assert engine.fetch("cp.out", _lib.CLOSEST_DTYPE, (1, 300)).tobytes() == got.tobytes()      # the results stay resident ...
    # with runs in flight
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        refused(engine, -3, "in flight")
    finally:
        engine.collect()
    assert engine.closest_points(v[:300].astype(np.float64) + (0.0, 0.0, 0.5)).tobytes() == got.tobytes()
    engine.store("verts", engine.fetch("verts", np.float32))                          # ... until the vertices are stored (even the same ones)
    with pytest.raises(ShoulderHipError):
        engine.fetch("cp.out", np.uint8)
    assert engine.closest_points(v[:300].astype(np.float64) + (0.0, 0.0, 0.5)).tobytes() == got.tobytes()
    engine.upload([f32(O.TETRA)])                                                      # ... or until the next upload: "cp.out" is gone
    with pytest.raises(ShoulderHipError):
        engine.fetch("cp.out", np.uint8)
    engine.closest_points(pts)
    assert engine.fetch("cp.out", _lib.CLOSEST_DTYPE, (1, 2))["face"].min() >= 0


def test_facade(engine, humerus_mesh):
    """9: Humerus.closest_point in the canal / transepicondylar system on the mesh's own vertices there (the vertices are resident as
    float32: 1e-4 mm; every returned triangle holds its vertex); surface_distance of the vertices lifted by 1 mm; and of a resected
    half against the intact bone -- everything the half shares with the bone lies on it, only a cap over the cut could lie off it"""
    engine.reset_params()
    try:
        hum = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        hum.apply_csys_canal_transepiconylar()
        mv, mf = np.asarray(hum.mesh.vertices, np.float64), np.asarray(hum.mesh.faces)
        ids = np.random.default_rng(9).choice(len(mv), 2000, replace=False)
        closest, dist, tri = hum.closest_point(mv[ids])
        assert closest.shape == (2000, 3) and dist.shape == (2000,) and tri.shape == (2000,)
        print("facade: max distance of the mesh's own vertices", dist.max())
        assert dist.max() <= 1e-4 and np.abs(closest - mv[ids]).max() <= 1e-4
        assert np.all((mf[tri] == ids[:, None]).any(axis=1))
        sd = hum.surface_distance(mv + [0.0, 0.0, 1.0])
        assert sd["n"] == len(mv) and 0.0 < sd["mean"] <= sd["rms"] <= sd["p95"] + 1e-12 <= sd["max"] + 1e-12 <= 1.0 + 1e-6 + 1e-12
        assert 0 <= sd["argmax"] < len(mv) and set(sd) == {"mean", "rms", "max", "p95", "n", "argmax"}
        ost = shoulder.HumeralHeadOsteotomy(hum)
        head, rest = ost.resect_mesh()
        cut = ost.plane
        for half in (head, rest):
            hv = np.asarray(half.vertices, np.float64)
            d = hum.closest_point(hv)[1]
            off_plane = np.abs((hv - cut.point) @ cut.normal) > 1e-3
            sd = hum.surface_distance(half)
            print("facade: half with", len(hv), "vertices: max", sd["max"], "max off the cut plane", d[off_plane].max())
            assert sd["max"] == d.max() and sd["argmax"] == int(np.argmax(d)) and off_plane.any() and (~off_plane).any()
            assert d[off_plane].max() <= 1e-4
            assert sd["max"] <= 1e-4 or not off_plane[sd["argmax"]]                     # the farthest point, if any is off the bone, lies on the cut plane
        assert hum.surface_distance(hum.mesh)["max"] <= 1e-4                            # an object with .vertices
        with pytest.raises(ValueError):
            hum.closest_point(np.zeros((0, 3)))
    finally:
        engine.reset_params()
