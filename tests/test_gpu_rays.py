"""Rays against the resident batch, every hit (include/shoulder_hip.h sh_ray_cast / sh_anp_axis_hits, k_rays.h) on the engine against
the NumPy statement of tests/ray_oracle.py (every ray against every face, np.lexsort on (face, t)).

Bounds.  Against NumPy: counts, faces and sides equal, t and point within 1e-6 mm, the project's bound.  Against the host twin and
between runs: bytes.  The small shapes have integer or float32 coordinates, which the upload keeps exactly."""
import os

import numpy as np
import pytest

import ray_oracle as O
import stem_oracle as SO
import shoulder_amd as shoulder
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
MM = 1e-6
T_TILT = SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75))                                 # CT -> frame, tilted and translated
NAMES = ["humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped"]
CHUNK = 256                                                                           # SH_RAY_CHUNK, the rays of one workgroup


def f32(vf):
    return np.ascontiguousarray(vf[0], np.float32), np.ascontiguousarray(vf[1], np.int32)


def frame_rays(T, origins, directions):
    """rays given in the frame of T -> CT"""
    return SO.to_ct(T, origins), np.asarray(directions, np.float64) @ T[:3, :3]


def check(hits, counts, v, f, o, d, skip=()):
    """one humerus' rows (R, cap) against the oracle"""
    cap = hits.shape[1]
    want, wn = O.cast(v, f, o, d, cap)
    for r in range(len(wn)):
        if r in skip:
            continue
        k = min(int(wn[r]), cap)
        assert counts[r] == wn[r], (r, counts[r], wn[r])
        assert np.array_equal(hits["face"][r], want["face"][r]) and np.array_equal(hits["side"][r], want["side"][r]), r
        assert np.abs(hits["t"][r] - want["t"][r]).max() <= MM and np.abs(hits["point"][r] - want["point"][r]).max() <= MM, r
        assert not hits["t"][r, k:].any() and not hits["point"][r, k:].any() and not hits["side"][r, k:].any() and np.all(hits["face"][r, k:] == -1)
        assert np.all(np.diff(hits["t"][r, :k]) >= 0)
    return want, wn


def prism130():
    return f32(SO.mesh_in_ct(T_TILT, *SO.prism(130, 5.0, -2.5, 2.5, 0.011)))


def tube24():
    return f32(SO.mesh_in_ct(T_TILT, *SO.tube(24, 4.0, 7.0, -5.0, 5.0, 0.05)))


@pytest.fixture(scope="module")
def humerus_mesh():
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def test_tetrahedron(engine):
    """1: through the interior (in, then out), through a vertex (three faces at one t, by face), through an edge (two faces at one t),
    missing, and starting on a face (its own face is not a hit)"""
    v, f = f32(O.TETRA)
    o = np.array([(1.0, 1.0, -2.0), (1.0, 1.0, 6.0), (2.0, -1.0, -1.0), (9.0, 9.0, -2.0), (1.0, 1.0, 0.0)])
    d = np.array([(0.0, 0.0, 1.0), (-1.0, -1.0, -2.0), (0.0, 1.0, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0)])
    engine.upload([(v, f)])
    hits, counts = engine.ray_cast(o, d, cap=8)
    assert hits.shape == (1, 5, 8) and counts.shape == (1, 5) and list(counts[0]) == [2, 3, 3, 0, 1]
    check(hits[0], counts[0], v, f, o, d)
    h = hits[0]
    assert list(h["t"][0, :2]) == [2.0, 4.0] and list(h["face"][0, :2]) == [0, 3] and list(h["side"][0, :2]) == [1, -1]
    assert np.array_equal(h["point"][0, :2], [(1.0, 1.0, 0.0), (1.0, 1.0, 2.0)])
    assert list(h["t"][1, :3]) == [1.0, 1.0, 1.0] and list(h["face"][1, :3]) == [1, 2, 3]
    assert list(h["t"][2, :3]) == [1.0, 1.0, 2.0] and list(h["face"][2, :3]) == [0, 1, 3] and list(h["side"][2, :3]) == [1, 1, -1]
    assert list(h["t"][4, :1]) == [2.0] and list(h["face"][4, :1]) == [3]
    assert engine.fetch("ray.hits", _lib.RAY_HIT_DTYPE, (1, 5, 8)).tobytes() == hits.tobytes()
    assert engine.fetch("ray.counts", np.int32, (1, 5)).tobytes() == counts.tobytes()


@pytest.mark.parametrize("R", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])      # (CHUNK + 1 = 257)
def test_prism_across_tile_and_chunk_edges(engine, R):
    """2: 520 faces, three tiles; rays from inside and outside the prism in every direction, the first two axial and radial"""
    v, f = prism130()
    rng = np.random.default_rng(R)
    o = rng.uniform(-6.0, 6.0, size=(R, 3))
    d = rng.normal(size=(R, 3))
    o[0], d[0] = (0.3, 0.2, -10.0), (0.0, 0.0, 1.0)
    if R > 1:
        o[1], d[1] = (-9.0, 0.1, 0.3), (1.0, 0.0, 0.0)
    o, d = frame_rays(T_TILT, o, d)
    engine.upload([(v, f)])
    hits, counts = engine.ray_cast(o, d, cap=4)
    check(hits[0], counts[0], v, f, o, d)
    assert counts[0, 0] == 2 and np.abs(hits[0]["t"][0, :2] - [7.5, 12.5]).max() <= MM and list(hits[0]["side"][0, :2]) == [1, -1]
    assert counts[0].max() == 2 and (R < 3 or (counts[0] == 1).any())                  # convex: in and out, or out from inside


def test_tube_on_a_diameter(engine):
    """2: from outside through both walls: in, out, in, out"""
    v, f = tube24()
    o, d = frame_rays(T_TILT, [(-20.0, 0.3, 0.2)], [(1.0, 0.0, 0.0)])
    engine.upload([(v, f)])
    hits, counts = engine.ray_cast(o, d, cap=8)
    check(hits[0], counts[0], v, f, o, d)
    assert counts[0, 0] == 4 and list(hits[0]["side"][0, :4]) == [1, -1, 1, -1]


def test_many_hits_and_caps(engine):
    """3: 40 plates; through the interiors 40 hits, along the shared diagonals 80 in 40 tied pairs (from below and from above); the
    counts are exact whatever cap, a smaller cap is a byte prefix of a larger one, the slots behind the count are zero with face -1"""
    v, f = f32(O.plates(40))
    o = np.array([(0.5, -0.25, 0.0), (0.0, 0.0, 0.0), (0.25, 0.25, 50.0), (3.0, 0.0, 0.0)])
    d = np.array([(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)])
    engine.upload([(v, f)])
    got = {cap: engine.ray_cast(o, d, cap=cap) for cap in (1, 8, 40, 64, 128)}
    for cap, (hits, counts) in got.items():
        assert list(counts[0]) == [40, 80, 80, 0], cap
        check(hits[0], counts[0], v, f, o, d)
        assert np.ascontiguousarray(got[128][0][0, :, :cap]).tobytes() == hits[0].tobytes(), cap
    h = got[128][0][0]
    assert np.array_equal(h["face"][0, :40], 2 * np.arange(40)) and np.array_equal(h["t"][0, :40], np.arange(1.0, 41.0))
    assert np.array_equal(h["face"][1, :80], np.arange(80)) and np.array_equal(h["t"][1, :80], np.repeat(np.arange(1.0, 41.0), 2))
    assert np.array_equal(h["face"][2, :80], (np.arange(80) ^ 1)[::-1]) and np.all(h["side"][2, :80] == 1) and np.all(h["side"][1, :80] == -1)
    grown = engine.ray_cast(o, d, cap=None)                                           # asks again with the largest count
    assert grown[0].shape == (1, 4, 80) and grown[0].tobytes() == np.ascontiguousarray(got[128][0][:, :, :80]).tobytes()


def mesh_rays(v, R, seed):
    """R rays about one mesh: origins within its box, blown up by a half, directions anywhere"""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    c, h = 0.5 * (lo + hi), 0.75 * (hi - lo) + 0.5
    return c + rng.uniform(-1.0, 1.0, size=(R, 3)) * h, rng.normal(size=(R, 3))


def test_results_do_not_depend_on_the_batch_the_ray_list_or_the_call(engine, humerus_mesh):
    """4: a ragged batch against each humerus alone; per-humerus rays against shared rays; a permuted ray list; the same call twice"""
    meshes = [f32(O.TETRA), prism130(), tube24(), f32(O.plates(40)), humerus_mesh]
    R = 65
    rays = [mesh_rays(m[0], R, 10 + b) for b, m in enumerate(meshes)]
    o, d = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
    engine.upload(meshes)
    hits, counts = engine.ray_cast(o, d, cap=8)
    assert all(counts[b].max() >= 1 for b in range(5))
    again = engine.ray_cast(o, d, cap=8)
    assert again[0].tobytes() == hits.tobytes() and again[1].tobytes() == counts.tobytes()
    for b in (0, 3):                                                                  # the small ones against the oracle as well
        check(hits[b], counts[b], meshes[b][0], meshes[b][1], o[b], d[b])
    # shared rays (the humerus') against the same rays handed over per humerus
    sh, sc = engine.ray_cast(o[4], d[4], cap=8)
    ph, pc = engine.ray_cast(np.broadcast_to(o[4], o.shape), np.broadcast_to(d[4], d.shape), cap=8)
    assert sh.tobytes() == ph.tobytes() and sc.tobytes() == pc.tobytes() and sh[4].tobytes() == hits[4].tobytes()
    # a permuted list, and a shorter one
    perm = np.random.default_rng(3).permutation(R)
    qh, qc = engine.ray_cast(np.ascontiguousarray(o[:, perm]), np.ascontiguousarray(d[:, perm]), cap=8)
    assert qh.tobytes() == np.ascontiguousarray(hits[:, perm]).tobytes() and qc.tobytes() == np.ascontiguousarray(counts[:, perm]).tobytes()
    th, tc = engine.ray_cast(np.ascontiguousarray(o[:, 7:8]), np.ascontiguousarray(d[:, 7:8]), cap=8)
    assert th.tobytes() == np.ascontiguousarray(hits[:, 7:8]).tobytes() and tc.tobytes() == np.ascontiguousarray(counts[:, 7:8]).tobytes()
    # the batch reversed, and every humerus alone
    engine.upload(meshes[::-1])
    rh, rc = engine.ray_cast(np.ascontiguousarray(o[::-1]), np.ascontiguousarray(d[::-1]), cap=8)
    assert np.ascontiguousarray(rh[::-1]).tobytes() == hits.tobytes() and np.ascontiguousarray(rc[::-1]).tobytes() == counts.tobytes()
    for b in range(5):
        engine.upload(meshes[b:b + 1])
        ah, ac = engine.ray_cast(o[b], d[b], cap=8)
        assert ah[0].tobytes() == hits[b].tobytes() and ac[0].tobytes() == counts[b].tobytes(), b


def test_humerus_left_from_inside_and_from_outside(engine, humerus_mesh):
    """5: 256 rays from the mean of the vertices (one hit each), 64 from 400 mm outside towards jittered vertices (5 miss, 55 with two
    hits, 4 with four).  A ray with a face within 1e-9 of a threshold of the rule may be left out, at most 1 % of the rays"""
    v, f = humerus_mesh
    v64 = O.widen(v)
    rng = np.random.default_rng(7)
    D = rng.normal(size=(256, 3))
    c = v64.mean(axis=0)
    Dh = D / np.linalg.norm(D, axis=1, keepdims=True)
    org = c + 400.0 * Dh[:64]
    tgt = v64[rng.integers(0, len(v), 64)] + rng.normal(size=(64, 3))
    o = np.concatenate([np.broadcast_to(c, (256, 3)), org])
    d = np.concatenate([D, tgt - org])
    engine.upload([(v, f)])
    hits, counts = engine.ray_cast(o, d, cap=8)
    doubt = [r for r in range(320) if O.in_doubt(v64, f, o[r], d[r])]
    print("rays left out as in doubt:", len(doubt), "of 320")
    assert len(doubt) <= 3
    want, wn = check(hits[0], counts[0], v, f, o, d, skip=doubt)
    print("max |t - oracle|", np.abs(hits[0]["t"] - want["t"]).max(), "max |point - oracle|", np.abs(hits[0]["point"] - want["point"]).max())
    assert np.all(wn[:256] == 1) and [int((wn[256:] == k).sum()) for k in (0, 2, 4)] == [5, 55, 4]
    two = hits[0][256:][wn[256:] == 2]
    assert np.all(two["side"][:, 0] == 1) and np.all(two["side"][:, 1] == -1) and np.all(hits[0]["side"][:256, 0] == -1)


def ray_t(engine, B):
    return engine.fetch("anp.ray_t", np.uint64, (B, 4)).view(np.float64)


def check_first_hits(hits, counts, status, lm, t):
    for b in range(len(lm)):
        assert status[b] == 0 and lm[b]["status"] == 0
        rows = np.concatenate([lm[b]["anp_axis_normal"], lm[b]["anp_axis_central"]])
        assert np.ascontiguousarray(hits[b, :, 0]["point"]).tobytes() == np.ascontiguousarray(rows).tobytes(), b
        assert np.ascontiguousarray(hits[b, :, 0]["t"]).tobytes() == t[b].tobytes(), b
        assert np.all(counts[b] >= 1)


@pytest.fixture(scope="module")
def fixture_run(engine):
    """the four fixture bones as one batch, STAGE_ALL with the f32 network: records, every hit of the four rays, the box planes"""
    meshes = [load_stl(os.path.join(BONES, n + ".stl")) for n in NAMES]
    engine.reset_params()
    engine.set_params(unet_dtype=_lib.UNET_F32)
    engine.upload(meshes)
    lm = engine.run(_lib.STAGE_ALL).copy()
    hits, counts, status = engine.anp_axis_hits(cap=8)
    out = dict(meshes=meshes, lm=lm, hits=hits, counts=counts, status=status, t=ray_t(engine, 4), plane=engine.fetch("anp.plane", np.float64, (4, 6)))
    engine.reset_params()
    return out


def test_anatomic_neck_rays_of_the_fixtures(engine, fixture_run):
    """6: every ray of every fixture bone has exactly one hit, which is the record's row and "anp.ray_t", as bytes"""
    S = fixture_run
    assert S["hits"].shape == (4, 4, 8) and np.all(S["counts"] == 1)
    check_first_hits(S["hits"], S["counts"], S["status"], S["lm"], S["t"])
    assert np.all(S["hits"][:, :, 1:]["face"] == -1) and not S["hits"][:, :, 1:]["t"].any()
    assert np.all(S["hits"][:, :, 0]["side"] == -1)                                   # from inside the bone outwards


@pytest.fixture(scope="module")
def cyst(engine, fixture_run):
    """humerus_left with an inward-facing box of half-size 3 mm at p0 + 8 n0 in the box frame (a subchondral cyst below the articular
    surface): its mesh, its record and every hit of its four rays"""
    from test_gpu_random_sweep import _box
    S = fixture_run
    v, f = S["meshes"][0]
    pl = S["plane"][0]
    n0 = pl[3:] if pl[5] >= 0 else -pl[3:]
    bv, bf = _box(pl[:3] + 8.0 * n0, 3.0, np.linalg.inv(S["lm"][0]["obb_transform"].reshape(4, 4)), inward=True)
    mv = np.concatenate([v, bv]).astype(np.float32)
    mf = np.concatenate([f, bf + len(v)]).astype(np.int32)
    engine.reset_params()
    engine.set_params(unet_dtype=_lib.UNET_F32)
    engine.upload([(mv, mf)])
    lm = engine.run(_lib.STAGE_ALL).copy()
    hits, counts, status = engine.anp_axis_hits(cap=8)
    out = dict(mesh=(mv, mf), lm=lm, hits=hits, counts=counts, status=status, t=ray_t(engine, 1), plane=engine.fetch("anp.plane", np.float64, (1, 6)))
    engine.reset_params()
    return out


def test_anatomic_neck_rays_through_a_cyst(engine, fixture_run, cyst):
    """6: the plane does not move; +normal and +central cross the cyst (out of the bone into it, out of it into the bone, out of the
    bone); the first hit is the cyst bone's own record, the last +normal hit the intact bone's"""
    S, C = fixture_run, cyst
    assert C["plane"][0].tobytes() == S["plane"][0].tobytes()
    assert list(C["counts"][0]) == [3, 1, 3, 1]
    check_first_hits(C["hits"], C["counts"], C["status"], C["lm"], C["t"])
    for ray in (0, 2):
        assert list(C["hits"][0, ray, :3]["side"]) == [-1, 1, -1] and np.all(C["hits"][0, ray, :3]["face"][:2] >= len(S["meshes"][0][1]))
    print("+normal t", C["hits"][0, 0, :3]["t"], "+central t", C["hits"][0, 2, :3]["t"])
    assert np.abs(C["hits"][0, 0, 2]["point"] - S["lm"][0]["anp_axis_normal"][0]).max() <= MM
    assert np.abs(C["hits"][0, 2, 2]["point"] - S["lm"][0]["anp_axis_central"][0]).max() <= MM
    assert np.abs(C["hits"][0, 0, :3]["t"] - [4.8529, 11.1471, 17.6612]).max() <= 1e-4   # the figures of the issue, four decimals
    assert np.linalg.norm(C["lm"][0]["anp_axis_normal"][0] - S["lm"][0]["anp_axis_normal"][0]) > 12.0      # the record stops at the cyst wall
    # the box-frame cast against NumPy on the box-frame corners: counts, faces and sides equal, t within the bound
    T = C["lm"][0]["obb_transform"].reshape(4, 4)
    vb = SO.map_points(T, C["mesh"][0])
    pl = C["plane"][0]
    n0 = pl[3:] if pl[5] >= 0 else -pl[3:]
    t, face, side = O.ray_hits(vb, C["mesh"][1], pl[:3], n0)
    assert np.array_equal(face, C["hits"][0, 0, :3]["face"]) and np.array_equal(side, C["hits"][0, 0, :3]["side"]) and np.abs(t - C["hits"][0, 0, :3]["t"]).max() <= MM


def write_stl(path, v, f):
    rec = np.zeros(len(f), dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    rec["v"] = v[f].astype(np.float32)
    with open(path, "wb") as fh:
        fh.write(b"\0" * 80 + np.uint32(len(f)).tobytes() + rec.tobytes())


def test_facade_on_the_cyst_bone(engine, fixture_run, cyst, tmp_path):
    """6: hits="all" is upper hits then lower hits, "outermost" the intact bone's axis, the default what it was; ray_hits in the current
    coordinate system is the transform of the CT locations"""
    S, C = fixture_run, cyst
    p = tmp_path / "humerus_left_cyst.stl"
    write_stl(p, *C["mesh"])
    engine.reset_params()
    engine.set_params(unet_dtype=_lib.UNET_F32)
    try:
        intact = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        want_outer, want_central = intact.anatomic_neck.axis_normal().copy(), intact.anatomic_neck.axis_central().copy()
        hum = shoulder.Humerus(p, engine=engine)
        near = hum.anatomic_neck.axis_normal().copy()
        every = hum.anatomic_neck.axis_normal(hits="all")
        outer = hum.anatomic_neck.axis_normal(hits="outermost")
        assert near.shape == (2, 3) and every.shape == (4, 3) and outer.shape == (2, 3)
        assert np.abs(outer - want_outer).max() <= MM and np.abs(hum.anatomic_neck.axis_central(hits="outermost") - want_central).max() <= MM
        assert every[0].tobytes() == near[0].tobytes() and every[3].tobytes() == near[1].tobytes() and every[2].tobytes() == outer[0].tobytes()
        assert hum.anatomic_neck.axis_normal().tobytes() == near.tobytes() and hum.anatomic_neck.axis_central(hits="all").shape == (4, 3)
        assert np.linalg.norm(near[0] - outer[0]) > 12.0
        with pytest.raises(ValueError):
            hum.anatomic_neck.axis_normal(hits="farthest")
        # rays in CT, then the same rays in the articular coordinate system
        c = C["mesh"][0].astype(np.float64).mean(axis=0)
        d = np.random.default_rng(1).normal(size=(6, 3))
        o = np.broadcast_to(c, d.shape)
        loc, ir, it = hum.ray_hits(o, d)
        assert len(loc) >= 6 and np.array_equal(ir, np.sort(ir)) and set(ir) == set(range(6))
        Tm = hum.apply_csys_canal_articular().copy()
        o2, d2 = engine.transform_points(o, Tm), d @ Tm[:3, :3].T
        loc2, ir2, it2 = hum.ray_hits(o2, d2)
        assert np.array_equal(ir2, ir) and np.array_equal(it2, it)
        assert np.abs(loc2 - engine.transform_points(loc, Tm)).max() <= MM
        assert hum.anatomic_neck.axis_normal(hits="all").shape == (4, 3)
        assert np.abs(hum.anatomic_neck.axis_normal(hits="outermost") - engine.transform_points(outer, Tm)).max() <= MM
    finally:
        engine.reset_params()


def test_state_and_arguments(engine, humerus_mesh):
    """7"""
    o, d = np.zeros((2, 3)), np.array([(0.0, 0.0, 1.0), (1.0, 0.0, 0.0)])

    def refused(e, code, word, fn="ray_cast", **kw):
        with pytest.raises(ShoulderHipError) as ex:
            e.anp_axis_hits(**kw) if fn == "anp" else e.ray_cast(**dict(dict(origins=o, directions=d, cap=8), **kw))
        assert ex.value.code == code and word in str(ex.value), str(ex.value)
    fresh = Engine(0)
    try:
        refused(fresh, -3, "no meshes")                                               # without a batch
        refused(fresh, -3, "no meshes", fn="anp")
    finally:
        fresh.close()
    v, f = humerus_mesh
    engine.reset_params()
    engine.upload([(v, f)])
    refused(engine, -3, "SH_STAGE_ANP", fn="anp")                                     # before a run
    engine.run(_lib.STAGE_OBB | _lib.STAGE_FULL)
    refused(engine, -3, "SH_STAGE_ANP", fn="anp")                                     # a run without the stage
    engine.ray_cast(o, d, cap=8)                                                      # a batch is enough for sh_ray_cast
    refused(engine, -1, "cap", cap=0)
    refused(engine, -1, "cap", cap=1025)
    refused(engine, -1, "cap", fn="anp", cap=0)
    refused(engine, -1, "cap", fn="anp", cap=1025)
    refused(engine, -1, "R", origins=np.zeros((0, 3)), directions=np.zeros((0, 3)))
    bad = d.copy()
    bad[1, 2] = np.nan
    refused(engine, -1, "ray 1", directions=bad)
    bad[1] = 0.0
    refused(engine, -1, "ray 1", directions=bad)
    worse = o.copy()
    worse[0, 0] = np.inf
    refused(engine, -1, "ray 0", origins=worse)
    # the records of a run, the profile and the stems are the same bytes before and after a cast
    lm = engine.run(_lib.STAGE_ALL)
    engine.resect(offsets=[dict(), dict(depth_canal_mm=-4.0)])
    engine.canal_profile(40.0, 4.0, 8, 16)
    engine.resect_stems([(100.0, 6.0, 3.5)])
    names = ("landmarks", "canal.near", "stem.out", "resect.out", "anp.ray_t", "anp.axes_obb", "verts_obb")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    hits, counts, status = engine.anp_axis_hits(cap=4)
    engine.ray_cast(v.astype(np.float64).mean(axis=0)[None] + np.zeros((3, 1)), np.eye(3), cap=4)
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before
    assert status[0] == 0 and np.ascontiguousarray(hits[0, :2, 0]["point"]).tobytes() == np.ascontiguousarray(lm[0]["anp_axis_normal"]).tobytes()
    assert engine.resect_stems([(100.0, 6.0, 3.5)]).shape == (1, 2, 1)                # the chain's state is what it was
    # with runs in flight
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        refused(engine, -3, "in flight")
        refused(engine, -3, "in flight", fn="anp", cap=4)
    finally:
        engine.collect()
    assert engine.anp_axis_hits(cap=4)[0].tobytes() == hits.tobytes()
