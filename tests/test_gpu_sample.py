"""Surface samples of the resident batch (include/shoulder_hip.h sh_sample_surface, k_sample.h) on the engine against the NumPy
statement of tests/sample_oracle.py.

Bounds.  The words are integer arithmetic, the rest + - x sqrt on float64 in a fixed order, every one correctly rounded on the device,
and the order of the cumulative areas and the rounds of the thinning are part of the definition: "samp.cdf", the records and the info
are held to the oracle as bytes.  The facade: a sample is a point of its face up to the rounding of A + (r1 ab + r2 ac) and of the
mapping into the current system and back, some eps of coordinates of a few hundred mm, about 1e-13 mm; 1e-9 mm is asserted, the bound of
test_gpu_closest.py's facade.  Recovering a pose: 1e-9 mm, the bound of test_gpu_multistart.py for humerus_left."""
import os

import numpy as np
import pytest

import closest_oracle as CO
import icp_oracle as IO
import sample_oracle as O
import shoulder_amd as shoulder
from conftest import BONES
from mass_oracle import int_box
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
NAMES = ["humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped"]
ONLY_FLAT = np.array([[0, 1, 1], [2, 2, 3], [4, 5, 4], [6, 6, 6]], np.int32)


def load(name):
    v, f = load_stl(os.path.join(BONES, name + ".stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


@pytest.fixture(scope="module")
def meshes():
    out = {n: load(n) for n in NAMES + ["proximal_left_cut"]}
    out["box"] = int_box()
    return out


@pytest.fixture(scope="module")
def oracle(meshes):
    """the oracle's (records, info, cdf) by (mesh name, N, seed, radius, max_rounds), each computed once"""
    cache = {}

    def get(name, N, seed, radius=0.0, max_rounds=32):
        key = (name, N, seed, radius, max_rounds)
        if key not in cache:
            cache[key] = O.sample(*meshes[name], N, seed, radius, max_rounds)
        return cache[key]
    return get


def device(engine, batch, N, seed, radius=None, max_rounds=32, upload=True):
    """-> (records (B, N), info (B,), the humeri's parts of "samp.cdf"); the resident records are what the call returned"""
    if upload:
        engine.upload(batch)
    rec, info = engine.sample_surface(N, seed=seed, radius=radius, max_rounds=max_rounds)
    assert rec.shape == (len(batch), N) and info.shape == (len(batch),)
    assert engine.fetch("samp.out", _lib.SAMPLE_DTYPE, rec.shape).tobytes() == rec.tobytes()
    assert engine.fetch("samp.info", _lib.SAMPLE_INFO_DTYPE, info.shape).tobytes() == info.tobytes()
    nf = [len(f) for _, f in batch]
    cdf = engine.fetch("samp.cdf", np.float64, (sum(nf),))
    return rec, info, np.split(cdf, np.cumsum(nf)[:-1])


def equal(got, b, want, tag):
    rec, info, cdf = got
    assert cdf[b].tobytes() == want[2].tobytes(), (tag, "samp.cdf")
    assert rec[b].tobytes() == want[0].tobytes(), (tag, "samp.out")
    assert info[b].tobytes() == want[1].tobytes(), (tag, info[b], want[1])


def test_box_block_edges_and_sample_counts(engine, meshes, oracle):
    """the box; prefixes of humerus_left at the edges of the 256-face blocks (an upload refuses fewer than four faces, so the smallest
    has 4; one face is held on the host twin); sample counts at the edges of the 256-sample chunks"""
    got = device(engine, [meshes["box"]], 1000, 7)
    equal(got, 0, oracle("box", 1000, 7), "box")
    assert got[1][0]["area"] == 2200.0 and got[1][0]["kept"] == 1000 and (got[0][0]["keep"] == 1).all()
    v, f = meshes["humerus_left"]
    for n in (4, 255, 256, 257, 513):
        fn = np.ascontiguousarray(f[:n])
        equal(device(engine, [(v, fn)], 300, n), 0, O.sample(v, fn, 300, n), f"{n} faces")
    fn = np.ascontiguousarray(f[:513])
    full = O.sample(v, fn, 1000, 5)
    for i, N in enumerate((1, 255, 256, 257, 1000)):
        got = device(engine, [(v, fn)], N, 5, upload=i == 0)
        equal(got, 0, O.sample(v, fn, N, 5), f"N = {N}")
        assert got[0][0].tobytes() == full[0][:N].tobytes()                           # a sample depends on its index, not on N


@pytest.mark.parametrize("name", NAMES)
def test_whole_fixtures(engine, meshes, oracle, name):
    got = device(engine, [meshes[name]], 1000, 7)
    equal(got, 0, oracle(name, 1000, 7), name)
    assert got[1][0]["status"] == 0 and (np.diff(got[2][0]) >= 0.0).all()


def test_thinning(engine, meshes, oracle):
    """N = 1 024 at 2 and 4 mm on a whole bone and a cut one, one radius that holds everything, and one round that is not enough"""
    names = ("humerus_left", "proximal_left_cut")
    batch = [meshes[n] for n in names]
    for i, (radius, max_rounds) in enumerate(((2.0, 32), (4.0, 32), (1e9, 32), (2.0, 1))):
        got = device(engine, batch, 1024, 7, radius=radius, max_rounds=max_rounds, upload=i == 0)
        for b, n in enumerate(names):
            want = oracle(n, 1024, 7, radius, max_rounds)
            equal(got, b, want, (n, radius, max_rounds))
            print(n, "radius", radius, "max_rounds", max_rounds, "kept", got[1][b]["kept"], "rounds", got[1][b]["rounds"], "status", got[1][b]["status"])
            if radius == 1e9:
                assert got[1][b]["kept"] == 1 and got[1][b]["rounds"] == 2 and got[0][b]["keep"][0] == 1 and not got[0][b]["keep"][1:].any()
            elif max_rounds == 1:
                assert got[1][b]["status"] == O.CAPACITY and got[1][b]["rounds"] == 1 and (got[0][b]["keep"] == -1).any() and (got[0][b]["keep"] == 1).any()
            else:
                assert got[1][b]["status"] == 0 and 1 < got[1][b]["rounds"] <= 32 and set(got[0][b]["keep"]) == {0, 1}
                assert got[1][b]["kept"] == (got[0][b]["keep"] == 1).sum()
    # the points of a thinned call are those of a plain one
    plain = device(engine, batch, 1024, 7, upload=False)
    assert plain[0]["point"].tobytes() == got[0]["point"].tobytes() and (plain[0]["keep"] == 1).all()


def test_a_record_does_not_depend_on_the_batch(engine, meshes, oracle):
    """[box, left, right, left] against the singles, with and without thinning; two seeds make the two lefts differ, equal seeds make
    them identical"""
    names = ("box", "humerus_left", "humerus_right", "humerus_left")
    batch = [meshes[n] for n in names]
    got = device(engine, batch, 1000, 7)
    for b, n in enumerate(names):
        equal(got, b, oracle(n, 1000, 7), n)
    assert got[0][1].tobytes() == got[0][3].tobytes() and got[1][1].tobytes() == got[1][3].tobytes()
    seeds = [7, 7, 7, 8]
    two = device(engine, batch, 1000, seeds, upload=False)
    equal(two, 3, O.sample(*meshes["humerus_left"], 1000, 8), "seed 8")
    assert two[0][1].tobytes() == got[0][1].tobytes() and two[0][3].tobytes() != two[0][1].tobytes()
    assert not np.array_equal(two[0][3]["face"], two[0][1]["face"])
    thin = device(engine, batch, 1024, 7, radius=2.0, upload=False)
    for b, n in enumerate(names):
        equal(thin, b, oracle(n, 1024, 7, 2.0, 32), (n, "thinned"))
    single = device(engine, [meshes["humerus_right"]], 1024, 7, radius=2.0)
    assert single[0][0].tobytes() == thin[0][2].tobytes() and single[1][0].tobytes() == thin[1][2].tobytes()


def test_zero_area_faces(engine, meshes):
    """a mesh with faces of zero area (in front, in the middle, at a block boundary, at the end), a mesh of ONLY such faces (four: an
    upload refuses fewer) and the box: the second has the status and zero records, its neighbours are what they are alone"""
    v, f = meshes["humerus_left"]
    where = (0, 1, 100, 255, 256, 300, 519)
    zv, zf = O.zero_area_mesh(v, f[:513], where)
    batch = [(zv, zf), (v, ONLY_FLAT), meshes["box"]]
    for radius in (0.0, 2.0):
        got = device(engine, batch, 1024, 3, radius=radius or None)
        for b, (vv, ff) in enumerate(batch):
            equal(got, b, O.sample(vv, ff, 1024, 3, radius), (b, radius))
        assert not np.isin(got[0][0]["face"], where).any() and all(got[2][0][k] == got[2][0][k - 1] for k in where[2:])
        assert got[1][1]["status"] == O.GEOMETRY and got[1][1]["kept"] == 0 and not np.frombuffer(got[0][1].tobytes(), np.uint8).any()
        assert got[1][0]["status"] == 0 and got[1][2]["status"] == 0 and not got[2][1].any()


def test_determinism_state_and_buffers(engine, meshes):
    fresh = Engine(0)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            fresh.sample_surface(10)
        assert ex.value.code == O.STATE and "sh_sample_surface" in str(ex.value) and "no meshes" in str(ex.value)
    finally:
        fresh.close()
    v, f = meshes["humerus_left"]
    engine.reset_params()
    engine.upload([(v, f)])
    pts = v[:300].astype(np.float64)
    engine.closest_points(pts)
    engine.mass_properties()
    names = ("cp.out", "mass.out", "mass.part", "verts", "faces")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    a = engine.sample_surface(1024, seed=9, radius=3.0)
    b = engine.sample_surface(1024, seed=9, radius=3.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()      # two calls, the same bytes
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before             # other queries' results survive
    for kw, text in ((dict(n=0), "N in 1.."), (dict(n=_lib.SAMPLE_MAX + 1), "N in 1.."), (dict(n=10, radius=-1.0), "options"),
                     (dict(n=10, radius=float("nan")), "options"), (dict(n=10, radius=1.0, max_rounds=0), "options"),
                     (dict(n=10, radius=1.0, max_rounds=33), "options"), (dict(n=_lib.SAMPLE_THIN_MAX + 1, radius=1.0), "with a radius")):
        with pytest.raises(ShoulderHipError) as ex:
            engine.sample_surface(**kw)
        assert ex.value.code == O.ARG and "sh_sample_surface" in str(ex.value) and text in str(ex.value), kw
    with pytest.raises(ValueError):
        engine.sample_surface(10, seed=[1, 2])
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            engine.sample_surface(10)
        assert ex.value.code == O.STATE and "in flight" in str(ex.value) and "sh_sample_surface" in str(ex.value)
    finally:
        engine.collect()
    assert engine.sample_surface(1024, seed=9, radius=3.0)[0].tobytes() == a[0].tobytes()
    engine.upload([(v, f)])                                                           # "samp.*" answer for their batch
    for name in ("samp.cdf", "samp.base", "samp.out", "samp.info", "samp.state"):
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)


def test_facade_samples_lie_on_the_surface(engine, meshes, oracle):
    engine.reset_params()
    try:
        h = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        ct, faces_ct = h.sample_surface(512, seed=7)
        want = oracle("humerus_left", 1000, 7)[0][:512]
        assert ct.shape == (512, 3) and faces_ct.dtype == np.int64 and np.array_equal(faces_ct, want["face"])
        assert np.abs(ct - want["point"]).max() <= 1e-9
        M = np.array(h.apply_csys_canal_transepiconylar(), dtype=np.float64)
        pts, faces = h.sample_surface(512, seed=7)
        assert np.array_equal(faces, faces_ct) and np.abs(pts - IO.apply(M, ct)).max() <= 1e-9
        closest, dist, tri = h.closest_point(pts)
        print("facade: largest closest_point distance of a sample", dist.max(), "samples whose closest face is another", int((tri != faces).sum()))
        assert dist.max() <= 1e-9
        v, f = meshes["humerus_left"]
        back = IO.apply(np.linalg.inv(M), pts)
        own = np.array([np.sqrt(CO.oracle_tri(back[i], v[f[faces[i]]].astype(np.float64))[3]) for i in range(len(pts))])
        assert own.max() <= 1e-9                                                      # the drawn face is among the faces at that distance
        even, even_faces = h.sample_surface(1024, seed=7, radius=4.0)                 # sample_surface_even: only the kept ones
        keep = oracle("humerus_left", 1024, 7, 4.0, 32)[0]["keep"] == 1
        assert len(even) == keep.sum() < 1024 and np.array_equal(even_faces, oracle("humerus_left", 1024, 7, 4.0, 32)[0]["face"][keep])
        d = even[:, None, :] - even[None, :, :]
        d2 = (d * d).sum(axis=2) + np.identity(len(even)) * 1e9
        assert np.sqrt(d2.min()) >= 4.0 - 1e-9
    finally:
        engine.reset_params()


def test_facade_register_and_surface_distance(engine, meshes):
    """register(other bone, sample=512, initial="principal") recovers the pose other was put in (140 degrees about (1, 2, 3) and
    (40, -25, 60) mm, the pose and the settings of test_gpu_multistart.py's "whole" case on this bone, and its bound: 1e-9 mm);
    surface_distance of a bone against itself through samples is zero both ways; the defaults are the vertex path"""
    engine.reset_params()
    try:
        path = os.path.join(BONES, "humerus_left.stl")
        h, other = shoulder.Humerus(path, engine=engine), shoulder.Humerus(path, engine=engine)
        truth = other.sample_surface(512, seed=3)[0]                                  # (CT: where the samples lie on h)
        same = h.surface_distance(other, sample=512, seed=3, symmetric=True)
        print("facade: a bone against itself", same)
        assert same["n"] == 512 and same["max"] <= 1e-9 and same["max_back"] <= 1e-9 and same["hausdorff"] == max(same["max"], same["max_back"]) <= 1e-9
        assert same["rms"] <= 1e-9 and same["rms_back"] <= 1e-9
        with pytest.raises(ValueError):
            h.surface_distance(other, symmetric=True)
        with pytest.raises(ValueError):
            h.surface_distance(truth, sample=16)
        # the defaults: the vertices of other, exactly as before
        assert h.surface_distance(other.mesh) == h.surface_distance(np.asarray(other.mesh.vertices, dtype=np.float64))
        verts = np.asarray(other.mesh.vertices, dtype=np.float64)[:2000]
        pose = IO.rigid((1.0, 2.0, 3.0), 4.0, (0.5, -0.25, 0.6), about=verts.mean(axis=0))
        moved = IO.apply(pose, verts)
        M_default, info_default = h.register(Points(moved), max_iter=4)
        M_explicit, info_explicit = h.register(moved, max_iter=4)
        assert M_default.tobytes() == M_explicit.tobytes() and info_default == info_explicit
        # an unknown pose, through samples
        T = IO.rigid((1.0, 2.0, 3.0), 140.0, (40.0, -25.0, 60.0), about=truth.mean(axis=0))
        other.apply_csys_custom(T)
        pts = other.sample_surface(512, seed=3)[0]
        assert np.abs(pts - IO.apply(T, truth)).max() <= 1e-9
        M, info = h.register(other, sample=512, seed=3, initial="principal", rolls=4, max_iter=8)
        err = float(np.abs(IO.apply(M, pts) - truth).max())
        print("facade register(sample=512, principal):", info, "max |M p - truth|", err)
        assert err < 1e-9 and info["winner"] >= 0
        M2, info2 = h.register(pts, initial="principal", rolls=4, max_iter=8)         # the same points, handed over by the caller
        assert M2.tobytes() == M.tobytes() and info2["rms"] == info["rms"]
        far = h.surface_distance(other, sample=512, seed=3, symmetric=True)
        assert far["hausdorff"] > 10.0 and far["max_back"] > 10.0
    finally:
        engine.reset_params()


class Points:
    """something with `.vertices`, as a Mesh has"""
    def __init__(self, p):
        self.vertices = p
