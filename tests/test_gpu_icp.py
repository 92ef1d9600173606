"""Rigid registration of point sets onto the resident batch (include/shoulder_hip.h sh_register_points, k_icp.h) on the engine against
the NumPy statement of tests/icp_oracle.py.

Bounds.  The chain is + - x / sqrt on float64 in a fixed order and every one of them is correctly rounded on the device, so the device
equals the oracle BIT FOR BIT (observed in every comparison when these tests were written): sums ("icp.part"), pairs ("icp.near"),
records, histories and everything compared between runs, batches, point lists and walk splits are held to equality as bytes.  The
bound the equality replaces is still computed and printed beside the observed maximum: max_p |T_dev p - T_oracle p| <=
64 max(E, 2^-52 max|coordinate|), E the same quantity between two runs of the ORACLE that differ only in summation order (the
defined tree against ndarray.sum), never taken from the device.  Reaching the truth: 1e-9 mm, asserted on the oracle first.  The
oracle pairs with closest_culled, held to the full walk on every point of the recovery cases at their start."""
import os

import numpy as np
import pytest

import closest_oracle as CO
import icp_oracle as O
import shoulder_amd as shoulder
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
NAMES = ["humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped"]
EPS = 2.0 ** -52
METRIC = {O.POINT: "point", O.PLANE: "plane"}


def f32(v, f):
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def load(name):
    return f32(*load_stl(os.path.join(BONES, name + ".stl")))


def spread(Ta, Tb, pts):
    """max_p |Ta p - Tb p|"""
    return float(np.abs(O.apply(np.asarray(Ta), pts) - O.apply(np.asarray(Tb), pts)).max())


def bound(E, pts, T):
    return 64.0 * max(E, EPS * max(float(np.abs(pts).max()), float(np.abs(O.apply(np.asarray(T), pts)).max())))


def both_oracles(v, f, pts, metric, max_iter, closest=None, **kw):
    """the oracle as defined, and E: how far the same oracle lands with ndarray.sum in place of the tree"""
    o = O.register(v, f, pts, None, metric, max_iter, closest=closest, **kw)
    o2 = O.register(v, f, pts, None, metric, max_iter, tree=False, closest=closest, **kw)
    return o, spread(o["T"], o2["T"], pts), float(np.abs(o["history"][:, 0] - o2["history"][:, 0]).max())


def against_oracle(tag, rec, o, E, pts):
    """the device's record against the oracle's: bytes (the bound the equality replaces is printed beside the observed maximum)"""
    for k in ("pairs", "iterations", "converged", "status"):
        assert rec[k] == o[k], (tag, k, rec[k], o[k])
    got, lim = spread(rec["T"], o["T"], pts), bound(E, pts, o["T"])
    same = rec.tobytes() == O.record(o).tobytes()
    print(f"{tag}: max |T_dev p - T_oracle p| = {got:.3e} mm (bound {lim:.3e}, E {E:.3e}); record byte-equal: {same}")
    assert got <= lim, (tag, got, lim)
    assert same, (tag, rec, O.record(o))
    return got


@pytest.fixture(scope="module")
def humerus_mesh():
    return load("humerus_left")


@pytest.fixture(scope="module")
def cases(humerus_mesh):
    """the inputs of the recovery tests: 300 vertices of the first 2 049 faces of humerus_left against those faces, and 96 vertices of
    the whole bone, moved by 4 degrees about (1, 2, 3) through their centroid and (1.5, -1.0, 0.8) mm; oracle runs are cached here"""
    v, f = humerus_mesh
    out = {}
    for name, faces, n in (("sub", np.ascontiguousarray(f[:2049]), 300), ("whole", f, 96)):
        ids = np.random.default_rng(1).choice(np.unique(faces), n, replace=False)
        truth = v[ids].astype(np.float64)
        M = O.rigid((1.0, 2.0, 3.0), 4.0, (1.5, -1.0, 0.8), about=truth.mean(axis=0))
        out[name] = dict(v=v, f=faces, truth=truth, pts=O.apply(M, truth), oracle={})
    for c in out.values():                                                            # the cull changes no byte: every point of both cases at T0
        assert O.closest_culled(v, c["f"], c["pts"]).tobytes() == CO.closest(v, c["f"], c["pts"]).tobytes()
    return out


def oracle_of(case, metric, max_iter, **kw):
    key = (metric, max_iter, tuple(sorted(kw.items())))
    if key not in case["oracle"]:
        case["oracle"][key] = both_oracles(case["v"], case["f"], case["pts"], metric, max_iter, closest=O.closest_culled, **kw)
    return case["oracle"][key]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [O.POINT, O.PLANE])
@pytest.mark.parametrize("Q", [6, 255, 256, 257, 513])
def test_scalene_box(engine, Q, metric):
    """1: points on all six faces of the 30 x 20 x 10 box moved by 3 degrees about (1, 2, 3) and (0.4, -0.3, 0.2) mm, Q at the block
    edges.  The sums as bytes: a humerus that is done keeps its "icp.part", so a call with max_iter = 1 leaves the rows of evaluation 1,
    taken at the returned T; they are held to the oracle's evaluation at that T, row by row and joined, and the pivot's mean and the
    history rows (rms, pairs of evaluations 0 and 1) to the oracle's loop.  Then the whole loop under the bound."""
    v, f = O.box()
    pts = O.apply(O.BOX_MOVE, O.box_points(Q, seed=Q))
    engine.upload([(v, f)])
    m = METRIC[metric]
    rec, hist = engine.register(pts, metric=m, max_iter=1, history=True)
    blocks = (Q + 255) // 256
    part = engine.fetch("icp.part", np.float64, (1, blocks, 32))[0]
    state = engine.fetch("icp.T", np.float64, (1, 20))[0]
    cbar = O.tree_sum(np.concatenate([np.ones((Q, 1)), pts], axis=1))[1:] / float(Q)
    assert state[16:19].tobytes() == cbar.tobytes()
    terms, near, pm = O.evaluate(v, f, pts, rec[0]["T"].reshape(16), metric, np.inf, cbar)
    assert part.tobytes() == O.block_rows(terms).tobytes()
    tot = np.zeros(32)
    for row in part:
        tot = tot + row
    assert tot.tobytes() == O.tree_sum(terms).tobytes() and tot[0] == Q
    assert engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (1, Q))[0].tobytes() == near.tobytes()
    assert engine.fetch("icp.moved", np.float64, (1, Q, 3))[0].tobytes() == pm.tobytes()
    o1 = O.register(v, f, pts, None, metric, 1)
    assert hist[0].tobytes() == o1["history"].tobytes()                               # evaluation 0: rms and pairs from the sums at T0; and 1
    assert rec[0].tobytes() == O.record(o1).tobytes()                                 # so the T the rows above were taken at is the oracle's
    K = 8 if metric == O.PLANE else 12
    o, E, _ = both_oracles(v, f, pts, metric, K)
    rec, hist = engine.register(pts, metric=m, max_iter=K, history=True)
    against_oracle(f"box Q={Q} {m}", rec[0], o, E, pts)
    assert hist[0].tobytes() == o["history"].tobytes()
    assert np.array_equal(hist[0, :, 1], o["history"][:, 1]) and rec[0]["rms"] == hist[0, rec[0]["iterations"], 0]


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sub", "whole"])
def test_recovery_plane_metric(engine, cases, name):
    """2: the oracle alone must bring max |T p - p_true| below 1e-9 mm within 8 evaluations; then the device must"""
    c = cases[name]
    o, E, _ = oracle_of(c, O.PLANE, 8)
    errs = [float(np.abs(O.apply(T, c["pts"]) - c["truth"]).max()) for T in o["Ts"]]
    print(name, "oracle rms", o["history"][:, 0], "oracle max |T p - truth| per evaluation", errs)
    assert o["status"] == 0 and min(errs[:8]) < 1e-9 and errs[-1] < 1e-9
    engine.upload([(c["v"], c["f"])])
    rec, hist = engine.register(c["pts"], metric="plane", max_iter=8, history=True)
    err = float(np.abs(O.apply(rec[0]["T"], c["pts"]) - c["truth"]).max())
    print(name, "device rms", hist[0, :, 0], "device max |T p - truth|", err, "min_pivot", rec[0]["min_pivot"])
    assert rec[0]["status"] == 0 and err < 1e-9 and rec[0]["pairs"] == len(c["pts"]) and rec[0]["iterations"] == 8
    assert 0.0 < rec[0]["min_pivot"] <= 1.0
    against_oracle(f"recovery {name} plane", rec[0], o, E, c["pts"])


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sub", "whole"])
def test_point_metric(engine, cases, name):
    """3: the same inputs, 12 updates.  The rms does not rise by more than the oracle's own largest rise; every history row agrees with
    the oracle's (bytes; the bound that replaces is 64 max(E_rms, 2^-52 rms), E_rms the largest difference between the two oracles'
    rows).  It
    is not asked to reach the truth: the point metric converges linearly"""
    c = cases[name]
    o, E, E_rms = oracle_of(c, O.POINT, 12)
    rises = np.diff(o["history"][:, 0])
    slack = max(0.0, float(rises.max()))
    engine.upload([(c["v"], c["f"])])
    rec, hist = engine.register(c["pts"], metric="point", max_iter=12, history=True)
    h = hist[0]
    print(name, "point metric rms", h[:, 0], "oracle's largest rise", slack)
    assert np.all(np.diff(h[:, 0]) <= slack) and h[-1, 0] < h[0, 0]
    assert np.array_equal(h[:, 1], o["history"][:, 1])
    d = float(np.abs(h[:, 0] - o["history"][:, 0]).max())
    print(name, "max |rms_dev - rms_oracle| over the history", d, "E_rms", E_rms)
    assert d <= 64.0 * max(E_rms, EPS * float(h[:, 0].max())) and h.tobytes() == o["history"].tobytes()
    assert rec[0]["min_pivot"] == 1.0 and rec[0]["rms"] == h[12, 0] and rec[0]["rms_first"] == h[0, 0]
    against_oracle(f"{name} point", rec[0], o, E, c["pts"])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_rejection(engine, cases):
    """4: 8 of the 96 points displaced by 200 mm along +y, reject = 10 mm: 88 pairs at every evaluation, the other 88 recovered"""
    c = cases["whole"]
    pts = c["pts"].copy()
    pts[:8, 1] += 200.0
    o, E, _ = both_oracles(c["v"], c["f"], pts, O.PLANE, 8, closest=O.closest_culled, reject=10.0)
    assert np.all(o["history"][:, 1] == 88) and o["status"] == 0
    assert float(np.abs(O.apply(o["T"], pts[8:]) - c["truth"][8:]).max()) < 1e-9
    engine.upload([(c["v"], c["f"])])
    rec, hist = engine.register(pts, metric="plane", max_iter=8, reject=10.0, history=True)
    err = float(np.abs(O.apply(rec[0]["T"], pts[8:]) - c["truth"][8:]).max())
    print("rejection: pairs", hist[0, :, 1], "max |T p - truth| on the 88", err)
    assert np.all(hist[0, :, 1] == 88) and rec[0]["pairs"] == 88 and rec[0]["status"] == 0 and err < 1e-9
    against_oracle("rejection", rec[0], o, E, pts[8:])
    free = engine.register(pts, metric="plane", max_iter=8)
    assert free[0]["pairs"] == 96 and free[0]["T"].tobytes() != rec[0]["T"].tobytes() and free[0]["rms"] > 10.0


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_singular_and_starved(engine):
    """5: one face of the axis-aligned box under the plane metric (a pivot is exactly 0), five points, every pair rejected; and a
    humerus that fails between two proper neighbours"""
    v, f = O.box()
    good = O.apply(O.BOX_MOVE, O.box_points(64, seed=3))
    flat = O.box_points(64, seed=5)
    flat[:, 2] = 10.5
    T0 = O.rigid((0.0, 0.0, 1.0), 0.0, (0.5, 0.25, 0.0))
    engine.upload([(v, f)])
    for tag, kw, pairs in (("one face", dict(points=flat, T0=T0[None]), 64), ("five points", dict(points=good[:5]), 5),
                           ("all rejected", dict(points=good, reject=1e-30), 0)):
        rec, hist = engine.register(metric="plane", max_iter=4, history=True, **kw)
        r = rec[0]
        o = O.register(v, f, kw["points"], kw.get("T0", [None])[0], O.PLANE, 4, kw.get("reject", np.inf))
        assert r.tobytes() == O.record(o).tobytes() and hist[0].tobytes() == o["history"].tobytes(), tag
        assert r["status"] == O.GEOMETRY and r["iterations"] == 0 and r["converged"] == 0 and r["pairs"] == pairs and not hist[0, 1:].any(), tag
        assert np.array_equal(r["T"], kw.get("T0", np.identity(4)[None])[0]), tag
    assert engine.register(flat, T0=T0[None], metric="point", max_iter=4)[0]["status"] == 0      # Horn's form has no trouble with a plane
    engine.upload([(v, f)] * 3)
    proper = engine.register(np.stack([good, good, good]), metric="plane", max_iter=6)
    near_p = engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (3, 64))
    mixed = engine.register(np.stack([good, flat, good]), metric="plane", max_iter=6)
    near_m = engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (3, 64))
    assert mixed[1]["status"] == O.GEOMETRY and mixed[1]["iterations"] == 0 and not proper["status"].any()
    for b in (0, 2):
        assert mixed[b].tobytes() == proper[b].tobytes() == proper[1].tobytes() and near_m[b].tobytes() == near_p[b].tobytes()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_determinism(engine, cases):
    """6: a ragged batch of the four fixture bones and the box: every humerus alone against itself in the batch, a permuted batch,
    shared against per-humerus points, one humerus against 64 copies (another split of the walk): "icp.out" and "icp.near" as bytes"""
    meshes = [load(n) for n in NAMES] + [O.box()]
    Q = 300
    pts = cases["sub"]["pts"]

    def run(batch, points, **kw):
        engine.upload(batch)
        rec = engine.register(points, **kw)
        B = len(batch)
        assert engine.fetch("icp.out", _lib.REGISTRATION_DTYPE, (B,)).tobytes() == rec.tobytes()
        return rec, engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (B, Q))
    for kw in (dict(metric="plane", max_iter=5), dict(metric="point", max_iter=5, reject=25.0), dict(metric="plane", max_iter=8, tol=1e-3)):
        rec, near = run(meshes, pts, **kw)
        print("determinism", kw, "status", rec["status"], "iterations", rec["iterations"], "rms", rec["rms"])
        for b, mesh in enumerate(meshes):
            r1, n1 = run([mesh], pts, **kw)
            assert r1[0].tobytes() == rec[b].tobytes() and n1[0].tobytes() == near[b].tobytes(), (kw, b)
        perm = [3, 0, 4, 2, 1]
        rp, np_ = run([meshes[i] for i in perm], pts, **kw)
        rs, ns = run(meshes, np.stack([pts] * 5), **kw)                               # per-humerus copies of the shared points
        assert rs.tobytes() == rec.tobytes() and ns.tobytes() == near.tobytes()
        for j, i in enumerate(perm):
            assert rp[j].tobytes() == rec[i].tobytes() and np_[j].tobytes() == near[i].tobytes()
    sub = (cases["sub"]["v"], cases["sub"]["f"])
    kw = dict(metric="plane", max_iter=6)
    r1, n1 = run([sub], pts, **kw)
    r64, n64 = run([sub] * 64, pts, **kw)
    assert all(r64[b].tobytes() == r1[0].tobytes() and n64[b].tobytes() == n1[0].tobytes() for b in range(64))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_stopping(engine, cases):
    """7: tol = 1e-6 stops the plane case of test 2 early with converged = 1; the history is zero behind the stop; the returned rms is
    the last history row and the rms recomputed from "icp.near" and "icp.moved" by the tree; one humerus converges early while its
    neighbour does not, and neither changes the other"""
    c = cases["sub"]
    engine.upload([(c["v"], c["f"])])
    rec, hist = engine.register(c["pts"], metric="plane", max_iter=8, tol=1e-6, history=True)
    r, h = rec[0], hist[0]
    k = int(r["iterations"])
    print("stopping: iterations", k, "rms", h[:, 0])
    assert r["converged"] == 1 and r["status"] == 0 and 0 < k < 8
    assert not h[k + 1:].any() and h[:k + 1, 1].all() and r["rms"] == h[k, 0] and r["pairs"] == h[k, 1] and r["rms_first"] == h[0, 0]
    assert abs(h[k - 1, 0] - h[k, 0]) <= 1e-6 and all(abs(h[j - 1, 0] - h[j, 0]) > 1e-6 for j in range(1, k))
    o = O.register(c["v"], c["f"], c["pts"], None, O.PLANE, 8, tol=1e-6, closest=O.closest_culled)
    assert o["iterations"] == k and o["converged"] == 1
    near = engine.fetch("icp.near", _lib.CLOSEST_DTYPE, (1, 300))[0]
    moved = engine.fetch("icp.moved", np.float64, (1, 300, 3))[0]
    assert moved.tobytes() == O.map_points(r["T"].reshape(16), c["pts"]).tobytes()
    e = near["point"] - moved
    e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert np.float64(np.sqrt(O.tree_sum(e2) / 300.0)).tobytes() == r["rms"].tobytes() and not near["status"].any()
    full = engine.register(c["pts"], metric="plane", max_iter=8)                       # tol = 0 runs every iteration
    assert full[0]["iterations"] == 8 and full[0]["converged"] == 0
    # the aligned points converge at evaluation 1, their neighbour several evaluations later
    engine.upload([(c["v"], c["f"])] * 2)
    rec, hist = engine.register(np.stack([c["truth"], c["pts"]]), metric="plane", max_iter=8, tol=1e-6, history=True)
    assert rec[0]["converged"] == 1 and rec[0]["iterations"] == 1 and not hist[0, 2:].any()
    assert rec[1].tobytes() == r.tobytes() and hist[1].tobytes() == h.tobytes()
    swapped = engine.register(np.stack([c["pts"], c["truth"]]), metric="plane", max_iter=8, tol=1e-6)
    assert swapped[0].tobytes() == r.tobytes() and swapped[1].tobytes() == rec[0].tobytes()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_state_arguments_and_buffers(engine, humerus_mesh):
    """8"""
    v, f = humerus_mesh
    pts = v[:300].astype(np.float64) + (0.0, 0.0, 0.5)

    def refused(e, code, word, **kw):
        with pytest.raises(ShoulderHipError) as ex:
            e.register(**dict(dict(points=pts), **kw))
        assert ex.value.code == code and word in str(ex.value), str(ex.value)
    fresh = Engine(0)
    try:
        refused(fresh, -3, "no meshes")
    finally:
        fresh.close()
    engine.reset_params()
    engine.upload([(v, f)])
    refused(engine, -1, "Q", points=np.zeros((0, 3)))
    refused(engine, -1, "options", max_iter=0)
    refused(engine, -1, "options", max_iter=65)
    refused(engine, -1, "options", reject=0.0)
    refused(engine, -1, "options", tol=-1.0)
    bad = pts.copy()
    bad[7, 1] = np.nan
    refused(engine, -1, "point 7", points=bad)
    shear, mirror = np.identity(4)[None].copy(), np.identity(4)[None].copy()
    shear[0, 0, 1], mirror[0, 1, 1] = 1e-6, -1.0
    refused(engine, -1, "humerus 0", T0=shear)
    refused(engine, -1, "humerus 0", T0=mirror)
    refused(engine, -1, "point 7", points=bad, T0=shear)                              # the coordinates come first
    with pytest.raises(ValueError):
        engine.register(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError):
        engine.register(pts, metric="affine")
    # the records of a run, the buffers of the chain and the other queries' results are the same bytes before and after
    engine.run(_lib.STAGE_ALL)
    engine.resect(offsets=[dict(), dict(depth_canal_mm=-4.0)], fit=True, heads=[(24.0, 18.0), (22.0, 16.0)])
    engine.canal_profile(40.0, 4.0, 8, 16)
    stems = engine.resect_stems([(100.0, 6.0, 3.5)])
    c = v.astype(np.float64).mean(axis=0)
    engine.ray_cast(c[None] + np.zeros((3, 1)), np.eye(3), cap=4)
    engine.closest_points(pts)
    engine.winding_numbers(pts)
    names = ("landmarks", "resect.out", "resect.fit_out", "resect.seat_out", "stem.out", "canal.near", "canal.levels", "ray.hits", "ray.counts", "anp.ray_t",
             "verts_obb", "cp.out", "cp.part", "wn.out", "verts", "faces")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    got = engine.register(pts, metric="plane", max_iter=4, reject=5.0)
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before
    assert got[0]["status"] == 0 and got[0]["rms"] <= got[0]["rms_first"] <= 0.5 + 1e-6
    assert engine.resect_stems([(100.0, 6.0, 3.5)]).tobytes() == stems.tobytes()     # the chain's state is what it was
    assert engine.fetch("icp.out", _lib.REGISTRATION_DTYPE, (1,)).tobytes() == got.tobytes()
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        refused(engine, -3, "in flight")
    finally:
        engine.collect()
    assert engine.register(pts, metric="plane", max_iter=4, reject=5.0).tobytes() == got.tobytes()
    engine.store("verts", engine.fetch("verts", np.float32))                          # "icp.out" and "icp.near" answer for their batch
    for name in ("icp.out", "icp.near"):
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)
    assert engine.register(pts, metric="plane", max_iter=4, reject=5.0).tobytes() == got.tobytes()
    engine.upload([O.box()])
    for name in ("icp.out", "icp.near"):
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_facade(engine):
    """9: Humerus.register in the canal / transepicondylar system, held to the oracle run on the SAME CT points against the resident
    mesh: the returned matrix equals M_cur T_oracle M_cur^-1 as bytes (the facade conjugates the device's T, and the device's T is the
    oracle's), the info equals the oracle's record, and both undo a known rigid motion of every 32nd vertex of the bone to below
    1e-9 mm, the criterion of test 2, asserted on the oracle first.  d, how far those vertices lie from the resident float32 surface
    before anything is moved, is measured with closest_point and printed; it must itself be far below that criterion.  The same with
    initial= at the answer (T0 = M_cur^-1 initial M_cur).  mirror="x" on points reflected beforehand gives the same matrix, bytes.
    Then humerus_right, mirrored, onto humerus_left, each in its own system: status 0 and rms <= rms_first only -- whether the two
    fixtures are a pair is not known."""
    engine.reset_params()
    try:
        left = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        left.apply_csys_canal_transepiconylar()
        mv = np.asarray(left.mesh.vertices, np.float64)[::32]
        d = float(left.closest_point(mv)[1].max())
        K = O.rigid((2.0, -1.0, 1.5), 3.0, (1.0, -0.8, 0.6), about=mv.mean(axis=0))
        moved = O.apply(K, mv)
        p_ct, Mc = left._points_ct(moved)                                             # what the facade hands to the engine
        Mi = np.linalg.inv(Mc)
        nv, nf = len(left.mesh.vertices), len(left.mesh.faces)                        # (the buffers may be larger than the batch)
        rv, rf = engine.fetch("verts", np.float32, (nv, 3)), engine.fetch("faces", np.int32, (nf, 3))

        def held_to_oracle(tag, M, info, o):
            want = Mc @ o["T"] @ Mi
            err_o, err = float(np.abs(O.apply(want, moved) - mv).max()), float(np.abs(O.apply(M, moved) - mv).max())
            print(f"facade {tag}: d {d:.3e} oracle max |M K p - p| {err_o:.3e} device {err:.3e} max |M - M_oracle| {np.abs(M - want).max():.3e}", info)
            assert o["status"] == 0 and err_o < 1e-9                                  # the oracle first
            assert err < 1e-9 and M.tobytes() == want.tobytes()
            assert info == dict(rms=o["rms"], rms_first=o["rms_first"], pairs=o["pairs"], iterations=o["iterations"], converged=bool(o["converged"]),
                                min_pivot=o["min_pivot"])
        M, info = left.register(moved, max_iter=8)
        assert d < 1e-9 / 64.0
        held_to_oracle("identity start", M, info, O.register(rv, rf, p_ct, None, O.PLANE, 8, closest=O.closest_culled))
        assert info["pairs"] == len(mv) and info["rms"] < info["rms_first"] and M.shape == (4, 4) and np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0))
        flipped = moved * (-1.0, 1.0, 1.0)
        M2, info2 = left.register(flipped, mirror="x", max_iter=8)
        assert np.array_equal(M2, M) and info2 == info
        Ki = np.linalg.inv(K)
        Ki[3] = (0.0, 0.0, 0.0, 1.0)
        T0 = Mi @ Ki @ Mc                                                             # the start in CT, as the facade forms it
        T0[3] = (0.0, 0.0, 0.0, 1.0)
        M3, info3 = left.register(moved, initial=Ki, max_iter=2)                      # started at the answer: nothing left to do
        held_to_oracle("started at the answer", M3, info3, O.register(rv, rf, p_ct, T0, O.PLANE, 2, closest=O.closest_culled))
        assert info3["rms_first"] < 1e-9
        with pytest.raises(ValueError):
            left.register(moved[:5])                                                  # fewer than six pairs: the status is raised
        with pytest.raises(ValueError):
            left.register(moved, mirror="w")
        right = shoulder.Humerus(os.path.join(BONES, "humerus_right.stl"), engine=engine)
        right.apply_csys_canal_transepiconylar()
        rpts = np.asarray(right.mesh.vertices, np.float64)[::16]
        M, info = left.register(rpts, mirror="x", reject=25.0, max_iter=20)
        print("facade: humerus_right mirrored onto humerus_left:", info, "translation", M[:3, 3],
              "rotation angle (deg)", np.degrees(np.arccos(np.clip((np.trace(M[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))
        assert info["rms"] <= info["rms_first"] and info["pairs"] >= 6
    finally:
        engine.reset_params()
