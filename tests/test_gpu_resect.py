"""Batched head resection on the engine (include/shoulder_hip.h sh_resect_*, k_resect.h) against oracle/clip.py and
oracle/osteotomy.py: B resident humeri x P planes in one device pass, one measurement record per cut.

Bounds.  Device and oracle add the same float64 terms in a different order, so a sum of n terms t_i is held to
|got - want| <= 4 n 2^-53 sum|t_i| (both orders stay within n 2^-53 sum|t_i| of the exact sum, terms that carry a few ulp of
their own included).  head_height is a maximum of identical expressions: exact.  Ring points: 1e-9 mm (the slice layer's bound)."""
import os

import numpy as np
import pytest
import scipy.spatial

from conftest import BONES, engine_with_env
from oracle import clip, xform
from oracle.osteotomy import OracleOsteotomy
from shoulder_amd import _lib
from shoulder_amd.engine import ShoulderHipError
from shoulder_amd.stl import load_stl
from test_gpu_highres import subdivide
from test_gpu_osteotomy import oracle_for, same_plane
from test_oracle_clip import area, cube, volume_about

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
GRID27 = [dict(retroversion_deg=r, neckshaft_deg=n, depth_canal_mm=d) for r in (-10.0, 0.0, 10.0) for n in (-10.0, 0.0, 10.0) for d in (-6.0, 0.0, 6.0)]
FIVE = [GRID27[i] for i in (0, 7, 13, 20, 26)]


def _mesh(name):
    v, f = load_stl(os.path.join(BONES, name + ".stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def apply_offsets(O, off):
    if off.get("retroversion_deg"):
        O.offset_retroversion(off["retroversion_deg"])
    if off.get("neckshaft_deg"):
        O.offest_neckshaft(off["neckshaft_deg"])
    if off.get("depth_canal_mm"):
        O.offset_depth(off["depth_canal_mm"], "canal")
    return O


def oracle_planes(h, grid):
    """(P, 6) planes in CT of the oracle humerus for the offsets of `grid`"""
    out = []
    for off in grid:
        O, _ = oracle_for(h)
        out.append(np.concatenate(apply_offsets(O, off).plane(np.identity(4))))
    return np.array(out)


def similarity(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return rng.uniform(0.9, 1.1), q, rng.normal(size=3) * 30.0


def sim_mesh(v, sim):
    s, R, t = sim
    return np.ascontiguousarray((s * (v.astype(np.float64) @ R.T) + t).astype(np.float32))


def sim_planes(pl, sim):
    s, R, t = sim
    return np.concatenate([s * (pl[:, :3] @ R.T) + t, pl[:, 3:] @ R.T], axis=1)


def basis(n):
    un = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    u = np.cross(un, [1.0, 0.0, 0.0] if abs(un[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return u, np.cross(un, u)


def ring_terms(ring, o, n):
    """closed ring (k + 1, 3) -> shoelace terms about o in base.Section's basis, x / y sums of the centroid, segment lengths"""
    u, w = basis(n)
    d = ring - o
    x = (d[:, 0] * u[0] + d[:, 1] * u[1]) + d[:, 2] * u[2]
    y = (d[:, 0] * w[0] + d[:, 1] * w[1]) + d[:, 2] * w[2]
    cr = x[:-1] * y[1:] - x[1:] * y[:-1]
    e = np.diff(ring, axis=0)
    return cr, (x[:-1] + x[1:]) * cr, (y[:-1] + y[1:]) * cr, np.sqrt((e[:, 0] ** 2 + e[:, 1] ** 2) + e[:, 2] ** 2), u, w


def bound(t):
    return 4.0 * len(t) * EPS * np.abs(t).sum()


class OracleCut:
    """oracle/clip.py's cut of (v64, f) by the plane (o, n): the numbers a sh_resection holds, with their terms"""

    def __init__(self, v64, f, o, n):
        self.o, self.n = o, n
        ov, of, oe = clip.slice_plane(v64, f, o, n)
        t = ov[of] - o
        self.vol_t = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2]))
        tri = ov[of]
        cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        self.area_t = np.sqrt((cr[:, 0] ** 2 + cr[:, 1] ** 2) + cr[:, 2] ** 2)
        used = np.unique(f)
        dots = clip._dot3(v64[used] - o, n)
        self.height = max(0.0, float(dots.max())) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        self.n_cut, self.n_faces = len(oe), len(of)
        self.ov, self.of = ov, of
        try:
            self.loops = clip.loops_from_edges(oe)
        except ValueError:
            self.loops = None
        self.rings = []
        if self.loops:
            for lp in self.loops:
                r = ov[lp + lp[:1]]
                if ring_terms(r, o, n)[0].sum() < 0:
                    r = r[::-1]
                self.rings.append(r)
            self.best = int(np.argmax([abs(ring_terms(r, o, n)[0].sum()) for r in self.rings]))


def check_face_sums(rec, C):
    assert rec["n_cut_faces"] == C.n_cut
    assert abs(rec["head_volume"] - C.vol_t.sum() / 6.0) <= bound(C.vol_t) / 6.0, (rec["head_volume"], C.vol_t.sum() / 6.0, bound(C.vol_t) / 6.0)
    assert abs(rec["head_area"] - 0.5 * C.area_t.sum()) <= 0.5 * bound(C.area_t)
    assert rec["head_height"] == C.height


def cyclic_match(got, want, tol):
    """closed rings, same direction: every point of `got` within tol of `want` rotated onto its start"""
    assert np.array_equal(got[0], got[-1]) and len(got) == len(want)
    g, w = got[:-1], want[:-1]
    k = int(np.argmin(np.linalg.norm(w - g[0], axis=1)))
    return float(np.abs(np.roll(w, -k, axis=0) - g).max()) <= tol


def check_ring(e, b, p, rec, C, v64, f):
    assert rec["status"] == 0 and C.loops is not None
    assert rec["n_loops"] == len(C.loops) and rec["n_ring"] == len(C.rings[C.best]) - 1
    want = C.rings[C.best]
    got = e.resect_ring(b, p)
    assert got.shape == (rec["n_ring"] + 1, 3)
    assert cyclic_match(got, want, 1e-9)
    cr, sx, sy, seg, u, w = ring_terms(want, C.o, C.n)
    assert ring_terms(got, C.o, C.n)[0].sum() > 0                                   # counter-clockwise seen from the normal's tip
    assert abs(rec["cut_area"] - 0.5 * abs(cr.sum())) <= 0.5 * bound(cr)
    assert abs(rec["cut_perimeter"] - seg.sum()) <= bound(seg)
    tot = [ring_terms(r, C.o, C.n)[0] for r in C.rings]
    assert abs(rec["cap_area"] - 0.5 * abs(sum(t.sum() for t in tot))) <= 0.5 * sum(bound(t) for t in tot)
    A2 = cr.sum()
    cen, err = C.o.copy(), 0.0
    for s_, ax in ((sx, u), (sy, w)):
        c1 = s_.sum() / (3.0 * A2)
        e1 = bound(s_) / (3.0 * abs(A2)) + abs(s_.sum()) * bound(cr) / (3.0 * A2 * A2) + 8 * EPS * abs(c1)
        cen, err = cen + c1 * ax, err + e1
    assert np.abs(rec["cut_centroid"] - cen).max() <= err + 8 * EPS * np.abs(cen).max()
    # rule B-1: the ring starts on the mesh edge with the smallest (min vid, max vid) key among the edges it crosses
    d = clip._dot3(v64 - C.o, C.n)
    ed = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    ed = ed[(d[ed[:, 0]] < -1e-8) != (d[ed[:, 1]] < -1e-8)]
    ed = ed[(np.abs(d[ed[:, 0]]) > 1e-8) & (np.abs(d[ed[:, 1]]) > 1e-8)]
    tt = d[ed[:, 0]] / (d[ed[:, 0]] - d[ed[:, 1]])
    pts = v64[ed[:, 0]] + tt[:, None] * (v64[ed[:, 1]] - v64[ed[:, 0]])
    dist, idx = scipy.spatial.cKDTree(pts).query(got[:-1])
    assert dist.max() < 1e-7
    keys = ed[idx, 0].astype(np.int64) * len(v64) + ed[idx, 1]
    assert int(np.argmin(keys)) == 0


@pytest.fixture(scope="module")
def cohort(oracle_bones):
    """humerus_left, humerus_right and two seeded similarity copies of each, ragged and shuffled; per mesh the 27 planes"""
    meshes, planes = [], []
    for i, name in enumerate(("humerus_left", "humerus_right")):
        h = oracle_bones(name)
        v, f = np.ascontiguousarray(h.verts, np.float32), np.ascontiguousarray(h.faces, np.int32)
        pl = oracle_planes(h, GRID27)
        meshes.append((v, f)); planes.append(pl)
        for k in range(2):
            sim = similarity(10 * i + k + 1)
            meshes.append((sim_mesh(v, sim), f)); planes.append(sim_planes(pl, sim))
    order = [3, 0, 5, 1, 4, 2]
    return [meshes[i] for i in order], np.array([planes[i] for i in order])


@pytest.fixture(scope="module")
def cohort_records(engine, cohort):
    meshes, planes = cohort
    engine.upload(meshes)
    recs = engine.resect(planes=planes)
    rings = [[engine.resect_ring(b, p) for p in range(27)] for b in range(len(meshes))]
    return recs, rings


def test_explicit_planes_against_the_oracle(engine, cohort, cohort_records):
    meshes, planes = cohort
    engine.upload(meshes)
    recs = engine.resect(planes=planes)
    assert recs.shape == (6, 27) and recs.tobytes() == cohort_records[0].tobytes()
    assert np.all(recs["status"] == 0)                                              # no case may be skipped
    assert np.array_equal(recs["plane_point"], planes[:, :, :3]) and np.array_equal(recs["plane_normal"], planes[:, :, 3:])
    for b, (v, f) in enumerate(meshes):
        v64 = v.astype(np.float64)
        for p in range(27):
            C = OracleCut(v64, f, planes[b, p, :3], planes[b, p, 3:])
            check_face_sums(recs[b, p], C)
            check_ring(engine, b, p, recs[b, p], C, v64, f)


def test_reproducible_and_position_independent(engine, cohort, cohort_records):
    meshes, planes = cohort
    recs, rings = cohort_records
    B = len(meshes)
    engine.upload(meshes[::-1])
    rev = engine.resect(planes=planes[::-1])
    again = engine.resect(planes=planes[::-1])
    assert again.tobytes() == rev.tobytes()
    assert rev[::-1].tobytes() == recs.tobytes()
    for b in (0, B - 1):
        for p in (0, 13, 26):
            assert engine.resect_ring(B - 1 - b, p).tobytes() == rings[b][p].tobytes()
    for b in (1, 4):
        engine.upload([meshes[b]])
        alone = engine.resect(planes=planes[b:b + 1])
        assert alone[0].tobytes() == recs[b].tobytes()
        assert all(engine.resect_ring(0, p).tobytes() == rings[b][p].tobytes() for p in range(27))
        one = engine.resect(planes=planes[b:b + 1, 13:14])
        assert one[0, 0].tobytes() == recs[b, 13].tobytes()
        assert engine.resect_ring(0, 0).tobytes() == rings[b][13].tobytes()


@pytest.mark.parametrize("dtype", [_lib.UNET_F32, _lib.UNET_BF16])
def test_offsets_from_the_device_records(engine, oracle_bones, dtype):
    names = ("humerus_left", "humerus_right")
    engine.upload([_mesh(n) for n in names])
    engine.set_params(unet_dtype=dtype)
    try:
        lm = engine.run(_lib.STAGE_ALL)
        recs = engine.resect(offsets=GRID27)
    finally:
        engine.set_params(unet_dtype=_lib.UNET_F32)
    assert recs.shape == (2, 27) and np.all(recs["status"] == 0)
    arr = np.zeros(27, dtype=_lib.CUT_OFFSET_DTYPE)
    for i, g in enumerate(GRID27):
        for k, v in g.items():
            arr[k][i] = v
    assert engine.resect(offsets=arr).tobytes() == recs.tobytes()
    if dtype == _lib.UNET_F32:
        for b, name in enumerate(names):
            want = oracle_planes(oracle_bones(name), GRID27)
            for p in range(27):
                same_plane(type("P", (), dict(point=recs[b, p]["plane_point"], normal=recs[b, p]["plane_normal"])), (want[p, :3], want[p, 3:]))
            np.testing.assert_allclose(recs[b, 13]["plane_point"], lm[b]["anp_plane_point"], rtol=0, atol=1e-9)      # all-zero offsets: the native plane
            np.testing.assert_allclose(recs[b, 13]["plane_normal"], lm[b]["anp_plane_normal"], rtol=0, atol=1e-12)
    back = engine.resect(planes=np.concatenate([recs["plane_point"], recs["plane_normal"]], axis=2))
    assert back.tobytes() == recs.tobytes()


@pytest.mark.parametrize("name", ["humerus_left", "proximal_left_cut"])
def test_against_the_one_at_a_time_path(engine, name):
    """measure() against resect_mesh() / points() of the same object.  The clipped mesh's vertices went through the 8-decimal merge
    (<= 5e-9 mm per coordinate): bounded with the terms' gradients on top of the summation bound."""
    import shoulder_amd as shoulder
    cls = shoulder.Humerus if name == "humerus_left" else shoulder.ProximalHumerus
    hum = cls(os.path.join(BONES, name + ".stl"), engine=engine)
    ost = shoulder.HumeralHeadOsteotomy(hum)
    ost.offset_depth(2.0)
    ost.offest_neckshaft(4.0)
    m = ost.measure()
    assert m["status"] == 0
    head = ost.resect_mesh()[0]
    pts = ost.points()
    o = ost.plane.point
    hv, hf = head.vertices, head.faces
    t = hv[hf] - o
    vt = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2]))
    grad = sum(np.linalg.norm(np.cross(t[:, i], t[:, (i + 1) % 3]), axis=1).sum() for i in range(3))
    assert abs(m["head_volume"] - volume_about(hv, hf, o)) <= (bound(vt) + 5e-9 * np.sqrt(3.0) * grad) / 6.0
    tri = hv[hf]
    at = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    edges = sum(np.linalg.norm(tri[:, i] - tri[:, (i + 1) % 3], axis=1).sum() for i in range(3))
    assert abs(m["head_area"] - area(hv, hf)) <= 0.5 * bound(at) + 5e-9 * np.sqrt(3.0) * edges / 2.0
    per = np.linalg.norm(np.diff(pts, axis=0), axis=1).sum()
    assert m["cut_perimeter"] == pytest.approx(per, rel=1e-9)
    ring = engine.resect_ring(0, 0)
    assert len(ring) == len(pts) == m["n_ring"] + 1
    assert cyclic_match(ring, pts, 1e-8) or cyclic_match(ring, pts[::-1], 1e-8)


def test_degenerate_planes_on_a_cube(engine):
    v, f = cube()
    engine.upload([(v.astype(np.float32), f.astype(np.int32))])
    planes = np.array([[[0, 0, 0.5, 0, 0, 1], [0, 0, 0, 1, -1, 0], [0, 0, 2, 0, 0, 1], [0, 0, 1, 0, 0, 1], [0, 0, 1, 0, 0, -1]]], dtype=np.float64)
    recs = engine.resect(planes=planes)[0]
    cuts = [OracleCut(v, f, pl[:3].copy(), pl[3:].copy()) for pl in planes[0]]
    for r, C in zip(recs, cuts):
        assert r["n_cut_faces"] == C.n_cut and r["head_height"] == C.height
        assert abs(r["head_volume"] - C.vol_t.sum() / 6.0) <= 1e-15 and abs(r["head_area"] - 0.5 * C.area_t.sum()) <= 1e-15
        if C.loops is None:
            assert r["status"] == -5 and r["n_loops"] == 0 and r["n_ring"] == 0
        else:
            assert r["status"] == 0 and r["n_loops"] == len(C.loops)
    assert recs[0]["head_volume"] == 0.5 and recs[0]["n_ring"] == 8 and recs[0]["cut_area"] == 1.0 and recs[0]["n_loops"] == 1
    assert recs[0]["cut_perimeter"] == 4.0 and np.array_equal(recs[0]["cut_centroid"], [0.5, 0.5, 0.5])
    ring = engine.resect_ring(0, 0)
    assert ring.shape == (9, 3) and np.all(ring[:, 2] == 0.5) and cyclic_match(ring, cuts[0].rings[0], 0.0)
    assert abs(recs[1]["head_volume"] - 0.5) <= 1e-15
    z = recs[2]
    assert z["status"] == 0 and z["n_loops"] == 0 and z["n_cut_faces"] == 0 and z["head_volume"] == 0 and z["head_area"] == 0 and z["head_height"] == 0
    assert engine.resect_ring(0, 2).shape == (0, 3)
    assert cuts[3].n_faces == 0 and recs[3]["head_area"] == 0.0 and recs[3]["n_cut_faces"] == 0
    assert cuts[4].n_faces == 12 and recs[4]["head_area"] == 6.0 and recs[4]["n_cut_faces"] == 0


def check_dense(engine, b, p, rec, C, v64, f):
    """The section-size rule of the header: up to SH_MAXSEG = 1 024 crossing segments a cut gives its ring, above that it is
    SH_ERR_CAPACITY for exactly that cut (not joined through the overflow pool) with valid face sums.  -> 1 if over."""
    check_face_sums(rec, C)
    if C.n_cut > 1024:
        assert rec["status"] == -4 and rec["n_loops"] == 0 and rec["n_ring"] == 0 and rec["cut_area"] == 0
        assert engine.resect_ring(b, p).shape == (0, 3)
        return 1
    check_ring(engine, b, p, rec, C, v64, f)
    return 0


def test_dense_meshes(engine, oracle_bones):
    """130 k triangles beside the plain fixture, five offsets: as for the fixtures; 519 k triangles alone: the same.  On the CPU
    oracle the five sections of the 130 k mesh have 1 568, 568, 612, 1 451 and 512 segments (the fixture's: 250 .. 799), so
    two of its cuts and every cut of the 519 k mesh fall under the capacity rule (check_dense)."""
    h = oracle_bones("humerus_left")
    v0, f0 = np.ascontiguousarray(h.verts, np.float32), np.ascontiguousarray(h.faces, np.int32)
    v1, f1 = subdivide(v0, f0)
    v2, f2 = subdivide(v1, f1)
    pl = oracle_planes(h, FIVE)
    engine.upload([(v1, f1), (v0, f0)])
    recs = engine.resect(planes=np.array([pl, pl]))
    over = [0, 0]
    for b, (v, f) in enumerate(((v1, f1), (v0, f0))):
        v64 = v.astype(np.float64)
        for p in range(5):
            over[b] += check_dense(engine, b, p, recs[b, p], OracleCut(v64, f, pl[p, :3], pl[p, 3:]), v64, f)
    assert over == [2, 0]
    engine.upload([(v0, f0)])
    assert engine.resect(planes=pl[None])[0].tobytes() == recs[1].tobytes()      # beside a dense mesh or alone: equal bytes
    engine.upload([(v2, f2)])
    recs = engine.resect(planes=pl[None])
    v64 = v2.astype(np.float64)
    assert sum(check_dense(engine, 0, p, recs[0, p], OracleCut(v64, f2, pl[p, :3], pl[p, 3:]), v64, f2) for p in range(5)) > 0


def test_a_hole_on_the_head(engine, cohort, cohort_records):
    """One triangle that the native plane cuts removed from humerus_left: cuts through the hole are SH_ERR_GEOMETRY with the
    oracle's face sums on that mesh, cuts that miss it are unaffected, the other humeri byte-equal."""
    meshes, planes = cohort
    b = 1                                                                         # the plain humerus_left of the cohort
    v, f = meshes[b]
    v64 = v.astype(np.float64)
    d = clip._dot3(v64 - planes[b, 13, :3], planes[b, 13, 3:])
    s = np.sign(d)[f]
    hole = int(np.nonzero((s.min(axis=1) < 0) & (s.max(axis=1) > 0))[0][0])
    fh = np.ascontiguousarray(np.delete(f, hole, axis=0))
    batch = list(meshes)
    batch[b] = (v, fh)
    engine.upload(batch)
    recs = engine.resect(planes=planes)
    kinds = set()
    for p in range(27):
        C = OracleCut(v64, fh, planes[b, p, :3], planes[b, p, 3:])
        check_face_sums(recs[b, p], C)
        kinds.add(C.loops is None)
        if C.loops is None:
            assert recs[b, p]["status"] == -5 and recs[b, p]["n_loops"] == 0
        else:
            # (the face sums run over other tiles now; the section is the intact mesh's: same ring, same ring numbers)
            assert recs[b, p]["status"] == 0 and engine.resect_ring(b, p).tobytes() == cohort_records[1][b][p].tobytes()
            for k in ("cut_area", "cut_perimeter", "cut_centroid", "cap_area", "n_loops", "n_ring", "n_cut_faces", "head_height"):
                assert np.array_equal(recs[b, p][k], cohort_records[0][b, p][k])
    assert kinds == {True, False}
    others = [i for i in range(len(meshes)) if i != b]
    assert recs[others].tobytes() == cohort_records[0][others].tobytes()


def test_errors(oracle_bones):
    h = oracle_bones("humerus_left")
    good = (np.ascontiguousarray(h.verts, np.float32), np.ascontiguousarray(h.faces, np.int32))
    one = [dict(depth_canal_mm=2.0)]
    with engine_with_env() as e:
        e.upload([good, good])
        for call in (lambda: e.resect(offsets=one), lambda: e.resect_ring(0, 0)):
            with pytest.raises(ShoulderHipError) as ex:
                call()
            assert ex.value.code == -3                                            # no run / no resection yet
        e.run(_lib.STAGE_OBB | _lib.STAGE_FULL)
        with pytest.raises(ShoulderHipError) as ex:
            e.resect(offsets=one)
        assert ex.value.code == -3
        e.run(_lib.STAGE_ALL)
        ref = e.resect(offsets=one)
        e.submit(_lib.STAGE_ALL)
        for call in (lambda: e.resect(offsets=one), lambda: e.resect(planes=np.ones((2, 1, 6))), lambda: e.resect_ring(0, 0)):
            with pytest.raises(ShoulderHipError) as ex:
                call()
            assert ex.value.code == -3
        e.collect()
        for bad in (np.array([0, 0, 0, 0, 0, 0.0]), np.array([0, 0, 0, np.nan, 0, 1.0]), np.array([np.inf, 0, 0, 0, 0, 1.0])):
            pl = np.ones((2, 1, 6))
            pl[1, 0] = bad
            with pytest.raises(ShoulderHipError) as ex:
                e.resect(planes=pl)
            assert ex.value.code == -1
        with pytest.raises(ValueError):
            e.resect()
        with pytest.raises(ShoulderHipError) as ex:
            e.resect(offsets=[{}] * 4097)
        assert ex.value.code == -1
        # a humerus whose record failed carries its status into its cuts; the other one is untouched
        zc = h.verts[:, 2][h.faces].mean(axis=1)
        keep = ~((zc > np.percentile(zc, 45)) & (zc < np.percentile(zc, 47)) & (h.verts[:, 0][h.faces].mean(axis=1) > np.median(h.verts[:, 0])))
        e.upload([(good[0], np.ascontiguousarray(good[1][keep])), good])
        with pytest.raises(ShoulderHipError) as ex:
            e.resect(offsets=one)                                                 # a new batch: its run is missing
        assert ex.value.code == -3
        lm = e.run(_lib.STAGE_ALL, strict=False)
        assert lm["status"][0] == -5 and lm["status"][1] == 0
        recs = e.resect(offsets=one)
        assert recs[0, 0]["status"] == -5 and recs[0, 0]["head_volume"] == 0 and recs[0, 0]["n_cut_faces"] == 0
        assert recs[1].tobytes() == ref[1].tobytes()
        assert e.resect_ring(0, 0).shape == (0, 3) and len(e.resect_ring(1, 0)) == ref[1, 0]["n_ring"] + 1
