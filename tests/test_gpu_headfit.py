"""Head fit of the cuts of a batched resection (include/shoulder_hip.h sh_head_fit, k_headfit.h) on the engine against the
lstsq / eigh oracle of tests/headfit_oracle.py.

Bounds.  Moments: the project's sum bound 4 n 2^-53 sum |t| (tests/test_gpu_resect.py).  Centre, radius, rms and semi-axes against
the oracle: 1e-6 mm (the level the landmarks agree with their oracle at); center_articular against the ORACLE's csys: 1e-4 mm, the
landmark budget (the two csys matrices are different computations of the same landmarks)."""
import os

import numpy as np
import pytest

import headfit_oracle as H
from conftest import BONES, engine_with_env
from shoulder_amd import _lib
from shoulder_amd.engine import ShoulderHipError
from shoulder_amd.stl import load_stl
from test_gpu_osteotomy import oracle_for
from test_gpu_resect import FIVE, sim_mesh, similarity
from test_oracle_clip import cube

pytestmark = pytest.mark.gpu
MM = 1e-6
CUBE_PLANES = np.array([[[0, 0, 0.5, 0, 0, 1], [0, 0, 0, 1, -1, 0], [0, 0, 2, 0, 0, 1], [0, 0, 1, 0, 0, 1], [0, 0, 1, 0, 0, -1]]], dtype=np.float64)
SPHERE_FIELDS = ("sphere_center", "sphere_radius", "sphere_rms", "cap_height", "fit_area")
RING_FIELDS = ("cut_semi_major", "cut_semi_minor", "cut_major_dir")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return H.build_shim(tmp_path_factory.mktemp("headfit_check"))


def cube_mesh():
    v, f = cube()
    return v.astype(np.float32), f.astype(np.int32)


def moments_of(engine, B, P):
    return engine.fetch("resect.fit_moments", np.float64, (B, P, 16))


def check_against_oracle(fit, mom, O, o, n):
    """one cut with a sphere and a ring against its OracleFit; -> largest centre / radius difference"""
    assert fit["sphere_status"] == 0 and fit["ring_status"] == 0
    assert np.all(np.abs(mom[:14] - O.moments[:14]) <= H.sum_bound(O.terms)) and not mom[14:].any()
    assert fit["fit_area"] == mom[0]
    dc, dr = np.abs(fit["sphere_center"] - O.center).max(), abs(fit["sphere_radius"] - O.radius)
    print("centre", dc, "radius", dr, "rms", abs(fit["sphere_rms"] - O.rms), "cap", abs(fit["cap_height"] - O.cap_height))
    assert dc <= MM and dr <= MM and abs(fit["sphere_rms"] - O.rms) <= MM and abs(fit["cap_height"] - O.cap_height) <= 2 * MM
    a, b, d3 = O.ellipse
    assert abs(fit["cut_semi_major"] - a) <= MM and abs(fit["cut_semi_minor"] - b) <= MM
    g = fit["cut_major_dir"]
    assert abs(np.linalg.norm(g) - 1.0) <= 1e-12 and g[np.nonzero(g)[0][0]] > 0
    # (the direction is conditioned by the gap between the axes: the semi-axis bound over the relative gap)
    assert min(np.abs(g - d3).max(), np.abs(g + d3).max()) <= MM * a / max(a - b, MM * a)
    return max(dc, dr)


def test_cube(engine):
    v, f = cube_mesh()
    engine.upload([(v, f)])
    plain = engine.resect(planes=CUBE_PLANES)
    recs, fits = engine.resect(planes=CUBE_PLANES, fit=True)
    assert recs.tobytes() == plain.tobytes() and fits.shape == (1, 5)
    mom = moments_of(engine, 1, 5)[0]
    v64 = v.astype(np.float64)
    for p in range(5):
        O = H.OracleFit(v64, f, CUBE_PLANES[0, p, :3].copy(), CUBE_PLANES[0, p, 3:].copy())
        assert np.all(np.abs(mom[p][:14] - O.moments[:14]) <= H.sum_bound(O.terms)) and not mom[p][14:].any()
        assert fits[0, p]["ring_status"] == recs[0, p]["status"]
    for p in (2, 3):                                                                  # nothing on the normal's side
        assert fits[0, p]["sphere_status"] == 0 and not mom[p].any()
        assert all(not np.any(fits[0, p][k]) for k in SPHERE_FIELDS + RING_FIELDS)
    z = fits[0, 0]
    assert abs(z["cut_semi_major"] - 2 * np.sqrt(1 / 12)) <= 1e-15 and abs(z["cut_semi_minor"] - 2 * np.sqrt(1 / 12)) <= 1e-15
    # closed form: area 1 + 4 x 0.5; vertex lumping integrates linear functions exactly: S1 = integral of q over the surface
    tb = H.sum_bound(H.OracleFit(v64, f, CUBE_PLANES[0, 0, :3].copy(), CUBE_PLANES[0, 0, 3:].copy()).terms)
    assert abs(mom[0][0] - 3.0) <= tb[0] and np.all(np.abs(mom[0][1:4] - [1.5, 1.5, 1.0]) <= tb[1:4])
    assert z["sphere_status"] == 0 and z["fit_area"] == mom[0][0] and z["sphere_radius"] > 0
    assert np.all(np.isnan(fits["center_articular"]))                                 # no run: no canal frame
    assert fits[0, 4]["sphere_status"] == 0 and abs(fits[0, 4]["fit_area"] - 6.0) <= 1e-14
    assert np.abs(fits[0, 4]["sphere_center"] - 0.5).max() <= 1e-12                   # the whole cube: the sphere through its corners
    assert abs(fits[0, 4]["sphere_radius"] - np.sqrt(0.75)) <= 1e-12


def test_flat_sheet(engine):
    """a flat 2 x 1 sheet cut across (four triangles: an upload takes no mesh of fewer than four faces; the cut goes through two)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 1, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32)
    f = np.array([[0, 1, 4], [0, 4, 5], [1, 2, 3], [1, 3, 4]], dtype=np.int32)
    engine.upload([(v, f), cube_mesh()])
    pl = np.array([[[1.5, 0, 0, 1, 0, 0]], [[0, 0, 0.5, 0, 0, 1]]], dtype=np.float64)
    recs, fits = engine.resect(planes=pl, fit=True)
    assert recs[0, 0]["status"] == -5 and fits[0, 0]["sphere_status"] == -5 and fits[0, 0]["ring_status"] == -5
    assert all(not np.any(fits[0, 0][k]) for k in SPHERE_FIELDS[:4] + RING_FIELDS) and abs(fits[0, 0]["fit_area"] - 0.5) <= 1e-14 and recs[0, 0]["n_cut_faces"] == 2
    assert recs[1, 0]["status"] == 0 and fits[1, 0]["sphere_status"] == 0 and fits[1, 0]["cut_semi_major"] > 0


def ico_planes(c):
    return np.array([[c[0], c[1], c[2] + 5.0, 0, 0, 1], [c[0] + 2.0, c[1], c[2] - 3.0, 0.3, -0.2, 1.0], [c[0], c[1] - 1.0, c[2] + 11.0, -0.5, 0.4, 2.0]], dtype=np.float64)


@pytest.mark.parametrize("split", [False, True])
def test_icosphere_beside_the_cube(engine, split):
    ctr = np.array([30.0, -40.0, 55.0])
    v, f = H.icosphere(3, 20.0, ctr)
    assert len(f) == 1280
    pl = ico_planes(ctr)
    v64 = v.astype(np.float64)
    if split:                                                                         # one face of the kept side in two: 1 281 faces, a partial sixth tile
        d = (v64[f].mean(axis=1) - pl[0, :3]) @ pl[0, 3:]
        k = int(np.argmax(d))
        a, b, c = f[k]
        m = ((v64[a] + v64[b]) / 2).astype(np.float32)
        v = np.concatenate([v, m[None]])
        f = np.concatenate([f[:k], [[a, len(v) - 1, c]], f[k + 1:], [[len(v) - 1, b, c]]]).astype(np.int32)
        v64 = v.astype(np.float64)
        assert len(f) == 1281
    engine.upload([cube_mesh(), (v, f)])
    planes = np.array([np.repeat(CUBE_PLANES[0, :1], 3, axis=0), pl])
    recs, fits = engine.resect(planes=planes, fit=True)
    assert recs.tobytes() == engine.resect(planes=planes).tobytes()
    mom = moments_of(engine, 2, 3)
    e = np.linalg.norm(v64[f] - v64[np.roll(f, 1, axis=1)], axis=2).max()
    for p in range(3):
        O = H.OracleFit(v64, f, pl[p, :3].copy(), pl[p, 3:].copy())
        check_against_oracle(fits[1, p], mom[1, p], O, pl[p, :3], pl[p, 3:])
        assert abs(fits[1, p]["sphere_radius"] - 20.0) < e * e / (8 * 20.0)
    engine.upload([(v, f)])
    alone = engine.resect(planes=pl[None], fit=True)[1]
    assert alone[0].tobytes() == fits[1].tobytes()


@pytest.fixture(scope="module")
def humeri(engine, oracle_bones):
    h = oracle_bones("humerus_left")
    v, f = np.ascontiguousarray(h.verts, np.float32), np.ascontiguousarray(h.faces, np.int32)
    meshes = [(v, f), (sim_mesh(v, similarity(3)), f)]
    engine.upload(meshes)
    lm = engine.run(_lib.STAGE_ALL)
    recs, fits = engine.resect(offsets=FIVE, fit=True)
    return h, meshes, lm.copy(), recs, fits, moments_of(engine, 2, 5)


def test_humerus_against_the_oracle(engine, humeri):
    h, meshes, lm, recs, fits, mom = humeri
    assert np.all(recs["status"] == 0) and np.all(fits["sphere_status"] == 0) and np.all(fits["ring_status"] == 0)
    T_oracle = oracle_for(h)[1]["csys_articular"]
    worst = 0.0
    for b, (v, f) in enumerate(meshes):
        v64 = v.astype(np.float64)
        for p in range(5):
            o, n = recs[b, p]["plane_point"].copy(), recs[b, p]["plane_normal"].copy()
            O = H.OracleFit(v64, f, o, n, csys=lm[b]["csys_articular"])
            worst = max(worst, check_against_oracle(fits[b, p], mom[b, p], O, o, n))
            assert np.abs(fits[b, p]["center_articular"] - O.center_articular).max() <= 2 * MM      # (a rotation of a difference <= MM per coordinate)
            if b == 0:
                want = T_oracle[:3, :3] @ O.center + T_oracle[:3, 3]
                assert np.abs(fits[b, p]["center_articular"] - want).max() <= 1e-4
    print("largest centre / radius difference to the oracle:", worst)
    print("sphere_radius of the native cut:", fits[0, 1]["sphere_radius"], "radius_curvature of the record:", lm[0]["radius_curvature"])


def test_humerus_bytes_do_not_depend_on_the_batch(engine, humeri):
    h, meshes, lm, recs, fits, mom = humeri
    engine.upload(meshes)
    engine.run(_lib.STAGE_ALL)
    r2, f2 = engine.resect(offsets=FIVE, fit=True)
    assert r2.tobytes() == recs.tobytes() and f2.tobytes() == fits.tobytes()
    assert r2.tobytes() == engine.resect(offsets=FIVE).tobytes()
    one = engine.resect(offsets=FIVE[2:3], fit=True)[1]
    assert one[:, 0].tobytes() == fits[:, 2].tobytes()                                # P = 1 against P = 5
    planes = np.concatenate([recs["plane_point"], recs["plane_normal"]], axis=2)
    back = engine.resect(planes=planes, fit=True)
    assert back[0].tobytes() == recs.tobytes() and back[1].tobytes() == fits.tobytes()
    engine.upload(meshes[::-1])                                                       # reversed; no run: every field but the canal-frame centre
    rev = engine.resect(planes=planes[::-1], fit=True)[1][::-1]
    assert np.all(np.isnan(rev["center_articular"]))
    for k in fits.dtype.names:
        if k != "center_articular":
            assert rev[k].tobytes() == fits[k].tobytes(), k
    assert moments_of(engine, 2, 5)[::-1].tobytes() == mom.tobytes()
    engine.upload(meshes[1:])                                                         # alone
    alone = engine.resect(planes=planes[1:], fit=True)[1]
    for k in fits.dtype.names:
        if k != "center_articular":
            assert alone[0][k].tobytes() == fits[1][k].tobytes(), k


def test_device_solve_against_the_host_compiled_source(shim, humeri):
    """the fetched moments through the host instantiation of head_sphere_from_moments: the record's centre and radius, bit for bit"""
    h, meshes, lm, recs, fits, mom = humeri
    for b in range(2):
        for p in range(5):
            rc, c, r, rms = H.host_sphere(shim, mom[b, p])
            assert rc == 0 and r == fits[b, p]["sphere_radius"] and rms == fits[b, p]["sphere_rms"]
            assert np.array_equal(recs[b, p]["plane_point"] + c, fits[b, p]["sphere_center"])


def test_errors_and_states(oracle_bones):
    h = oracle_bones("humerus_left")
    good = (np.ascontiguousarray(h.verts, np.float32), np.ascontiguousarray(h.faces, np.int32))
    one = [dict(depth_canal_mm=2.0)]
    with engine_with_env() as e:
        e.upload([good, good])
        with pytest.raises(ShoulderHipError) as ex:
            e.resect(offsets=one, fit=True)
        assert ex.value.code == -3                                                    # no run yet
        pl = np.tile(np.concatenate([good[0].mean(axis=0), [0, 0, 1.0]]), (2, 1, 1))
        recs, fits = e.resect(planes=pl, fit=True)                                    # plane mode needs none: everything but the canal frame
        assert np.all(np.isnan(fits["center_articular"])) and np.all(fits["sphere_status"] == 0) and np.all(fits["ring_status"] == recs["status"])
        assert np.all(fits["sphere_radius"] > 0) and fits[0].tobytes() == fits[1].tobytes()
        e.run(_lib.STAGE_OBB | _lib.STAGE_FULL)
        with pytest.raises(ShoulderHipError) as ex:
            e.resect(offsets=one, fit=True)
        assert ex.value.code == -3
        e.run(_lib.STAGE_ALL)
        ref = e.resect(offsets=one, fit=True)
        assert np.all(np.isfinite(ref[1]["center_articular"]))
        e.submit(_lib.STAGE_ALL)
        for call in (lambda: e.resect(offsets=one, fit=True), lambda: e.resect(planes=np.ones((2, 1, 6)), fit=True)):
            with pytest.raises(ShoulderHipError) as ex:
                call()
            assert ex.value.code == -3
        e.collect()
        for bad in (np.array([0, 0, 0, 0, 0, 0.0]), np.array([0, 0, 0, np.nan, 0, 1.0]), np.array([np.inf, 0, 0, 0, 0, 1.0])):
            pl = np.ones((2, 1, 6))
            pl[1, 0] = bad
            with pytest.raises(ShoulderHipError) as ex:
                e.resect(planes=pl, fit=True)
            assert ex.value.code == -1
        with pytest.raises(ShoulderHipError) as ex:
            e.resect(offsets=[{}] * 4097, fit=True)
        assert ex.value.code == -1
        zc = h.verts[:, 2][h.faces].mean(axis=1)
        keep = ~((zc > np.percentile(zc, 45)) & (zc < np.percentile(zc, 47)) & (h.verts[:, 0][h.faces].mean(axis=1) > np.median(h.verts[:, 0])))
        e.upload([(good[0], np.ascontiguousarray(good[1][keep])), good])
        lm = e.run(_lib.STAGE_ALL, strict=False)
        assert lm["status"][0] == -5 and lm["status"][1] == 0
        recs, fits = e.resect(offsets=one, fit=True)
        assert fits[0, 0]["sphere_status"] == -5 and fits[0, 0]["ring_status"] == -5 and fits[0, 0]["sphere_radius"] == 0 and fits[0, 0]["fit_area"] == 0
        assert recs[1].tobytes() == ref[0][1].tobytes() and fits[1].tobytes() == ref[1][1].tobytes()


def test_a_sweep_of_more_than_one_pass(engine):
    """two cubes, P = 2 049: 4 098 cuts, one more than a fitted pass takes for B = 2 (4 096 / B planes); cut by cut the single-pass records"""
    engine.upload([cube_mesh(), cube_mesh()])
    P = 2049
    z = np.linspace(0.05, 0.95, P)
    pl = np.zeros((2, P, 6))
    pl[:, :, 2], pl[:, :, 5], pl[:, :, 3] = z, 1.0, np.linspace(-0.04, 0.04, P)
    recs, fits = engine.resect(planes=pl, fit=True)
    assert recs.tobytes() == engine.resect(planes=pl).tobytes() and np.all(fits["sphere_status"] == 0) and np.all(recs["status"] == 0)
    for lo in (0, 1024, 2047):                                                        # windows on both sides of the split at plane 2 048
        r1, f1 = engine.resect(planes=np.ascontiguousarray(pl[:, lo:lo + 2]), fit=True)
        assert r1.tobytes() == recs[:, lo:lo + 2].tobytes() and f1.tobytes() == fits[:, lo:lo + 2].tobytes()
