"""Open contours, the general rule on the device: patch holes of several adjacent triangles (bridges that are not a missing
segment, several chains per plane competing for the same heads) against the NumPy restatement of the rule
(test_open_contours_rule.bridge_loops) on the oracle's sections, in the small, large and overflow join tiers; and an open sheet
inside the canal whose chains are dropped while the bone's loops survive (max_gap = 0: the oracle's drop rule)."""
import os

import numpy as np
import pytest

from conftest import BONES, engine_with_env
from oracle.section import ZSlicer
from shoulder_amd import _lib
from shoulder_amd.engine import ShoulderHipError
from shoulder_amd.stl import load_stl
from test_gpu_highres import subdivide
from test_open_contours_rule import bridge_loops

pytestmark = pytest.mark.gpu

SLICES = _lib.STAGE_OBB | _lib.STAGE_FULL | _lib.STAGE_NECK | _lib.STAGE_CANAL | _lib.STAGE_PROXIMAL | _lib.STAGE_DISTAL
PATCH_GAP = 8.0      # mm: wider than a patch hole of the fixture (two vertex fans a few edges apart)


def _humerus_left(level):
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    for _ in range(level):
        v, f = subdivide(v, f)
    return v, f


def _patch(v, f, vobb, z, side, avoid):
    """The faces around two vertices near height z (box frame) on one side of the bone, a few edge lengths apart: a hole of
    several adjacent triangles whose planes fall into two chains, with a strip of surface between the two fans."""
    e = np.linalg.norm(v[f] - v[np.roll(f, -1, axis=1)], axis=2)
    med = float(np.median(e))
    near = np.flatnonzero(np.abs(vobb[:, 2] - z) < 0.5 * med)
    if len(avoid):
        near = np.array([i for i in near if np.min(np.linalg.norm(avoid - v[i], axis=1)) > 5.0])
    v1 = near[np.argmax(side * vobb[near, 0])]
    fan1 = np.flatnonzero((f == v1).any(axis=1))
    ring1 = np.unique(f[fan1])
    cand = near[~np.isin(near, ring1)]
    d = np.linalg.norm(vobb[cand] - vobb[v1], axis=1)
    cand, d = cand[d > 2.5 * med], d[d > 2.5 * med]
    v2 = cand[np.argmin(d)]
    fan2 = np.flatnonzero((f == v2).any(axis=1))
    return np.union1d(fan1, fan2)


def _expected(vobb, f, z, gap):
    sk, ek, sp, ep = ZSlicer(vobb, f).segments(z)
    loops, bridged, dropped = bridge_loops([int(k) for k in sk], [int(k) for k in ek], sp, ep, gap)
    return loops, bridged, dropped


def _ring_of(loops):
    """The largest loop (slice.py:53-59), CCW from the same start, closed -- oracle/section.py's orientation rule."""
    areas = []
    for _, pts in loops:
        x, y = pts[:, 0], pts[:, 1]
        areas.append(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    pts = loops[int(np.argmax(np.abs(areas)))][1]
    if areas[int(np.argmax(np.abs(areas)))] < 0:
        pts = np.r_[pts[:1], pts[1:][::-1]]
    return np.r_[pts, pts[:1]]


@pytest.mark.parametrize("level", [0, 1, 2], ids=["small_tier", "large_tier", "overflow_tier"])
def test_patch_holes_match_the_restated_rule(level):
    v, f = _humerus_left(level)
    with engine_with_env() as e:
        e.upload([(v, f)])
        e.run(SLICES, fetch=False)
        vobb = e.fetch("verts_obb", np.float64).reshape(-1, 3)
        zp, zd = e.fetch("prox.zeff", np.float64), e.fetch("distal.zeff", np.float64)
        patch = np.union1d(_patch(v, f, vobb, zp[560], +1, []), _patch(v, f, vobb, zd[100], -1, []))
        fh = np.delete(f, patch, axis=0)
        e.set_open_contours("bridge", PATCH_GAP)
        e.upload([(v, fh)])
        e.run(SLICES, fetch=False)
        bridged, dropped = e.open_contour_stats()
        assert bridged[0] > 0
        assert np.array_equal(e.fetch("verts_obb", np.float64).reshape(-1, 3), vobb)
        pz = vobb[f[patch], 2]
        most_chains, checked = 0, 0
        for s in ("prox", "distal"):
            zs = e.fetch(s + ".zeff", np.float64)
            cnt = e.fetch(s + ".seg_count", np.int32)
            nloops = e.fetch(s + ".nloops", np.int32)
            cen = e.fetch(s + ".centroids", np.float64).reshape(-1, 2)
            through = [k for k in range(len(zs)) if pz.min() < zs[k] < pz.max()]
            assert through, s
            for k in through:
                loops, br, dr = _expected(vobb, fh, zs[k], PATCH_GAP)
                most_chains = max(most_chains, br + dr)
                assert int(nloops[k]) == len(loops), (s, k)
                allp = np.concatenate([p for _, p in loops])
                assert cen[k].tobytes() == (0.5 * (allp.min(axis=0) + allp.max(axis=0))).tobytes(), (s, k)
                got = e.ring(s, 0, k)
                exp = _ring_of(loops)
                assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), (s, k, got.shape, exp.shape)
                checked += 1
            if level == 1:
                assert cnt.max() > 384      # (planes of the large tier exist)
            if level == 2:
                assert cnt.max() > 1024     # (overflow planes exist)
        assert checked >= 4 and most_chains >= 2      # planes where several chains compete for the heads


# measured on the MI355X (humerus_left, both patches, bridge mode, f32 UNet): canal / TE / groove axes 0,
# anatomic-neck central 1.3e-4 mm, normal 1.1e-3 mm, neck-shaft 2.1e-3 deg, retroversion 2.6e-4 deg -- bounds about 4x that
LANDMARK_BOUNDS_MM = {"canal_axis": 1e-6, "te_axis": 1e-6, "groove_axis": 1e-6, "anp_axis_central": 5e-4, "anp_axis_normal": 5e-3}
ANGLE_BOUNDS_DEG = {"neckshaft": 1e-2, "retroversion": 1e-3}


def test_patch_holes_keep_the_landmarks_near_the_intact_ones():
    v, f = _humerus_left(0)
    with engine_with_env() as e:
        e.upload([(v, f)])
        intact = e.run(_lib.STAGE_ALL)
        vobb = e.fetch("verts_obb", np.float64).reshape(-1, 3)
        zp, zd = e.fetch("prox.zeff", np.float64), e.fetch("distal.zeff", np.float64)
        anp = np.array(intact[0]["anp_points"][: int(intact[0]["n_anp"])], dtype=np.float64)
        patch = np.union1d(_patch(v, f, vobb, zp[560], +1, anp), _patch(v, f, vobb, zd[100], -1, anp))
        e.set_open_contours("bridge", PATCH_GAP)
        e.upload([(v, np.delete(f, patch, axis=0))])
        got = e.run(_lib.STAGE_ALL)
        diffs = {k: float(np.abs(got[k] - intact[k]).max()) for k in list(LANDMARK_BOUNDS_MM) + list(ANGLE_BOUNDS_DEG)}
        print("patch-hole landmark differences:", diffs)
        for k, bound in {**LANDMARK_BOUNDS_MM, **ANGLE_BOUNDS_DEG}.items():
            assert diffs[k] <= bound, (k, diffs[k])


def _sheet(a, b, r=1.5, ns=30, nu=5):
    """A quarter-cylinder strip of radius r around the segment a-b: an open surface inside the bone."""
    ax = (b - a) / np.linalg.norm(b - a)
    e1 = np.cross(ax, [1.0, 0.0, 0.0] if abs(ax[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(ax, e1)
    s = np.linspace(0.1, 0.9, ns)
    u = np.linspace(0.0, 0.5 * np.pi, nu)
    P = a + s[:, None, None] * (b - a) + r * (np.cos(u)[None, :, None] * e1 + np.sin(u)[None, :, None] * e2)
    idx = np.arange(ns * nu).reshape(ns, nu)
    q0, q1, q2, q3 = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.c_[q0, q1, q2], np.c_[q0, q2, q3]])
    return P.reshape(-1, 3).astype(np.float32), faces.astype(np.int32)


def _np_open_edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return int(np.count_nonzero(cnt != 2))


def test_open_sheet_in_the_canal_is_dropped_and_the_records_stay():
    v, f = _humerus_left(0)
    with engine_with_env() as e:
        e.upload([(v, f)])
        intact = e.run(_lib.STAGE_ALL)
        ca = np.array(intact[0]["canal_axis"], dtype=np.float64)
        sv, sf = _sheet(ca[0], ca[1])
        vs = np.concatenate([v, sv])
        fs = np.concatenate([f, sf + len(v)])
        e.upload([(vs, fs)])
        assert e.open_edges().tolist() == [_np_open_edges(fs)] and _np_open_edges(fs) > 0
        with pytest.raises(ShoulderHipError) as ex:      # the default mode: the sheet's open chains fail the humerus
            e.run(_lib.STAGE_ALL)
        assert ex.value.code == -5
        e.set_open_contours("bridge", 0.0)
        got = e.run(_lib.STAGE_ALL)
        bridged, dropped = e.open_contour_stats()
        assert bridged[0] == 0 and dropped[0] > 0
        for name in intact.dtype.names:
            assert intact[name].tobytes() == got[name].tobytes(), name
