"""The slice join (k_slice_link, k_slices.h) against oracle.slices.Slices on the inputs that take it through each of its paths: every
trip count of its per-lane loops (at most 128 crossings on a plane, 129-256, 257-384, and the large tier above 384), sections with a
second loop and with a clockwise loop, and bridge mode's start points.  The oracle's OBB transform is injected, as in
test_gpu_slices.py, whose tolerances these are: integer results exact, coordinates to 1e-9 mm."""
import os

import numpy as np
import pytest

from conftest import BONES
from oracle.humerus import OracleHumerus
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl
from test_gpu_highres import subdivide

pytestmark = pytest.mark.gpu
TOL = 1e-9
SETS = (("full", "full", 200, False), ("distal", "distal", 200, True))      # (buffer prefix, oracle attribute, planes, keeps a ring)


def _run_sets(engine, hs):
    engine.reset_params()
    engine.set_params(unet_dtype=_lib.UNET_F32)
    engine.upload([(h.verts, h.faces) for h in hs])
    engine.store("obb_transform", np.stack([h.T_obb for h in hs]))
    engine.run(_lib.STAGE_FULL | _lib.STAGE_DISTAL, fetch=False)


def _compare(engine, hs):
    """full and distal of the resident batch against the oracle's: .centroids, .areas, .nloops, .ring_n and ring[:ring_n + 1] (the
    full set keeps no ring).  -> {prefix: nloops [B, N]}"""
    B = len(hs)
    out = {}
    for pfx, attr, N, has_ring in SETS:
        cen = engine.fetch(pfx + ".centroids", np.float64, (B, N, 2))
        areas = engine.fetch(pfx + ".areas", np.float64, (B, N))
        nl = engine.fetch(pfx + ".nloops", np.int32, (B, N))
        ring_n = engine.fetch(pfx + ".ring_n", np.int32, (B, N))
        ring = engine.fetch(pfx + ".ring", np.float64, (B, N, 1025, 2)) if has_ring else None
        for b, h in enumerate(hs):
            s = getattr(h, attr)
            np.testing.assert_array_equal(nl[b], s.n_loops, err_msg=f"{pfx} humerus {b}")
            np.testing.assert_array_equal(ring_n[b], [len(r) - 1 for r in s.largest], err_msg=f"{pfx} humerus {b}")
            np.testing.assert_allclose(cen[b], s.centroids_all, rtol=0, atol=TOL, err_msg=f"{pfx} humerus {b}")
            np.testing.assert_allclose(areas[b], s.areas1_all, rtol=1e-12, atol=1e-9, err_msg=f"{pfx} humerus {b}")
            if ring is not None:
                for k in range(N):
                    r = s.largest[k]
                    assert len(r) == ring_n[b, k] + 1
                    np.testing.assert_allclose(ring[b, k, :len(r)], r, rtol=0, atol=TOL, err_msg=f"{pfx} humerus {b} plane {k}")      # same start, same direction
        out[pfx] = nl
    return out


@pytest.fixture(scope="module")
def both_tiers(engine, rfc_tables, unet_weights, oracle_bones):
    """humerus_left beside the same mesh subdivided once (twice the crossings per plane), run once for the two tests below."""
    h0 = oracle_bones("humerus_left")
    v2, f2 = subdivide(*load_stl(os.path.join(BONES, "humerus_left.stl")))
    hs = [h0, OracleHumerus(v2, f2, rfc_tables, unet_weights, unet_eval="chain")]
    _run_sets(engine, hs)
    cnt = np.concatenate([engine.fetch(pfx + ".seg_count", np.int32, (2, N)).ravel() for pfx, _, N, _ in SETS])
    return hs, cnt


def test_planes_on_both_sides_of_the_tier_boundary(engine, both_tiers):
    hs, _ = both_tiers
    _compare(engine, hs)


def test_every_trip_count_of_the_lane_loops_is_exercised(both_tiers):
    """A lane of the join takes a plane's crossings 128 apart: one, two and three trips in the small tier, more in the large one."""
    _, cnt = both_tiers
    assert np.any((cnt >= 3) & (cnt <= 128)), "no plane with at most 128 segments"
    assert np.any((cnt >= 129) & (cnt <= 256)), "no plane with 129-256 segments"
    assert np.any((cnt >= 257) & (cnt <= 384)), "no plane with 257-384 segments"
    assert np.any((cnt > 384) & (cnt <= 1024)), "no plane above 384 segments"


def _box(center_obb, half, Tinv, inward=False):
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * half + center_obb
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([tri for a, b, cc, d in quads for tri in ((a, b, cc), (a, cc, d))], dtype=np.int32)
    if inward:
        t = t[:, ::-1]
    return ((np.c_[c, np.ones(8)] @ Tinv.T)[:, :3]).astype(np.float32), t


@pytest.mark.parametrize("case", ["fragment beside the shaft", "cavity inside the head"])
def test_sections_with_a_second_loop(engine, oracle_bones, rfc_tables, unet_weights, case):
    """The two two-component meshes of test_gpu_random_sweep.py: a detached box beside the shaft (a second, counter-clockwise loop)
    and an inward-facing box inside the head (a clockwise loop)."""
    h0 = oracle_bones("humerus_left")
    Tinv = np.linalg.inv(h0.T_obb)
    zmax = h0.verts_obb[:, 2].max()
    bv, bf = (_box(np.array([45.0, 3.0, -20.0]), np.array([2.5, 2.0, 3.0]), Tinv) if case.startswith("fragment")
              else _box(np.array([0.0, 0.0, zmax - 22.0]), np.array([3.0, 3.5, 4.0]), Tinv, inward=True))
    mv = np.concatenate([h0.verts, bv]).astype(np.float32)
    mf = np.concatenate([h0.faces, bf + len(h0.verts)]).astype(np.int32)
    h = OracleHumerus(mv, mf, rfc_tables, unet_weights, unet_eval="chain")
    _run_sets(engine, [h])
    nl = _compare(engine, [h])
    assert max(int(a.max()) for a in nl.values()) == 2


def test_bridge_mode_start_points_repeat(engine):
    """Bridge mode (sh_set_open_contours) on a humerus with one triangle removed from the shaft: the join's open-contour
    instantiation, whose bridges take their start points from the keys.  The same engine gives the same records twice, status 0."""
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    c = v[f].astype(np.float64).mean(axis=1)
    longest = np.linalg.norm(v[f] - v[np.roll(f, -1, axis=1)], axis=2).max(axis=1)
    zmid = 0.5 * (c[:, 2].min() + c[:, 2].max())
    order = np.argsort(np.abs(c[:, 2] - zmid), kind="stable")
    hole = int(next(i for i in order if longest[i] < 2.0))      # a small triangle at mid height: a gap well below max_gap
    engine.reset_params()
    engine.set_params(unet_dtype=_lib.UNET_F32)
    engine.set_open_contours("bridge", 4.0)
    try:
        engine.upload([(v, np.delete(f, hole, axis=0))])
        first = engine.run(_lib.STAGE_ALL).copy()
        bridged, dropped = engine.open_contour_stats()
        bufs = [engine.fetch(k, dt).copy() for k, dt in (("full.centroids", np.float64), ("full.areas", np.float64), ("full.nloops", np.int32),
                                                         ("distal.centroids", np.float64), ("distal.ring_n", np.int32))]
        second = engine.run(_lib.STAGE_ALL).copy()
        assert first["status"][0] == 0 and second["status"][0] == 0
        assert bridged[0] > 0 and dropped[0] == 0, (bridged, dropped)
        assert first.tobytes() == second.tobytes()
        for a, (k, dt) in zip(bufs, (("full.centroids", np.float64), ("full.areas", np.float64), ("full.nloops", np.int32),
                                     ("distal.centroids", np.float64), ("distal.ring_n", np.int32))):
            assert a.tobytes() == engine.fetch(k, dt).tobytes(), k
    finally:
        engine.set_open_contours("error")
