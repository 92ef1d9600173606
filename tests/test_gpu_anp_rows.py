"""The neck-image kernels (k_anp_rows, k_anp_scale, k_anp_edge_count, k_anp_edges, k_anp_plane) on rows no bone has produced: the cases of
tests/row_cases.py are stored over a real batch's "prox.itr_start" (the network's 512 rows), "prox.zs" and "groove.bg_theta", SH_STAGE_ANP
runs alone with a threshold network (make_teacher_weights(base=32, depth=1, eps=0): logit = 8 (x - 0.6), f32), and the products are held to
oracle.anp evaluated on the logits fetched from the device -- the f32 network is held bit for bit elsewhere and is not under test here.
Roll exact, raw rows 1e-12 (the project's figure for f64 computed with the same arithmetic; the worst difference is printed), image within
2 float32 eps, counts / row counts / mask bits exact, edge points 1e-9 in row-major order, plane point 1e-6 and normal 1e-9; `bare` (4
edge pixels) carries a status.  The stage's ray casts run against the uploaded bone; their results are not compared."""
import os

import numpy as np
import pytest

import row_cases as rc
from conftest import BONES
from shoulder_amd import _lib, unet_spec

pytestmark = pytest.mark.gpu
PRE = _lib.STAGE_OBB | _lib.STAGE_FULL | _lib.STAGE_NECK | _lib.STAGE_CANAL | _lib.STAGE_PROXIMAL
B = len(rc.ANP_CASES)
IMG = (B, rc.ANP_ROWS, rc.M)


@pytest.fixture(scope="module")
def ran():
    """name -> (case, the device's products of its item, oracle.anp on the device's logits)"""
    from oracle.stl import load_stl
    from shoulder_amd.engine import Engine
    mesh = load_stl(os.path.join(BONES, "humerus_left.stl"))[:2]
    cases = [rc.anp_case(n) for n in rc.ANP_CASES]
    e = Engine(0)
    try:
        e.load_rfc()
        e.load_unet(unet_spec.make_teacher_weights(base=32, depth=1, eps=0.0), 32, 1)
        e.set_params(unet_dtype=_lib.UNET_F32)
        e.set_keep_products(True)
        e.upload([mesh] * B)
        e.run(PRE, fetch=False)
        rows = e.fetch("prox.itr_start", np.float64, (B, rc.NPROX, 2, rc.M))
        zs = e.fetch("prox.zs", np.float64, (B, rc.NPROX))
        for b, c in enumerate(cases):
            rows[b, rc.ANP0:], zs[b, rc.ANP0:] = c["itr"], c["zs"]
        e.store("prox.itr_start", rows)
        e.store("prox.zs", zs)
        e.store("groove.bg_theta", np.array([c["bg_theta"] for c in cases]))
        lm = e.run(_lib.STAGE_ANP, strict=False)
        got = {k: e.fetch(k, dt, shp) for k, dt, shp in (
            ("anp.roll", np.int32, (B, rc.ANP_ROWS)), ("anp.raw", np.float64, IMG), ("anp.image", np.float32, IMG), ("anp.logits", np.float32, IMG),
            ("anp.counts", np.int32, (B, 2)), ("anp.rowcnt", np.int32, (B, rc.ANP_ROWS, 2)), ("anp.maskbits", np.uint64, (B, rc.ANP_ROWS, rc.M // 64)),
            ("anp.plane", np.float64, (B, 6)))}
        pts = e.fetch("anp.points_obb", np.float64, (B, rc.ANP_ROWS * rc.M, 3))
        out = {}
        for b, c in enumerate(cases):
            item = {k: v[b] for k, v in got.items()}
            item["status"] = int(lm["status"][b])
            item["anp.points_obb"] = pts[b, :max(int(got["anp.counts"][b, 0]), 0)].copy()
            out[c["name"]] = (c, item, rc.anp_expect(c, item["anp.logits"]))
        return out
    finally:
        e.close()


@pytest.mark.parametrize("name", rc.ANP_CASES)
def test_roll_raw_rows_and_image(ran, name):
    _, got, want = ran[name]
    np.testing.assert_array_equal(got["anp.roll"], want["roll"])
    worst = float(np.abs(got["anp.raw"] - want["itr_shft"][:, 1]).max())
    print("%s: worst |anp.raw - oracle| = %.3g" % (name, worst))
    assert worst <= 1e-12
    exp = want["image"].astype(np.float32)
    assert np.abs(got["anp.image"] - exp).max() <= 2 * np.finfo(np.float32).eps


@pytest.mark.parametrize("name", rc.ANP_CASES)
def test_threshold_network_draws_the_level_set(ran, name):
    _, got, _ = ran[name]
    img = got["anp.image"]
    clear = np.abs(img - np.float32(rc.LEVEL)) >= 1e-6
    assert clear.mean() > 0.999
    np.testing.assert_array_equal((got["anp.logits"] > 0)[clear], (img > np.float32(rc.LEVEL))[clear])


@pytest.mark.parametrize("name", rc.ANP_CASES)
def test_mask_counts_bits_and_points(ran, name):
    _, got, want = ran[name]
    edge, mask = want["edge"], want["mask"]
    assert tuple(got["anp.counts"]) == (edge.sum(), mask.sum())
    np.testing.assert_array_equal(got["anp.rowcnt"], np.c_[edge.sum(axis=1), mask.sum(axis=1)])
    bits = np.packbits(got["anp.logits"] > 0, axis=1, bitorder="little").view("<u8")      # pixel 64 c + l is bit l of word c
    np.testing.assert_array_equal(got["anp.maskbits"], bits)
    assert got["anp.points_obb"].shape == want["points_obb"].shape
    np.testing.assert_allclose(got["anp.points_obb"], want["points_obb"], rtol=0, atol=1e-9)      # row-major, like the reference's boolean index


@pytest.mark.parametrize("name", rc.ANP_PLANE_CASES)
def test_plane(ran, name):
    _, got, want = ran[name]
    point, normal = want["plane"]
    np.testing.assert_allclose(got["anp.plane"][:3], point, rtol=0, atol=1e-6)
    np.testing.assert_allclose(got["anp.plane"][3:], normal, rtol=0, atol=1e-9)


def test_bare_carries_a_status(ran):
    _, got, want = ran["bare"]
    assert want["plane"] is None and 0 < got["anp.counts"][0] < 6
    assert got["status"] != 0 and (got["anp.plane"] == 0.0).all()


def test_cases_drew_what_they_mean(ran):
    """on the device's own logits: stripes are stripes (pixel 0 on, >= 200 edges in a row, every ballot seam, a ragged total), the rolls
    of `outside` are 0 and 511, the rows of `unsorted` went through the sequential replay (their abscissae descend somewhere)"""
    e = ran["striped"][2]["edge"]
    assert e[:, 0].any() and e.sum(axis=1).max() >= 200 and all(e[:, 64 * s].any() for s in range(1, 8)) and e.sum() % 256 != 0
    assert (ran["outside_lo"][1]["anp.roll"] == 0).all() and (ran["outside_hi"][1]["anp.roll"] == rc.M - 1).all()
    assert (np.diff(ran["unsorted"][0]["itr"][:, 0, :rc.M - 1], axis=1) < 0).any(axis=1).sum() == 40
