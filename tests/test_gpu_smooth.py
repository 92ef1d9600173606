"""Smoothing of the vertices of the resident batch (include/shoulder_hip.h sh_smooth_vertices, k_smooth.h) on the engine against the
NumPy statement of tests/smooth_oracle.py.

Bounds.  The rule is + - x / sqrt on float64 in a fixed order, so there is no tolerance: "smooth.nrow", "smooth.nbr", "smooth.w",
"smooth.pos" and "smooth.info" are held to the oracle AS BYTES, and a mesh in a batch to its single upload as bytes.  The one inequality
(the round trip) compares the device with itself: the standard deviation of the mean curvature after the smoothing against before."""
import os

import numpy as np
import pytest

import shoulder_amd as shoulder
import smooth_oracle as O
from conftest import BONES
from mass_oracle import int_box
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
FIXTURES = ["humerus_left", "humerus_left_flipped", "humerus_right", "humerus_left_trab", "proximal_left_cut"]
FILTERS = {O.LAPLACIAN: "laplacian", O.TAUBIN: "taubin", O.HC: "hc"}
WEIGHTS = {O.UNIFORM: "uniform", O.INVLEN: "invlen"}
RESIDENT = ("smooth.pos", "smooth.nrow", "smooth.nbr", "smooth.w", "smooth.info", "smooth.plane", "smooth.pin", "smooth.mask", "smooth.part")


def load(name):
    v, f = load_stl(os.path.join(BONES, name + ".stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


@pytest.fixture(scope="module")
def meshes():
    out = {n: load(n) for n in FIXTURES}
    out["box"] = int_box()
    return out


@pytest.fixture(scope="module")
def cases(meshes):
    return O.small_cases(meshes)


def device(engine, batch, upload=True, **kw):
    """-> per mesh dict(nrow, nbr, w, pos, info), cut out of the resident buffers; what the call returned is what is resident.  kw are
    smooth_oracle.smooth's; pin: one mask per mesh, or None"""
    if upload:
        engine.upload(batch)
    B = len(batch)
    voff, foff = np.cumsum([0] + [len(v) for v, _ in batch]), np.cumsum([0] + [len(f) for _, f in batch])
    kw = dict(kw)
    pin = kw.pop("pin", None)
    if pin is not None:
        pin = np.concatenate([np.asarray(p, np.uint8) for p in pin])
    r = engine.smooth_vertices(filter=FILTERS[kw.pop("filter", O.TAUBIN)], weight=WEIGHTS[kw.pop("weight", O.UNIFORM)], pin=pin, **kw)
    assert np.array_equal(r["voff"], voff) and r["info"].shape == (B,) and r["vertices"].shape == (voff[-1], 3)
    assert engine.fetch("smooth.pos", np.float64, (voff[-1], 3)).tobytes() == r["vertices"].tobytes()
    assert engine.fetch("smooth.info", _lib.SMOOTH_INFO_DTYPE, (B,)).tobytes() == r["info"].tobytes()
    nrow = engine.fetch("smooth.nrow", np.int32, (voff[-1] + B,))
    nbr, w = engine.fetch("smooth.nbr", np.int32, (6 * max(foff[-1], 1),)), engine.fetch("smooth.w", np.float64, (6 * max(foff[-1], 1),))
    out, pairs = [], engine.vertex_neighbors()
    for b in range(B):
        row = nrow[voff[b] + b:voff[b + 1] + b + 1]
        n = int(row[-1])
        a, c = pairs[b]
        assert a.tobytes() == row.tobytes() and c.tobytes() == nbr[6 * foff[b]:6 * foff[b] + n].tobytes()
        out.append(dict(nrow=row, nbr=nbr[6 * foff[b]:6 * foff[b] + n], w=w[6 * foff[b]:6 * foff[b] + n], pos=r["vertices"][voff[b]:voff[b + 1]], info=r["info"][b]))
    return out


def per_mesh(kw):
    """the kwargs of the oracle for one mesh -> those of device() for a batch of that one mesh"""
    return {k: ([v] if k == "pin" else v) for k, v in kw.items()}


def test_small_cases_against_the_oracle(engine, cases):
    for name, mesh in cases.items():
        for i, (tag, kw) in enumerate(O.variants(len(mesh[0]))):
            got = device(engine, [mesh], upload=i == 0, **per_mesh(kw))[0]
            O.same_bytes(got, O.reference(name, mesh, tag, kw), (name, tag))
    got = device(engine, [cases["boxes sharing an edge"]], filter=O.HC, pin_border=True)[0]
    assert got["info"]["pinned"] == 2 and got["info"]["isolated"] == 2 and list(got["nbr"][:got["nrow"][1]]).count(1) == 1
    got = device(engine, [cases["fan of 300"]], iterations=1)[0]
    assert got["nrow"][1] == 301 and got["nbr"][300] == 301
    got = device(engine, [cases["only degenerate faces"]], filter=O.LAPLACIAN, iterations=2, keep_volume=True)[0]
    assert got["info"]["status"] == O.GEOMETRY and got["info"]["isolated"] == len(got["pos"]) and got["nrow"][-1] == 0


@pytest.mark.parametrize("name,tag,kw", O.WHOLE)
def test_whole_meshes_against_the_oracle(engine, meshes, name, tag, kw):
    mesh = meshes[name]
    got = device(engine, [mesh], **per_mesh(kw))[0]
    O.same_bytes(got, O.reference(name, mesh, tag, kw), (name, tag))
    assert got["info"]["status"] == 0 and got["info"]["max_disp"] > 0.0
    print(f"{name}, {tag}: volume {got['info']['volume_before']:.3f} -> {got['info']['volume_after']:.3f}, scale {got['info']['scale']:.9f}, largest displacement "
          f"{got['info']['max_disp']:.4f} mm, rms {np.sqrt(got['info']['sum_sq_disp'] / len(mesh[0])):.4f} mm, pinned {got['info']['pinned']}")


def test_odd_launch_counts_read_back_the_plane_written_last(engine, cases):
    for name in ("box", "humerus_left[:257]"):
        mesh = cases[name]
        for tag, kw in (("laplacian 7", dict(filter=O.LAPLACIAN, weight=O.INVLEN, iterations=7, lamb=0.3)), ("taubin 3", dict(filter=O.TAUBIN, iterations=3)),
                        ("laplacian 1", dict(filter=O.LAPLACIAN, iterations=1)), ("hc 1", dict(filter=O.HC, iterations=1))):
            O.same_bytes(device(engine, [mesh], upload=tag == "laplacian 7", **kw)[0], O.reference(name, mesh, tag, kw), (name, tag))


def test_a_result_does_not_depend_on_the_batch(engine, cases, meshes):
    names = ("box", "humerus_left", "fan of 300", "humerus_left")
    pool = dict(cases, humerus_left=meshes["humerus_left"])
    batch = [pool[n] for n in names]
    for kw in (dict(filter=O.LAPLACIAN, weight=O.INVLEN, iterations=0), dict(filter=O.HC, weight=O.INVLEN, iterations=1), dict(filter=O.LAPLACIAN, iterations=7, lamb=0.3),
               dict(filter=O.TAUBIN, weight=O.INVLEN, iterations=7, keep_volume=True)):
        single = {n: device(engine, [pool[n]], **kw)[0] for n in set(names)}
        got = device(engine, batch, **kw)
        for b, n in enumerate(names):
            O.same_bytes(got[b], single[n], (n, kw, "in the batch"))
        again = device(engine, batch, upload=False, **kw)
        for a, b in zip(got, again):
            O.same_bytes(a, b, "two calls")
        if kw["iterations"] == 0:
            assert all(g["pos"].tobytes() == m[0].astype(np.float64).tobytes() and g["info"]["max_disp"] == 0.0 for g, m in zip(got, batch))
    # a mask over the whole batch: each mesh takes its own part of it
    masks = [O.pin_mask(len(v), seed=11 + b) for b, (v, _) in enumerate(batch)]
    got = device(engine, batch, upload=False, filter=O.HC, iterations=2, pin=masks)
    for b, n in ((0, "box"), (2, "fan of 300")):
        O.same_bytes(got[b], O.smooth(*pool[n], filter=O.HC, iterations=2, pin=masks[b]), (n, "mask in the batch"))
    assert [int(g["info"]["pinned"]) for g in got] == [int((m != 0).sum()) for m in masks]


def test_lifetime_and_refusals(engine, meshes):
    fresh = Engine(0)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            fresh.smooth_vertices()
        assert ex.value.code == O.STATE and "sh_smooth_vertices" in str(ex.value) and "no meshes" in str(ex.value)
    finally:
        fresh.close()
    v, f = meshes["humerus_left"]
    engine.reset_params()
    engine.upload([(v, f)])
    # the C call without a topology refuses; the engine's runs one first
    assert engine.L.sh_smooth_vertices(engine.h, 1, 0, 10, 0, 0.5, -0.53, None, None, None) == O.STATE
    assert b"sh_smooth_vertices: no incidence of the resident batch: call sh_mesh_topology first" in engine.L.sh_last_error(engine.h)
    first = engine.smooth_vertices()
    assert first["info"][0]["status"] == 0 and first["vertices"].shape == (len(v), 3) and engine._has_buffer("topo.vrow")
    engine.vertex_fields(smooth=2)
    engine.closest_points(v[:300].astype(np.float64))
    engine.mass_properties()
    names = ("cp.out", "mass.out", "mass.part", "verts", "faces", "topo.vrow", "topo.vface", "topo.adj", "topo.label", "topo.info", "topo.shells", "topo.state", "topo.cursor",
             "topo.tmp", "topo.p", "vert.face", "vert.normal", "vert.fields", "vert.flags", "vert.status", "vert.a2", "vert.plane", "vert.state")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    rows = [engine.fetch(n, np.uint8).tobytes() for n in ("smooth.nrow", "smooth.nbr", "smooth.w")]
    again = engine.smooth_vertices(filter="hc", weight="invlen", iterations=4, pin_border=True)
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before             # other queries' results survive, "verts" among them
    assert [engine.fetch(n, np.uint8).tobytes() for n in ("smooth.nrow", "smooth.nbr", "smooth.w")] == rows      # the rows are built once
    assert again["info"][0]["pinned"] == 0 and again["vertices"].tobytes() != first["vertices"].tobytes()
    assert engine.smooth_vertices()["vertices"].tobytes() == first["vertices"].tobytes()
    refused = (dict(filter=3), dict(filter=-1), dict(weight=2), dict(iterations=-1), dict(iterations=257), dict(lamb=1.5), dict(mu=0.1), dict(lamb=float("nan")),
               dict(mu=float("nan")), dict(filter="hc", alpha=1.5), dict(filter="hc", beta=-0.5), dict(keep_volume=True, pin_border=True),
               dict(keep_volume=True, pin=np.zeros(len(v), np.uint8)))
    for kw in refused:
        with pytest.raises(ShoulderHipError) as ex:
            engine.smooth_vertices(**kw)
        assert ex.value.code == O.ARG and "sh_smooth_vertices: bad argument" in str(ex.value), kw
    assert engine.L.sh_smooth_vertices(engine.h, 1, 0, 10, 4, 0.5, -0.53, None, None, None) == O.ARG      # an unknown flag bit
    assert b"flags 0..3" in engine.L.sh_last_error(engine.h)
    with pytest.raises(ShoulderHipError) as ex:
        engine.smooth_vertices(lamb=1.5)
    assert "lambda in 0..1" in str(ex.value)
    with pytest.raises(ShoulderHipError) as ex:
        engine.smooth_vertices(mu=0.1)
    assert "mu in -1..0" in str(ex.value)
    with pytest.raises(ValueError):
        engine.smooth_vertices(filter="bilateral")
    with pytest.raises(ValueError):
        engine.smooth_vertices(pin=np.zeros(3, np.uint8))
    assert engine.smooth_vertices(iterations=O.MAX_ITER, filter="laplacian", lamb=0.01)["info"][0]["status"] == 0
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            engine.smooth_vertices()
        assert ex.value.code == O.STATE and "in flight" in str(ex.value) and "sh_smooth_vertices" in str(ex.value)
    finally:
        engine.collect()
    engine.upload([(v, f)])                                                           # "smooth.*" answer for their batch
    for name in RESIDENT:
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)
    assert engine.smooth_vertices()["vertices"].tobytes() == first["vertices"].tobytes()       # on a fresh upload: the topology runs first
    engine.store("verts", v)                                                          # ... and for their vertices
    for name in RESIDENT:
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)
    nrow, nbr = engine.vertex_neighbors(0)                                            # without rows: a call with no iteration makes them
    assert nrow.tobytes() == O.neighbours(f, len(v))[0].tobytes() and nbr.tobytes() == O.neighbours(f, len(v))[1].tobytes()


def test_a_topology_out_of_rounds_is_accepted(engine, cases):
    mesh = cases["strip of 600, shuffled"]
    engine.upload([mesh])
    assert engine.topology(max_rounds=4)[0][0]["status"] == -4
    kw = dict(filter=O.TAUBIN, weight=O.INVLEN, iterations=3, pin_border=True)
    O.same_bytes(device(engine, [mesh], upload=False, **kw)[0], O.smooth(*mesh, **kw), "strip after a topology out of rounds")


def test_round_trip_through_the_resident_vertices(engine, meshes):
    v, f = meshes["humerus_left"]
    engine.upload([(v, f)])
    before = engine.vertex_fields()["mean"].std()
    r = engine.smooth_vertices()
    engine.store("verts", r["vertices"].astype(np.float32))
    after = engine.vertex_fields()
    print(f"humerus_left: std of the mean curvature {before:.5f} -> {after['mean'].std():.5f} / mm after ten Taubin iterations")
    assert after["status"][0] == 0 and after["mean"].std() < before
    assert engine.fetch("verts", np.float32, (len(v), 3)).tobytes() == r["vertices"].astype(np.float32).tobytes()


def test_the_facade(engine):
    engine.reset_params()
    try:
        h = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        volume = h.mass_properties()["volume"]      # (the bone is in CT: the current coordinate system is the upload's)
        verts, faces = h.smoothed_mesh()
        kept = h.smoothed_mesh(filter="laplacian", iterations=5, keep_volume=True)[0]
        assert verts.shape == (len(h._verts), 3) and verts.dtype == np.float64 and faces.shape == h._faces.shape and not np.isnan(verts).any()
        engine.upload([(verts.astype(np.float32), faces)])
        m = engine.mass_properties()[0]
        assert m["status"] == 0 and m["vstatus"] == 0 and m["volume"] > 0.0 and m["faces"] == len(faces)
        print(f"humerus_left: volume {volume:.3f}, after ten Taubin iterations {m['volume']:.3f}")
        engine.upload([(kept.astype(np.float32), faces)])
        # the scaling restores the volume in float64; the upload rounds every coordinate to float32, by at most 2^-24 of the largest,
        # and a surface of area A whose every point moves by at most d encloses at most sqrt(3) d A more or less (d per axis)
        m = engine.mass_properties()[0]
        bound = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(kept).max()) * m["area"] / volume
        print(f"humerus_left, keep_volume: volume off by {abs(m['volume'] / volume - 1.0):.3g} <= {bound:.3g}")
        assert abs(m["volume"] / volume - 1.0) <= bound
    finally:
        engine.reset_params()
