"""Vertex normals and discrete curvatures of the resident batch (include/shoulder_hip.h sh_vertex_fields, k_vert.h) on the engine against
the NumPy statement of tests/vert_oracle.py.

Bounds.  Everything but atan2 is + - x / sqrt on float64 in a fixed order, so n, A2 and cot of "vert.face", area, the flags, the status
and, with area weights, the normals, mean and mean_smooth are held to the oracle as bytes.  The angles and what they enter (angle_sum,
defect, gauss, gauss_smooth; with angle weights the normals, mean and mean_smooth) are held within vert_oracle.bound: 4 ulp per atan2
term between two math libraries (the project's figure, winding_oracle.bound) and one rounding per later operation in each evaluation;
the largest difference of every comparison is printed beside its bound.  Device against device (a mesh in a batch against its single
upload, two calls) everything is bytes, the atan2 fields included.

Figures of a run on an MI355X (largest difference <= its bound at that element): on humerus_left with 8 rounds, angle 4.44e-16 <=
1.78e-15, angle_sum and defect 2.66e-15 <= 1.9e-14, gauss 8.79e-15 <= 7.84e-14, gauss_smooth 1.08e-15 <= 4.28e-14, and with angle
weights the normals 1.54e-14 <= 2.38e-12, mean 8.88e-16 <= 3.56e-12, mean_smooth 8.33e-17 <= 1.33e-14; DESIGN.md 10.13."""
import os

import numpy as np
import pytest

import shoulder_amd as shoulder
import topo_oracle as TO
import vert_oracle as O
from conftest import BONES
from mass_oracle import int_box
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
FIXTURES = ["humerus_left", "humerus_left_flipped", "humerus_right", "humerus_left_trab", "proximal_left_cut"]
WEIGHTS = {O.AREA: "area", O.ANGLE: "angle"}
FIELD_NAMES = ("area", "angle_sum", "defect", "gauss", "mean", "gauss_smooth", "mean_smooth")
BUFFERS = ("face", "normals", "fields", "flags", "status")
TWO_PI = 6.283185307179586


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
    out = O.small_cases(meshes)
    out.update({n: meshes[n] for n in ("humerus_left", "humerus_left_trab", "proximal_left_cut")})
    out["humerus_left, shuffled"] = TO.further(meshes)["humerus_left, shuffled"]
    return out


def device(engine, batch, weight=O.AREA, smooth=0, upload=True):
    """-> per mesh dict(face, normals, fields, flags, status), cut out of the resident buffers; what the call returned is what is resident"""
    if upload:
        engine.upload(batch)
    r = engine.vertex_fields(weight=WEIGHTS[weight], smooth=smooth)
    B = len(batch)
    voff, foff = np.cumsum([0] + [len(v) for v, _ in batch]), np.cumsum([0] + [len(f) for _, f in batch])
    assert np.array_equal(r["voff"], voff) and r["status"].shape == (B,)
    face = engine.fetch("vert.face", np.float64, (foff[-1], O.FACE))
    fields = engine.fetch("vert.fields", np.float64, (voff[-1], O.FIELDS))
    assert engine.fetch("vert.normal", np.float64, (voff[-1], 3)).tobytes() == r["normals"].tobytes()
    assert engine.fetch("vert.flags", np.int32, (voff[-1],)).tobytes() == r["flags"].tobytes()
    assert engine.fetch("vert.status", np.int32, (B,)).tobytes() == r["status"].tobytes()
    for i, n in enumerate(FIELD_NAMES):
        assert np.ascontiguousarray(fields[:, i]).tobytes() == r[n].tobytes(), n
    return [dict(face=face[foff[b]:foff[b + 1]], normals=r["normals"][voff[b]:voff[b + 1]], fields=fields[voff[b]:voff[b + 1]], flags=r["flags"][voff[b]:voff[b + 1]],
                 status=r["status"][b]) for b in range(B)]


def same_bytes(a, b, tag):
    for n in BUFFERS:
        assert np.ascontiguousarray(a[n]).tobytes() == np.ascontiguousarray(b[n]).tobytes(), (tag, n)


SMALL = ["tetrahedron", "box", "box without face 0", "box, face 5 flipped", "boxes sharing an edge", "fan of 300", "strip of 600, shuffled", "humerus_left[:255]",
         "humerus_left[:256]", "humerus_left[:257]", "degenerate faces", "degenerate faces, four faces", "only degenerate faces", "box with a flat face", "icosphere 2"]


def test_small_cases_against_the_oracle(engine, cases):
    for name in SMALL:
        mesh = cases[name]
        for weight in (O.AREA, O.ANGLE):
            got = device(engine, [mesh], weight, 3, upload=weight == O.AREA)[0]
            O.compare(got, O.vertex_fields(*mesh, weight=weight, smooth=3), name)
    got = device(engine, [cases["boxes sharing an edge"]])[0]
    assert ((got["flags"] & O.NONMANIFOLD) != 0).sum() == 2
    got = device(engine, [cases["box without face 0"]])[0]
    b = (got["flags"] & O.BORDER) != 0
    assert b.sum() == 3 and np.array_equal(got["fields"][b, 2], 3.141592653589793 - got["fields"][b, 1])
    got = device(engine, [cases["box with a flat face"]])[0]
    assert got["flags"][8] == (O.USED | O.BORDER | O.FLAT) and not got["fields"][8].any() and not got["face"][12].any() and got["status"] == 0
    v, f = cases["icosphere 2"]
    got = device(engine, [(v, f)])[0]
    assert (got["fields"][:, 3] * 625 >= 0.99).all() and (got["fields"][:, 4] * 25 <= 1.16).all() and (O._dot(got["normals"], v.astype(np.float64)) > 0).all()


def test_a_mesh_of_degenerate_faces_has_the_status_and_the_batch_goes_on(engine, cases):
    box = cases["box"]
    got = device(engine, [cases["only degenerate faces"], box, cases["only degenerate faces"]], O.ANGLE, 2)
    for b in (0, 2):
        assert got[b]["status"] == O.GEOMETRY and not got[b]["fields"].any() and not got[b]["normals"].any() and not got[b]["flags"].any() and not got[b]["face"].any()
    O.compare(got[1], O.vertex_fields(*box, weight=O.ANGLE, smooth=2), "box between two meshes of degenerate faces")


@pytest.mark.parametrize("name,weight,smooth", [("humerus_left", O.AREA, 8), ("humerus_left", O.ANGLE, 8), ("humerus_left_trab", O.ANGLE, 1),
                                                 ("proximal_left_cut", O.AREA, 1), ("humerus_left, shuffled", O.ANGLE, 0)])
def test_whole_meshes_against_the_oracle(engine, cases, name, weight, smooth):
    mesh = cases[name]
    got = device(engine, [mesh], weight, smooth)[0]
    O.compare(got, O.vertex_fields(*mesh, weight=weight, smooth=smooth), name)
    # Gauss-Bonnet against the device's own Euler characteristic
    euler = int(engine.topology()[0][0]["euler"])
    dev = abs(got["fields"][:, 2].sum() / TWO_PI - euler)
    print(f"{name}: |sum defect / 2 pi - euler {euler}| = {dev:.3g}")
    assert dev <= 1e-10 and euler == (0 if "trab" in name else 2)


def test_a_record_does_not_depend_on_the_batch(engine, cases):
    names = ("box", "humerus_left", "fan of 300", "humerus_left")
    batch = [cases[n] for n in names]
    for weight in (O.AREA, O.ANGLE):
        for smooth in (0, 1, 8):
            single = {n: device(engine, [cases[n]], weight, smooth)[0] for n in set(names)}
            got = device(engine, batch, weight, smooth)
            for b, n in enumerate(names):
                same_bytes(got[b], single[n], (n, weight, smooth, "in the batch"))
            again = device(engine, batch, weight, smooth, upload=False)
            for a, b in zip(got, again):
                same_bytes(a, b, "two calls")
            if smooth == 0:
                assert all(np.array_equal(g["fields"][:, 5:7], g["fields"][:, 3:5]) for g in got)


def test_lifetime_and_refusals(engine, meshes):
    fresh = Engine(0)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            fresh.vertex_fields()
        assert ex.value.code == O.STATE and "sh_vertex_fields" in str(ex.value) and "no meshes" in str(ex.value)
    finally:
        fresh.close()
    v, f = meshes["humerus_left"]
    engine.reset_params()
    engine.upload([(v, f)])
    # the C call without a topology refuses; the engine's runs one first
    assert engine.L.sh_vertex_fields(engine.h, 0, 0, None, None, None, None) == O.STATE
    assert b"sh_vertex_fields: no incidence of the resident batch: call sh_mesh_topology first" in engine.L.sh_last_error(engine.h)
    first = engine.vertex_fields()
    assert first["status"][0] == 0 and first["normals"].shape == (len(v), 3)
    engine.closest_points(v[:300].astype(np.float64))
    engine.mass_properties()
    engine.sample_surface(512, seed=3, radius=2.0)
    names = ("cp.out", "mass.out", "mass.part", "samp.cdf", "samp.base", "samp.out", "samp.info", "samp.state", "verts", "faces",
             "topo.vrow", "topo.vface", "topo.adj", "topo.label", "topo.info", "topo.shells", "topo.state", "topo.cursor", "topo.tmp", "topo.p")
    before = [engine.fetch(n, np.uint8).tobytes() for n in names]
    again = engine.vertex_fields(weight="angle", smooth=4)
    assert [engine.fetch(n, np.uint8).tobytes() for n in names] == before             # other queries' results survive
    assert again["area"].tobytes() == first["area"].tobytes() and again["gauss"].tobytes() == first["gauss"].tobytes()
    unit, area, angles = engine.face_normals(0)
    assert unit.shape == (len(f), 3) and np.allclose(np.linalg.norm(unit, axis=1), 1.0, atol=1e-12) and np.allclose(angles.sum(axis=1), np.pi, atol=1e-12)
    assert abs(area.sum() - engine.mass_properties()[0]["area"]) <= 1e-9 * area.sum()
    for kw, code in ((dict(weight=2), O.ARG), (dict(weight=-1), O.ARG), (dict(smooth=-1), O.ARG), (dict(smooth=65), O.ARG)):
        with pytest.raises(ShoulderHipError) as ex:
            engine.vertex_fields(**kw)
        assert ex.value.code == code and "sh_vertex_fields" in str(ex.value) and "smooth_rounds in 0..64" in str(ex.value), kw
    with pytest.raises(ValueError):
        engine.vertex_fields(weight="volume")
    assert engine.vertex_fields(smooth=64)["status"][0] == 0
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            engine.vertex_fields()
        assert ex.value.code == O.STATE and "in flight" in str(ex.value) and "sh_vertex_fields" in str(ex.value)
    finally:
        engine.collect()
    engine.upload([(v, f)])                                                           # "vert.*" answer for their batch
    for name in ("vert.face", "vert.normal", "vert.fields", "vert.flags", "vert.status", "vert.a2", "vert.plane", "vert.state", "topo.vrow"):
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)
    assert engine.vertex_fields()["area"].tobytes() == first["area"].tobytes()       # on a fresh upload: the topology runs first


def test_a_topology_out_of_rounds_is_accepted(engine, cases):
    mesh = cases["strip of 600, shuffled"]
    engine.upload([mesh])
    info = engine.topology(max_rounds=4)[0][0]
    assert info["status"] == TO.CAPACITY
    got = device(engine, [mesh], upload=False)[0]
    O.compare(got, O.vertex_fields(*mesh), "strip after a topology out of rounds", show=False)


def test_the_facade(engine):
    engine.reset_params()
    try:
        h = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        c = h.curvature(smooth=4)
        assert (c["k1"] >= c["k2"]).all() and not any(np.isnan(c[k]).any() for k in ("k1", "k2", "gauss", "mean", "normals")) and not c["border"].any()
        convex = float((h.curvature()["mean"] > 0).mean())
        assert 0.75 <= convex <= 0.90
        n = h.vertex_normals()
        assert n.shape == c["normals"].shape and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
        assert float(O._dot(n, c["normals"]).mean()) > 0.99      # the angle-weighted normals against the area-weighted: the same surface
    finally:
        engine.reset_params()
