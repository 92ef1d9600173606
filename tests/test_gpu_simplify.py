"""Simplification of the resident batch (include/shoulder_hip.h sh_mesh_simplify, k_simplify.h) on the engine against the NumPy
statement of tests/simplify_oracle.py.

Bounds.  Keys, clusters, faces, map and counts are integer work; quadrics, positions and max_move are + - x / sqrt on float64 in a fixed
order: "simp.verts", "simp.faces", "simp.map" and "simp.info" are held to the oracle AS BYTES.  Two bounds are conditions of use, from
reasoning: the image of an input vertex is an output vertex, which lies on the output surface, so the distance of an input vertex to
the re-uploaded result is at most max_move, plus 1e-4 mm for the float32 positions and the closest-point arithmetic at some hundred mm;
the volume of the re-upload is the mass oracle's on the same mesh as bytes, as tests/test_gpu_mass.py holds it."""
import os

import numpy as np
import pytest

import mass_oracle as MO
import simplify_oracle as O
import vert_oracle as VO
import shoulder_amd as shoulder
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
RESIDENT = ("simp.verts", "simp.faces", "simp.map", "simp.info", "simp.state", "simp.seg", "simp.cell", "simp.key", "simp.sorted", "simp.ukey", "simp.start", "simp.cid",
            "simp.mark", "simp.rank", "simp.quad", "simp.pos", "simp.keep", "simp.frank", "simp.tmp")
FOUR = ("humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped")


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name in FOUR:
        v, f = load_stl(os.path.join(BONES, name + ".stl"))
        out[name] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    out["box"] = MO.int_box()
    out["icosphere"] = VO.icosphere(3)
    return out


@pytest.fixture(scope="module")
def oracle(meshes):
    """the oracle's answers, computed once and shared: (mesh name, cell, place) -> dict"""
    cache = {}

    def get(name, cell, place=O.QUADRIC):
        k = (name, float(cell), place)
        if k not in cache:
            cache[k] = O.simplify(*meshes[name], cell, place=place)
        return cache[k]
    return get


def device(engine, batch, cells, place="quadric", upload=True, **kw):
    """-> per mesh the dict of simplify_oracle.simplify (info, verts, faces, map), cut out of what Engine.simplify returned; what it
    returned is what is resident"""
    if upload:
        engine.upload(batch)
    B = len(batch)
    voff, foff = np.cumsum([0] + [len(v) for v, _ in batch]), np.cumsum([0] + [len(f) for _, f in batch])
    ms, info, vmap = engine.simplify(cells, place=place, **kw)
    assert info.shape == (B,) and vmap.shape == (voff[-1],) and len(ms) == B
    assert engine.fetch("simp.info", _lib.SIMPLIFY_INFO_DTYPE)[:B].tobytes() == info.tobytes()
    assert engine.fetch("simp.map", np.int32)[:voff[-1]].tobytes() == vmap.tobytes()
    sv, sf = engine.fetch("simp.verts", np.float32)[:3 * voff[-1]].reshape(-1, 3), engine.fetch("simp.faces", np.int32)[:3 * foff[-1]].reshape(-1, 3)
    for b in range(B):
        nv, nf = int(info[b]["verts_out"]), int(info[b]["faces_out"])
        assert sv[voff[b]:voff[b] + nv].tobytes() == ms[b][0].tobytes() and sf[foff[b]:foff[b] + nf].tobytes() == ms[b][1].tobytes()
        assert not sv[voff[b] + nv:voff[b + 1]].any() and not sf[foff[b] + nf:foff[b + 1]].any()          # the tail of a region is zero
    return [dict(info=info[b], verts=ms[b][0], faces=ms[b][1], map=vmap[voff[b]:voff[b + 1]]) for b in range(B)]


@pytest.mark.parametrize("place,tag", [(O.QUADRIC, "quadric"), (O.MEAN, "mean")])
def test_the_bone_against_the_oracle(engine, meshes, oracle, place, tag):
    """2 mm: 7 590 clusters, 61 of which fall back to the mean (both branches of the solve); 8 mm: a cluster of 118 members, more than a
    wave.  One batch, a cell per mesh."""
    bone = meshes["humerus_left"]
    got = device(engine, [bone, bone], [2.0, 8.0], place=tag)
    for b, h in enumerate((2.0, 8.0)):
        want = oracle("humerus_left", h, place)
        O.same_bytes(got[b], want, ("humerus_left", h, tag))
    assert got[1]["info"]["largest_cluster"] == 118 and got[0]["info"]["clusters"] == 7590 and got[0]["info"]["fallbacks"] == (61 if place == O.QUADRIC else 0)


def test_the_icosphere_comes_back_watertight(engine, meshes, oracle):
    """the test that cannot pass without the feature: the simplified sphere, uploaded again, is watertight and consistent"""
    ico = meshes["icosphere"]
    got = device(engine, [ico, ico], [5.0, 10.0])
    for b, h in enumerate((5.0, 10.0)):
        O.same_bytes(got[b], oracle("icosphere", h), ("icosphere", h))
    assert (int(got[0]["info"]["verts_out"]), int(got[0]["info"]["faces_out"])) == (339, 674)
    assert (int(got[1]["info"]["clusters"]), int(got[1]["info"]["verts_out"]), int(got[1]["info"]["faces_out"])) == (93, 90, 176)
    engine.upload([(g["verts"], g["faces"]) for g in got])
    info, _ = engine.topology()
    for b in range(2):
        assert info[b]["flags"] == _lib.TOPO_WATERTIGHT | _lib.TOPO_CONSISTENT and info[b]["euler"] == 2 and info[b]["border_edges"] == 0 and info[b]["nonmanifold_edges"] == 0


def test_a_ragged_batch_equals_single_uploads(engine, meshes, oracle):
    names = FOUR + ("icosphere",)
    cells = [2.0, 3.0, 4.0, 8.0, 5.0]
    got = device(engine, [meshes[n] for n in names], cells)
    for b, (n, h) in enumerate(zip(names, cells)):
        O.same_bytes(got[b], oracle(n, h), ("ragged", n, h))
    for b in (1, 4):
        alone = device(engine, [meshes[names[b]]], cells[b])[0]
        O.same_bytes(alone, got[b], ("alone", names[b]))


def test_the_same_call_twice(engine, meshes):
    engine.upload([meshes["humerus_left"], meshes["icosphere"]])
    engine.topology()
    keep = ("verts", "faces", "topo.vrow", "topo.vface", "topo.adj", "topo.label", "topo.info", "topo.shells")
    before = [engine.fetch(n, np.uint8).tobytes() for n in keep]
    engine.simplify([2.0, 5.0])
    first = [engine.fetch(n, np.uint8).tobytes() for n in RESIDENT[:4]]
    engine.simplify([2.0, 5.0])
    assert [engine.fetch(n, np.uint8).tobytes() for n in RESIDENT[:4]] == first
    assert [engine.fetch(n, np.uint8).tobytes() for n in keep] == before


def test_small_shapes_against_the_oracle(engine, meshes):
    """255 / 256 / 257 faces: a block of the face kernels less one, full, and one more; unused vertices, degenerate and zero-area faces;
    two sheets half a millimetre apart, where every second face is a duplicate and the smaller index stays"""
    batch = [O.strip_of(255), O.strip_of(256), O.strip_of(257), O.awkward(meshes["box"]), O.two_sheets(), meshes["box"]]
    cells = [1.5, 1.5, 0.5, 5.0, 2.0, 5.0]
    got = device(engine, batch, cells)
    for b, (m, h) in enumerate(zip(batch, cells)):
        O.same_bytes(got[b], O.simplify(*m, h), ("small", b))
    assert got[3]["map"][0] == -1 and got[3]["info"]["verts_used"] == 10
    sheets = got[4]["info"]
    assert sheets["faces_duplicate"] == sheets["faces_out"] > 0
    got = device(engine, batch, cells, place="mean", upload=False)
    for b, (m, h) in enumerate(zip(batch, cells)):
        O.same_bytes(got[b], O.simplify(*m, h, place=O.MEAN), ("small, mean", b))


def test_one_cluster_and_a_refused_grid_beside_a_box(engine, meshes):
    """a cell above the diagonal: one cluster, every face collapsed, SH_ERR_GEOMETRY; a cell that asks for more than 2^20 cells on an
    axis: SH_ERR_CAPACITY for that mesh alone; the box between them is untouched by either"""
    box = meshes["box"]
    ext = float((box[0].max(axis=0) - box[0].min(axis=0)).max())
    cells = [1000.0, 5.0, ext / (O.MAX_CELLS + 1)]
    got = device(engine, [box, box, box], cells)
    for b, h in enumerate(cells):
        O.same_bytes(got[b], O.simplify(*box, h), ("box", h))
    assert got[0]["info"]["status"] == O.GEOMETRY and got[0]["info"]["clusters"] == 1 and got[0]["info"]["faces_out"] == 0
    assert got[1]["info"]["status"] == 0 and got[1]["info"]["faces_out"] == 12
    assert got[2]["info"]["status"] == O.CAPACITY and (got[2]["map"] == -1).all()


def test_the_result_is_usable(engine, meshes, oracle):
    """re-upload the 2 mm bone: every input vertex is within max_move of it, and its volume is the oracle's on the same mesh"""
    bone = meshes["humerus_left"]
    want = oracle("humerus_left", 2.0)
    got = device(engine, [bone], 2.0)[0]
    O.same_bytes(got, want, "humerus_left at 2 mm")
    engine.upload([(got["verts"], got["faces"])])
    near = engine.closest_points(bone[0].astype(np.float64))[0]
    assert (near["status"] == 0).all()
    print("largest distance of an input vertex to the result %.4f mm, max_move %.4f mm" % (float(near["dist"].max()), float(got["info"]["max_move"])))
    assert float(near["dist"].max()) <= float(got["info"]["max_move"]) + 1e-4
    vol, ref = engine.mass_properties()[0]["volume"], MO.mass(want["verts"], want["faces"])[0]["volume"]
    print("volume of the re-upload %.6f mm^3, the oracle's %.6f" % (float(vol), float(ref)))
    assert vol.tobytes() == ref.tobytes()


def test_simplify_to_a_face_count(engine, meshes):
    bone = meshes["humerus_left"]
    engine.upload([bone])
    ms, info, vmap = engine.simplify_to(5000)
    h = float(info[0]["cell"])
    assert info[0]["status"] == 0 and 0 < info[0]["faces_out"] <= 5000
    print("simplify_to(5000): cell %.6f mm, %d faces" % (h, int(info[0]["faces_out"])))
    again = device(engine, [bone], h, upload=False)[0]
    got = dict(info=info[0], verts=ms[0][0], faces=ms[0][1], map=vmap)
    O.same_bytes(got, again, "simplify_to against simplify at its cell")
    O.same_bytes(got, O.simplify(*bone, h), "simplify_to against the oracle at its cell")


def test_the_facade(engine):
    engine.reset_params()
    try:
        h = shoulder.Humerus(os.path.join(BONES, "humerus_left.stl"), engine=engine)
        verts, faces = h.simplified_mesh(cell=4.0)          # (the bone is in CT: the current coordinate system is the upload's)
        want = O.simplify(np.asarray(h._verts, np.float32), np.asarray(h._faces, np.int32), 4.0)
        assert verts.dtype == np.float64 and faces.dtype == np.int32 and faces.tobytes() == want["faces"].tobytes()
        assert verts.astype(np.float32).tobytes() == want["verts"].tobytes()
        v2, f2 = h.simplified_mesh(target_faces=3000, place="mean")
        assert 0 < len(f2) <= 3000 and f2.max() == len(v2) - 1
        with pytest.raises(ValueError):
            h.simplified_mesh()
        with pytest.raises(ValueError):
            h.simplified_mesh(cell=2.0, target_faces=100)
    finally:
        engine.reset_params()


def test_lifetime_and_refusals(engine, meshes):
    fresh = Engine(0)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            fresh.simplify(2.0)
        assert ex.value.code == O.STATE and "sh_mesh_simplify" in str(ex.value) and "no meshes" in str(ex.value)
    finally:
        fresh.close()
    v, f = meshes["humerus_left"]
    engine.reset_params()
    engine.upload([(v, f)])
    opt = np.zeros(1, dtype=_lib.SIMPLIFY_OPTIONS_DTYPE)
    opt["place"], opt["reg"], opt["clamp"] = 1, 1e-3, 1.0
    cell = np.array([2.0])
    call = lambda o, c: engine.L.sh_mesh_simplify(engine.h, o.ctypes.data, c.ctypes.data if c is not None else None, None, None, None, None)
    assert call(opt, cell) == O.STATE                                                      # the C call without a topology refuses; the engine's runs one first
    assert b"sh_mesh_simplify: no incidence of the resident batch: call sh_mesh_topology first" in engine.L.sh_last_error(engine.h)
    assert call(opt, None) == O.ARG and b"sh_mesh_simplify" in engine.L.sh_last_error(engine.h) and b"cell" in engine.L.sh_last_error(engine.h)
    first = engine.simplify(2.0)
    assert first[1][0]["status"] == 0
    for kw in (dict(place=2), dict(place=-1), dict(reg=-0.1), dict(reg=1.5), dict(reg=np.nan), dict(clamp=0.0), dict(clamp=np.inf)):
        with pytest.raises(ShoulderHipError) as ex:
            engine.simplify(2.0, **kw)
        assert ex.value.code == O.ARG and "sh_mesh_simplify: bad options" in str(ex.value), kw
    for bad in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(ShoulderHipError) as ex:
            engine.simplify(bad)
        assert ex.value.code == O.ARG and "sh_mesh_simplify" in str(ex.value) and "cell[0]" in str(ex.value), bad
    opt["reserved"] = 1
    assert call(opt, cell) == O.ARG
    with pytest.raises(ValueError):
        engine.simplify(2.0, place="median")
    with pytest.raises(ValueError):
        engine.simplify([2.0, 3.0])
    engine.submit(_lib.STAGE_ALL, fetch=False)
    try:
        with pytest.raises(ShoulderHipError) as ex:
            engine.simplify(2.0)
        assert ex.value.code == O.STATE and "in flight" in str(ex.value) and "sh_mesh_simplify" in str(ex.value)
    finally:
        engine.collect()
    engine.upload([(v, f)])                                                               # "simp.*" answer for their batch
    for name in RESIDENT:
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)
    again = engine.simplify(2.0)                                                          # on a fresh upload: the topology runs first
    assert again[1].tobytes() == first[1].tobytes() and again[0][0][0].tobytes() == first[0][0][0].tobytes()
    engine.store("verts", v)                                                              # ... and for their vertices
    for name in RESIDENT:
        with pytest.raises(ShoulderHipError):
            engine.fetch(name, np.uint8)
