"""Simplification of the resident batch (include/shoulder_hip.h sh_mesh_simplify), the parts that need no GPU: conditions on the NumPy
statement of tests/simplify_oracle.py, the host twin of the kernels (the device source's scalar rules, host-compiled through
tests/hostcheck/simplify_check.cpp, with the kernels' sorts, bisection and row walk) against the oracle, the argument checks, the buffer
plan and the layout of the records.

Bounds.  Keys, cluster numbers, faces, map and counts are integer work; quadrics, positions and max_move are + - x / sqrt on float64 in
a fixed order: every comparison of the twin with the oracle is on bytes.  The figures of the bone are what this oracle gives (printed
below); the integers are those of the issue's table, the volume changes are not the prototype's (see test_the_table_of_the_bone).
max_move: a vertex and its cluster's position lie in one cell, clamped to max(1, clamp) of it, so they are at most the cell's diagonal
sqrt(3) h max(1, clamp) apart, up to the float32 rounding of the position (2^-24 of a coordinate of some hundred mm, below 1e-4)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mass_oracle as MO
import simplify_oracle as O
import topo_oracle as TO
import vert_oracle as VO
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

TWIN = ("info", "verts", "faces", "map", "key", "cid", "quad", "pos")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("simplify_check"))


@pytest.fixture(scope="module")
def bone():
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


@pytest.fixture(scope="module")
def table(bone):
    """the oracle on the bone at 1, 2, 4 and 8 mm, both placements: computed once"""
    return {(h, p): O.simplify(*bone, h, place=p) for h in (1.0, 2.0, 4.0, 8.0) for p in (O.MEAN, O.QUADRIC)}


def bound(info, clamp=1.0):
    return np.sqrt(3.0) * float(info["cell"]) * max(1.0, clamp) + 1e-4


def both(shim, mesh, cell, tag, **kw):
    want = O.simplify(*mesh, cell, **kw)
    O.same_bytes(O.host_simplify(shim, *mesh, cell, **kw), want, tag, TWIN)
    assert want["info"]["max_move"] <= bound(want["info"], kw.get("clamp", 1.0)), tag
    return want


def test_the_table_of_the_bone(table, bone):
    """exact integers at 1, 2, 4 and 8 mm (clusters, faces, duplicates: the issue's table; fallbacks and the largest cluster: the
    issue's test list) and both volumes.  A clustered bone has border edges, so its volume depends on the point it is taken about: the
    table's changes are about the origin of the CT coordinates (trimesh's mesh.volume), held here to the table's rounding; the changes
    about the mesh's own reference point (sh_mass_properties) are printed beside them."""
    V0 = O.volume(*bone)
    assert len(bone[0]) == 16222 and len(bone[1]) == 32440 and abs(V0 - 183371.55) < 0.01 and abs(O.volume_about_origin(*bone) - V0) < 1e-6 * V0
    want = {1.0: (14130, 28276, 26, -0.08, -0.07), 2.0: (7590, 15241, 101, -0.49, -0.15), 4.0: (2463, 4979, 125, -2.9, 0.39), 8.0: (650, 1312, 44, -12.0, -5.7)}
    change = {}
    for (h, p), r in table.items():
        i = r["info"]
        assert (int(i["clusters"]), int(i["faces_out"]), int(i["faces_duplicate"])) == want[h][:3] and i["status"] == 0 and i["verts_used"] == 16222, (h, p)
        assert i["verts_out"] == i["clusters"] and i["faces_collapsed"] + i["faces_duplicate"] + i["faces_out"] == 32440
        assert i["max_move"] <= bound(i)
        change[(h, p)] = O.volume_about_origin(r["verts"], r["faces"]) - V0
        print(f"humerus_left at {h:g} mm, place {p}: clusters {int(i['clusters'])} faces {int(i['faces_out'])} duplicates {int(i['faces_duplicate'])} fallbacks "
              f"{int(i['fallbacks'])} largest {int(i['largest_cluster'])} volume {100.0 * change[(h, p)] / V0:+.3f} % about the origin, "
              f"{100.0 * (O.volume(r['verts'], r['faces']) / V0 - 1.0):+.3f} % about its own point, max_move {float(i['max_move']):.3f}")
    digits = {1.0: (2, 2), 2.0: (2, 2), 4.0: (1, 2), 8.0: (1, 1)}                             # the decimals the table gives each change with
    for h in want:
        for p, col in ((O.MEAN, 0), (O.QUADRIC, 1)):
            assert abs(100.0 * change[(h, p)] / V0 - want[h][3 + col]) <= 0.5 * 10.0 ** -digits[h][col] + 1e-9, (h, p)
    for h in (2.0, 4.0, 8.0):
        assert abs(change[(h, O.QUADRIC)]) < abs(change[(h, O.MEAN)]), h
    assert table[(2.0, O.QUADRIC)]["info"]["fallbacks"] == 61 and table[(8.0, O.QUADRIC)]["info"]["largest_cluster"] == 118
    assert O.edges_left(table[(2.0, O.QUADRIC)]["verts"], table[(2.0, O.QUADRIC)]["faces"])[:2] == (104, 166)
    for (h, p), r in table.items():      # the placements share everything but the positions
        assert r["faces"].tobytes() == table[(h, O.MEAN)]["faces"].tobytes() and r["map"].tobytes() == table[(h, O.MEAN)]["map"].tobytes()


def test_host_twin_against_the_oracle_on_the_bone(shim, bone, table):
    for (h, p), want in table.items():
        O.same_bytes(O.host_simplify(shim, *bone, h, place=p), want, ("humerus_left", h, p), TWIN)
    both(shim, bone, 3.0, "reg 0, clamp 2", reg=0.0, clamp=2.0)
    both(shim, bone, 3.0, "reg 1, clamp 0.25", reg=1.0, clamp=0.25)


def test_the_icosphere_stays_closed(shim):
    sv, sf = VO.icosphere(3)
    for h, figures in ((5.0, (339, 339, 674)), (10.0, (93, 90, 176))):
        r = both(shim, (sv, sf), h, ("icosphere", h))
        i = r["info"]
        assert (int(i["clusters"]), int(i["verts_out"]), int(i["faces_out"])) == figures and O.edges_left(r["verts"], r["faces"]) == (0, 0, 2)
        assert TO.topology(r["verts"], r["faces"])["info"]["flags"] == TO.WATERTIGHT | TO.CONSISTENT
        assert len(np.unique(r["faces"])) == len(r["verts"])                                  # no unreferenced vertex: the drop rule at 10 mm
        dropped = np.setdiff1d(np.arange(int(i["clusters"])), r["cid"][sf[kept_faces(r, sf)]])
        assert len(dropped) == (0 if h == 5.0 else 3) and int((r["map"] == -1).sum()) == int(np.isin(r["cid"], dropped).sum())

def kept_faces(r, faces):
    """the input faces that stay: not collapsed, and the first of their set"""
    tri = r["cid"][faces]
    ok = np.nonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2]))[0]
    _, first = np.unique(np.sort(tri[ok], axis=1), axis=0, return_index=True)
    return ok[np.sort(first)]


def test_small_shapes(shim):
    box = MO.int_box()
    r = both(shim, box, 5.0, "box, mean", place=O.MEAN)
    assert r["info"]["clusters"] == 8 and r["faces"].shape == (12, 3) and r["info"]["max_move"] == 0.0 and r["verts"].tobytes() == box[0][np.argsort(r["map"])].tobytes()
    r = both(shim, box, 1000.0, "box, one cluster")
    assert r["info"]["status"] == O.GEOMETRY and r["info"]["clusters"] == 1 and r["info"]["faces_collapsed"] == 12 and r["info"]["faces_out"] == 0 and (r["map"] == -1).all()
    r = both(shim, O.two_sheets(), 2.0, "two sheets")
    i = r["info"]
    assert i["faces_duplicate"] == i["faces_out"] > 0 and i["largest_cluster"] >= 2
    v, f = O.two_sheets()
    kept = kept_faces(r, f)
    assert (kept % 2 == 0).all()                                                              # the smaller index of every pair stays
    for nf in (255, 256, 257):
        m = O.strip_of(nf)
        assert len(m[1]) == nf
        both(shim, m, 1.5, ("strip", nf))
        both(shim, m, 0.5, ("strip, fine", nf), place=O.MEAN)
    aw = O.awkward(box)
    r = both(shim, aw, 5.0, "awkward")
    assert r["info"]["verts_used"] == 10 and r["map"][0] == -1 and r["map"][9] == -1 and r["map"][10] == r["map"][1]
    assert r["info"]["faces_out"] == 13 and r["info"]["faces_collapsed"] == 1      # the zero-area face on the midpoint is no duplicate and stays; the one on the copy collapses
    empty = (box[0], np.zeros((4, 3), np.int32))
    r = both(shim, empty, 5.0, "no used vertex")
    assert r["info"]["status"] == O.GEOMETRY and r["info"]["verts_used"] == 0


def test_a_grid_too_fine_is_refused_for_that_mesh(shim, bone):
    box = MO.int_box()
    ext = float((box[0].max(axis=0) - box[0].min(axis=0)).max())
    r = both(shim, box, ext / (O.MAX_CELLS + 1), "2^20 + 1 cells")
    assert r["info"]["status"] == O.CAPACITY and r["info"]["verts_used"] == 8 and r["info"]["faces_out"] == 0 and len(r["verts"]) == 0 and (r["map"] == -1).all()
    r = both(shim, box, ext / (O.MAX_CELLS - 1), "2^20 cells", place=O.MEAN)
    assert r["info"]["status"] == 0 and r["info"]["clusters"] == 8
    assert O.simplify(*bone, 1e-5)["info"]["status"] == O.CAPACITY and O.simplify(*box, 5.0)["info"]["status"] == 0       # that mesh alone: the rule is per mesh


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)

    def pre(ctx=1, opt=1, place=1, reserved=0, reg=1e-3, clamp=1.0, cells=(2.0,), incidence=1, B=1, pending=0):
        c = np.asarray(cells, np.float64) if cells is not None else None
        code = shim.sc_precheck(ctx, opt, place, reserved, reg, clamp, int(c is not None), c.ctypes.data if c is not None else None, incidence, B, pending, text, 256)
        return code, text.value.decode()
    assert pre() == (0, "") and pre(place=0, reg=0.0, clamp=1e-9)[0] == 0 and pre(reg=1.0)[0] == 0
    assert pre(ctx=0, place=9, B=0)[0] == O.ARG and pre(opt=0, B=0) == (O.ARG, "bad argument (context and options must be given)")
    for kw in (dict(place=2), dict(place=-1), dict(reserved=1), dict(reg=-1e-9), dict(reg=1.5), dict(reg=np.nan), dict(reg=np.inf), dict(clamp=0.0), dict(clamp=-1.0),
               dict(clamp=np.inf), dict(clamp=np.nan)):
        code, msg = pre(B=0, incidence=0, cells=None, **kw)                                   # the options before everything else
        assert code == O.ARG and msg.startswith("bad options (place 0 or 1"), kw
    assert pre(cells=None, B=0)[0] == O.ARG and "cell" in pre(cells=None, B=0)[1]
    for bad in (0.0, -1.0, np.nan, np.inf):
        code, msg = pre(cells=(2.0, bad), B=2, pending=1, incidence=0)                         # the cells before the state
        assert code == O.ARG and "cell[1]" in msg, bad
    assert pre(B=0, incidence=0) == (O.STATE, "no meshes uploaded")                           # the batch before the incidence
    code, msg = pre(pending=1, incidence=0)
    assert code == O.STATE and "in flight" in msg
    assert pre(incidence=0) == (O.STATE, "no incidence of the resident batch: call sh_mesh_topology first")
    L = _lib.load()
    assert L.sh_mesh_simplify(None, None, None, None, None, None, None) == O.ARG
    assert "sh_mesh_simplify" in _lib.EXPORTS and _lib.SIGNATURES["sh_mesh_simplify"][2]
    assert (_lib.SIMPLIFY_MEAN, _lib.SIMPLIFY_QUADRIC, _lib.SIMPLIFY_MAX_CELLS, _lib.SIMPLIFY_MAX_CLUSTERS) == (O.MEAN, O.QUADRIC, O.MAX_CELLS, O.MAX_CLUSTERS)


def test_record_layout(shim):
    out = np.zeros(2 + 4 + 13, np.int32)
    shim.sc_sizes(out.ctypes.data)
    dtypes = (_lib.SIMPLIFY_OPTIONS_DTYPE, _lib.SIMPLIFY_INFO_DTYPE)
    assert [int(x) for x in out[:2]] == [d.itemsize for d in dtypes] == [24, 64]
    assert [int(x) for x in out[2:]] == [d.fields[n][1] for d in dtypes for n in d.names]
    assert _lib.SIMPLIFY_INFO_DTYPE == O.INFO_DTYPE and _lib.SIMPLIFY_INFO_DTYPE.fields["cell"][1] == 40


def test_buffer_plan(shim):
    voff, foff = np.array([0, 8, 308, 400], np.int64), np.array([0, 12, 612, 700], np.int64)
    out = np.zeros(3 + 4 + 18, dtype=np.uintp)
    assert shim.sc_plan(3, voff.ctypes.data, foff.ctypes.data, out.ctypes.data) == 0
    got = [int(x) for x in out]
    assert got[:7] == [3, 2, 3, 0, 8, 308, 400]                                               # blocks of 256: of either, of vertices, of faces; the segments
    v, f = 400, 700
    # verts, faces, map, info, state, seg, cell, key, sorted, ukey, start, cid, mark, rank, quad, pos, keep, frank
    assert got[7:] == [v * 12, f * 12, v * 4, 3 * 64, 3 * 20 * 4, 16, 24, v * 8, v * 8, v * 8, v * 4, v * 4, v * 4, v * 4, v * 80, v * 12, f * 4, f * 4]
    big = np.array([0, 2 ** 31], np.int64)
    assert shim.sc_plan(1, big.ctypes.data, foff[:2].ctypes.data, out.ctypes.data) == O.NOMEM


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/simplify_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "simplify_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
