"""Repair of the resident batch (include/shoulder_hip.h sh_mesh_repair), the parts that need no GPU: conditions on the NumPy statement of
tests/repair_oracle.py, the host twin of the kernels (the device source's scalar rules, host-compiled through
tests/hostcheck/repair_check.cpp, with the kernels' pointer doubling) against the oracle, the argument checks, the buffer plan and the
layout of the records.

Bounds.  Flips, V6, records, holes, output faces and output vertices are integer work or + - x / on float64 in a fixed order: every
comparison of the twin with the oracle is on bytes.  W is an atan2 sum: within winding_oracle.bound(F, sum |omega| / 4 pi).  The
volumes are conditions on the oracle: the refilled bone (fan) has 183 371.50 against 183 371.55 mm^3 (printed below; the fan flattens
the two removed one-rings), held to 1e-5 relative: a removed one-ring of a 32 440-face bone spans about 1e-4 of its area and bulges by
a fraction of an edge."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mass_oracle as MO
import repair_oracle as O
import stem_oracle as SO
import topo_oracle as TO
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("repair_check"))


@pytest.fixture(scope="module")
def meshes():
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    return {"humerus_left": (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)), "box": MO.int_box()}


@pytest.fixture(scope="module")
def cases(meshes):
    return O.small_cases(meshes)


def both(shim, mesh, tag, **kw):
    want = O.repair(*mesh, **kw)
    O.same_bytes(O.host_repair(shim, *mesh, **kw), want, tag)
    return want


def test_host_twin_against_the_oracle_small(shim, cases):
    for name, mesh in list(cases.items()) + list(O.lone_cases().items()):
        for tag, kw in O.VARIANTS:
            both(shim, mesh, (name, tag), **kw)


def test_small_shapes(cases):
    r = O.repair(*cases["mobius strip"])
    assert r["info"]["shells_nonorientable"] == 1 and r["shells"][0]["status"] == O.NONORIENTABLE and r["info"]["flags"] == 0 and not r["flip"].any()
    assert r["info"]["blocked_edges"] + int(r["holes"]["edges"].sum()) == 10 and r["info"]["holes_filled"] == 0 and r["faces"].tobytes() == cases["mobius strip"][1].tobytes()
    r = O.repair(*cases["fin on an open box"])
    assert r["info"]["holes"] == 0 and r["info"]["blocked_edges"] == 5 and r["info"]["faces_added"] == 0
    r = O.repair(*cases["box inside out"])
    assert r["shells"][0]["V6"] == -36000.0 and r["shells"][0]["inverted"] == 1 and r["faces"].tobytes() == cases["box"][1].tobytes()
    r = O.repair(*cases["box, face 5 flipped"], orient=O.WINDING)
    assert r["info"]["faces_flipped"] == 1 and r["flip"][5] == 1 and r["faces"].tobytes() == cases["box"][1].tobytes()
    assert O.repair(*cases["box, face 5 flipped"], orient=O.NONE)["faces"].tobytes() == cases["box, face 5 flipped"][1].tobytes()
    lone = O.lone_cases()
    r = O.repair(*lone["single triangle, alone"])
    assert r["info"]["holes"] == 1 and r["info"]["faces_out"] == 4 and r["info"]["verts_out"] == 5 and TO.topology(r["verts"], r["faces"])["info"]["flags"] == 3
    assert O.repair(*cases["single triangle"])["info"]["faces_out"] == 12 + 4
    r = O.repair(*lone["tetrahedron minus one face, alone"], fill=O.FAN)
    t = TO.topology(r["verts"], r["faces"])["info"]
    assert r["info"]["faces_added"] == 1 and t["flags"] == 3 and MO.mass(r["verts"], r["faces"])[0]["volume"] > 0.0
    r = O.repair(*cases["degenerate faces"])
    assert not r["flip"][TO.degenerate(cases["degenerate faces"][1])].any() and r["faces"][:2].tobytes() == cases["degenerate faces"][1][:2].tobytes()
    soup = O.repair(*TO.loose_triangles(100), max_holes=16)
    assert soup["info"]["holes"] == 100 and soup["info"]["holes_written"] == 16 and soup["info"]["flags"] == O.CHANGED | O.SHELLS_LEFT and soup["holes"][15]["edges"] == 3


def test_reversed_faces_and_inside_out(shim, meshes):
    v, f = meshes["humerus_left"]
    rf, mask = O.reversed_faces(f)
    assert TO.topology(v, rf)["info"]["inconsistent_edges"] == 20542
    r = both(shim, (v, rf), "30 % reversed")
    assert r["faces"].tobytes() == f.tobytes() and r["info"]["faces_flipped"] == int(mask.sum()) and r["levels"] == 311
    assert MO.mass(r["verts"], r["faces"])[0]["volume"].tobytes() == MO.mass(v, f)[0]["volume"].tobytes()
    r = both(shim, (v, np.ascontiguousarray(f[:, [0, 2, 1]])), "inside out")
    assert r["shells"][0]["V6"] < 0.0 and r["shells"][0]["inverted"] == 1 and r["faces"].tobytes() == f.tobytes()
    r = both(shim, (v, f), "out of levels", max_rounds=100)
    assert r["info"]["status"] == O.CAPACITY and r["faces"].tobytes() == f.tobytes()


def test_holes_of_the_bone(shim, meshes):
    v, f = meshes["humerus_left"]
    (hv, hf), gone = O.with_holes(v, f)
    r = both(shim, (hv, hf), "holes, fan", fill=O.FAN)
    assert r["info"]["holes"] == 5 and sorted(int(x) for x in r["holes"][:5]["edges"]) == [3, 3, 3, 5, 6] and len(gone) == 14
    rot = lambda t: min(tuple(int(x) for x in np.roll(t, k)) for k in range(3))
    assert {rot(r["faces"][int(h["first_face"])]) for h in r["holes"][:5] if h["edges"] == 3} == {rot(f[i]) for i in (100, 20000, 20001)}
    t = TO.topology(r["verts"], r["faces"])["info"]
    assert (t["border_edges"], t["nonmanifold_edges"], t["inconsistent_edges"], t["flags"]) == (0, 0, 0, 3)
    vol, whole = MO.mass(r["verts"], r["faces"])[0]["volume"], MO.mass(v, f)[0]["volume"]
    print(f"humerus_left with five holes, fan: volume {vol:.2f} against {whole:.2f} mm^3")
    assert abs(vol / whole - 1.0) <= 1e-5
    r = both(shim, (hv, hf), "holes, centroid")
    assert r["info"]["verts_added"] == 5 and TO.topology(r["verts"], r["faces"])["info"]["flags"] == 3
    r = both(shim, (hv, hf), "holes, reported", fill=O.FILL_NONE)
    assert r["info"]["holes"] == 5 and r["info"]["faces_added"] == 0 and set(r["holes"][:5]["status"]) == {O.HOLE_OPEN}


def test_two_holes_that_touch_in_a_vertex(shim, meshes):
    """two holes of 3, not one of 6: the rotation alone gives one cycle that passes the shared vertex twice; it is cut there.  Two sheets
    that touch in a vertex keep their own borders: their half-edges lie on different cycles."""
    mesh = O.touching_holes(*meshes["humerus_left"])
    r = both(shim, mesh, "touching holes", fill=O.FAN)
    print("touching holes: holes", int(r["info"]["holes"]), "edges", [int(x) for x in r["holes"][:2]["edges"]])
    assert r["info"]["holes"] == 2 and [int(x) for x in r["holes"][:2]["edges"]] == [3, 3]
    assert TO.topology(r["verts"], r["faces"])["info"]["flags"] == 3 and r["faces"].shape == meshes["humerus_left"][1].shape
    ids, succ = O.successors(*O.oriented(mesh[1], TO.adjacency(mesh[1])[0], np.zeros(len(mesh[1]), np.uint8)))
    assert [len(c) for c in O.cycles(succ)[0]] == [6]                                   # what the rotation alone gives
    # two open boxes that share vertex 0, each without a face at it: two sheets, two cycles, nothing to cut
    bv, bf = MO.int_box()
    fan0 = [i for i in range(12) if 0 in bf[i]]
    sheets = TO.boxes_sharing((bv, np.delete(bf, fan0[0], axis=0)), (0,))
    r = both(shim, sheets, "two sheets", fill=O.FAN)
    assert r["info"]["holes"] == 2 and [int(x) for x in r["holes"][:2]["edges"]] == [3, 3] and r["info"]["holes_filled"] == 2


@pytest.mark.parametrize("stored_inward", [True, False])
def test_nested_prisms(shim, stored_inward):
    vo, fo = SO.prism(130, 10.0, -6.0, 6.0, 0.011)
    vi, fi = SO.prism(130, 5.0, -3.0, 3.0, 0.011, reverse=stored_inward)
    mesh = (np.concatenate([vo, vi]).astype(np.float32), np.concatenate([fo, fi + len(vo)]).astype(np.int32))
    r = both(shim, mesh, "nested", orient=O.NESTED)
    assert [int(x) for x in r["shells"][:2]["depth"]] == [0, 1] and abs(r["shells"][1]["W"] - 1.0) < 1e-12 and r["shells"][1]["inverted"] == int(stored_inward)
    assert r["flip"][len(fo):].all() != stored_inward and not r["flip"][:len(fo)].any()       # the inner wall is left, or made, inward
    r = both(shim, mesh, "outward", orient=O.OUTWARD)
    assert [int(x) for x in r["shells"][:2]["depth"]] == [-1, -1] and r["flip"][len(fo):].all() == stored_inward
    # a shell whose first corner lies on another closed shell: W near a half, ambiguous, depth 0
    box = MO.int_box()
    r = both(shim, TO.boxes_sharing(box, (0,)), "shared vertex", orient=O.NESTED)
    assert r["shells"][1]["status"] == O.AMBIGUOUS or r["shells"][0]["status"] == O.AMBIGUOUS or abs(r["shells"][0]["W"]) <= 0.25


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)

    def pre(ctx=1, opt=1, orient=2, fill=2, edges=4096, holes=64, rounds=1000, reserved=0, topology=1, B=1, pending=0):
        code = shim.rc_precheck(ctx, opt, orient, fill, edges, holes, rounds, reserved, topology, B, pending, text, 256)
        return code, text.value.decode()
    assert pre() == (0, "") and pre(orient=0, fill=0, edges=3, holes=O.MAX_HOLES, rounds=O.MAX_ROUNDS)[0] == 0
    assert pre(ctx=0, orient=9, B=0)[0] == O.ARG and pre(opt=0, B=0) == (O.ARG, "bad argument (context and options must be given)")
    for kw in (dict(orient=4), dict(orient=-1), dict(fill=3), dict(fill=-1), dict(edges=2), dict(holes=0), dict(holes=O.MAX_HOLES + 1), dict(rounds=0),
               dict(rounds=O.MAX_ROUNDS + 1), dict(reserved=1)):
        code, msg = pre(B=0, topology=0, **kw)                                              # the options before the state
        assert code == O.ARG and msg.startswith("bad options (orient in 0..3"), kw
    assert pre(B=0, topology=0) == (O.STATE, "no meshes uploaded")                          # the batch before the topology
    code, msg = pre(pending=1, topology=0)
    assert code == O.STATE and "in flight" in msg
    assert pre(topology=0) == (O.STATE, "no topology of the resident batch: call sh_mesh_topology first")
    L = _lib.load()
    assert L.sh_mesh_repair(None, None, None, None, None, None) == O.ARG
    assert "sh_mesh_repair" in _lib.EXPORTS and _lib.SIGNATURES["sh_mesh_repair"][2]
    assert (_lib.REPAIR_NONE, _lib.REPAIR_WINDING, _lib.REPAIR_OUTWARD, _lib.REPAIR_NESTED, _lib.REPAIR_FILL_NONE, _lib.REPAIR_FAN, _lib.REPAIR_CENTROID) == (0, 1, 2, 3, 0, 1, 2)
    assert (_lib.REPAIR_MAX_HOLES, _lib.REPAIR_MAX_ROUNDS, _lib.REPAIR_LDS_FACES) == (O.MAX_HOLES, O.MAX_ROUNDS, O.LDS_FACES)


def test_record_layout(shim):
    """the four records of the header (two statements each, so the one probe of the header does not see them) against _lib's dtypes"""
    out = np.zeros(42, np.int32)
    shim.rc_sizes(out.ctypes.data)
    dtypes = (_lib.REPAIR_OPTIONS_DTYPE, _lib.REPAIR_INFO_DTYPE, _lib.REPAIR_SHELL_DTYPE, _lib.REPAIR_HOLE_DTYPE)
    assert [int(x) for x in out[:4]] == [d.itemsize for d in dtypes] == [24, 64, 40, 32]
    assert [int(x) for x in out[4:]] == [d.fields[n][1] for d in dtypes for n in d.names]
    assert _lib.REPAIR_INFO_DTYPE.names[:4] == ("status", "shells_nonorientable", "shells_inverted", "faces_flipped") and _lib.REPAIR_SHELL_DTYPE.fields["V6"][1] == 24


def test_buffer_plan(shim):
    voff, foff = np.array([0, 8, 308, 400], np.int64), np.array([0, 12, 312, 500], np.int64)
    info = np.zeros(3, dtype=_lib.TOPOLOGY_DTYPE)
    info["border_edges"] = (0, 302, 7)
    out = np.zeros(1 + 12 + 11, dtype=np.uintp)
    shim.rc_plan(3, 64, 16, voff.ctypes.data, foff.ctypes.data, info.ctypes.data, out.ctypes.data)
    got = [int(x) for x in out]
    # blocks; the starts of the faces, the vertices and the border arrays; the bytes of flip, faces, verts, info, shells, holes, off, par, work, edge, term
    assert got[:13] == [2, 0, 12, 614, 809, 0, 8, 408, 502, 0, 0, 302, 309]
    assert got[13:] == [500, 809 * 12, 502 * 12, 192, 3 * 64 * 40, 3 * 16 * 32, 96, 500, (2500 + 48) * 4, 18 * 309 * 4, 8000]


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/repair_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "repair_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
