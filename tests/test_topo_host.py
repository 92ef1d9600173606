"""Mesh topology of the resident batch (include/shoulder_hip.h sh_mesh_topology), the parts that need no GPU (the record layouts:
test_abi_exports.py): the NumPy statement of tests/topo_oracle.py against the figures a CPU run of the rule gave (conditions on
the oracle), the host twin of the kernels (the device source's scalar rules, host-compiled through tests/hostcheck/topo_check.cpp)
against the oracle as bytes, the argument checks and the buffer plan.

Bounds.  Everything is an integer but the box corners, which are minima and maxima of float32 under a total order: bytes.  Every input
except the capacity case finishes within max_rounds = 32 in the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import topo_oracle as O
from conftest import BONES
from mass_oracle import int_box
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

FIXTURES = ["humerus_left", "humerus_left_flipped", "humerus_right", "humerus_left_trab", "proximal_left_cut"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("topo_check"))


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for n in FIXTURES:
        v, f = load_stl(os.path.join(BONES, n + ".stl"))
        out[n] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    out["box"] = int_box()
    return out


@pytest.fixture(scope="module")
def table(meshes):
    return O.table(meshes, big=True)


@pytest.fixture(scope="module")
def oracle(table, meshes):
    """the oracle's buffers of every row of the table and every further case, computed once"""
    out = {name: O.topology(*mesh) for name, (mesh, _) in table.items()}
    out.update({name: O.topology(*mesh) for name, mesh in O.further(meshes).items()})
    return out


def test_the_oracle_shows_the_figures_of_the_table(table, oracle):
    """conditions on the oracle: the counts and the rounds of every row, and the second way to the labels (held equal inside it)"""
    for name, (mesh, figures) in table.items():
        info = oracle[name]["info"]
        O.holds(info, figures, len(mesh[1]))
        assert info["rounds"] <= O.MAX_ROUNDS, name
    left = oracle["humerus_left"]
    assert left["info"]["flags"] == 3 and left["info"]["euler"] == 2 and oracle["humerus_left_trab"]["info"]["flags"] == 3
    assert oracle["humerus_left_flipped"]["info"]["flags"] == 3      # flipped as a whole: every edge still runs both ways
    assert oracle["humerus_left, shuffled"]["info"]["rounds"] in (10, 11, 12)
    # why the rule is FastSV: the plain minimum over neighbours needs hundreds of rounds on a shuffled mesh
    adj = oracle["strip of 600, shuffled"]["adj"].reshape(-1, 3)
    assert O.naive_rounds(adj) > 100 and oracle["strip of 600, shuffled"]["info"]["rounds"] == 11
    # the shells of the bone with 40 loose triangles in front: the triangles first, one face each, the bone last and largest
    t = oracle["humerus_left + 40 loose triangles in front"]
    assert (t["shells"]["faces"][:40] == 1).all() and (t["shells"]["border_slots"][:40] == 3).all() and t["info"]["largest_shell"] == 40
    assert t["shells"][40]["faces"] == 32440 and t["shells"][40]["first_face"] == 40 and t["shells"][40]["manifold_edges"] == 48660
    assert t["shells"][40]["lo"].tobytes() == left["shells"][0]["lo"].tobytes() and t["shells"][40]["hi"].tobytes() == left["shells"][0]["hi"].tobytes()


def same(shim, name, mesh, want, **kw):
    got = O.host_topology(shim, *mesh, **kw)
    for n in O.NAMES:
        assert got[n].tobytes() == want[n].tobytes(), (name, "topo." + n, got["info"], want["info"])
    return got


def test_host_twin_gives_the_oracle_bytes(shim, table, meshes, oracle):
    for name, (mesh, _) in table.items():
        same(shim, name, mesh, oracle[name])
    for name, mesh in O.further(meshes).items():
        same(shim, name, mesh, oracle[name])


def test_further_cases(shim, meshes, oracle):
    t = oracle["boxes sharing an edge"]
    assert t["info"]["nonmanifold_edges"] == 1 and (t["adj"] == O.NONMANIFOLD).sum() == 4 and t["info"]["n_shells"] == 2 and t["info"]["edges"] == 35
    assert not t["info"]["flags"] & O.WATERTIGHT and (t["shells"]["nonmanifold_slots"][:2] == 2).all()
    # degenerate faces in front, in the middle, on both sides of a 256 boundary and at the end
    where = np.array((0, 1, 100, 255, 256, 300, 519))
    v, f = O.further(meshes)["degenerate faces"]
    t, plain = oracle["degenerate faces"], oracle["humerus_left[:513]"]
    assert len(f) == 520 and (t["label"][where] == -1).all() and (t["adj"].reshape(-1, 3)[where] == O.DEGENERATE).all() and t["info"]["faces_degenerate"] == 7
    for k in ("edges", "border_edges", "n_shells", "largest_faces", "euler", "vertices_used", "max_valence"):
        assert t["info"][k] == plain["info"][k], k      # they take no part in anything else
    assert not t["info"]["flags"] & O.WATERTIGHT and np.array_equal(np.delete(t["label"], where), plain["label"])
    assert (t["vface"][-21:] == -1).all() and t["vface"][-22] >= 0 and t["vrow"][-1] == 3 * 513
    # a degenerate face between two faces leaves them neighbours; one that replaces a face makes its neighbours' slots border
    bv, bf = meshes["box"]
    holed = bf.copy()
    holed[0] = (0, 0, 1)
    t = O.topology(bv, holed)
    same(shim, "box with face 0 degenerate", (bv, holed), t)
    assert t["info"]["border_edges"] == 3 and t["info"]["faces_degenerate"] == 1 and t["label"][0] == -1 and (t["adj"] == O.BORDER).sum() == 3
    t = oracle["only degenerate faces"]
    assert t["info"]["n_shells"] == 0 and t["info"]["status"] == 0 and t["info"]["largest_shell"] == -1 and (t["label"] == -1).all() and t["info"]["rounds"] == 1


def test_out_of_rounds(shim, oracle):
    """the strip of 600 needs 11 rounds: with 4 it has the status, labels -1 and no shell records; adjacency and counts intact"""
    mesh = O.strip(600)
    full = oracle["strip of 600"]
    for rounds in (4, 10):
        want = O.topology(*mesh, max_rounds=rounds)
        got = same(shim, ("strip", rounds), mesh, want, max_rounds=rounds)
        i = got["info"]
        assert i["status"] == O.CAPACITY and i["rounds"] == rounds and i["n_shells"] == 0 and i["shells_written"] == 0 and i["largest_shell"] == -1
        assert (got["label"] == -1).all() and not np.frombuffer(got["shells"].tobytes(), np.uint8).any()
        assert got["adj"].tobytes() == full["adj"].tobytes() and got["vface"].tobytes() == full["vface"].tobytes() and got["vrow"].tobytes() == full["vrow"].tobytes()
        assert all(i[k] == full["info"][k] for k in ("edges", "border_edges", "inconsistent_edges", "euler", "max_valence", "vertices_used", "flags"))
    same(shim, "strip, 11 rounds", mesh, full, max_rounds=11)
    # the shell capacity: n_shells exact, the first records only
    many = O.join(O.loose_triangles(40), int_box())
    want = O.topology(*many, max_shells=8)
    got = same(shim, "41 shells, 8 records", many, want, max_shells=8)
    assert got["info"]["n_shells"] == 41 and got["info"]["shells_written"] == 8 and got["info"]["largest_shell"] == 40 and got["info"]["largest_faces"] == 12
    assert got["shells"].tobytes() == O.topology(*many)["shells"][:8].tobytes()


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)

    def pre(ctx=1, opt=1, max_shells=64, max_rounds=32, reserved=0, B=1, pending=0):
        code = shim.tc_precheck(ctx, opt, max_shells, max_rounds, reserved, B, pending, text, 256)
        return code, text.value.decode()
    assert pre() == (0, "")
    for kw in (dict(ctx=0), dict(opt=0)):      # the context and the pointer rank before the options, the options before the state
        code, msg = pre(max_shells=0, B=0, **kw)
        assert code == O.ARG and "must be given" in msg
    for kw in (dict(max_shells=0), dict(max_shells=O.MAX_SHELLS + 1), dict(max_rounds=0), dict(max_rounds=O.MAX_ROUNDS + 1), dict(reserved=1), dict(reserved=-1)):
        assert pre(B=0, **kw) == (O.ARG, "bad options (max_shells in 1..65536, max_rounds in 1..32, reserved 0)"), kw
    assert pre(max_shells=O.MAX_SHELLS, max_rounds=1)[0] == 0 and pre(max_shells=1, max_rounds=O.MAX_ROUNDS)[0] == 0
    assert pre(B=0) == (O.STATE, "no meshes uploaded") and pre(pending=1)[0] == O.STATE and "in flight" in pre(pending=1)[1]
    L = _lib.load()
    opt = _lib.TopologyOptions(64, 32, 0)
    assert L.sh_mesh_topology(None, ctypes.byref(opt), None, None) == O.ARG      # (no context)
    assert "sh_mesh_topology" in _lib.EXPORTS and _lib.TOPOLOGY_OPTIONS is _lib.TopologyOptions


def test_buffer_plan(shim):
    def plan(B, max_shells, maxF, sumV, sumF):
        out = np.zeros(11, dtype=np.uintp)
        shim.tc_plan(B, max_shells, maxF, sumV, sumF, out.ctypes.data)
        return [int(x) for x in out]
    # blocks, then the bytes of vrow, vface, adj, label, info, shells, state, cursor, tmp, p
    assert plan(3, 64, 513, 900, 1200) == [3, 903 * 4, 14400, 14400, 4800, 3 * 64, 3 * 64 * 48, 3 * 64 * 4, 903 * 4, 14400, 9600]
    assert plan(1, 1, 4, 4, 4) == [1, 20, 48, 48, 16, 64, 48, 256, 20, 48, 32]
    assert plan(1, 1, 256, 130, 256)[0] == 1 and plan(1, 1, 257, 130, 257)[0] == 2
    big = plan(64, O.MAX_SHELLS, 2080000, 64 * 1040002, 64 * 2080000)
    assert big[0] == 8125 and big[6] == 64 * 65536 * 48 and big[2] == 3 * 64 * 2080000 * 4 and big[1] == (64 * 1040002 + 64) * 4


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/topo_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "topo_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
