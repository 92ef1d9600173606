"""Vertex normals and discrete curvatures of the resident batch (include/shoulder_hip.h sh_vertex_fields), the parts that need no GPU:
the NumPy statement of tests/vert_oracle.py against figures a prototype of the rule gave (conditions on the oracle), the host twin of
the kernels (the device source's scalar rules, host-compiled through tests/hostcheck/vert_check.cpp) against the oracle, the argument
checks and the buffer plan.

Bounds.  Everything but atan2 is + - x / sqrt on float64 in a fixed order: n, A2 and cot of the face records, area, the flags, the
status and, with area weights, the normals, mean and mean_smooth are held as bytes.  The angles and what they enter (angle_sum, defect,
gauss, gauss_smooth; with angle weights the normals, mean and mean_smooth) are held within vert_oracle.bound: 4 ulp per atan2 term, the
project's figure for two math libraries, and one rounding per later operation in each evaluation.  The host twin calls libm's atan2
and NumPy its own: the two already differ by an ulp or two, which the printed differences show; the bound is not tuned to either."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import topo_oracle as TO
import vert_oracle as O
from conftest import BONES
from mass_oracle import int_box
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

FIXTURES = ["humerus_left", "humerus_left_flipped", "humerus_right", "humerus_left_trab", "proximal_left_cut"]
TWO_PI = 6.283185307179586


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("vert_check"))


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for n in FIXTURES:
        v, f = load_stl(os.path.join(BONES, n + ".stl"))
        out[n] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    out["box"] = int_box()
    return out


@pytest.fixture(scope="module")
def left(meshes):
    """the oracle on humerus_left, area weights, 8 rounds: computed once"""
    return O.vertex_fields(*meshes["humerus_left"], smooth=8)


def ulps(x, y):
    return np.abs(x - y) / np.spacing(np.abs(y))


def test_box_conditions(meshes):
    r = O.vertex_fields(*meshes["box"])
    assert (ulps(r["defect"], np.pi / 2) <= 4).all() and (r["flags"] == O.USED).all() and r["status"] == 0
    want = np.array([550, 1000, 950, 800, 800, 950, 1000, 550]) / 3.0
    assert np.allclose(r["area"], want, rtol=1e-14, atol=0) and abs(r["area"].sum() - 2200.0) < 1e-9
    assert (r["mean"] > 0).all() and (r["gauss"] > 0).all()
    centre = meshes["box"][0].astype(np.float64).mean(axis=0)
    assert (O._dot(r["normals"], meshes["box"][0] - centre) > 0).all()
    # without face 0: its three corners are border vertices and use pi
    v, f = meshes["box"]
    r = O.vertex_fields(v, f[1:])
    b = (r["flags"] & O.BORDER) != 0
    assert b.sum() == 3 and set(np.nonzero(b)[0]) == set(int(x) for x in f[0])
    assert np.array_equal(r["defect"][b], 3.141592653589793 - r["angle_sum"][b]) and np.array_equal(r["defect"][~b], TWO_PI - r["angle_sum"][~b])


def test_gauss_bonnet(meshes):
    """sum defect / 2 pi is the Euler characteristic of topo_oracle.topology: 2 on the closed bones, 0 on the genus-1 mesh"""
    for name, euler in (("humerus_left", 2), ("humerus_right", 2), ("proximal_left_cut", 2), ("humerus_left_trab", 0)):
        assert int(TO.topology(*meshes[name])["info"]["euler"]) == euler
        r = O.vertex_fields(*meshes[name])
        dev = abs(r["defect"].sum() / TWO_PI - euler)
        print(f"{name}: |sum defect / 2 pi - euler| = {dev:.3g}")
        assert dev <= 1e-10, (name, dev)


def test_icosphere():
    R = 25.0
    for sub, nv in ((3, 642), (2, 162)):
        v, f = O.icosphere(sub, R)
        assert len(v) == nv
        for weight in (O.AREA, O.ANGLE):
            r = O.vertex_fields(v, f, weight=weight)
            g, m = r["gauss"] * R * R, r["mean"] * R
            print(f"icosphere {sub} weight {weight}: gauss R^2 {g.min():.4f} .. {g.max():.4f}, mean R {m.min():.4f} .. {m.max():.4f}")
            assert g.min() >= 0.99 and g.max() <= 1.16 and m.min() >= 0.99 and m.max() <= 1.16
            assert (O._dot(r["normals"], v.astype(np.float64)) > 0.999 * R).all()      # outward
        assert (r["flags"] == O.USED).all() and abs(r["defect"].sum() / TWO_PI - 2) < 1e-12


def test_swapping_two_columns_negates_normals_and_mean_as_bytes(meshes, left):
    v, f = meshes["humerus_left"]
    a = left
    b = O.vertex_fields(v, np.ascontiguousarray(f[:, [0, 2, 1]]), smooth=8)
    assert (-b["normals"]).tobytes() == a["normals"].tobytes() and (-b["mean"]).tobytes() == a["mean"].tobytes()
    for n in ("area", "angle_sum", "defect", "gauss", "flags"):
        assert b[n].tobytes() == a[n].tobytes(), n
    # (not the smoothed fields: a face's mean is ((s[f0] + s[f1]) + s[f2]) / 3, and the swap changes which two are added first)
    assert np.allclose(b["gauss_smooth"], a["gauss_smooth"], rtol=1e-12, atol=1e-15) and np.allclose(-b["mean_smooth"], a["mean_smooth"], rtol=1e-12, atol=1e-15)


def test_humerus_conditions(left):
    convex = float((left["mean"] > 0).mean())
    print(f"humerus_left: {100 * convex:.1f} % convex, median mean {np.median(left['mean']):.4f} / mm")
    assert 0.75 <= convex <= 0.90
    assert left["mean_smooth"].std() < left["mean"].std()
    a, b = (left["gauss_smooth"] * left["area"]).sum(), (left["gauss"] * left["area"]).sum()
    print(f"humerus_left, 8 rounds: sum gauss_smooth area {a:.6f}, sum gauss area {b:.6f}")
    assert abs(a - b) <= 0.01 * abs(b)
    none = O.vertex_fields(*int_box())      # without a round the smoothed fields are the raw ones
    assert none["gauss_smooth"].tobytes() == none["gauss"].tobytes() and none["mean_smooth"].tobytes() == none["mean"].tobytes()


def test_flat_and_degenerate_faces(meshes):
    cases = O.small_cases(meshes)
    r = O.vertex_fields(*cases["box with a flat face"])
    plain = O.vertex_fields(*meshes["box"])
    assert r["status"] == 0 and r["flags"][8] == (O.USED | O.BORDER | O.FLAT) and not r["fields"][8].any() and not r["normals"][8].any() and not r["face"][12].any()
    assert (r["flags"][:2] & O.FLAT).all() and (r["flags"][:2] & O.NONMANIFOLD).all()
    # the flat face adds nothing to a sum; its border slots at corners 0 and 1 make those two use pi
    assert r["fields"][:8][:, [0, 1, 4]].tobytes() == plain["fields"][:, [0, 1, 4]].tobytes() and r["fields"][2:8, :5].tobytes() == plain["fields"][2:, :5].tobytes()
    assert np.array_equal(r["defect"][:2], 3.141592653589793 - r["angle_sum"][:2])
    r = O.vertex_fields(*cases["only degenerate faces"], weight=O.ANGLE, smooth=2)
    assert r["status"] == O.GEOMETRY and not r["fields"].any() and not r["normals"].any() and not r["flags"].any() and not r["face"].any()
    nm = O.vertex_fields(*cases["boxes sharing an edge"])
    assert ((nm["flags"] & O.NONMANIFOLD) != 0).sum() == 2 and not (nm["flags"] & O.BORDER).any()


def test_host_twin_against_the_oracle(shim, meshes):
    shuffled = TO.further(meshes)["humerus_left, shuffled"]
    runs = [(n, m, w, 3) for n, m in O.small_cases(meshes).items() for w in (O.AREA, O.ANGLE)]
    runs += [("humerus_left", meshes["humerus_left"], O.AREA, 8), ("humerus_left", meshes["humerus_left"], O.ANGLE, 8),
             ("humerus_left_trab", meshes["humerus_left_trab"], O.ANGLE, 1), ("proximal_left_cut", meshes["proximal_left_cut"], O.AREA, 1),
             ("humerus_left, shuffled", shuffled, O.ANGLE, 0)]
    for name, mesh, weight, smooth in runs:
        want = O.vertex_fields(*mesh, weight=weight, smooth=smooth)
        O.compare(O.host_fields(shim, *mesh, weight=weight, smooth=smooth), want, name)


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)

    def pre(ctx=1, weight=0, smooth=0, incidence=1, B=1, pending=0):
        code = shim.vc_precheck(ctx, weight, smooth, incidence, B, pending, text, 256)
        return code, text.value.decode()
    assert pre() == (0, "") and pre(weight=1, smooth=O.MAX_SMOOTH)[0] == 0
    assert pre(ctx=0, weight=5, B=0) == (O.ARG, "bad argument (no context)")      # the context ranks before the scalars
    for kw in (dict(weight=2), dict(weight=-1), dict(smooth=-1), dict(smooth=O.MAX_SMOOTH + 1)):      # the scalars before the state
        assert pre(B=0, incidence=0, **kw) == (O.ARG, "bad argument (weight 0 or 1, smooth_rounds in 0..64)"), kw
    assert pre(B=0, incidence=0) == (O.STATE, "no meshes uploaded")      # the batch before the incidence
    code, msg = pre(pending=1, incidence=0)
    assert code == O.STATE and "in flight" in msg
    assert pre(incidence=0) == (O.STATE, "no incidence of the resident batch: call sh_mesh_topology first")
    L = _lib.load()
    assert L.sh_vertex_fields(None, 0, 0, None, None, None, None) == O.ARG      # (no context)
    assert "sh_vertex_fields" in _lib.EXPORTS and _lib.SIGNATURES["sh_vertex_fields"][2]
    assert (_lib.VERT_WEIGHT_AREA, _lib.VERT_WEIGHT_ANGLE, _lib.VERT_MAX_SMOOTH, _lib.VERT_FIELDS) == (O.AREA, O.ANGLE, O.MAX_SMOOTH, O.FIELDS)
    assert (_lib.VERT_USED, _lib.VERT_BORDER, _lib.VERT_NONMANIFOLD, _lib.VERT_FLAT) == (O.USED, O.BORDER, O.NONMANIFOLD, O.FLAT)


def test_buffer_plan(shim):
    def plan(B, maxV, maxF, sumV, sumF):
        out = np.zeros(10, dtype=np.uintp)
        shim.vc_plan(B, maxV, maxF, sumV, sumF, out.ctypes.data)
        return [int(x) for x in out]
    # face blocks, vertex blocks, then the bytes of face, normal, fields, flags, status, a2, plane, state
    assert plan(3, 300, 513, 900, 1200) == [3, 2, 96000, 21600, 57600, 3600, 12, 9600, 28800, 12]
    assert plan(1, 4, 4, 4, 4) == [1, 1, 320, 96, 256, 16, 4, 32, 128, 4]
    assert plan(1, 256, 256, 256, 256)[:2] == [1, 1] and plan(1, 257, 257, 257, 257)[:2] == [2, 2]
    big = plan(64, 1040002, 2080000, 64 * 1040002, 64 * 2080000)
    assert big[:2] == [8125, 4063] and big[2] == 64 * 2080000 * 80 and big[8] == 4 * 64 * 1040002 * 8


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/vert_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "vert_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
