"""Smoothing of the vertices of the resident batch (include/shoulder_hip.h sh_smooth_vertices), the parts that need no GPU: conditions on
the NumPy statement of tests/smooth_oracle.py, the host twin of the kernels (the device source's scalar rules, host-compiled through
tests/hostcheck/smooth_check.cpp) against the oracle, the argument checks and the buffer plan.

Bounds.  The rule is + - x / sqrt on float64 in a fixed order, so every comparison of the twin with the oracle is on bytes: rows,
weights, positions and info.  The two tolerances below are conditions on the oracle and come from the arithmetic: 1e-12 relative for the
volume after the scaling (s^3 r = 1 to 2^-48 after ten Newton steps, and the volume sum of ~32 000 signed terms carries a few 1e-13 of
cancellation), and 2^-48 for the Newton steps themselves (quadratic convergence from 1.0 reaches the rounding of s^3 long before step
ten; the residual is a handful of ulps of 2^-52).

Figures of the noisy icosphere (3 subdivisions, radius 25, sigma 0.2 mm, 10 iterations, uniform weights), printed by
test_noisy_icosphere: the standard deviation of the radius falls from 0.1856 to 0.1170 (Laplacian 0.5: ratio 0.631), 0.0807 (Taubin 0.5 /
-0.53: 0.435) and 0.0758 (HC 0.1 / 0.5: 0.409) mm; the mean radius changes by -1.3742, +0.0760 and -0.0106 mm; DESIGN.md 10.17."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mass_oracle as MO
import smooth_oracle as O
import topo_oracle as TO
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

FIXTURES = ["humerus_left", "humerus_left_flipped", "humerus_right", "humerus_left_trab", "proximal_left_cut"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("smooth_check"))


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for n in FIXTURES:
        v, f = load_stl(os.path.join(BONES, n + ".stl"))
        out[n] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    out["box"] = MO.int_box()
    return out


@pytest.fixture(scope="module")
def cases(meshes):
    return O.small_cases(meshes)


def test_nothing_moves_without_an_iteration_a_step_or_a_free_vertex(meshes, cases):
    for name in ("box", "fan of 300", "humerus_left[:257]", "coincident vertices"):
        v, f = cases[name]
        p0 = v.astype(np.float64)
        everything = np.ones(len(v), np.uint8)
        for filt in (O.LAPLACIAN, O.TAUBIN, O.HC):
            for weight in (O.UNIFORM, O.INVLEN):
                assert O.smooth(v, f, filter=filt, weight=weight, iterations=0)["pos"].tobytes() == p0.tobytes(), (name, filt, "0 iterations")
                r = O.smooth(v, f, filter=filt, weight=weight, iterations=4, pin=everything)
                assert r["pos"].tobytes() == p0.tobytes() and r["info"]["pinned"] == len(v) and r["info"]["max_disp"] == 0.0, (name, filt, "all pinned")
                if filt != O.HC:
                    assert O.smooth(v, f, filter=filt, weight=weight, iterations=4, lamb=0.0, mu=-0.0)["pos"].tobytes() == p0.tobytes(), (name, filt, "lambda 0")


def test_a_flat_strip_stays_flat(cases):
    v, f = cases["strip of 600, shuffled"]
    assert not v[:, 2].any()
    for filt in (O.LAPLACIAN, O.TAUBIN, O.HC):
        for weight in (O.UNIFORM, O.INVLEN):
            r = O.smooth(v, f, filter=filt, weight=weight, iterations=5)
            assert (r["pos"][:, 2] == 0.0).all() and r["info"]["max_disp"] > 0.0, (filt, weight)


def test_border_pins(meshes):
    v, f = meshes["box"]
    assert O.smooth(v, f, iterations=1, pin_border=True)["info"]["pinned"] == 0      # a closed box has no border
    r = O.smooth(v, f[1:], iterations=3, pin_border=True)
    assert set(np.nonzero(r["pinned"])[0]) == set(int(x) for x in f[0]) and r["info"]["pinned"] == 3
    assert r["pos"][r["pinned"]].tobytes() == v.astype(np.float64)[r["pinned"]].tobytes() and (r["pos"][~r["pinned"]] != v[~r["pinned"]]).any()


def test_noisy_icosphere():
    v, f = O.noisy_icosphere()
    radius = lambda p: np.linalg.norm(np.asarray(p, np.float64), axis=1)
    r0 = radius(v)
    shift = {}
    for name, kw in (("laplacian", dict(filter=O.LAPLACIAN, lamb=0.5)), ("taubin", dict(filter=O.TAUBIN, lamb=0.5, mu=-0.53)), ("hc", dict(filter=O.HC, alpha=0.1, beta=0.5))):
        r = radius(O.smooth(v, f, iterations=10, **kw)["pos"])
        shift[name] = abs(r.mean() - r0.mean())
        print(f"noisy icosphere, {name}: std of the radius {r0.std():.4f} -> {r.std():.4f} (ratio {r.std() / r0.std():.3f}), mean radius {r.mean() - r0.mean():+.4f} mm")
        assert r.std() < r0.std(), name
    assert shift["taubin"] < shift["laplacian"] and shift["hc"] < shift["laplacian"]


def test_keep_volume_and_the_newton_steps(meshes):
    for name, kw in (("humerus_left", dict(filter=O.LAPLACIAN, iterations=10)), ("box", dict(filter=O.HC, iterations=1, weight=O.INVLEN)),
                     ("humerus_left_trab", dict(filter=O.TAUBIN, iterations=2))):
        v, f = meshes[name]
        r = O.smooth(v, f, keep_volume=True, **kw)
        info = r["info"]
        # mass_oracle measures float32 vertices: the volume of the float64 result in its tree, through the same terms
        got = float(O.IO.tree_sum(O.volume_terms(r["pos"], f, v[0].astype(np.float64)))[0] / 6.0)
        assert info["status"] == 0 and info["volume_before"] == MO.mass(v, f)[0]["volume"] and info["scale"] != 1.0
        print(f"{name}: volume {info['volume_before']:.6f} -> {info['volume_after']:.6f}, scale {info['scale']:.9f}, after the scaling off by {abs(got / info['volume_before'] - 1):.3g}")
        assert abs(got / info["volume_before"] - 1.0) <= 1e-12
        # ... and independently of the oracle's own helpers: the signed tetrahedra about the mean vertex (the meshes are closed), a plain float64 sum
        A, B, C = (r["pos"][f[:, k]] - r["pos"].mean(axis=0) for k in range(3))
        plain = float(np.einsum("ij,ij->i", A, np.cross(B, C)).sum() / 6.0)
        print(f"{name}: the plain sum of det / 6 is off by {abs(plain / info['volume_before'] - 1):.3g}")
        assert abs(plain / info["volume_before"] - 1.0) <= 1e-12
    v, f = meshes["box"]
    assert O.volume_terms(v.astype(np.float64), f, v[0].astype(np.float64)).tobytes() == np.ascontiguousarray(MO.face_terms(v, f)[0][:, 13:17]).tobytes()
    for r in np.concatenate([np.linspace(0.125, 1.0, 200), np.linspace(1.0, 8.0, 200)]):
        s = O.cube_root(float(r))
        assert abs((s * s) * s / r - 1.0) <= 2.0 ** -48, r
    # a mesh that lost seven eighths of its volume, and one without a volume: the status, and no scaling
    gone = O.smooth(v, f, filter=O.HC, iterations=2, keep_volume=True)
    assert gone["info"]["status"] == O.GEOMETRY and gone["info"]["scale"] == 1.0 and gone["info"]["volume_after"] < 6000.0 / 8
    flat = O.smooth(*TO.fan(300), iterations=2, keep_volume=True)
    assert flat["info"]["status"] == O.GEOMETRY and flat["info"]["scale"] == 1.0
    assert flat["pos"].tobytes() == O.smooth(*TO.fan(300), iterations=2)["pos"].tobytes()


def test_rows_are_the_sets_of_a_plain_loop(cases, meshes):
    for name, (v, f) in list(cases.items()) + [("humerus_left", meshes["humerus_left"])]:
        want = [set() for _ in range(len(v))]
        for a, b, c in f.tolist():
            if a == b or b == c or a == c:
                continue
            want[a] |= {b, c}
            want[b] |= {a, c}
            want[c] |= {a, b}
        nrow, nbr = O.neighbours(f, len(v))
        assert nrow[0] == 0 and nrow[-1] == len(nbr) == sum(len(s) for s in want), name
        for i, s in enumerate(want):
            row = nbr[nrow[i]:nrow[i + 1]].tolist()
            assert row == sorted(s), (name, i)
    nrow, _ = O.neighbours(cases["unused vertex"][1], 9)
    assert nrow[4] == nrow[3]
    v, f = cases["coincident vertices"]
    r = O.smooth(v, f, weight=O.INVLEN, iterations=0)
    at = r["nrow"][1] + list(r["nbr"][r["nrow"][1]:r["nrow"][2]]).index(4)
    assert r["w"][at] == 0.0 and (r["w"] == 0.0).sum() == 2      # the pair {1, 4}, both directions


def test_host_twin_against_the_oracle_small(shim, cases):
    for name, (v, f) in cases.items():
        for tag, kw in O.variants(len(v)):
            O.same_bytes(O.host_smooth(shim, v, f, **kw), O.reference(name, (v, f), tag, kw), (name, tag))


@pytest.mark.parametrize("name,tag,kw", O.WHOLE)
def test_host_twin_against_the_oracle_whole(shim, meshes, name, tag, kw):
    v, f = meshes[name]
    O.same_bytes(O.host_smooth(shim, v, f, **kw), O.reference(name, (v, f), tag, kw), (name, tag))


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)

    def pre(ctx=1, filter=O.TAUBIN, weight=0, iterations=10, flags=0, p0=0.5, p1=-0.53, has_pin=0, incidence=1, maxF=1000, B=1, pending=0):
        code = shim.sc_precheck(ctx, filter, weight, iterations, flags, p0, p1, has_pin, incidence, maxF, B, pending, text, 256)
        return code, text.value.decode()
    assert pre() == (0, "") and pre(filter=O.HC, weight=1, iterations=O.MAX_ITER, flags=O.KEEP_VOLUME, p0=0.0, p1=1.0)[0] == 0
    assert pre(ctx=0, filter=7, B=0) == (O.ARG, "bad argument (no context)")      # the context ranks before the scalars
    scalars = "bad argument (filter 0, 1 or 2, weight 0 or 1, iterations in 0..256, flags 0..3)"
    for kw in (dict(filter=3), dict(filter=-1), dict(weight=2), dict(iterations=-1), dict(iterations=257), dict(flags=4), dict(flags=-1)):
        assert pre(B=0, incidence=0, p0=7.0, **kw) == (O.ARG, scalars), kw                 # the scalars before the parameters and the state
    for kw, word in ((dict(p0=1.5), "lambda in 0..1"), (dict(p0=-0.1), "lambda"), (dict(p0=float("nan")), "lambda"), (dict(p1=0.1), "mu in -1..0"), (dict(p1=-1.5), "mu"),
                     (dict(p1=float("nan")), "mu"), (dict(filter=O.LAPLACIAN, p1=float("inf")), "mu"), (dict(filter=O.HC, p0=1.5, p1=0.5), "alpha in 0..1"),
                     (dict(filter=O.HC, p0=0.1, p1=-0.53), "beta in 0..1"), (dict(filter=O.HC, p0=0.1, p1=float("nan")), "beta")):
        code, msg = pre(B=0, incidence=0, **kw)                                            # the parameters before the state
        assert code == O.ARG and word in msg, (kw, msg)
    assert pre(filter=O.LAPLACIAN, p1=5.0)[0] == 0                                          # p1 of the Laplacian: finite, else unused
    for kw in (dict(flags=O.KEEP_VOLUME | O.PIN_BORDER), dict(flags=O.KEEP_VOLUME, has_pin=1)):
        code, msg = pre(B=0, incidence=0, **kw)
        assert code == O.ARG and "SH_SMOOTH_KEEP_VOLUME with a pin" in msg, kw
    assert pre(B=0, incidence=0) == (O.STATE, "no meshes uploaded")                       # the batch before the incidence
    code, msg = pre(pending=1, incidence=0)
    assert code == O.STATE and "in flight" in msg
    assert pre(incidence=0) == (O.STATE, "no incidence of the resident batch: call sh_mesh_topology first")
    assert pre(maxF=400000000)[0] == -6
    L = _lib.load()
    assert L.sh_smooth_vertices(None, 1, 0, 10, 0, 0.5, -0.53, None, None, None) == O.ARG      # (no context)
    assert "sh_smooth_vertices" in _lib.EXPORTS and _lib.SIGNATURES["sh_smooth_vertices"][2]
    assert (_lib.SMOOTH_LAPLACIAN, _lib.SMOOTH_TAUBIN, _lib.SMOOTH_HC, _lib.SMOOTH_UNIFORM, _lib.SMOOTH_INVLEN) == (O.LAPLACIAN, O.TAUBIN, O.HC, O.UNIFORM, O.INVLEN)
    assert (_lib.SMOOTH_PIN_BORDER, _lib.SMOOTH_KEEP_VOLUME, _lib.SMOOTH_MAX_ITER, _lib.SMOOTH_INFO_BYTES) == (O.PIN_BORDER, O.KEEP_VOLUME, O.MAX_ITER, 64)
    assert _lib.SMOOTH_INFO_DTYPE.names[:5] == ("volume_before", "volume_after", "scale", "max_disp", "sum_sq_disp") and _lib.SMOOTH_INFO_DTYPE.fields["pinned"][1] == 40


def test_buffer_plan(shim):
    def plan(B, filter, iterations, maxV, maxF, sumV, sumF):
        out = np.zeros(16, dtype=np.uintp)
        shim.sc_plan(B, filter, iterations, maxV, maxF, sumV, sumF, out.ctypes.data)
        return [int(x) for x in out]
    # face blocks, vertex blocks, steps, last plane, the offsets vol1, disp and head, then the bytes of nbr, w, pos, info, plane, pin, mask, part, nrow
    assert plan(3, O.TAUBIN, 3, 300, 513, 900, 1200) == [3, 2, 6, 0, 36, 72, 84, 28800, 57600, 21600, 192, 64800, 3600, 900, 864, 3612]
    assert plan(1, O.LAPLACIAN, 7, 4, 4, 4, 4) == [1, 1, 7, 1, 4, 8, 10, 96, 192, 96, 64, 288, 16, 4, 144, 20]
    assert plan(1, O.HC, 7, 256, 256, 256, 256)[:4] == [1, 1, 14, 0] and plan(1, O.TAUBIN, 0, 257, 257, 257, 257)[:4] == [2, 2, 0, 0]
    big = plan(64, O.LAPLACIAN, 256, 1040002, 2080000, 64 * 1040002, 64 * 2080000)
    assert big[:4] == [8125, 4063, 256, 0] and big[8] == 6 * 64 * 2080000 * 8 and big[11] == 9 * 64 * 1040002 * 8
    # the sizes do not depend on the filter or the iterations: a second call allocates nothing
    assert plan(2, O.HC, 200, 50, 90, 80, 150)[7:] == plan(2, O.LAPLACIAN, 0, 50, 90, 80, 150)[7:]


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/smooth_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "smooth_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
