"""Geodesic distances and shortest paths on the resident batch (include/shoulder_hip.h sh_geodesic), the parts that need no GPU: the NumPy
statement of tests/geo_oracle.py against figures a prototype of the rule gave (conditions on the oracle), the host twin of the kernels
(the device source's scalar rules, host-compiled through tests/hostcheck/geo_check.cpp) against the oracle, the argument checks and the
buffer plan.

Nothing in the rule is transcendental, so everything is held as bytes and no tolerance appears: the Jacobi rounds against SciPy's
Dijkstra, the host twin in both of the device's schedules against the oracle.  `sweeps` is informational and compared with nothing.
Symmetry (a to b against b to a) holds to rounding, not as bytes: the fold runs from the source."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import geo_oracle as O
import topo_oracle as TO
import vert_oracle
from conftest import BONES
from mass_oracle import int_box
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

FIXTURES = ["humerus_left", "humerus_right", "humerus_left_trab", "proximal_left_cut"]
NEEDED = FIXTURES + ["humerus_left_flipped"]      # (topo_oracle.table reads it)
MODES = (O.EDGES, O.UNFOLD)
INF = np.inf


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("geo_check"))


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for n in NEEDED:
        v, f = load_stl(os.path.join(BONES, n + ".stl"))
        out[n] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    out["box"] = int_box()
    return out


@pytest.fixture(scope="module")
def bone(meshes):
    """(name, mode) -> the oracle on a whole bone, computed once: the graph; K = 3 (top; bottom; top, bottom, top with offsets 5.0, 0.0,
    2.5: the 5.0 entry roots nothing); the topmost vertex with max_dist = 30.  Every evaluation asserts Jacobi == Dijkstra as bytes."""
    @functools.lru_cache(maxsize=None)
    def get(name, mode):
        v, f = meshes[name]
        g = O.graph(v, f, mode)
        top, bot = O.topmost(v), O.bottommost(v)
        three = O.geodesic(v, f, [[top], [bot], [top, bot, top]], d0=[None, None, [5.0, 0.0, 2.5]], mode=mode, g=g)
        cut = O.geodesic(v, f, [[top]], mode=mode, max_dist=30.0, g=g)
        return dict(g=g, top=top, bot=bot, three=three, cut=cut)
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FIXTURES)
def test_jacobi_equals_dijkstra_and_the_arcs_hold(bone, meshes, name, mode):
    r = bone(name, mode)
    three, cut, (t, h, w) = r["three"], r["cut"], r["g"]["arcs"]
    assert len(three["rounds"]) == 3 and len(cut["rounds"]) == 1      # (O.geodesic compared the two as bytes for each of them)
    rev = set(zip(h.tolist(), t.tolist(), w.tolist()))
    assert all((a, b, c) in rev for a, b, c in zip(t.tolist(), h.tolist(), w.tolist())), "an arc without its reverse of the same bytes"
    for k in range(3):
        d, pred, source, info = three["dist"][k], three["pred"][k], three["source"][k], three["info"][k]
        with np.errstate(all="ignore"):
            cand = d[t] + w
        assert (cand[np.isfinite(cand)] >= d[h][np.isfinite(cand)]).all()      # for every arc fl(d[u] + w) >= d[v]
        on = pred >= 0
        vs = np.nonzero(on)[0]
        best = np.full(len(d), INF)
        np.minimum.at(best, h, np.where(t == pred[h], cand, INF))
        assert np.array_equal(best[vs], d[vs]) and (d[pred[vs]] < d[vs]).all()      # equality along pred, and d falls strictly
        assert info["no_pred"] == 0 and info["reached"] == len(d) and info["status"] == 0
        assert (source[on] >= 0).all() and info["roots"] == (2 if k == 2 else 1)
    assert three["info"]["roots"][2] == 2 and set(three["source"][2]) == {1, 2}      # the 5.0 entry roots nothing
    # d >= the straight distance from a single source, up to rounding
    v = meshes[name][0].astype(np.float64)
    straight = np.linalg.norm(v - v[r["top"]], axis=1)
    assert (three["dist"][0] >= straight * (1 - 1e-12)).all()
    # the cut-off: what is kept equals the unlimited call as bytes, the rest is +inf
    kept = np.isfinite(cut["dist"][0])
    assert cut["dist"][0][kept].tobytes() == three["dist"][0][kept].tobytes() and (three["dist"][0][~kept] > 30.0).all() and cut["info"]["reached"][0] == kept.sum()
    assert (cut["pred"][0][~kept] == O.UNREACHED).all() and (cut["source"][0][~kept] == -1).all()


def test_figures_of_the_prototype(bone, meshes):
    box = meshes["box"]
    assert [float(O.geodesic(*box, [[0]], mode=m)["info"]["far_dist"][0]) for m in MODES] == [60.0, pytest.approx(46.055513, abs=5e-7)]
    two = O.geodesic(*TO.two_boxes(box), [[0]])
    assert two["info"]["reached"][0] == 8 and (two["pred"][0][8:] == O.UNREACHED).all() and np.isinf(two["dist"][0][8:]).all()
    e, u = bone("humerus_left", O.EDGES), bone("humerus_left", O.UNFOLD)
    assert float(e["three"]["info"]["far_dist"][0]) == pytest.approx(371.068246, abs=5e-7) and float(u["three"]["info"]["far_dist"][0]) == pytest.approx(364.211040, abs=5e-7)
    assert (int(e["cut"]["info"]["reached"][0]), int(u["cut"]["info"]["reached"][0])) == (1055, 1181)
    # top to bottom against bottom to top: the same to rounding, not as bytes
    a, b = u["three"]["dist"][0][u["bot"]], u["three"]["dist"][1][u["top"]]
    print(f"humerus_left, unfolded: top to bottom {a!r}, bottom to top {b!r}, difference {a - b:.3g}")
    assert a == pytest.approx(361.28, abs=5e-3) and abs(a - b) <= 1e-12 * a and 0 < abs(a - b)


@pytest.mark.parametrize("name", FIXTURES)
def test_unfolded_is_never_longer_than_edges(bone, name):
    e, u = bone(name, O.EDGES)["three"]["dist"], bone(name, O.UNFOLD)["three"]["dist"]
    assert (u <= e).all()
    with np.errstate(all="ignore"):
        ratio = float(np.nanmean(np.where(e[0] > 0, u[0] / e[0], np.nan)))
    print(f"{name}: mean unfolded / edges {ratio:.4f}")
    assert 0.953 - 5e-4 <= ratio <= 0.981 + 5e-4


def test_icosphere_against_the_great_circle():
    """the accuracy statement of the feature: d / true on spheres of radius 25, sources 0, 12 and V - 1"""
    R = 25.0
    table = {2: ((0.9956, 1.1813), (0.9913, 1.0292)), 3: ((None, 1.2073), (0.9977, 1.0380)), 4: ((None, 1.2214), (None, 1.0436))}
    for sub, want in table.items():
        v, f = vert_oracle.icosphere(sub, R)
        p = v.astype(np.float64)
        for mode, (lo, hi) in zip(MODES, want):
            g = O.graph(v, f, mode)
            r = O.geodesic(v, f, [[0], [12], [len(v) - 1]], mode=mode, g=g, check=sub < 4)
            ratios = []
            for k, s in enumerate((0, 12, len(v) - 1)):
                cosine = np.clip((p @ p[s]) / (np.linalg.norm(p, axis=1) * np.linalg.norm(p[s])), -1.0, 1.0)
                true = R * np.arccos(cosine)
                far = true > 1e-3
                ratios.append(r["dist"][k][far] / true[far])
            ratios = np.concatenate(ratios)
            print(f"icosphere {sub}, mode {mode}: d / true {ratios.min():.4f} .. {ratios.max():.4f}")
            assert ratios.max() == pytest.approx(hi, abs=6e-5) and (lo is None or ratios.min() == pytest.approx(lo, abs=6e-5))


def test_small_cases_hold_the_rule(meshes):
    cases = O.small_cases(meshes)
    for name, (mesh, single) in cases.items():
        for mode in MODES:
            r = O.geodesic(*mesh, O.case_sets(mesh, single), mode=mode)
            assert r["info"]["reached"][2] == 0 and (r["pred"][2] == O.UNREACHED).all() and r["info"]["farthest"][2] == -1, name
            assert r["pred"][0][single] == O.ROOT and r["source"][0][single] == 0 and r["info"]["roots"][0] == 1, name
    twin = O.geodesic(*cases["box with a twin of vertex 0"][0], [[8], [0]])
    assert twin["pred"][0][0] == O.NO_PRED and twin["dist"][0][0] == 0.0 and twin["source"][0][0] == -1 and twin["info"]["no_pred"][0] == 1
    assert twin["pred"][1][8] == O.NO_PRED and twin["info"]["no_pred"][1] == 1      # (the arc of length 0 works both ways: d[u] < d[v] never holds over it)
    shared = cases["boxes sharing an edge"][0]
    g = O.graph(*shared, O.UNFOLD)
    adj = TO.adjacency(shared[1])[0]
    assert (adj == TO.NONMANIFOLD).sum() == 4 and np.isinf(g["face"][:, 3:][adj == TO.NONMANIFOLD]).all()      # no diagonal across the non-manifold edge


def test_host_twin_against_the_oracle(shim, meshes, bone):
    for name, (mesh, single) in O.small_cases(meshes).items():
        for mode in MODES:
            sets = O.case_sets(mesh, single)
            want = O.geodesic(*mesh, sets, mode=mode, check=False)
            for lds in (True, False):
                O.compare(O.host_geodesic(shim, *mesh, sets, mode=mode, lds=lds), want, (name, mode, lds))
    v, f = meshes["humerus_left"]
    for mode in MODES:
        r = bone("humerus_left", mode)
        sets, d0 = [[r["top"]], [r["bot"]], [r["top"], r["bot"], r["top"]]], [None, None, [5.0, 0.0, 2.5]]
        O.compare(O.host_geodesic(shim, v, f, sets, d0=d0, mode=mode, lds=True), r["three"], ("humerus_left", mode))
        O.compare(O.host_geodesic(shim, v, f, [[r["top"]]], mode=mode, max_dist=30.0, lds=False), r["cut"], ("humerus_left, max_dist 30", mode))
    shuffled = TO.further(meshes)["humerus_left, shuffled"]
    for name, mesh in (("humerus_left_trab", meshes["humerus_left_trab"]), ("proximal_left_cut", meshes["proximal_left_cut"]), ("humerus_left, shuffled", shuffled)):
        top = O.topmost(mesh[0])
        O.compare(O.host_geodesic(shim, *mesh, [[top]], lds=name != "proximal_left_cut"), O.geodesic(*mesh, [[top]], check=False), name)


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)
    voff = np.array([0, 8, 20], np.int64)

    def pre(ctx=1, mode=1, K=2, max_dist=INF, off=(0, 1, 1, 3, 4), src=(7, 0, 11, 3), d0=(0.0, 1.5, 0.0, 2.0), incidence=1, B=2, pending=0):
        o, s = np.array(off if off is not None else [0], np.int32), np.array(src, np.int32)
        z = None if d0 is None else np.array(d0, np.float64)
        code = shim.gc_precheck(ctx, mode, K, max_dist, int(off is not None), 1, o.ctypes.data, s.ctypes.data, z.ctypes.data if z is not None else None,
                                voff.ctypes.data if B else None, incidence, B, pending, text, 256)
        return code, text.value.decode()
    scalars = "bad argument (mode 0 or 1, K in 1..16, max_dist +inf or > 0, src_off)"
    assert pre() == (0, "") and pre(mode=0, max_dist=30.0, d0=None)[0] == 0
    assert pre(ctx=0, mode=5, B=0) == (O.ARG, "bad argument (no context)")      # the context ranks before the scalars
    for kw in (dict(mode=2), dict(mode=-1), dict(K=0), dict(K=17), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=-1.0), dict(off=None)):
        assert pre(B=0, incidence=0, **kw) == (O.ARG, scalars), kw      # the scalars before the lists and the state
    # the lists before the state, each offence with its (mesh, set, position)
    assert pre(src=(7, 0, 12, 3), incidence=0, pending=1) == (O.ARG, "bad argument (mesh 1, set 0, position 1: source vertex 12 is not in [0, 12))")
    assert pre(src=(8, 0, 11, 3), incidence=0) == (O.ARG, "bad argument (mesh 0, set 0, position 0: source vertex 8 is not in [0, 8))")
    assert pre(src=(7, -1, 11, 3))[1] == "bad argument (mesh 1, set 0, position 0: source vertex -1 is not in [0, 12))"
    assert pre(d0=(0.0, 1.5, 0.0, -1.0), pending=1) == (O.ARG, "bad argument (mesh 1, set 1, position 0: d0 is not finite and >= 0)")
    assert pre(d0=(0.0, float("nan"), 0.0, 0.0))[1] == "bad argument (mesh 1, set 0, position 0: d0 is not finite and >= 0)"
    assert pre(d0=(INF, 0.0, 0.0, 0.0))[1] == "bad argument (mesh 0, set 0, position 0: d0 is not finite and >= 0)"
    assert pre(off=(0, 1, 0, 3, 4))[1] == "bad argument (mesh 0, set 1: src_off does not ascend)"
    assert pre(B=0, incidence=0) == (O.STATE, "no meshes uploaded")      # the batch before the incidence
    code, msg = pre(pending=1, incidence=0)
    assert code == O.STATE and "in flight" in msg
    assert pre(incidence=0) == (O.STATE, "no incidence of the resident batch: call sh_mesh_topology first")
    L = _lib.load()
    assert L.sh_geodesic(None, 1, 1, INF, None, None, None, None, None, None, None) == O.ARG      # (no context)
    assert "sh_geodesic" in _lib.EXPORTS and _lib.SIGNATURES["sh_geodesic"][2]
    assert (_lib.GEO_EDGES, _lib.GEO_UNFOLD, _lib.GEO_MAX_SETS, _lib.GEO_LDS_VERTICES, _lib.GEO_CHUNK, _lib.GEO_INFO_BYTES) == (O.EDGES, O.UNFOLD, O.MAX_SETS, O.LDS_VERTICES,
                                                                                                                                 O.CHUNK, O.INFO_BYTES)
    assert (_lib.GEO_ROOT, _lib.GEO_NO_PRED, _lib.GEO_UNREACHED) == (O.ROOT, O.NO_PRED, O.UNREACHED) and _lib.GEO_INFO_DTYPE == O.INFO_DTYPE


def test_buffer_plan(shim):
    def plan(B, K, S, lds, maxV, maxF, sumV, sumF):
        out = np.zeros(16, dtype=np.uintp)
        shim.gc_plan(B, K, S, lds, maxV, maxF, sumV, sumF, out.ctypes.data)
        return [int(x) for x in out]
    # face blocks, vertex blocks, jumps, general, rounds_max, then the bytes of face, dist, pred, source, info, opp, plane, jump, src, d0, state
    assert plan(3, 2, 5, 20000, 300, 513, 900, 1200) == [3, 2, 9, 0, 0, 57600, 14400, 7200, 7200, 192, 14400, 0, 7200, 48, 40, 224]
    assert plan(1, 1, 0, 20000, 4, 4, 4, 4) == [1, 1, 2, 0, 0, 192, 32, 16, 16, 32, 48, 0, 16, 8, 8, 64]
    assert plan(1, 16, 3, 20000, 20000, 39996, 20000, 39996)[:5] == [157, 79, 15, 0, 0]      # the largest mesh of the LDS path
    over = plan(1, 16, 3, 20000, 20001, 39998, 20001, 39998)
    assert over[:5] == [157, 79, 15, 1, 20002] and over[11] == over[6] == 16 * 20001 * 8      # one vertex more: the second plane
    assert plan(2, 1, 1, 0, 8, 12, 16, 24)[3:5] == [1, 9] and plan(2, 1, 1, 0, 8, 12, 16, 24)[11] == 128      # the threshold lowered to 0
    big = plan(64, 4, 64, 20000, 1040002, 2080000, 64 * 1040002, 64 * 2080000)
    assert big[:5] == [8125, 4063, 20, 1, 1040003] and big[5] == 64 * 2080000 * 48 and big[6] == 4 * 64 * 1040002 * 8


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/geo_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "geo_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
