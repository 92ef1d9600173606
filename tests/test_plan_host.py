"""Implant plans (include/shoulder_hip.h sh_resect_plan), the parts that need no GPU (record layouts: test_abi_exports.py): argument checks, the arithmetic
the device runs (sh_scalar.h plan_*, host-compiled with -ffp-contract=off through tests/hostcheck/plan_check.cpp) against numbers
worked by hand, and the host twins of the selection and of the reference against the NumPy statement of tests/plan_oracle.py.

Bounds.  Hand-worked numbers are chosen exactly representable: equality.  Twins against the oracle: bytes (integers, and doubles that
the same operations in the same order produce)."""
import ctypes

import numpy as np
import pytest

import plan_oracle as O
import stem_oracle as SO
from shoulder_amd import _lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("plan_check"))


def test_plan_entry_point_checks_its_arguments_without_a_gpu():
    assert _lib.PLAN_TERM_DTYPE == O.TERM_DTYPE and O.TERM_DTYPE.itemsize == 16
    assert [n for n, _ in _lib.PlanRule._fields_] == list(O.RULE_FIELDS)
    L = _lib.load()
    out = np.zeros(64, dtype=_lib.PLAN_DTYPE)
    ptr = ctypes.c_void_p(out.ctypes.data)

    def call(r, N=8, o=ptr):
        rule = _lib.PlanRule(**r) if r is not None else None
        return L.sh_resect_plan(None, ctypes.byref(rule) if rule is not None else None, None, None, N, o, None)
    good = O.rule(w_uncovered=1.0, margin=2.0)
    assert call(good) == -1                                                         # (no context)
    assert call(good, N=0) == -1 and call(good, N=65) == -1 and call(None) == -1 and call(good, o=None) == -1
    for k in O.RULE_FIELDS:
        assert call(dict(good, **{k: np.nan})) == -1, k
    for k in O.RULE_FIELDS[6:]:
        assert call(dict(good, **{k: -1.0})) == -1 and call(dict(good, **{k: np.inf})) == -1, k
    assert call(dict(good, margin=-0.5)) == -1
    assert "sh_resect_plan" in _lib.EXPORTS


def head(shim, r, coverage=0.75, overhang=1.5, cs=(1.0, 2.0, 2.0), sc=(3.0, 4.0, 2.0), n=(0.0, 0.0, 2.0), h=18.0, T=np.eye(4), apex_z=20.0):
    rule = _lib.PlanRule(**r)
    cs, sc, n, T = (np.ascontiguousarray(a, np.float64) for a in (cs, sc, n, T))
    vals, out = np.zeros(8), np.zeros(2)
    shim.pc_head_term(ctypes.byref(rule), coverage, overhang, cs.ctypes.data, sc.ctypes.data, n.ctypes.data, h, T.ctypes.data, apex_z, vals.ctypes.data, out.ctypes.data)
    return out[0], int(out[1]), vals


def cut(shim, r, sc=(3.0, 4.0, 2.0), plane=(0, 0, 2.0, 0, 0, 2.0), T=np.eye(4), status=(0, 0, 1, 0, 0)):
    rule = _lib.PlanRule(**r)
    sc, plane, T = (np.ascontiguousarray(a, np.float64) for a in (sc, plane, T))
    out = np.zeros(3)
    shim.pc_cut_term(ctypes.byref(rule), *status, sc.ctypes.data, T.ctypes.data, plane.ctypes.data, out.ctypes.data)
    return out[0], int(out[1]), out[2]


def stem(shim, r, status=0, fits=1, clearance=0.5, fill_mean=0.75):
    rule = _lib.PlanRule(**r)
    out = np.zeros(3)
    shim.pc_stem_term(ctypes.byref(rule), status, fits, clearance, fill_mean, out.ctypes.data)
    return out[0], int(out[1]), out[2]


def test_parts_of_a_cost_worked_by_hand(shim):
    w1 = O.rule(w_uncovered=1.0, w_overhang=2.0, w_cor=4.0, w_height=8.0, w_eccentricity=0.5, w_fill=16.0, fill_target=0.5)
    # a head whose apex is exactly the native apex: seat centre (3, 4, 2), thickness 18 along the normal (0, 0, 2) / 2 -> z = 20
    cost, ok, v = head(shim, w1)
    assert ok == 1 and list(v) == [0.25, 1.5, 3.0, 0.0, 3.0, 4.0, 20.0, 20.0] and cost == (1.0 * 0.25 + 2.0 * 1.5) + 4.0 * 3.0
    cost, ok, v = head(shim, w1, apex_z=17.5)
    assert v[3] == 2.5 and cost == ((0.25 + 3.0) + 12.0) + 8.0 * 2.5
    cost, ok, v = head(shim, w1, apex_z=23.0)                                       # (the height term is a distance: |20 - 23|)
    assert v[3] == 3.0
    T = SO.rigid((0.0, 0.0, np.pi / 2), (0.0, 0.0, 1.0))                              # a frame turned about z and lifted by 1: apex_z = 21
    assert abs(head(shim, w1, T=T)[2][7] - 21.0) <= 1e-15
    # an eccentricity of exactly 3-4-5: the axis pierces the plane z = 2 at (0, 0, 2), the seat centre is (3, 4, 2)
    cost, ok, ecc = cut(shim, w1)
    assert ecc == 5.0 and cost == 2.5 and ok == 1
    for st in ((-5, 0, 1, 0, 0), (0, -5, 1, 0, 0), (0, 0, 0, 0, 0), (0, 0, 1, -5, 0)):     # humerus, cut, no loop, seat: no cut part
        assert cut(shim, w1, status=st) == (0.0, 0, 0.0)
    assert cut(shim, w1, plane=(0, 0, 2.0, 1.0, 0, 0)) == (0.0, 0, 0.0)                # a plane that holds the axis: no entry
    assert cut(shim, w1, status=(0, 0, 1, 0, -5))[1] == 0 and cut(shim, dict(w1, w_cor=0.0), status=(0, 0, 1, 0, -5))[1] == 1      # a sphere only when w_cor > 0
    cost, ok, fill = stem(shim, w1)
    assert fill == 0.25 and cost == 4.0 and ok == 1
    assert stem(shim, w1, status=-1)[1] == 0 and stem(shim, w1, fits=0)[1] == 0
    assert stem(shim, w1, fill_mean=0.25)[2] == 0.25                                   # |0.25 - 0.5|


def test_each_limit_at_inside_and_outside_its_bound(shim):
    up, dn = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
    for lim, want in ((1.5, 1), (up(1.5), 1), (dn(1.5), 0), (np.inf, 1)):
        assert head(shim, O.rule(max_overhang=lim))[1] == want, lim
    for lim, want in ((0.75, 1), (dn(0.75), 1), (up(0.75), 0), (-np.inf, 1)):
        assert head(shim, O.rule(min_coverage=lim))[1] == want, lim
    for lim, want in ((0.5, 1), (dn(0.5), 1), (up(0.5), 0), (-np.inf, 1)):
        assert stem(shim, O.rule(min_clearance=lim))[1] == want, lim
    for lim, want in ((5.0, 1), (up(5.0), 1), (dn(5.0), 0), (np.inf, 1)):
        assert cut(shim, O.rule(max_eccentricity=lim))[1] == want, lim


def test_a_nan_cost_is_not_a_candidate(shim):
    t = np.zeros(3, dtype=O.TERM_DTYPE)
    t["feasible"] = 1
    t["cost"] = [0.25, 0.5, 1.0]
    cost = ctypes.c_double()

    def cand(word=~0, ks=3):
        return shim.pc_candidate(t[0:1].ctypes.data, t[1:2].ctypes.data, t[2:3].ctypes.data, word & 0xFFFFFFFFFFFFFFFF, ks, ctypes.byref(cost))
    assert cand() == 1 and cost.value == (0.5 + 1.0) + 0.25                            # (head + stem) + cut
    assert cand(word=1 << 3) == 1 and cand(word=~(1 << 3)) == 0 and cand(word=1 << 63, ks=63) == 1
    t["cost"][1] = np.nan
    assert cand() == 0
    t["cost"][1] = np.inf                                                             # an infinite cost is ordered, not dropped
    assert cand() == 1 and cost.value == np.inf
    t["cost"][2] = -np.inf                                                            # inf - inf
    assert cand() == 0
    # the stem part of a record with an infinite fill against an infinite target: |inf - inf| is NaN, and so is the cost
    c, ok, fill = stem(shim, O.rule(w_fill=1.0, fill_target=np.inf), fill_mean=np.inf)
    assert np.isnan(fill) and np.isnan(c) and ok == 1


def random_terms(rng, P, Kh, Ks, share=0.8):
    """parts quantised to eight levels, so that ties dominate"""
    def part(shape):
        t = np.zeros(shape, dtype=O.TERM_DTYPE)
        t["cost"] = rng.integers(0, 8, size=shape) / 8.0
        t["feasible"] = rng.random(size=shape) < share
        return t
    return part((P,)), part((P, Kh)), part((P, Ks))


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 9), (1, 15, 17), (257, 1, 1), (25, 50, 56)])
def test_selection_twin_against_lexsort_on_quantised_terms(shim, shape):
    """candidate counts 1, 63, 255, 257 and 70 000; N = 1, 8, 64 including N greater than the count; a single-bit mask and one with an
    empty row"""
    P, Kh, Ks = shape
    rng = np.random.default_rng(P * 4096 + Kh * 64 + Ks)
    ct, ht, st = random_terms(rng, P, Kh, Ks)
    if Kh > 1:                                                                        # a NaN among the costs drops its candidates only
        ht["cost"][rng.integers(P), rng.integers(Kh)] = np.nan
    elif P > 1:
        ct["cost"][rng.integers(P)] = np.nan
    one_bit = np.zeros((Kh, Ks), dtype=bool)
    one_bit[Kh // 2, Ks - 1] = True
    empty_row = np.ones((Kh, Ks), dtype=bool)
    empty_row[0] = False
    ties = 0
    for compat in (None, one_bit, empty_row):
        for N in (1, 8, 64):
            got, nf = O.host_select(shim, ct, ht, st, compat, N, tuberosity_z=0.5)
            idx, cost, want_nf = O.rank_fetched(ct, ht, st, compat, N)
            assert nf == want_nf
            k = len(idx)
            assert k == min(N, want_nf)
            i_got = (got["cut"][:k].astype(np.int64) * Kh + got["head"][:k]) * Ks + got["stem"][:k]
            assert np.array_equal(i_got, idx) and got["cost"][:k].tobytes() == cost.tobytes() and np.all(got["status"][:k] == 0)
            assert np.all(got["head_height"][:k] == got["apex_z"][:k] - 0.5)
            rest = got[k:]
            assert np.all(rest["cut"] == -1) and np.all(rest["head"] == -1) and np.all(rest["stem"] == -1) and np.all(rest["status"] == O.GEOMETRY)
            assert not any(np.any(rest[f]) for f in rest.dtype.names if f not in ("cut", "head", "stem", "status"))
            ties += int((np.diff(cost) == 0).sum())
    if P * Kh * Ks >= 255:
        assert ties > 0


def test_selection_twin_with_all_weights_zero_gives_index_order(shim):
    rng = np.random.default_rng(3)
    ct, ht, st = random_terms(rng, 4, 5, 6)
    for t in (ct, ht, st):
        t["cost"] = 0.0
    got, nf = O.host_select(shim, ct, ht, st, None, 64)
    i = (got["cut"][:min(nf, 64)].astype(np.int64) * 5 + got["head"][:min(nf, 64)]) * 6 + got["stem"][:min(nf, 64)]
    assert nf > 8 and np.all(np.diff(i) > 0) and np.array_equal(i, O.rank_fetched(ct, ht, st, None, 64)[0])


def check_ref(got, want):
    for k in ("status", "tuberosity_vid", "head_apex_vid"):
        assert got[k] == want[k], k
    for k in ("tuberosity_top", "tuberosity_z", "head_apex", "head_apex_z", "head_height"):
        assert np.asarray(got[k], np.float64).tobytes() == np.asarray(want[k], np.float64).tobytes(), k
    assert got["n_feasible"] == 0 and got["pad"] == 0


def test_reference_twin_on_prisms_with_exact_ties(shim):
    """identity frame, the top ring at exactly z = 6: every vertex of the ring ties and the smallest id of each side wins -- inside one
    wave (the octagon) and across waves and tiles (a 300-gon: 602 vertices, three tiles, the ring is vertices 300 .. 599)"""
    plane = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    v8 = np.ascontiguousarray(SO.prism(8, 10.0, -4.0, 6.0, 0.0)[0], np.float32)
    r = O.host_ref(shim, v8, np.eye(4), plane, 0.0)
    check_ref(r, O.reference(v8, np.eye(4), plane, 0.0))
    assert r["status"] == 0 and r["head_apex_vid"] == 8 and r["tuberosity_vid"] == 11 and r["head_apex_z"] == 6.0 and r["tuberosity_z"] == 6.0 and r["head_height"] == 0.0
    assert np.array_equal(r["head_apex"], [10.0, 0.0, 6.0])
    r = O.host_ref(shim, v8, np.eye(4), plane, 8.0)                                   # the margin moves the tuberosity to x <= -8: vertex 12 at (-10, 0)
    check_ref(r, O.reference(v8, np.eye(4), plane, 8.0))
    assert r["tuberosity_vid"] == 12
    r = O.host_ref(shim, v8, np.eye(4), 2.0 * plane, 4.0)                             # the margin counts in mm whatever the normal's length
    assert r["tuberosity_vid"] == 11 and O.host_ref(shim, v8, np.eye(4), 2.0 * plane, 8.0)["tuberosity_vid"] == 12
    for margin in (10.5, np.inf):                                                     # a margin that empties the tuberosity side
        r = O.host_ref(shim, v8, np.eye(4), plane, margin)
        check_ref(r, O.reference(v8, np.eye(4), plane, margin))
        assert r["status"] == O.GEOMETRY and r["tuberosity_vid"] == -1 and r["head_apex_vid"] == -1 and not r["head_apex"].any() and r["head_apex_z"] == 0.0
    assert O.host_ref(shim, v8, np.eye(4), plane, 0.0, status=-4)["status"] == -4      # a failed humerus passes its status on
    v300 = np.ascontiguousarray(SO.prism(300, 10.0, -4.0, 6.0, 0.0)[0], np.float32)
    r = O.host_ref(shim, v300, np.eye(4), plane, 0.0)
    check_ref(r, O.reference(v300, np.eye(4), plane, 0.0))
    assert r["head_apex_vid"] == 300 and 300 < r["tuberosity_vid"] < 600 and v300[r["tuberosity_vid"] - 1, 0] > 0.0
    # a tilted frame and an oblique plane: no ties, the same bits as the oracle
    T = SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75))
    pl = np.array([0.5, -0.25, 1.0, 0.3, 0.1, 1.0])
    for margin in (0.0, 1.0, 3.0):
        check_ref(O.host_ref(shim, v300, T, pl, margin), O.reference(v300, T, pl, margin))


def test_oracle_plans_follow_the_twin_on_synthetic_records(shim):
    """the oracle's own chain (terms from records, ranking, plan rows) against the host-compiled parts on a few synthetic records"""
    rng = np.random.default_rng(11)
    P, Kh, Ks = 3, 4, 5
    rec, fit = np.zeros(P, dtype=_lib.RESECTION_DTYPE), np.zeros(P, dtype=_lib.HEAD_FIT_DTYPE)
    seat, st = np.zeros((P, Kh), dtype=_lib.SEAT_DTYPE), np.zeros((P, Ks), dtype=_lib.STEM_FIT_DTYPE)
    T = SO.rigid((0.1, 0.2, -0.3), (2.0, 1.0, -3.0))
    rec["plane_point"], rec["plane_normal"], rec["n_loops"] = rng.normal(size=(P, 3)), rng.normal(size=(P, 3)) + [0, 0, 3.0], 1
    rec["status"][2] = -5
    sc = rng.normal(size=(P, 3))
    seat["seat_center"], seat["coverage"], seat["max_overhang"], seat["cor_shift"] = sc[:, None, :], rng.random((P, Kh)), rng.random((P, Kh)), rng.normal(size=(P, Kh, 3))
    st["fits"], st["min_clearance"], st["fill_mean"] = rng.random((P, Ks)) < 0.7, rng.random((P, Ks)), rng.random((P, Ks))
    heads = np.c_[rng.random(Kh) * 5 + 20, rng.random(Kh) * 5 + 14]
    ref = dict(status=0, head_apex_z=4.0, tuberosity_z=-2.0)
    r = O.rule(w_uncovered=1.0, w_overhang=0.5, w_cor=0.25, w_height=0.125, w_eccentricity=2.0, w_fill=3.0, fill_target=0.6, max_overhang=0.9, min_clearance=0.1)
    t = O.terms(r, rec, fit, seat, st, heads, T, ref)
    for p in range(P):
        pl = np.concatenate([rec["plane_point"][p], rec["plane_normal"][p]])
        c, ok, ecc = cut(shim, r, sc=sc[p], plane=pl, T=T, status=(0, int(rec["status"][p]), 1, 0, 0))
        assert (c, ok, ecc) == (t["cut_cost"][p], int(t["cut_ok"][p]), t["ecc"][p])
        for k in range(Kh):
            c, ok, v = head(shim, r, seat["coverage"][p, k], seat["max_overhang"][p, k], seat["cor_shift"][p, k], sc[p], rec["plane_normal"][p], heads[k, 1], T, 4.0)
            assert c == t["head_cost"][p, k] and ok == int(t["head_ok"][p, k]) and v[7] == t["apex_z"][p, k] and np.array_equal(v[4:7], t["apex"][p, k])
        for k in range(Ks):
            c, ok, f = stem(shim, r, 0, int(st["fits"][p, k]), st["min_clearance"][p, k], st["fill_mean"][p, k])
            assert c == t["stem_cost"][p, k] and ok == int(t["stem_ok"][p, k]) and f == t["fill"][p, k]
    got, nf = O.plans(r, rec, fit, seat, st, heads, T, ref, None, 8)
    assert nf > 0 and np.all(got["cut"][:min(nf, 8)] < 2) and np.all(np.diff(got["cost"][:min(nf, 8)]) >= 0)
    assert np.all(got["head_height"][:min(nf, 8)] == got["apex_z"][:min(nf, 8)] + 2.0)
