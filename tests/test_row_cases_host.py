"""The cases of tests/row_cases.py before any GPU sees them (CPU only): every case carries the fact its table row names (from SciPy alone),
the oracle alone returns a result or exactly the named exception for every (case, forest) pairing, the host twins of the row kernels
(sh_scalar.h through tests/hostcheck: groove rows, forest walk, local minimum, np.interp) agree with the oracle on every row of every
case, the plane cases are well conditioned, and the whole costs at most 60 s of oracle time (printed)."""
import ctypes

import numpy as np
import pytest
import scipy.signal

import row_cases as rc
from oracle import groove, xform
from hostcheck_lib import dp, hc, I  # noqa: F401  (hc: the fixture that builds and loads the shim)

ORACLE_BUDGET_S = 60.0


@pytest.fixture(scope="module")
def cases():
    return {n: rc.groove_case(n) for n in rc.GROOVE_CASES}


@pytest.fixture(scope="module")
def facts(cases):
    return {n: rc.case_facts(c) for n, c in cases.items()}


@pytest.fixture(scope="module")
def verdicts(cases, rfc_tables):
    """(forest name, case name) -> (tables, groove_expect)"""
    out = {}
    for fname, cname, tables in rc.groove_pairings(cases, rfc_tables):
        out[fname, cname] = (tables, rc.groove_expect(cases[cname], tables))
    return out


# ---- carried facts --------------------------------------------------------------------------------------------------------------------
def test_plain_has_one_to_six_peaks_per_row(facts):
    f = facts["plain"]
    assert f["n_pass"].min() >= 1 and f["n_pass"].max() <= 6 and f["n_max"].max() <= 64


def test_rough_overflows_sixty_four_candidates(facts):
    f = facts["rough"]
    print("rough: rows with > 64 maxima %d, rows with a passing peak beyond the 64th %d, most maxima %d" % ((f["n_max"] > 64).sum(), (f["beyond"] > 0).sum(), f["n_max"].max()))
    assert (f["n_max"] > 64).sum() >= 30 and (f["beyond"] > 0).sum() >= 5 and f["n_max"].max() <= 255


def test_crowded_keeps_seven_of_at_least_eight(facts, cases):
    f = facts["crowded"]
    assert f["n_pass"].min() >= 8 and f["gap78"].min() > 1e-9
    # rows 300-309: more than 64 PASSING peaks, so the cut to the 7 most prominent runs over more than one batch of 64 candidates
    assert (f["n_pass"][300:310] > 64).all() and (f["n_max"][300:310] > 64).all() and f["n_max"].max() <= 255
    X, X_raw, _, rows = rc.features(cases["crowded"])
    assert (np.bincount(rows, minlength=rc.R) == 7).all() and (X_raw[:, 8] == 1.0).all() and (X[:, 8] == 0.0).all() and not np.signbit(X[:, 8]).any()


def test_terraced_has_flat_tops_and_flat_valleys(facts, cases):
    f = facts["terraced"]
    r = cases["terraced"]["polar"][:, 1, :]
    for row in r[::37]:
        runs = np.diff(np.flatnonzero(np.r_[True, np.diff(row) != 0, True]))
        assert runs.min() >= 12
    assert f["flat_odd"].sum() >= 50 and f["flat_even"].sum() >= 50 and f["flat_valley"].sum() >= 50


@pytest.mark.parametrize("name", ["seam_lo", "seam_hi"])
def test_seams(facts, cases, verdicts, name):
    f = facts[name]
    at_seam = f["amin"] <= 2 if name == "seam_lo" else f["amin"] >= 509
    assert at_seam.sum() >= 20 and (f["seam"] & at_seam).sum() >= 1
    g = verdicts["shipped", name][1]
    th = cases[name]["polar"][:, 0, :]
    esti = np.array([np.searchsorted(t, g["bg_theta"], side="left") for t in th])
    if name == "seam_lo":
        assert abs(g["bg_theta"] - (-np.pi + 0.03)) < 0.01 and (esti < rc.IVAR).all()
        assert (g["local_idx"] < 0).sum() >= 20      # negative Python indices of the local minimum
    else:
        assert abs(g["bg_theta"] - (np.pi - 0.01)) < 0.01 and (esti == rc.M).all()


def test_sparse_is_nearly_peakless(facts, cases):
    f = facts["sparse"]
    assert (f["n_pass"] > 0).sum() == 3 and f["n_pass"].sum() < 8 and np.ptp(cases["sparse"]["zs"]) == 0.0
    # (its 1e-3 mm of noise leaves more than 64 local maxima in every row, and the three rows' peaks lie behind the 64th)
    assert (f["n_max"] > 64).all() and (f["beyond"] > 0).sum() == 3


def test_pinched_has_two_peaks_within_4_mrad(facts):
    f = facts["pinched"]
    assert (f["close"] < 0.004).sum() == 1 and f["n_pass"][f["close"] < 0.004][0] == 2


def test_forests_pass_the_forest_check(cases, rfc_tables):
    for fname, cname, tables in rc.groove_pairings(cases, rfc_tables):
        assert rc.forest_ok(tables), (fname, cname)
    ch = rc.chain(rc.features(cases["plain"])[0])
    assert list(ch["roots"]) == [0]
    d, i = 0, 0
    while ch["true_idx"][i] >= 0:      # the deep side
        i = max(ch["true_idx"][i], ch["false_idx"][i])
        d += 1
    assert d == 40


# ---- oracle verdicts ------------------------------------------------------------------------------------------------------------------
def test_oracle_verdicts(verdicts):
    for (fname, cname), (_, g) in verdicts.items():
        want = "ValueError" if fname == "mute" else ("IndexError" if cname == "pinched" else None)
        if want:
            assert g == want, (fname, cname, g)
        else:
            assert isinstance(g, dict), (fname, cname, g)
            assert np.isfinite(g["points_ct"]).all() and np.isfinite(g["axis_ct"]).all()


def test_bracket_thresholds_part_the_peak_from_its_values(cases, verdicts):
    for cname in ("plain", "rough"):
        tables, g = verdicts["bracket", cname]
        _, picks = rc.bracket(rc.features(cases[cname])[0])
        leaves = rc.stump_leaves(g["proba"], len(tables["roots"]))
        for j, (p, f) in enumerate(picks):
            assert not leaves[p, 2 * j] and leaves[p, 2 * j + 1], (cname, p, f)
            x = g["X"][p, f]
            lo, hi = float(tables["thr"][tables["roots"][2 * j]]), float(tables["thr"][tables["roots"][2 * j + 1]])
            assert lo < x < hi and np.nextafter(np.float32(lo), np.float32(np.inf)) == np.float32(hi)
            assert min(x - lo, hi - x) > rc.BRACKET_MARGIN
        assert any(float(np.float32(g["X"][p, f])) < g["X"][p, f] for p, f in picks)      # a walk narrowed to float would send these the wrong way


def test_equal0_sends_zero_true_true_false(verdicts):
    tables, g = verdicts["equal0", "crowded"]
    leaves = rc.stump_leaves(g["proba"], 3)
    assert leaves[:, 0].all() and leaves[:, 1].all() and not leaves[:, 2].any()


def test_chain_reaches_every_depth_class(verdicts):
    _, g = verdicts["chain", "plain"]
    depth = np.round(g["proba"].astype(np.float64) * 64).astype(int)
    assert depth.min() <= 2 and depth.max() == 41 and len(np.unique(depth)) >= 20


# ---- host twin ------------------------------------------------------------------------------------------------------------------------
def _twin_rows(hc, case):
    polar, zc = case["polar"], case["zs"]
    cu = xform.unit_vector(case["canal"][0], case["canal"][1])
    rng = zc.max() - zc.min()
    scale = 1.0 / (rng if rng != 0 else 1.0)
    zsc = zc * scale + (0.0 - zc.min() * scale)
    Xraw, pth, npk = [], [], []
    for i in range(len(zc)):
        X, th, pidx = np.zeros((7, 9)), np.zeros(7), np.zeros(7, dtype=np.int32)
        k = hc.hc_groove_row(dp(np.ascontiguousarray(polar[i, 0])), dp(np.ascontiguousarray(polar[i, 1])), rc.M, ctypes.c_double(zc[i]),
                             ctypes.c_double(zsc[i]), dp(cu), dp(X), dp(th), pidx.ctypes.data_as(I))
        Xraw.append(X[:k]), pth.append(th[:k]), npk.append(k)
    return np.concatenate(Xraw), np.concatenate(pth), np.array(npk)


@pytest.mark.parametrize("name", rc.GROOVE_CASES)
def test_host_twin_rows(hc, cases, name):
    case = cases[name]
    bad = None
    if name == "pinched":      # the reference stops at the pinched row: the twin says NaN there, and is compared on the case without it
        bad = int(np.flatnonzero(rc.case_facts(case)["close"] < 0.004)[0])
        Xr, _, npk = _twin_rows(hc, case)
        at = npk[:bad].sum()
        assert npk[bad] == 2 and np.isnan(Xr[at:at + 2, 1]).all() and np.isfinite(np.delete(Xr, [at, at + 1], axis=0)).all()
        case = dict(case, polar=case["polar"].copy())
        case["polar"][bad] = cases["plain"]["polar"][bad]
    _, X_raw, peak_theta, rows = rc.features(case)
    Xr, pth, npk = _twin_rows(hc, case)
    np.testing.assert_array_equal(npk, np.bincount(rows, minlength=rc.R))
    np.testing.assert_array_equal(pth, peak_theta)
    worst = float(np.abs(Xr - X_raw).max()) if len(Xr) else 0.0
    print("%s: twin rows, worst |X_raw - oracle| = %.3g over %d peaks" % (name, worst, len(Xr)))
    np.testing.assert_allclose(Xr, X_raw, rtol=0, atol=1e-12)


def test_host_twin_forest_and_local_min(hc, cases, verdicts):
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for (fname, cname), (t, g) in verdicts.items():
        if not isinstance(g, dict):
            continue
        t = {k: np.ascontiguousarray(v) for k, v in t.items()}
        pr = np.array([hc.hc_rfc(ip(t["feat"]), fp(t["thr"]), ip(t["true_idx"]), ip(t["false_idx"]), fp(t["leaf_weight"]), ip(t["roots"]), len(t["roots"]),
                                 dp(np.ascontiguousarray(x))) for x in g["X"]], dtype=np.float32)
        np.testing.assert_array_equal(pr, g["proba"], err_msg="%s on %s" % (fname, cname))
        polar = cases[cname]["polar"]
        r0 = np.apply_along_axis(lambda x: x - np.mean(x), axis=1, arr=polar[:, 1, :])
        got = [hc.hc_local_min(dp(np.ascontiguousarray(polar[i, 0])), dp(np.ascontiguousarray(r0[i])), rc.M, ctypes.c_double(g["bg_theta"]), rc.IVAR) for i in range(rc.R)]
        np.testing.assert_array_equal(got, g["local_idx"], err_msg="%s on %s" % (fname, cname))


# ---- neck-image cases -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anp(request):
    """case name -> (case, oracle result under the threshold network evaluated on the host)"""
    out = {}
    for n in rc.ANP_CASES:
        c = rc.anp_case(n)
        out[n] = (c, rc.anp_expect(c))
    return out


def test_anp_cases_carry_their_facts(anp):
    th = {n: c["itr"][:, 0, :rc.M - 1] for n, (c, _) in anp.items()}
    d = {n: np.diff(t, axis=1) for n, t in th.items()}
    for n in ("sorted", "outside_lo", "outside_hi", "striped", "bare"):
        assert (d[n] > 0).all(), n
    assert len(np.unique(np.round(d["sorted"], 6))) > 1000      # non-uniform
    # unsorted: one descending pair in each of 40 rows, at index 1, 509, 510 and in the middle; runs of equal abscissae in ten of them
    rows, at = np.nonzero(d["unsorted"] < 0)
    assert len(rows) == 40 and len(np.unique(rows)) == 40 and {1, 509, 510} <= set(at + 1) and ((at + 1 > 10) & (at + 1 < 500)).sum() >= 10
    assert ((d["unsorted"] == 0).any(axis=1) & (d["unsorted"] < 0).any(axis=1)).sum() == 10
    # repeated: non-decreasing, runs of 2 and of 3 equal abscissae in 40 rows, unequal r across half of them, samples landing on ten
    c = anp["repeated"][0]
    assert (d["repeated"] >= 0).all() and (d["repeated"] == 0).any(axis=1).sum() == 40
    assert {1, 2} <= set((d["repeated"] == 0).sum(axis=1)[(d["repeated"] == 0).any(axis=1)])
    rows, at = np.nonzero(d["repeated"] == 0)
    unequal = c["itr"][rows, 1, at] != c["itr"][rows, 1, at + 1]
    assert unequal.sum() >= 10 and (~unequal).sum() >= 10
    hits = sum(int(th["repeated"][i, j] in np.linspace(th["repeated"][i, 0], th["repeated"][i, rc.M - 2], rc.M)) for i, j in zip(rows, at))
    assert hits >= 5
    # outside: bg_theta beyond every row's range
    assert anp["outside_lo"][0]["bg_theta"] < th["outside_lo"].min() and (anp["outside_lo"][1]["roll"] == 0).all()
    assert anp["outside_hi"][0]["bg_theta"] > th["outside_hi"].max() and (anp["outside_hi"][1]["roll"] == rc.M - 1).all()
    # striped: mask on in pixel 0, >= 200 edges in a row, edges on every ballot seam, a total that is no multiple of 256, every run length
    g = anp["striped"][1]
    e, m = g["edge"], g["mask"]
    assert m[:, 0].sum() >= 10 and (e[:, 0] == m[:, 0]).all() and e.sum(axis=1).max() >= 200 and e.sum() % 256 != 0
    assert all(e[:, 64 * s].any() for s in range(1, 8))
    runs = set()
    for row in m[e.sum(axis=1) > 2]:
        runs |= set(np.diff(np.flatnonzero(np.r_[True, row[1:] != row[:-1], True])).tolist())
    assert {1, 2, 63, 64, 65} <= runs
    assert m.all(axis=1).sum() >= 10 and (~m).all(axis=1).sum() >= 10
    # sorted: the level set is one closed curve -- the mask's rows are consecutive and each holds one run (two where the roll cuts it)
    g = anp["sorted"][1]
    on = np.flatnonzero(g["mask"].any(axis=1))
    assert len(on) > 100 and on[-1] - on[0] == len(on) - 1 and g["edge"].sum(axis=1).max() <= 3 and not g["mask"][[0, -1]].any()
    # bare: fewer than 6 edge pixels
    assert 0 < anp["bare"][1]["edge"].sum() < 6 and anp["bare"][1]["plane"] is None
    # the threshold network draws what the cases mean: no pixel sits on the level
    for n, (_, g) in anp.items():
        assert (np.abs(g["image"].astype(np.float32) - np.float32(rc.LEVEL)) > 1e-6).all(), n


@pytest.mark.parametrize("name", rc.ANP_PLANE_CASES)
def test_plane_cases_are_well_conditioned(anp, name):
    g = anp[name][1]
    w = np.linalg.eigvalsh(np.cov(g["points_obb"].T))
    print("%s: %d edge points, covariance eigenvalues %s" % (name, len(g["points_obb"]), w))
    assert w[1] >= 2.0 * w[0] > 0 and g["plane"] is not None and np.isfinite(np.r_[g["plane"][0], g["plane"][1]]).all()


def test_host_interp_on_the_sorted_rows(hc, anp):
    """sh::interp1 (np.interp without a guess, what k_anp_rows' parallel search restates) on rows with repeated abscissae"""
    c, g = anp["repeated"]
    th = c["itr"][:, 0, :rc.M - 1]
    for i in np.flatnonzero((np.diff(th, axis=1) == 0).any(axis=1))[::4]:
        xp, fp = np.ascontiguousarray(th[i]), np.ascontiguousarray(c["itr"][i, 1, :rc.M - 1])
        t = np.linspace(xp[0], xp[-1], rc.M)
        got = np.array([hc.hc_interp(ctypes.c_double(x), dp(xp), dp(fp), rc.M - 1) for x in t])
        np.testing.assert_array_equal(np.roll(got, -int(g["roll"][i])), g["itr_shft"][i, 1])


# ---- runtime --------------------------------------------------------------------------------------------------------------------------
def test_zz_oracle_time(verdicts, anp):
    """(runs last in this file: the fixtures above have spent the time by now)"""
    print("oracle time of the row cases: %.1f s" % rc.ORACLE_SECONDS[0])
    assert rc.ORACLE_SECONDS[0] <= ORACLE_BUDGET_S
