"""Polar rows no bone has produced, for the row kernels around the network (k_groove_rows, k_groove_scale, k_groove_rfc, k_groove_tail,
k_anp_rows, k_anp_edge_count, k_anp_edges, k_anp_plane) and for their host twins in sh_scalar.h.  Helper of test_row_cases_host.py,
test_gpu_groove_rows.py and test_gpu_anp_rows.py: generators, forests and oracle wrappers; no test functions, no library code under test.
NumPy and SciPy only, seeded, reads no file (the shipped forest is handed in by the caller).

Groove cases (one batch item each: 330 rows x (theta, r) x 512 for the rows [GA, GB) of the proximal set, zs, centroids, canal axis, frame).
theta ascends from -pi as roll_to_argmin_theta leaves it, r is a per-row seeded sum of low harmonics plus the case's own feature; what
each case carries is computed from SciPy alone by case_facts and asserted in test_row_cases_host.py:
  plain     1-6 passing peaks per row, 0.02 mm noise
  rough     0.5 mm noise: rows with more than 64 local maxima of the rolled filtered row, some with a passing peak beyond the 64th
  crowded   >= 8 passing peaks in every row, 7th and 8th prominence apart by > 1e-9; every row keeps 7, feature 8 is exactly 1 -> scaled 0
  terraced  r piecewise constant in runs of >= 12 samples: true plateaus of the filtered row, flat tops of even and odd length, flat valleys
  seam_lo   deepest minimum of the filtered row at index <= 2, a peak within 5 samples of the roll seam, the groove at theta ~ -pi + 0.03
  seam_hi   ... at index >= 509, the groove at theta ~ pi - 0.01 behind every row's last theta (searchsorted == M)
  sparse    all rows but three peakless, fewer than 8 peaks in the item, all zs equal
  pinched   two passing peaks of one row within 0.004 rad: the reference raises IndexError

Forests (tables in the format of rfc_bg3.npz; all pass sh_params.h's forest_check, which asks for ids and indices in range, children both
or neither, every node reached once -- a root that is a leaf is accepted, so is a single tree, so no shape had to be dropped):
  bracket(X)  per chosen (peak, feature) two one-split trees, thresholds the float32 just below and just above X[p, f]
  equal0      splits on feature 8 at 0.0, -0.0 and -1e-30
  chain       ONE tree (roots = [0]), 40 levels deep on one side
  mute        every leaf sum <= 0.4: no candidate

Neck-image cases: 512 rows x (theta, r) x 512 of the rows the network reads, bg_theta, zs (see anp_case)."""
import time

import numpy as np
import scipy.signal

from oracle import anp as o_anp
from oracle import groove as o_groove
from oracle import rfc as o_rfc
from oracle import slices as o_slices

M = 512
NPROX = 600
GA, GB = o_slices.cutoff_range(NPROX, (0.2, 0.75))
R = GB - GA
ANP0, ANP_ROWS = 88, 512
IVAR = int(round(7 / (360 / M)))
TWO_PI = 2.0 * np.pi

GROOVE_CASES = ("plain", "rough", "crowded", "terraced", "seam_lo", "seam_hi", "sparse", "pinched")
ORACLE_SECONDS = [0.0]      # time spent inside the oracle by the wrappers below (test_row_cases_host.py prints and bounds it)


# ---- groove cases ---------------------------------------------------------------------------------------------------------------------
def _theta(rng, rows=R, jitter=0.3):
    """ascending from -pi: one sample per cell of 2 pi / 512, jittered inside its cell"""
    k = np.arange(M)[None, :]
    return -np.pi + (k + 0.5 + rng.uniform(-jitter, jitter, (rows, M))) * (TWO_PI / M)


def _harmonics(rng, th, orders, lo, hi):
    r = np.zeros_like(th)
    for h in orders:
        a = rng.uniform(lo, hi, (len(th), 1))
        p = rng.uniform(0, TWO_PI, (len(th), 1))
        r += a * np.cos(h * th + p)
    return r


def _frame(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-50, 50, 3)
    return T


def _valley(th, centre, depth, width):
    """a groove: -depth at centre, `width` rad wide (wrapped)"""
    d = np.arctan2(np.sin(th - centre), np.cos(th - centre))
    return -depth * np.exp(-0.5 * (d / width) ** 2)


def groove_case(name):
    """-> dict(name, polar (330, 2, 512), zs (330,), centroids (330, 2), canal (2, 3), T_obb (4, 4))"""
    rng = np.random.default_rng([GROOVE_CASES.index(name), 20240])
    th = _theta(rng)
    zs = np.linspace(rng.uniform(40, 60), rng.uniform(-60, -40), R)
    if name == "plain":
        r = 20.0 + _harmonics(rng, th, (2, 3, 5), 0.8, 1.8) + rng.normal(0, 0.02, th.shape)
    elif name == "rough":
        r = 20.0 + 3.0 * np.cos(2 * th) + 1.5 * np.cos(5 * th + 1.0) + _harmonics(rng, th, (3,), 0.0, 0.4) + rng.normal(0, 0.5, th.shape)
    elif name == "crowded":
        amp = 2.0 + _harmonics(rng, th, (1, 3), 0.2, 0.5)
        r = 20.0 + amp * np.cos(10 * th + rng.uniform(0, TWO_PI, (R, 1)))
        # rows 300-309: teeth 7 samples apart and 24-36 mm high -- what the 10-tap filter leaves of them is > 64 PASSING peaks, so the cut
        # to the 7 most prominent has more than one batch of candidates to choose from
        k = np.arange(M)[None, :]
        r[300:310] = 60.0 + np.where(k % 7 < 3, 1.0, -1.0) * (30.0 + _harmonics(rng, th[300:310], (1, 3), 1.0, 3.0))
    elif name == "terraced":
        # Every terrace has a level of its own (the smooth curve at its middle + a draw): where the filter's ten samples lie inside one
        # run it repeats one sum, so tops and valleys are flat in ANY arithmetic.  Levels shared between terraces, or an extreme
        # terrace at the row's ends (whose five edge samples are a fitted line), would tie only up to the rounding of SciPy's
        # taps (0.1 +- 3e-17, LAPACK-dependent) -- nothing to hold a kernel to -- so the levels are distinct and rise or fall
        # steadily across the last two and the first two terraces (rows are drawn again until they do).
        r = np.zeros_like(th)
        for i in range(R):
            while True:
                smooth = 20.0 + _harmonics(rng, th[i:i + 1], (2, 3, 4), 0.8, 1.8)[0]
                k, lv = 0, []
                while k < M:
                    n = int(rng.integers(12, 22))
                    if M - (k + n) < 12:
                        n = M - k
                    lv.append(smooth[k + n // 2] + rng.uniform(-0.3, 0.3))
                    r[i, k:k + n] = lv[-1]
                    k += n
                d = np.diff([lv[-2], lv[-1], lv[0], lv[1]])
                if (d > 0.05).all() or (d < -0.05).all():
                    break
    elif name in ("seam_lo", "seam_hi"):
        lo = name == "seam_lo"
        # the last samples of seam_hi share one theta ramp in every row, so that the KDE's grid point lies behind all of them
        if not lo:
            grid = np.linspace(-np.pi, np.pi, 1024)[1021]
            th[:, 500:] = grid - 2e-4 + (np.arange(500, M) - 506)[None, :] * 3e-5
        else:
            th[:, :14] = -np.pi + 0.03 + (np.arange(14) - 6)[None, :] * 0.004
        r = 20.0 + _harmonics(rng, th, (2, 3), 0.3, 0.8) + rng.normal(0, 0.02, th.shape)
        k = np.arange(M)[None, :]
        # Rows 40 on: a smooth groove at sample 6 (seam_lo) / 505.5 (seam_hi).  Rows 0-39: the first (last) ten samples are a shelf of
        # five at +2.5 and a slot of five at -10, a shelf at +3 behind them.  The edge samples of the filter are the least-squares
        # line through those ten, which ends 4.8 below the mean at sample 0 (511) -- the row's deepest minimum, so the roll is 0
        # (511) -- and the first sample of the box filter, 5 (506), is a passing peak between the line and the shelf behind it.
        if lo:
            r += -4.0 * np.exp(-0.5 * ((k - 6) / 2.5) ** 2)
            r[:40, :22] = 20.0 + rng.normal(0, 0.02, (40, 22)) + np.r_[np.full(5, 2.5), np.full(5, -10.0), np.full(12, 3.0)]
            r[100:140] -= 6.0 * np.exp(-0.5 * (k - 510.0) ** 2)      # the radius minimum of the window in the row's tail: negative local index
        else:
            r += -4.0 * np.exp(-0.5 * ((k - 505.5) / 2.5) ** 2)
            r[:40, M - 22:] = 20.0 + rng.normal(0, 0.02, (40, 22)) + np.r_[np.full(12, 3.0), np.full(5, -10.0), np.full(5, 2.5)]
    elif name == "sparse":
        r = 20.0 + rng.normal(0, 1e-3, th.shape)
        for i, c in ((17, 0.4), (150, 0.45), (301, 0.5)):
            r[i] += _valley(th[i], c, 3.0, 0.12) + _valley(th[i], c + 2.0, 2.0, 0.12)
        zs = np.full(R, 12.5)
    elif name == "pinched":
        r = 20.0 + _harmonics(rng, th, (2, 3, 5), 0.8, 1.8) + rng.normal(0, 0.02, th.shape)
        i = 77      # this row: two grooves 40 samples apart on a circle, theta squeezed to 1e-4 rad per sample between them
        k = np.arange(M)
        r[i] = 20.0 + rng.normal(0, 1e-3, M) - 3.0 * np.exp(-0.5 * ((k - 200) / 6.0) ** 2) - 2.5 * np.exp(-0.5 * ((k - 236) / 6.0) ** 2)
        step = np.full(M, 0.0)
        step[1:] = np.where((k[1:] > 190) & (k[1:] <= 246), 1e-4, (TWO_PI - 0.02 - 56e-4) / (M - 1 - 56))
        th[i] = -np.pi + 0.01 + np.cumsum(step)
    else:
        raise KeyError(name)
    assert (np.diff(th, axis=1) > 0).all() and th.min() >= -np.pi and th.max() <= np.pi
    polar = np.ascontiguousarray(np.stack([th, r], axis=1))
    canal = np.array([[rng.uniform(-3, 3), rng.uniform(-3, 3), 110.0], [rng.uniform(-3, 3), rng.uniform(-3, 3), -120.0]])
    return dict(name=name, polar=polar, zs=zs, centroids=rng.uniform(-4, 4, (R, 2)), canal=canal, T_obb=_frame(rng))


def filtered_rolled(case):
    """SciPy's view of every row: (amin (330,), rolled filtered rows (330, 512))"""
    r = case["polar"][:, 1, :]
    r0 = np.apply_along_axis(lambda x: x - np.mean(x), axis=1, arr=r)
    filt = scipy.signal.savgol_filter(-1 * r0, 10, 1, axis=1)
    amin = np.argmin(filt, axis=1)
    return amin, np.stack([np.roll(f, -a) for f, a in zip(filt, amin)])


def case_facts(case):
    """What the case carries, from SciPy alone -> dict of per-row arrays: n_max (local maxima of the rolled filtered row), n_pass (peaks
    find_peaks keeps), beyond (passing peaks behind the 64th maximum), amin, gap78 (7th minus 8th prominence, inf below 8 peaks), seam
    (a passing peak within 5 samples of either end of the rolled row), flat_odd / flat_even (passing peaks with a flat top of odd / even
    length > 1), flat_valley (a prominence base that is one of several equal samples), close (least theta distance of two passing peaks)."""
    amin, rolled = filtered_rolled(case)
    th = case["polar"][:, 0, :]
    keys = ("n_max", "n_pass", "beyond", "gap78", "seam", "flat_odd", "flat_even", "flat_valley", "close")
    f = {k: [] for k in keys}
    for i, x in enumerate(rolled):
        allmax, _ = scipy.signal.find_peaks(x)
        pk, pr = scipy.signal.find_peaks(x, height=-10, prominence=0.6, width=0.1, plateau_size=1)
        f["n_max"].append(len(allmax))
        f["n_pass"].append(len(pk))
        f["beyond"].append(int((np.searchsorted(allmax, pk) >= 64).sum()))
        p = np.sort(pr["prominences"])[::-1]
        f["gap78"].append(p[6] - p[7] if len(p) >= 8 else np.inf)
        f["seam"].append(bool(((pk <= 5) | (pk >= M - 6)).any()))
        f["flat_odd"].append(int(((pr["plateau_sizes"] > 1) & (pr["plateau_sizes"] % 2 == 1)).sum()))
        f["flat_even"].append(int(((pr["plateau_sizes"] > 1) & (pr["plateau_sizes"] % 2 == 0)).sum()))
        fv = 0
        for b, side in zip(np.r_[pr["left_bases"], pr["right_bases"]], np.r_[np.full(len(pk), -1), np.full(len(pk), 1)]):
            nb = b + side
            fv += int(0 <= nb < M and x[nb] == x[b])
        f["flat_valley"].append(fv)
        t = th[i][(pk + amin[i]) % M]
        d = np.abs(np.arctan2(np.sin(t[:, None] - t[None, :]), np.cos(t[:, None] - t[None, :]))) + 10.0 * np.identity(len(t))
        f["close"].append(d.min() if len(t) > 1 else np.inf)
    out = {k: np.array(v) for k, v in f.items()}
    out["amin"] = amin
    return out


def groove_expect(case, tables):
    """oracle.groove.groove_points / groove_axis of the case under the forest `tables`: the result dict (+ "axis_ct"), or the name of the
    exception it raised"""
    t0 = time.perf_counter()
    try:
        g = o_groove.groove_points(case["polar"], case["zs"], case["centroids"], case["canal"], case["T_obb"], tables)
        g["axis_ct"] = o_groove.groove_axis(g["points_obb"], case["T_obb"])
        return g
    except (IndexError, ValueError) as e:
        return type(e).__name__
    finally:
        ORACLE_SECONDS[0] += time.perf_counter() - t0


def features(case):
    """the oracle's (X scaled, X raw, peak_theta, rows) of a case: what a forest walks (needs no forest)"""
    t0 = time.perf_counter()
    try:
        polar = case["polar"]
        polar_0 = polar.copy()
        polar_0[:, 1, :] = np.apply_along_axis(lambda x: x - np.mean(x), axis=1, arr=polar[:, 1, :])
        return o_groove.x_process(polar, polar_0, case["zs"], case["canal"], M)
    finally:
        ORACLE_SECONDS[0] += time.perf_counter() - t0


# ---- forests --------------------------------------------------------------------------------------------------------------------------
def _tables(feat, thr, ti, fi, lw, roots):
    ti = np.asarray(ti, np.int32)
    return dict(feat=np.asarray(feat, np.int32), thr=np.asarray(thr, np.float32), true_idx=ti, false_idx=np.asarray(fi, np.int32),
                leaf_weight=np.asarray(lw, np.float32), is_leaf=ti < 0, roots=np.asarray(roots, np.int32))


def _stumps(splits):
    """one tree per (feature, float32 threshold): root, true leaf 2^-(2t+1), false leaf 2^-(2t+2) -- the sum names every leaf reached"""
    assert len(splits) <= 11      # 22 significant bits: the float32 sum is exact
    feat, thr, ti, fi, lw, roots = [], [], [], [], [], []
    for t, (f, v) in enumerate(splits):
        n = len(feat)
        roots.append(n)
        feat += [f, 0, 0]
        thr += [v, 0.0, 0.0]
        ti += [n + 1, -1, -1]
        fi += [n + 2, -1, -1]
        lw += [0.0, 2.0 ** -(2 * t + 1), 2.0 ** -(2 * t + 2)]
    return _tables(feat, thr, ti, fi, lw, roots)


def stump_leaves(proba, n_trees):
    """the leaves a _stumps forest reached, from its float32 sum -> bool (n, n_trees), True = the true child"""
    bits = np.round(np.asarray(proba, np.float64) * 2.0 ** (2 * n_trees)).astype(np.int64)
    out = np.zeros((len(bits), n_trees), dtype=bool)
    for t in range(n_trees):
        two = (bits >> (2 * (n_trees - 1 - t))) & 3
        assert ((two == 1) | (two == 2)).all()
        out[:, t] = two == 2
    return out


BRACKET_MARGIN = 1e-8      # ten times the 1e-9 by which the project lets groove.xs differ


def bracket(X, pairs=5, seed=0):
    """-> (tables, picks): picks = [(p, f)], tree 2 j splits on the float32 just below X[p, f] (p goes to the FALSE child), tree 2 j + 1
    on the float32 just above (TRUE child).  Only (p, f) whose value lies more than BRACKET_MARGIN from every other peak's value of that
    feature AND from both thresholds (so that a device value 1e-9 off still falls between them); values that round DOWN to float32 first:
    those a walk that narrows the feature to float sends the wrong way."""
    rng = np.random.default_rng(seed)
    picks, splits = [], []
    cand = [(int(p), int(f)) for f in rng.permutation(9) for p in rng.permutation(len(X))[:40]]
    for want_down in (True, False):
        for p, f in cand:
            if len(picks) >= pairs or any(f == g for _, g in picks):
                continue
            x = X[p, f]
            mid = np.float32(x)
            below = mid if float(mid) < x else np.nextafter(mid, np.float32(-np.inf))
            above = mid if float(mid) > x else np.nextafter(mid, np.float32(np.inf))
            others = np.abs(np.delete(X[:, f], p) - x).min()
            if float(mid) == x or others <= BRACKET_MARGIN or x - float(below) <= BRACKET_MARGIN or float(above) - x <= BRACKET_MARGIN:
                continue
            if want_down and not float(mid) < x:
                continue
            picks.append((p, f))
            splits += [(f, below), (f, above)]
    assert len(picks) == pairs
    return _stumps(splits), picks


def equal0():
    """feature 8 at 0.0, -0.0, -1e-30: x = 0 goes true, true, false"""
    return _stumps([(8, np.float32(0.0)), (8, np.float32(-0.0)), (8, np.float32(-1e-30))])


def chain(X, depth=40):
    """one tree: node i splits feature i % 9 at that column's q (even i) or 1 - q (odd i) quantile, q = 3, 6, 9 %; the rarer side is a leaf of weight
    (i + 1) / 64, the other the next node; the last node's common side a leaf of weight 41 / 64"""
    feat, thr, ti, fi, lw = [], [], [], [], []
    for i in range(depth):
        f = i % 9
        low = i % 2 == 0
        node, leaf, nxt = 2 * i, 2 * i + 1, 2 * i + 2
        feat += [f, 0]
        q = 0.03 * (1 + i // 18)      # (a feature comes back on the same side every 18 levels: cut deeper then)
        thr += [np.float32(np.quantile(X[:, f], q if low else 1.0 - q)), 0.0]
        ti += [leaf if low else nxt, -1]
        fi += [nxt if low else leaf, -1]
        lw += [0.0, (i + 1) / 64.0]
    feat.append(0), thr.append(0.0), ti.append(-1), fi.append(-1), lw.append((depth + 1) / 64.0)
    return _tables(feat, thr, ti, fi, lw, [0])


def mute():
    """two stumps whose leaf sums are 0.375 at most"""
    t = _stumps([(0, np.float32(0.0)), (4, np.float32(0.0))])
    t["leaf_weight"] = (t["leaf_weight"] * np.float32(0.5)).astype(np.float32)
    return t


FOREST_CASES = {"shipped": GROOVE_CASES, "bracket": ("plain", "rough"), "equal0": ("crowded", "plain"),
                "chain": ("plain", "terraced", "sparse", "seam_lo"), "mute": ("plain", "crowded")}


def forest_for(fname, cname, cases, shipped):
    """the tables of forest `fname` as paired with case `cname` (bracket is built on that case's own features, chain on plain's)"""
    if fname == "shipped":
        return shipped
    if fname == "bracket":
        return bracket(features(cases[cname])[0])[0]
    if fname == "chain":
        return chain(features(cases["plain"])[0])
    return {"equal0": equal0, "mute": mute}[fname]()


def groove_pairings(cases, shipped):
    """every (forest name, case name, tables) the tests run"""
    for fname, names in FOREST_CASES.items():
        for cname in names:
            yield fname, cname, forest_for(fname, cname, cases, shipped)


def forest_ok(t):
    """sh_params.h's forest_check restated: ids in range, children both or neither and in range, roots in range, every node reached once"""
    n = len(t["feat"])
    ti, fi = t["true_idx"], t["false_idx"]
    if ((t["feat"] < 0) | (t["feat"] >= 9)).any() or ((ti < 0) != (fi < 0)).any() or (ti >= n).any() or (fi >= n).any():
        return False
    if ((t["roots"] < 0) | (t["roots"] >= n)).any():
        return False
    seen = np.zeros(n, bool)
    stack = [int(r) for r in t["roots"]][::-1]
    while stack:
        i = stack.pop()
        if seen[i]:
            return False
        seen[i] = True
        if ti[i] >= 0:
            stack += [int(ti[i]), int(fi[i])]
    return True


def save_forest(path, t):
    np.savez(path, **t)
    return str(path)


# ---- neck-image cases -----------------------------------------------------------------------------------------------------------------
ANP_CASES = ("sorted", "unsorted", "repeated", "outside_lo", "outside_hi", "striped", "bare")
ANP_PLANE_CASES = ANP_CASES[:-1]      # `bare` has fewer than 6 edge pixels: a geometry error, no plane
LEVEL = 0.6                           # the threshold network's level: logit = 8 (x - 0.6)


def _cap(th, centre):
    """a cap-like surface over (row, theta): its 0.6 level set (after min-max scaling) is one closed curve"""
    i = np.arange(ANP_ROWS)[:, None]
    d = np.arctan2(np.sin(th - centre), np.cos(th - centre))
    return 20.0 + 10.0 * np.exp(-((i - 256.0) / 110.0) ** 2 - (d / 0.9) ** 2) + 0.3 * np.cos(3.0 * th)


def anp_case(name):
    """-> dict(name, itr (512, 2, 512): the rows [88, 600) of "prox.itr_start", bg_theta, zs (512,)).  Column 511 of a row closes the
    contour and is not read (anatomic_neck.py:40-47 samples and interpolates theta[:-1]).
      sorted      theta strictly ascending, non-uniform; r a cap
      unsorted    as sorted, one descending pair of abscissae in each of 40 rows (at index 1, 509, 510 and in the middle: the kernel's
                  sequential replay of np.interp); ten of them also carry a run of equal abscissae with equal r (NumPy's NaN retry)
      repeated    as sorted, runs of 2-3 equal abscissae in 40 rows, every other one with unequal r across the run, and (every fourth)
                  a sample of the row's grid landing exactly on the repeated abscissa
      outside_lo / outside_hi   bg_theta below every row's first theta (roll 0) / above every last one (roll 511)
      striped     the abscissae ARE the row's sampling grid (samples 0-509 and 511), so pixel j is r[j] exactly: r alternates across the
                  level every 1, 2, 63, 64 and 65 pixels in 15 rows, every 16th row wholly above it, the rest wholly below
      bare        a flat surface with one bump of 2 rows x 3 pixels: 4 edge pixels"""
    rng = np.random.default_rng([ANP_CASES.index(name), 515])
    n = M - 1
    k = np.arange(n)[None, :]
    th = -np.pi + 0.01 + (k + 0.5 + rng.uniform(-0.3, 0.3, (ANP_ROWS, n))) * ((TWO_PI - 0.02) / n)
    bg = {"sorted": 0.3, "unsorted": -1.1, "repeated": 2.0, "outside_lo": -3.5, "outside_hi": 3.5, "striped": -3.5, "bare": 0.7}[name]
    zs = np.linspace(100.0, -20.0, ANP_ROWS) + rng.uniform(-0.01, 0.01, ANP_ROWS)      # (steep enough that the cap's curve is longer in z than deep)
    r = _cap(th, bg + rng.uniform(-0.5, 0.5))
    rows40 = np.arange(40) * 12 + 9
    if name == "unsorted":
        for q, i in enumerate(rows40):
            at = (1, 509, 510, int(rng.integers(20, 490)))[q % 4]      # theta[at] < theta[at - 1]
            th[i, [at - 1, at]] = th[i, [at, at - 1]]
            if q % 4 == 3:
                j = (at + 100) % 480 + 10
                th[i, j + 1] = th[i, j]
                r[i, j + 1] = r[i, j]
    elif name == "repeated":
        for q, i in enumerate(rows40):
            j, run = int(rng.integers(5, 500)), 2 + q % 2
            if q % 4 == 0:      # a sample of linspace(theta[0], theta[510], 512) itself (the ends stay)
                j = int(rng.integers(100, 400))
                grid = np.linspace(th[i, 0], th[i, n - 1], M)
                th[i, j] = grid[np.searchsorted(grid, th[i, j])]
            th[i, j:j + run] = th[i, j]
            if q % 2 == 1:
                r[i, j:j + run] = r[i, j]
            assert (np.diff(th[i]) >= 0).all()
    elif name == "striped":
        grid = np.linspace(-3.1, 3.1, M)
        th = np.repeat(np.r_[grid[:M - 2], grid[M - 1]][None, :], ANP_ROWS, axis=0)
        j = np.arange(n)[None, :]
        i = np.arange(ANP_ROWS)[:, None]
        period = np.array([1, 2, 63, 64, 65])[i % 5]
        on = (j // period) % 2 == 0
        # 15 striped rows in three places, every 16th row wholly above the level, the rest below it: ~2 500 edge pixels in all (the
        # reference's plane fit is a full SVD of the 3 x K point matrix -- K x K doubles -- so K stays in the thousands)
        striped_row = ((i >= 96) & (i < 101)) | ((i >= 250) & (i < 255)) | ((i >= 400) & (i < 405))
        on = np.where(i % 16 == 7, True, np.where(striped_row, on, False))
        r = np.where(on, 25.0, 15.0) + rng.uniform(-0.5, 0.5, (ANP_ROWS, n))
        zs = np.linspace(52.0, 48.0, ANP_ROWS)
    elif name == "bare":
        r = 20.0 + rng.uniform(0.0, 0.5, (ANP_ROWS, n))
        r[200:202, 300:303] = 30.0
    itr = np.zeros((ANP_ROWS, 2, M))
    itr[:, 0, :n], itr[:, 1, :n] = th, r
    itr[:, :, n] = itr[:, :, 0]
    return dict(name=name, itr=itr, bg_theta=float(bg), zs=zs)


def threshold_logits(image):
    """what the threshold network makes of an image, on the host (the GPU tests take the device's logits instead)"""
    return (np.float32(8.0) * (image.astype(np.float32) - np.float32(LEVEL))).astype(np.float32)


def anp_expect(case, logits=None):
    """oracle.anp of the case: anp_image (roll, itr_shft, image), then -- from the logits fetched from the device, or the threshold
    network's on the host -- mask_points and neck_plane (None with fewer than 6 edge pixels: the reference's ellipse fit fails)"""
    t0 = time.perf_counter()
    try:
        image, itr_shft, roll = o_anp.anp_image(case["itr"], case["bg_theta"])
        lg = threshold_logits(image) if logits is None else logits
        mp = o_anp.mask_points(lg, itr_shft, case["zs"])
        plane = o_anp.neck_plane(mp["points_obb"]) if len(mp["points_obb"]) >= 6 else None
        return dict(image=image, itr_shft=itr_shft, roll=roll, edge=mp["edge"], mask=mp["mask"], points_obb=mp["points_obb"], plane=plane)
    finally:
        ORACLE_SECONDS[0] += time.perf_counter() - t0
