"""Rigid registration onto the resident batch (include/shoulder_hip.h sh_register_points), the parts that need no GPU (the record and
options layout: test_abi_exports.py): the ordered argument checks, sym4_jacobi against numpy.linalg.eigh, chol6_solve
against numpy.linalg.solve, the summation tree, and the host twins of one evaluation and of the whole loop (the device source,
host-compiled with -ffp-contract=off through tests/hostcheck/icp_check.cpp) against the NumPy statement of tests/icp_oracle.py.

Bounds.  Twins against the oracle: bytes (the same + - x / sqrt in the same order).  sym4_jacobi against eigh: both are backward
stable, so an eigenvalue differs by a modest multiple of eps ||A||; 64 eps ||A||_F is asserted (cyclic Jacobi after 12 sweeps of a
4 x 4 is converged to rounding, eigh's own error is a few eps ||A||).  chol6_solve against solve: the forward error of either is
bounded by a small multiple of cond(A) eps |x|; 64 cond(A) eps max|x| is asserted."""
import ctypes
import subprocess

import numpy as np
import pytest

import icp_oracle as O
from shoulder_amd import _lib

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("icp_check"))


def ptr(a):
    return a.ctypes.data if a is not None else None


def test_entry_point_checks_its_arguments_in_order_without_a_gpu(shim):
    L = _lib.load()
    pts, good = np.zeros((4, 3)), _lib.IcpOptions(_lib.ICP_PLANE, 8, np.inf, 0.0)
    assert L.sh_register_points(None, ctypes.c_void_p(pts.ctypes.data), 4, 0, None, ctypes.byref(good), None, None) == O.ARG      # (no context)
    assert "sh_register_points" in _lib.EXPORTS

    def pre(p=pts, Q=4, per=0, T0=None, opt=good, B=2, pend=0, ctx=1):
        return shim.ic_precheck(ctx, ptr(p), Q, per, ptr(T0), ctypes.addressof(opt) if opt is not None else None, B, pend)
    assert pre() == 0 and pre(Q=1) == 0
    # 1 the context and the pointers
    assert pre(ctx=0) == O.ARG and pre(p=None) == O.ARG and pre(opt=None) == O.ARG
    # 2 Q
    assert pre(Q=0) == O.ARG and pre(Q=-1) == O.ARG and pre(Q=_lib.CLOSEST_MAX + 1) == O.ARG
    # 3 the options
    opts = lambda **kw: _lib.IcpOptions(**{**dict(metric=1, max_iter=8, reject=np.inf, tol=0.0), **kw})
    for ok in (opts(metric=0), opts(max_iter=1), opts(max_iter=64), opts(reject=1e-300), opts(tol=5.0)):
        assert pre(opt=ok) == 0
    for bad in (opts(metric=2), opts(metric=-1), opts(max_iter=0), opts(max_iter=65), opts(reject=0.0), opts(reject=-1.0), opts(reject=np.nan),
                opts(tol=-1e-300), opts(tol=np.nan), opts(tol=np.inf)):
        assert pre(opt=bad) == O.ARG and pre(opt=bad, B=0) == O.ARG          # (before the state)
    # 4 the state
    assert pre(B=0) == O.STATE and pre(pend=1) == O.STATE
    # 5 the coordinates: after the state, before T0
    for k, v in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        p = pts.copy()
        p[3, k] = v
        assert pre(p=p) == O.ARG and pre(p=p, Q=3) == 0 and pre(p=p, B=0) == O.STATE
    per = np.zeros((2, 2, 3))
    assert pre(p=per, Q=2, per=1) == 0
    per[1, 1, 2] = np.nan
    assert pre(p=per, Q=2, per=1) == O.ARG and pre(p=per, Q=2, per=0) == 0
    # 6 T0: every humerus' matrix, rigid to 1e-9
    I2 = np.stack([np.identity(4)] * 2)
    rot = O.rigid((1.0, 2.0, 3.0), 40.0, (5.0, -6.0, 7.0))
    assert pre(T0=I2) == 0 and pre(T0=np.stack([rot, rot])) == 0
    reflect, shear, row, tiny, nan = (I2.copy() for _ in range(5))
    reflect[1, 0, 0] = -1.0                       # a reflection: det < 0
    shear[1, 0, 1] = 1e-6                         # a shear of 1e-6: R^T R is off by 1e-6
    row[1, 3, 3] = 1.0 + 1e-12                    # the last row must be exact
    tiny[1, 0, 1] = 1e-10                         # within the 1e-9 of the definition
    nan[0, 2, 3] = np.nan
    assert pre(T0=reflect) == O.ARG and pre(T0=shear) == O.ARG and pre(T0=row) == O.ARG and pre(T0=nan) == O.ARG and pre(T0=tiny) == 0
    assert pre(T0=reflect, B=1) == 0              # (only the B matrices of the batch are read)
    assert pre(T0=shear, B=0) == O.STATE and pre(T0=shear, Q=0) == O.ARG
    p = pts.copy()
    p[0, 0] = np.nan
    assert pre(p=p, T0=shear, pend=1) == O.STATE


def random_symmetric():
    """400 symmetric 4 x 4: general ones at scales 1e-6 .. 1e6, 80 with a repeated largest eigenvalue, 40 diagonal or zero"""
    rng = np.random.default_rng(17)
    out = []
    for k in range(400):
        if k < 280:
            A = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-6, 7)
            A = A + A.T
        elif k < 360:
            Qm = np.linalg.qr(rng.normal(size=(4, 4)))[0]
            w = np.array([2.0, 2.0, rng.uniform(-1.0, 1.0), rng.uniform(-3.0, 1.0)]) if k % 2 else np.array([1.5, 1.5, 1.5, -rng.uniform(0.0, 2.0)])
            A = (Qm * w) @ Qm.T
            A = (A + A.T) * 0.5
        else:
            A = np.diag(rng.integers(-3, 4, 4).astype(np.float64)) if k % 4 else np.zeros((4, 4))
        out.append(A)
    return out


def test_sym4_jacobi_against_eigh(shim):
    worst = 0.0
    for A in random_symmetric():
        D, V = np.ascontiguousarray(A.copy()), np.zeros((4, 4))
        shim.ic_jacobi(D.ctypes.data, V.ctypes.data)
        Ao, Vo = O.sym4_jacobi([list(map(float, r)) for r in A])
        assert np.array(Ao).tobytes() == D.tobytes() and np.array(Vo).tobytes() == V.tobytes()      # the twin is the oracle
        w = np.linalg.eigh(A)[0]
        norm = np.linalg.norm(A)
        lam = np.diag(D)
        assert np.abs(np.sort(lam) - w).max() <= 64 * EPS * norm
        worst = max(worst, np.abs(np.sort(lam) - w).max() / (EPS * norm) if norm else 0.0)
        assert np.abs(V.T @ V - np.identity(4)).max() <= 64 * EPS and np.abs(A @ V - V * lam).max() <= 64 * EPS * max(norm, 1e-300)
    print("largest |lambda - eigh| / (eps ||A||):", worst)
    # which eigenvector wins among equal eigenvalues: the first.  A diagonal matrix is left alone (every a_pq is 0.0)
    for diag, want in (((2.0, 2.0, 1.0, 0.0), 0), ((1.0, 3.0, 3.0, 3.0), 1), ((0.0, 0.0, 0.0, 0.0), 0), ((-1.0, -2.0, -1.0, -3.0), 0)):
        A = [[diag[i] if i == j else 0.0 for j in range(4)] for i in range(4)]
        Ao, Vo = O.sym4_jacobi(A)
        best = 0
        for i in range(1, 4):
            if Ao[i][i] > Ao[best][best]:
                best = i
        assert best == want and np.array_equal(np.array(Vo), np.identity(4))


def test_chol6_solve_against_numpy_and_its_failure(shim):
    rng = np.random.default_rng(23)
    worst = 0.0
    for k in range(200):
        J = rng.normal(size=(rng.integers(6, 40), 6)) * 10.0 ** rng.uniform(-2, 2, size=6)
        A, b = J.T @ J, rng.normal(size=6)
        A = (A + A.T) * 0.5
        up = np.ascontiguousarray(A[np.triu_indices(6)])
        x, mp = np.zeros(6), np.zeros(1)
        assert shim.ic_chol(up.ctypes.data, b.ctypes.data, x.ctypes.data, mp.ctypes.data) == 1
        xo, mpo = O.chol6_solve(up, b)
        assert np.array(xo).tobytes() == x.tobytes() and np.float64(mpo).tobytes() == mp.tobytes()
        ref, cond = np.linalg.solve(A, b), np.linalg.cond(A)
        err = np.abs(x - ref).max()
        assert err <= 64 * cond * EPS * np.abs(ref).max(), (k, err, cond)
        worst = max(worst, err / (cond * EPS * np.abs(ref).max()))
        Lref = np.linalg.cholesky(A)
        assert 0.0 < mp[0] <= 1.0 and abs(mp[0] - (np.diag(Lref) ** 2 / np.diag(A)).min()) <= 1e-6 * max(mp[0], 64 * cond * EPS)
    print("largest |x - solve| / (cond eps |x|):", worst)
    # an exactly zero pivot: the third row and column are zeros (points on one axis-aligned face: no rotation about its normal seen)
    A = np.diag([4.0, 9.0, 0.0, 1.0, 1.0, 16.0])
    A[0, 1] = A[1, 0] = 1.0
    up, b, x, mp = np.ascontiguousarray(A[np.triu_indices(6)]), np.ones(6), np.zeros(6), np.zeros(1)
    assert shim.ic_chol(up.ctypes.data, b.ctypes.data, x.ctypes.data, mp.ctypes.data) == 0 and O.chol6_solve(up, b) is None
    for bad in (-1.0, np.nan, np.inf):
        A[2, 2] = bad
        up = np.ascontiguousarray(A[np.triu_indices(6)])
        assert shim.ic_chol(up.ctypes.data, b.ctypes.data, x.ctypes.data, mp.ctypes.data) == 0 and O.chol6_solve(up, b) is None
    # a pivot that cancels to zero exactly: rows 0 and 1 are the same
    A = np.identity(6)
    A[0, 1] = A[1, 0] = 1.0
    up = np.ascontiguousarray(A[np.triu_indices(6)])
    assert shim.ic_chol(up.ctypes.data, b.ctypes.data, x.ctypes.data, mp.ctypes.data) == 0 and O.chol6_solve(up, b) is None


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_the_summation_tree(shim, n):
    rng = np.random.default_rng(n)
    vals = np.ascontiguousarray(rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, size=n))
    out = np.zeros(1)
    shim.ic_tree(vals.ctypes.data, n, out.ctypes.data)
    assert out.tobytes() == np.float64(O.tree_sum(vals)).tobytes()
    # the tree by hand: pairs at distance 128, 64, .., 1 within a block, the blocks left to right
    tot = 0.0
    for b0 in range(0, n, 256):
        s = list(vals[b0:b0 + 256]) + [0.0] * (256 - len(vals[b0:b0 + 256]))
        h = 128
        while h:
            s = [s[i] + s[i + h] for i in range(h)]
            h //= 2
        tot = tot + s[0]
    assert np.float64(tot).tobytes() == out.tobytes()
    assert O.tree_sum(np.array([-0.0])) == 0.0 and not np.signbit(O.tree_sum(np.array([-0.0])))      # the sum starts at +0.0


def host_evaluate(shim, v, f, pts, T, cbar, metric, reject):
    v, f, pts = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(pts, np.float64)
    Tst = np.concatenate([np.asarray(T, np.float64).reshape(16), np.asarray(cbar, np.float64), [0.0]])
    rows = np.zeros(((len(pts) + 255) // 256, 32))
    shim.ic_evaluate(v.ctypes.data, f.ctypes.data, len(f), pts.ctypes.data, len(pts), Tst.ctypes.data, metric, float(reject), rows.ctypes.data)
    return rows


def host_register(shim, v, f, pts, T0, metric, max_iter, reject=np.inf, tol=0.0):
    v, f, pts = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(pts, np.float64)
    opt = _lib.IcpOptions(metric, max_iter, reject, tol)
    rec, hist = np.zeros(1, dtype=_lib.REGISTRATION_DTYPE), np.zeros((max_iter + 1, 2))
    T0 = None if T0 is None else np.ascontiguousarray(T0, np.float64)
    rc = shim.ic_register(v.ctypes.data, f.ctypes.data, len(f), pts.ctypes.data, len(pts), ptr(T0), ctypes.addressof(opt), rec.ctypes.data, hist.ctypes.data)
    assert rc == rec[0]["status"]
    return rec[0], hist


@pytest.mark.parametrize("metric", [O.POINT, O.PLANE])
@pytest.mark.parametrize("Q", [6, 257, 513])
def test_one_evaluation_twin_against_the_oracle_sums_as_bytes(shim, metric, Q):
    v, f = O.box()
    pts = O.apply(O.BOX_MOVE, O.box_points(Q, seed=Q))
    cbar = O.tree_sum(np.concatenate([np.ones((Q, 1)), pts], axis=1))[1:] / float(Q)
    for T, reject in ((np.identity(4), np.inf), (O.rigid((3.0, -1.0, 2.0), 1.0, (0.1, 0.2, -0.1)), 0.5)):
        rows = host_evaluate(shim, v, f, pts, T, cbar, metric, reject)
        terms, near, pm = O.evaluate(v, f, pts, T.reshape(16), metric, reject, cbar)
        assert rows.tobytes() == O.block_rows(terms).tobytes()
        assert 0 < rows[:, 0].sum() <= Q and (reject == np.inf) == (rows[:, 0].sum() == Q)
    # the centroid pass
    rows = host_evaluate(shim, v, f, pts, np.identity(4), np.zeros(3), -1, 0.0)
    t = np.zeros((Q, 32))
    t[:, 0], t[:, 2:5] = 1.0, pts
    assert rows.tobytes() == O.block_rows(t).tobytes()


@pytest.mark.parametrize("metric,max_iter", [(O.POINT, 12), (O.PLANE, 8)])
def test_whole_loop_twin_against_the_oracle_on_the_scalene_box(shim, metric, max_iter):
    v, f = O.box()
    truth = O.box_points(257, seed=2)
    pts = O.apply(O.BOX_MOVE, truth)
    for T0, reject, tol in ((None, np.inf, 0.0), (O.rigid((0.0, 0.0, 1.0), 1.0, (0.1, 0.0, 0.0)), 2.0, 1e-6)):
        rec, hist = host_register(shim, v, f, pts, T0, metric, max_iter, reject, tol)
        o = O.register(v, f, pts, T0, metric, max_iter, reject, tol)
        assert rec.tobytes() == O.record(o).tobytes() and hist.tobytes() == o["history"].tobytes(), (rec, o["history"])
        assert rec["status"] == 0 and rec["rms"] <= rec["rms_first"]
    rec, hist = host_register(shim, v, f, pts, None, metric, max_iter)
    err = np.abs(O.apply(np.array(rec["T"]), pts) - truth).max()
    print("metric", metric, "rms history", hist[:, 0], "max |T p - truth|", err)
    if metric == O.PLANE:
        assert err < 1e-9 and rec["iterations"] == max_iter and 0.0 < rec["min_pivot"] <= 1.0
    else:
        assert rec["min_pivot"] == 1.0
    # failures: one face (exactly singular under the plane metric), five points, every pair rejected
    flat = O.box_points(64, seed=5)
    flat[:, 2] = 10.5
    for case, (p, rej, T0) in dict(one_face=(flat, np.inf, O.rigid((0.0, 0.0, 1.0), 0.0, (0.5, 0.25, 0.0))), five=(pts[:5], np.inf, None), rejected=(pts, 1e-30, None)).items():
        rec, hist = host_register(shim, v, f, p, T0, metric, 4, rej)
        o = O.register(v, f, p, T0, metric, 4, rej)
        assert rec.tobytes() == O.record(o).tobytes() and hist.tobytes() == o["history"].tobytes(), case
        if case == "one_face" and metric == O.POINT:
            assert rec["status"] == 0                 # Horn's form has no trouble with a plane
            continue
        assert rec["status"] == O.GEOMETRY and rec["iterations"] == 0 and not hist[1:].any(), case
        assert np.array_equal(rec["T"], np.identity(4) if T0 is None else T0)
        assert rec["pairs"] == (0 if case == "rejected" else len(p))


def test_the_buffer_plan(shim):
    for B, Q, per, maxF, K in ((1, 1, 0, 12, 1), (64, 4096, 1, 32440, 8), (5, 513, 0, 2049, 64)):
        out = (ctypes.c_size_t * 11)()
        shim.ic_plan(B, Q, per, maxF, K, out)
        chunks, S = out[0], out[1]
        tiles = max(1, -(-maxF // 256))
        assert chunks == -(-Q // 256) and S == max(1, min(tiles, -(-1024 // (B * chunks))))
        n = B * Q
        assert list(out[2:]) == [(n if per else Q) * 24, n * 24, n * S * 16, n * 48, B * chunks * 32 * 8, B * 20 * 8, B * (K + 1) * 16, B * 4, B * 168]


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/icp_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "icp_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
