"""Multi-start registration (include/shoulder_hip.h sh_register_multistart), the parts that need no GPU, through the shim
tests/hostcheck/mass_check.cpp: the ordered argument checks of sh_query.h, the pick rule that k_ms_pick folds the candidates under,
the subsample rule and the buffer plan; and Engine.principal_starts' arithmetic, which is plain NumPy."""
import ctypes

import numpy as np
import pytest

import icp_oracle as IO
import mass_oracle as O
from shoulder_amd import _lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("ms_check"))


def ptr(a):
    return a.ctypes.data if a is not None else None


def test_entry_point_checks_its_arguments_in_order_without_a_gpu(shim):
    L = _lib.load()
    pts, good = np.zeros((8, 3)), _lib.IcpOptions(_lib.ICP_PLANE, 4, np.inf, 0.0)
    I = np.stack([np.identity(4)] * 6).reshape(2, 3, 4, 4)                            # B = 2, K = 3
    assert L.sh_register_multistart(None, ptr(pts), 8, 0, ptr(I), 3, ctypes.byref(good), 0, 6, ctypes.byref(good), None, None, None) == IO.ARG
    text = ctypes.create_string_buffer(256)

    def pre(p=pts, Q=8, per=0, T0s=I, K=3, coarse=good, cp=0, mp=6, fine=good, B=2, pend=0, ctx=1):
        adr = lambda o: ctypes.addressof(o) if o is not None else None
        return shim.mc_precheck_ms(ctx, ptr(p), Q, per, ptr(T0s), K, adr(coarse), cp, mp, adr(fine), B, pend, ctypes.addressof(text), 256)
    assert pre() == 0 and pre(Q=1) == 0 and pre(cp=4) == 0 and pre(cp=10 ** 6) == 0 and pre(K=1) == 0
    # 1 the context and the pointers
    for kw in (dict(ctx=0), dict(p=None), dict(T0s=None), dict(coarse=None), dict(fine=None)):
        assert pre(**kw) == IO.ARG
    # 2 Q; 3 K, coarse_points, min_pairs
    assert pre(Q=0) == IO.ARG and pre(Q=_lib.CLOSEST_MAX + 1) == IO.ARG
    for kw in (dict(K=0), dict(K=65), dict(cp=-1), dict(mp=5), dict(mp=0)):
        assert pre(**kw) == IO.ARG and pre(B=0, **kw) == IO.ARG                       # (before the state)
    assert pre(K=64, T0s=np.stack([np.identity(4)] * 128)) == 0
    # 4 the options, coarse before fine
    bad = _lib.IcpOptions(2, 4, np.inf, 0.0)
    assert pre(coarse=bad) == IO.ARG and b"coarse" in text.value
    assert pre(fine=bad) == IO.ARG and b"fine" in text.value
    assert pre(coarse=bad, fine=bad, B=0) == IO.ARG and b"coarse" in text.value
    # 5 the state
    assert pre(B=0) == IO.STATE and pre(pend=1) == IO.STATE
    # 6 the coordinates, 7 the starts: the refusal names the humerus and the start
    p = pts.copy()
    p[5, 1] = np.nan
    assert pre(p=p) == IO.ARG and b"point 5" in text.value and pre(p=p, B=0) == IO.STATE
    for b, k in ((0, 0), (0, 2), (1, 1)):
        T = I.copy()
        T[b, k, 0, 1] = 1e-6                                                          # a shear of 1e-6
        assert pre(T0s=T) == IO.ARG and ("start %d of humerus %d" % (k, b)).encode() in text.value, text.value
        assert pre(T0s=T, p=p) == IO.ARG and b"point 5" in text.value                 # the coordinates come first
    T = I.copy()
    T[1, 2, 1, 1] = -1.0                                                              # a reflection
    assert pre(T0s=T) == IO.ARG and b"start 2 of humerus 1" in text.value and pre(T0s=T, B=1) == 0
    T[0, 1, 2, 2], T[0, 2, 3, 3] = np.nan, 2.0
    assert pre(T0s=T) == IO.ARG and b"start 1 of humerus 0" in text.value             # the first one in (b, k) order


def records(rms, pairs=None, status=None):
    r = np.zeros(len(rms), dtype=_lib.REGISTRATION_DTYPE)
    r["rms"], r["pairs"], r["status"] = rms, (10 if pairs is None else pairs), (0 if status is None else status)
    return r


def test_the_pick_rule(shim):
    pick = lambda r, mp: shim.mc_pick(r.ctypes.data, len(r), mp)
    # order by (rms, k): the smallest rms, among equals the first
    assert pick(records([3.0, 1.0, 2.0, 1.0]), 6) == 1 and pick(records([1.0, 1.0, 1.0]), 6) == 0 and pick(records([2.0, 1.5, 1.0]), 6) == 2
    assert pick(records([0.0, -0.0]), 6) == 0
    # a status or too few pairs exclude a start, whatever its rms
    assert pick(records([0.1, 1.0, 2.0], status=[IO.GEOMETRY, 0, 0]), 6) == 1
    assert pick(records([0.1, 1.0, 2.0], pairs=[5, 6, 600]), 6) == 1 and pick(records([0.1, 1.0, 2.0], pairs=[5, 6, 600]), 7) == 2
    assert pick(records([np.nan, 5.0]), 6) == 1 and pick(records([5.0, np.nan]), 6) == 0
    # no winner
    assert pick(records([1.0, 2.0], pairs=[9, 9]), 10) == -1 and pick(records([1.0], status=[IO.GEOMETRY]), 6) == -1 and pick(records([np.nan]), 6) == -1
    # the fold is the oracle's pick on random records
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 65))
        r = records(rng.integers(0, 6, n).astype(np.float64) * 0.25, rng.integers(0, 20, n), np.where(rng.random(n) < 0.2, IO.GEOMETRY, 0))
        mp = int(rng.integers(6, 20))
        want = O.pick(r, mp)
        ok = [k for k in range(n) if r[k]["status"] == 0 and r[k]["pairs"] >= mp]
        assert pick(r, mp) == want == (min(ok, key=lambda k: (r[k]["rms"], k)) if ok else -1)


def test_the_subsample_rule_and_the_plan(shim):
    for Q, cp in ((513, 256), (96, 512), (4096, 512), (7, 0), (1000, 999), (2 ** 20, 2 ** 20 - 1)):
        Qc = Q if cp == 0 or cp > Q else cp
        js = range(Qc) if Qc < 5000 else (0, 1, Qc // 2, Qc - 2, Qc - 1)
        idx = [shim.mc_coarse_index(j, Q, Qc) for j in js]
        assert idx == [j * Q // Qc for j in js] and idx[0] == 0 and idx[-1] < Q and all(x < y for x, y in zip(idx, idx[1:]))
    pts = np.arange(513 * 3, dtype=np.float64).reshape(513, 3)
    assert np.array_equal(O.coarse_set(pts, 256), pts[[j * 513 // 256 for j in range(256)]]) and len(O.coarse_set(pts, 0)) == 513 == len(O.coarse_set(pts, 600))
    for B, Q, per, maxF, K, cp, ci, fi in ((1, 96, 0, 12, 1, 0, 1, 1), (64, 4096, 1, 32440, 16, 512, 4, 20), (5, 513, 0, 2049, 64, 256, 64, 8)):
        out = (ctypes.c_size_t * 18)()
        shim.mc_plan(B, Q, per, maxF, K, cp, ci, fi, out)
        Qc = Q if cp == 0 or cp > Q else cp
        tiles = max(1, -(-maxF // 256))
        assert out[0] == Qc and out[1] == tiles and list(out[2:4]) == [B * tiles * 24 * 8, B * 400]

        def icp(q, it):
            chunks = -(-q // 256)
            S = max(1, min(tiles, -(-1024 // (B * chunks))))
            n = B * q
            return [(n if per else q) * 24, n * 24, n * S * 16, n * 48, B * chunks * 32 * 8, B * 20 * 8, B * (it + 1) * 16, B * 4, B * 168]
        assert list(out[4:13]) == [max(a, b) for a, b in zip(icp(Qc, ci), icp(Q, fi))]
        assert list(out[13:18]) == [B * K * 128, (B * Qc if per else Qc) * 24, B * K * 168, B * 8, B * 4]


def test_principal_starts_arithmetic():
    """Engine.principal_starts' matrices from given frames: proper rotations that map the points' frame onto the mesh's, two directions
    of the long axis times `rolls` turns about it"""
    from shoulder_amd.engine import principal_start_matrices
    rng = np.random.default_rng(2)
    Xm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    Xm[:, 2] = np.cross(Xm[:, 0], Xm[:, 1])
    pts = rng.normal(size=(200, 3)) * (40.0, 6.0, 3.0) + (10.0, -20.0, 30.0)
    cm = np.array([1.0, 2.0, 3.0])
    T, ratio = principal_start_matrices(cm, Xm.T, pts, rolls=4)
    assert T.shape == (8, 4, 4) and ratio > 10.0
    cp = pts.mean(axis=0)
    w, V = np.linalg.eigh(np.cov((pts - cp).T, bias=True))
    long_p = V[:, 2]
    for k in range(8):
        R, t = T[k, :3, :3], T[k, :3, 3]
        assert np.abs(R.T @ R - np.identity(3)).max() <= 1e-12 and np.linalg.det(R) > 0 and np.array_equal(T[k, 3], (0.0, 0.0, 0.0, 1.0))
        assert np.abs(R @ cp + t - cm).max() <= 1e-9
        along = float((R @ long_p) @ Xm[:, 0])
        assert abs(abs(along) - 1.0) <= 1e-9
    assert np.sign((T[0, :3, :3] @ long_p) @ Xm[:, 0]) == -np.sign((T[4, :3, :3] @ long_p) @ Xm[:, 0])
    rolls = [np.degrees(np.arccos(np.clip((np.trace(T[0, :3, :3].T @ T[k, :3, :3]) - 1.0) / 2.0, -1.0, 1.0))) for k in range(4)]
    assert np.allclose(rolls, [0.0, 90.0, 180.0, 90.0], atol=1e-6)
