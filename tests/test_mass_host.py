"""Mass properties of the resident batch (include/shoulder_hip.h sh_mass_properties), the parts that need no GPU (the record layout:
test_abi_exports.py): the argument check, sym3_jacobi against numpy.linalg.eigh, the host twin of the kernels (the device
source, host-compiled with -ffp-contract=off through tests/hostcheck/mass_check.cpp) against the NumPy statement of
tests/mass_oracle.py, and the closed forms of a box.

Bounds.  Twin against the oracle: bytes (the same + - x / sqrt in the same order).  sym3_jacobi against eigh: 64 eps ||A||_F, as for
sym4_jacobi in test_icp_host.py.  The box: derived in test_box_closed_forms."""
import os
import subprocess

import numpy as np
import pytest

import icp_oracle as IO
import mass_oracle as O
from conftest import BONES
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("mass_check"))


@pytest.fixture(scope="module")
def humerus():
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def host_mass(shim, v, f):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    rec, rows = np.zeros(1, dtype=_lib.MASS_DTYPE), np.zeros((max(1, (len(f) + 255) // 256), 24))
    shim.mc_mass(v.ctypes.data, len(v), f.ctypes.data, len(f), rec.ctypes.data, rows.ctypes.data)
    return rec[0], rows[:(len(f) + 255) // 256]


def test_entry_point_checks_its_arguments_without_a_gpu(shim):
    assert "sh_mass_properties" in _lib.EXPORTS and "sh_register_multistart" in _lib.EXPORTS
    L = _lib.load()
    assert L.sh_mass_properties(None, None) == IO.ARG                                 # (no context)
    assert shim.mc_precheck_mass(1, 1, 0) == 0 and shim.mc_precheck_mass(0, 1, 0) == IO.ARG
    assert shim.mc_precheck_mass(1, 0, 0) == IO.STATE and shim.mc_precheck_mass(1, 2, 1) == IO.STATE


def test_sym3_jacobi_against_eigh(shim):
    rng = np.random.default_rng(31)
    worst = 0.0
    for k in range(300):
        if k < 200:
            A = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-6, 7)
            A = A + A.T
        elif k < 260:
            Qm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            A = (Qm * np.array([2.0, 2.0, rng.uniform(-1.0, 1.0)])) @ Qm.T
            A = (A + A.T) * 0.5
        else:
            A = np.diag(rng.integers(-3, 4, 3).astype(np.float64))
        D, V = np.ascontiguousarray(A.copy()), np.zeros((3, 3))
        shim.mc_jacobi(D.ctypes.data, V.ctypes.data)
        Ao, Vo = O.sym3_jacobi([list(map(float, r)) for r in A])
        assert np.array(Ao).tobytes() == D.tobytes() and np.array(Vo).tobytes() == V.tobytes()      # the twin is the oracle
        w, norm, lam = np.linalg.eigh(A)[0], np.linalg.norm(A), np.diag(D)
        assert np.abs(np.sort(lam) - w).max() <= 64 * EPS * norm
        worst = max(worst, np.abs(np.sort(lam) - w).max() / (EPS * norm) if norm else 0.0)
        assert np.abs(V.T @ V - np.identity(3)).max() <= 64 * EPS and np.abs(A @ V - V * lam).max() <= 64 * EPS * max(norm, 1e-300)
    print("largest |lambda - eigh| / (eps ||A||):", worst)
    # a diagonal matrix is left alone; ties go to the first, ascending and descending
    for diag, asc, desc in (((2.0, 2.0, 1.0), [2, 0, 1], [0, 1, 2]), ((1.0, 3.0, 3.0), [0, 1, 2], [1, 2, 0]), ((0.0, 0.0, 0.0), [0, 1, 2], [0, 1, 2])):
        up = [diag[0], 0.0, 0.0, diag[1], 0.0, diag[2]]
        for descending, want in ((False, asc), (True, desc)):
            eig, axes = O.frame(up, descending)
            assert eig == [diag[i] for i in want]
            assert [int(np.argmax(np.abs(a))) for a in axes[:2]] == want[:2] and all(max(a) == 1.0 for a in axes[:2])
            assert np.array_equal(np.array(axes[2]), np.cross(axes[0], axes[1]))


def test_host_twin_gives_the_oracle_bytes(shim, humerus):
    v, f = humerus
    bv, bf = O.int_box()
    for tag, vv, ff in (("box", bv, bf), ("humerus_left", v, f), ("257 faces", v, f[:257]), ("513 faces", v, f[:513]), ("one face", v, f[:1]),
                        ("zero area", v, np.array([[0, 1, 1]], np.int32)), ("no faces", v, f[:0])):
        rec, rows = host_mass(shim, vv, ff)
        want, want_rows = O.mass(vv, ff)
        assert rows.tobytes() == want_rows.tobytes(), tag
        assert rec.tobytes() == want.tobytes(), (tag, rec, want)
    rec, _ = host_mass(shim, v, f)
    print("humerus_left:", {k: rec[k] for k in ("area", "volume", "closure", "shell_eig", "principal", "degenerate")})
    assert rec["status"] == 0 and rec["vstatus"] == 0 and rec["closure"] <= 1e-12 and rec["volume"] > 0.0
    assert host_mass(shim, v, f[:2049])[0]["closure"] > 1e-3
    one, flat, none = host_mass(shim, v, f[:1])[0], host_mass(shim, v, np.array([[0, 1, 1]], np.int32))[0], host_mass(shim, v, f[:0])[0]
    assert one["status"] == 0 and one["vstatus"] == O.GEOMETRY and one["volume"] == 0.0 and not one["inertia"].any()
    assert flat["status"] == O.GEOMETRY and flat["degenerate"] == 1 and none["status"] == O.GEOMETRY and none["faces"] == 0


def test_against_plain_numpy_sums(humerus):
    """the record against the textbook integrals summed by ndarray.sum about the mesh's own centroid: another pivot and another order.
    The sums run over F = 32 440 faces of terms up to (300 mm)^5, so the two agree to a small multiple of F eps relative to the sum of
    magnitudes; 1e-9 relative to the largest entry is asserted, three orders above F eps and five below any error of method."""
    v, f = humerus
    rec, _ = O.mass(v, f)
    p = v.astype(np.float64)
    tri = p[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * np.linalg.norm(n, axis=1)
    assert abs(rec["area"] - area.sum()) <= 1e-9 * area.sum()
    c0 = p.mean(axis=0)
    q = tri - c0
    d = np.einsum("ij,ij->i", q[:, 0], np.cross(q[:, 1], q[:, 2]))
    vol = d.sum() / 6.0
    com = (d[:, None] * q.sum(axis=1)).sum(axis=0) / (24.0 * vol) + c0
    assert abs(rec["volume"] - vol) <= 1e-9 * abs(vol) and np.abs(rec["center_mass"] - com).max() <= 1e-9 * np.abs(p).max()
    q = tri - com
    s = q.sum(axis=1)
    P = (d[:, None, None] * (s[:, :, None] * s[:, None, :] + np.einsum("fki,fkj->fij", q, q))).sum(axis=0) / 120.0
    I = np.trace(P) * np.identity(3) - P
    assert np.abs(rec["inertia"] - I).max() <= 1e-9 * np.abs(I).max()
    w = np.linalg.eigh(I)[0]
    assert np.abs(rec["principal"] - w).max() <= 1e-9 * w.max()
    assert np.abs(rec["principal_axes"] @ rec["principal_axes"].T - np.identity(3)).max() <= 1e-12 and np.linalg.det(rec["principal_axes"]) > 0
    assert np.abs(rec["shell_axes"] @ rec["shell_axes"].T - np.identity(3)).max() <= 1e-12 and np.linalg.det(rec["shell_axes"]) > 0
    assert rec["shell_eig"][0] > 50 * rec["shell_eig"][1] > 0                        # the long axis is sharp, the transverse ones are not


def test_box_closed_forms(shim):
    """The 30 x 20 x 10 box at integer CT coordinates.  The pivot is a corner, so a, b, c have components in {0, 10, 20, 30}; every face is
    axis-aligned, so n has one non-zero component, an integer, and A2 = |that| exactly.  Every term is then a product and sum of integers
    far below 2^53: the 24 totals are exact.  area = T0 / 2, volume = T13 / 6 = 6000 and P_ij = T / 120 divide an exact integer by
    an integer with a representable quotient, and a correctly rounded division of such a pair is exact; cm' = (15, 10, 5) likewise;
    S_ij and I are sums of integers.  So every figure asserted below carries no rounding at all, and the 4 ulp the issue allows (one
    half ulp each for the division, the product volume cm'_i cm'_j, the difference and the sum of I, rounded up) is not used."""
    v, f = O.int_box()
    rec, rows = host_mass(shim, v, f)
    assert rec.tobytes() == O.mass(v, f)[0].tobytes()
    assert rec["status"] == 0 and rec["vstatus"] == 0 and rec["faces"] == 12 and rec["degenerate"] == 0
    assert rec["area"] == 2200.0 and rec["volume"] == 6000.0 and rec["closure"] == 0.0
    m, (a, b, c) = 6000.0, (30.0, 20.0, 10.0)
    want_c = np.array([120.0 + 15.0, -85.0 + 10.0, 410.0 + 5.0])
    want_I = np.diag([m / 12.0 * (b * b + c * c), m / 12.0 * (a * a + c * c), m / 12.0 * (a * a + b * b)])
    ulp = lambda x: np.spacing(np.abs(x))
    for got, want in ((rec["center_mass"], want_c), (rec["shell_centroid"], want_c), (np.diag(rec["inertia"]), np.diag(want_I)), (rec["principal"], np.diag(want_I))):
        err = np.abs(got - want) / ulp(want)
        print("box: error in ulp", err)
        assert np.all(err <= 4.0)
    assert not (rec["inertia"] - np.diag(np.diag(rec["inertia"]))).any()
    assert np.array_equal(rec["principal_axes"], np.identity(3)) and np.array_equal(rec["shell_axes"], np.identity(3))
    # turned inside out: the volume and the inertia change sign, the shell does not
    flipped, _ = host_mass(shim, v, f[:, [0, 2, 1]])
    assert flipped["volume"] == -6000.0 and flipped["area"] == 2200.0 and np.array_equal(flipped["center_mass"], rec["center_mass"])


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/mass_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mass_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
