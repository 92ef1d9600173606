"""NumPy statement of sh_mass_properties (include/shoulder_hip.h "mass properties of the resident batch"): the 24 terms of every face,
the tree of 256-face blocks (icp_oracle.tree_sum), mass_finish and sym3_jacobi, on float64 and written operation by operation in the
order of sh_scalar.h (mass_face_terms, sym3_jacobi, mass_frame, mass_finish), so that it gives the bytes the host-compiled statement
gives (tests/hostcheck/mass_check.cpp, -ffp-contract=off) and the device can give: the chain is + - x / sqrt, all correctly rounded.
The per-face terms are NumPy element-wise expressions, the finish plain Python floats.  Also the composition of
sh_register_multistart from icp_oracle.register, and the ctypes side of the host twins."""
import ctypes
import math

import numpy as np

import host_twin
import icp_oracle as IO
from ray_oracle import cross3, dot3, widen

GEOMETRY = -5
BLOCK, TERMS, SWEEPS, FMAX = 256, 24, 12, 1.7976931348623157e308
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def face_terms(verts, faces):
    """(F, 24) terms of the faces (mass_face_terms), and the pivot o: vertex 0 of the vertex array, widened"""
    v, faces = widen(verts), np.asarray(faces).reshape(-1, 3)
    o = v[0] if len(v) else np.zeros(3)
    A, B, C = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    a, b, c = A - o, B - o, C - o
    n = cross3(B - A, C - A)
    A2 = np.sqrt(dot3(n, n))
    s = (a + b) + c
    d = dot3(a, cross3(b, c))
    t = np.zeros((len(faces), TERMS))
    t[:, 0], t[:, 13] = A2, d
    for k in range(3):
        t[:, 1 + k], t[:, 10 + k], t[:, 14 + k] = A2 * s[:, k], n[:, k], d * s[:, k]
    for q, (i, j) in enumerate(PAIRS):
        m = ((s[:, i] * s[:, j] + a[:, i] * a[:, j]) + b[:, i] * b[:, j]) + c[:, i] * c[:, j]
        t[:, 4 + q], t[:, 17 + q] = A2 * m, d * m
    t[:, 23] = np.where(A2 == 0.0, 1.0, 0.0)
    return t, o


def block_rows(terms):
    """the rows of "mass.part": one tree sum per block of 256 faces"""
    return np.stack([IO.tree_sum(terms[b0:b0 + BLOCK]) for b0 in range(0, len(terms), BLOCK)]) if len(terms) else np.zeros((0, TERMS))


def finite(x):
    return abs(x) <= FMAX


def sym3_jacobi(A):
    """A: 3 x 3 nested lists of floats, destroyed -> (A, V)"""
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        for p in range(2):
            for q in range(p + 1, 3):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = A[q][p] = 0.0
                for k in range(3):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return A, V


def frame(up, descending):
    """mass_frame -> (eig [3], axes 3 x 3 rows) or None"""
    A = [[up[0], up[1], up[2]], [up[1], up[3], up[4]], [up[2], up[4], up[5]]]
    if not all(finite(x) for r in A for x in r):
        return None
    A, V = sym3_jacobi(A)
    order = [0, 1, 2]
    for i in range(1, 3):
        j = i
        while j > 0:
            x, y = A[order[j]][order[j]], A[order[j - 1]][order[j - 1]]
            if not (x > y if descending else x < y):
                break
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    eig = [A[r][r] for r in order]
    axes = [[V[k][r] for k in range(3)] for r in order]
    for r in range(2):
        big = 0
        for k in range(1, 3):
            if abs(axes[r][k]) > abs(axes[r][big]):
                big = k
        if axes[r][big] < 0.0:
            axes[r] = [-x for x in axes[r]]
    a, b = axes[0], axes[1]
    axes[2] = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    if not all(finite(x) for x in eig) or not all(finite(x) for r in axes for x in r):
        return None
    return eig, axes


def finish(T, o, nf):
    """mass_finish -> one _lib.MASS_DTYPE record"""
    from shoulder_amd import _lib
    T, o = [float(x) for x in T], [float(x) for x in o]
    r = np.zeros((), dtype=_lib.MASS_DTYPE)
    r["faces"], r["degenerate"] = nf, int(T[23])
    T0, T13 = T[0], T[13]
    ok = nf > 0 and T0 != 0.0
    with np.errstate(all="ignore"):
        if ok:
            area = T0 / 2.0
            cs = [np.float64(T[1 + k]) / np.float64(3.0 * T0) for k in range(3)]
            C = [float(np.float64(T[4 + q]) / np.float64(12.0 * T0) - cs[i] * cs[j]) for q, (i, j) in enumerate(PAIRS)]
            N = T[10:13]
            closure = math.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]) / T0
            fr = frame(C, True) if finite(area) and finite(closure) else None
            ok = fr is not None and all(finite(float(cs[k]) + o[k]) for k in range(3))
            if ok:
                r["area"], r["closure"], r["shell_cov"], r["shell_eig"], r["shell_axes"] = area, closure, C, fr[0], fr[1]
                r["shell_centroid"] = [float(cs[k]) + o[k] for k in range(3)]
        vok = nf > 0 and T13 != 0.0
        if vok:
            volume = T13 / 6.0
            cm = [float(np.float64(T[14 + k]) / np.float64(4.0 * T13)) for k in range(3)]
            S = [float(np.float64(T[17 + q]) / 120.0 - np.float64(volume * cm[i]) * cm[j]) for q, (i, j) in enumerate(PAIRS)]
            I = [S[3] + S[5], -S[1], -S[2], S[0] + S[5], -S[4], S[0] + S[3]]
            fr = frame(I, False) if finite(volume) else None
            vok = fr is not None and all(finite(cm[k] + o[k]) for k in range(3))
            if vok:
                r["volume"], r["principal"], r["principal_axes"] = volume, fr[0], fr[1]
                r["center_mass"] = [cm[k] + o[k] for k in range(3)]
                r["inertia"] = [[I[0], I[1], I[2]], [I[1], I[3], I[4]], [I[2], I[4], I[5]]]
    r["status"], r["vstatus"] = (0 if ok else GEOMETRY), (0 if vok else GEOMETRY)
    return r


def mass(verts, faces):
    """-> (record, block rows) of one mesh"""
    terms, o = face_terms(verts, faces)
    T = IO.tree_sum(terms) if len(terms) else np.zeros(TERMS)
    return finish(T, o, len(terms)), block_rows(terms)


def int_box(shift=(120, -85, 410)):
    """icp_oracle.box() shifted to integer CT coordinates"""
    v, f = IO.box()
    return (v + np.asarray(shift, np.float32)).astype(np.float32), f


# ---- sh_register_multistart composed from icp_oracle.register ---------------------------------------------------------------------
def coarse_set(points, coarse_points):
    points = np.asarray(points, np.float64).reshape(-1, 3)
    Q = len(points)
    Qc = Q if coarse_points == 0 or coarse_points > Q else coarse_points
    return points[[j * Q // Qc for j in range(Qc)]]


def pick(records, min_pairs):
    """the winner among candidate records in ascending k: the smallest (rms, k) with status 0 and pairs >= min_pairs, or -1"""
    best = -1
    for k, r in enumerate(records):
        if r["status"] != 0 or r["pairs"] < min_pairs or r["rms"] != r["rms"]:
            continue
        if best < 0 or r["rms"] < records[best]["rms"]:
            best = k
    return best


def multistart(verts, faces, points, T0s, coarse, coarse_points, min_pairs, fine, closest=None):
    """one humerus -> (out record, coarse records [K], winner, the fine oracle dict or None); coarse / fine: dict(metric, max_iter, reject, tol)"""
    from shoulder_amd import _lib
    cs = coarse_set(points, coarse_points)
    cand = [IO.record(IO.register(verts, faces, cs, T0, closest=closest, **coarse)) for T0 in T0s]
    w = pick(cand, min_pairs)
    if w < 0:
        out = np.zeros((), dtype=_lib.REGISTRATION_DTYPE)
        out["T"], out["status"] = np.asarray(T0s[0]).reshape(4, 4), GEOMETRY
        return out, np.array(cand), w, None
    o = IO.register(verts, faces, points, cand[w]["T"], closest=closest, **fine)
    return IO.record(o), np.array(cand), w, o


# ---- the ctypes side of the host twins (tests/hostcheck/mass_check.cpp) ----------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("mass", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.mc_mass.argtypes, L.mc_mass.restype = [vp, i, vp, i, vp, vp], None
    L.mc_jacobi.argtypes, L.mc_jacobi.restype = [vp, vp], None
    L.mc_precheck_mass.argtypes = [i, i, i]
    L.mc_precheck_ms.argtypes = [i, vp, i, i, vp, i, vp, i, i, vp, i, i, vp, i]
    L.mc_pick.argtypes = [vp, i, i]
    L.mc_plan.argtypes, L.mc_plan.restype = [i, i, i, ctypes.c_longlong, i, i, i, i, vp], None
    L.mc_coarse_index.argtypes, L.mc_coarse_index.restype = [i, i, i], ctypes.c_longlong
    return L
