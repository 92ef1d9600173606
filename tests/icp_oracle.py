"""NumPy statement of sh_register_points (include/shoulder_hip.h "rigid registration of point sets onto the resident batch"): the loop of
move, pair (closest_oracle.closest: every face, no cull), sum (the tree of 256-point blocks), report, stop or solve, on float64 and
written operation by operation in the order of sh_scalar.h (icp_pair_terms, sym4_jacobi, icp_horn_solve, chol6_solve,
icp_plane_solve, icp_compose, icp_step), so that it gives the bytes the host-compiled statement gives
(tests/hostcheck/icp_check.cpp, -ffp-contract=off) and the device can give: the chain is + - x / sqrt, all correctly rounded.  The
per-point terms are NumPy element-wise expressions, the solves plain Python floats.  tree=False replaces the defined tree by
ndarray.sum: a second run of the same oracle that differs only in summation order, the yardstick of the tests' bound."""
import ctypes
import math

import numpy as np

import closest_oracle as CO
import host_twin
from ray_oracle import cross3, dot3, widen

ARG, STATE, GEOMETRY = -1, -3, -5
POINT, PLANE, BLOCK, TERMS, SWEEPS = 0, 1, 256, 32, 12
FMAX = 1.7976931348623157e308


def map_points(T, p):
    """canal_map_point on (n, 3): row r is ((T[4r] x + T[4r+1] y) + T[4r+2] z) + T[4r+3]"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=-1)


def tree_sum(vals, tree=True):
    """(n, K) -> (K,): blocks of 256 rows, slot[i] += slot[i + h] for h = 128 .. 1, the block sums added in block order from 0.0"""
    vals = np.asarray(vals, np.float64)
    if vals.ndim == 1:
        return tree_sum(vals[:, None], tree)[0]
    if not tree:
        return vals.sum(axis=0)
    tot = np.zeros(vals.shape[1])
    for b0 in range(0, len(vals), BLOCK):
        slot = np.zeros((BLOCK, vals.shape[1]))
        slot[:len(vals[b0:b0 + BLOCK])] = vals[b0:b0 + BLOCK]
        h = BLOCK // 2
        while h >= 1:
            slot[:h] = slot[:h] + slot[h:2 * h]
            h //= 2
        tot = tot + slot[0]
    return tot


def block_rows(vals):
    """the rows of "icp.part": one tree sum per block"""
    return np.stack([tree_sum(vals[b0:b0 + BLOCK]) for b0 in range(0, len(vals), BLOCK)])


def pair_terms(metric, pm, near, ab, ac, c, reject):
    """(Q, 32) terms of the pairs (icp_pair_terms); ab, ac: the winning faces' edges (Q, 3), rows of zeros where there is none"""
    q = np.array(near["point"], np.float64)
    e = q - pm
    e2 = dot3(e, e)
    acc = (near["status"] == 0) & (np.sqrt(e2) <= reject)
    t = np.zeros((len(pm), TERMS))
    if metric == PLANE:
        nn = cross3(ab, ac)
        ln = np.sqrt(dot3(nn, nn))
        acc = acc & (ln > 0.0) & (ln <= FMAX)
        with np.errstate(divide="ignore", invalid="ignore"):
            n = nn / ln[:, None]
        d = pm - np.asarray(c)[None, :]
        J = np.concatenate([cross3(d, n), n], axis=1)
        r = dot3(e, n)
        idx = 2
        for i in range(6):
            for j in range(i, 6):
                t[:, idx] = J[:, i] * J[:, j]
                idx += 1
        for i in range(6):
            t[:, 23 + i] = J[:, i] * r
    else:
        t[:, 2:5], t[:, 5:8] = pm, q
        for i in range(3):
            for j in range(3):
                t[:, 8 + 3 * i + j] = pm[:, i] * q[:, j]
    t[:, 0], t[:, 1] = 1.0, e2
    t[~acc] = 0.0
    return t


def sym4_jacobi(A):
    """A: 4 x 4 nested lists of floats, destroyed -> (A, V)"""
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
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
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return A, V


def quat_rot(w, x, y, z):
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def pack(R, t):
    return [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0]


def finite(x):
    return abs(x) <= FMAX


def horn_matrix(tot):
    n = tot[0]
    pb = [tot[2 + i] / n for i in range(3)]
    qb = [tot[5 + i] / n for i in range(3)]
    S = [tot[8 + 3 * i + j] - tot[2 + i] * qb[j] for i in range(3) for j in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (S[0] + S[4]) + S[8]; N[0][1] = S[5] - S[7]; N[0][2] = S[6] - S[2]; N[0][3] = S[1] - S[3]
    N[1][1] = (S[0] - S[4]) - S[8]; N[1][2] = S[1] + S[3]; N[1][3] = S[6] + S[2]
    N[2][2] = (S[4] - S[0]) - S[8]; N[2][3] = S[5] + S[7]
    N[3][3] = (S[8] - S[0]) - S[4]
    for i in range(4):
        for j in range(i):
            N[i][j] = N[j][i]
    return N, pb, qb


def horn_solve(tot):
    tot = [float(x) for x in tot]
    with np.errstate(all="ignore"):
        N, pb, qb = horn_matrix(tot)
    if not all(finite(x) for row in N for x in row):
        return None
    N, V = sym4_jacobi(N)
    best = 0
    for i in range(1, 4):
        if N[i][i] > N[best][best]:
            best = i
    w, x, y, z = V[0][best], V[1][best], V[2][best], V[3][best]
    ln = math.sqrt(((w * w + x * x) + y * y) + z * z)
    if not (ln > 0.0) or not finite(ln):
        return None
    w, x, y, z = w / ln, x / ln, y / ln, z / ln
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    R = quat_rot(w, x, y, z)
    t = [qb[i] - ((R[3 * i] * pb[0] + R[3 * i + 1] * pb[1]) + R[3 * i + 2] * pb[2]) for i in range(3)]
    return pack(R, t)


def chol6_solve(up, b):
    """-> (x, min_pivot) or None"""
    up, b = [float(v) for v in up], [float(v) for v in b]
    A = [[0.0] * 6 for _ in range(6)]
    idx = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = up[idx]
            idx += 1
    L = [[0.0] * 6 for _ in range(6)]
    mp = 1.0
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0.0) or not finite(s):
            return None
        l = math.sqrt(s)
        L[j][j] = l
        ratio = (l * l) / A[j][j]
        if ratio < mp:
            mp = ratio
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / l
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x, mp


def plane_solve(tot, c):
    got = chol6_solve(tot[2:23], tot[23:29])
    if got is None:
        return None
    x, mp = got
    c = [float(v) for v in c]
    hx, hy, hz = 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]
    ln = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    if not finite(ln):
        return None
    R = quat_rot(1.0 / ln, hx / ln, hy / ln, hz / ln)
    t = [(c[i] - ((R[3 * i] * c[0] + R[3 * i + 1] * c[1]) + R[3 * i + 2] * c[2])) + x[3 + i] for i in range(3)]
    return pack(R, t), mp


def compose(D, T):
    Tn = [0.0] * 16
    for i in range(3):
        for j in range(4):
            Tn[4 * i + j] = (D[4 * i] * T[j] + D[4 * i + 1] * T[4 + j]) + D[4 * i + 2] * T[8 + j]
        Tn[4 * i + 3] = Tn[4 * i + 3] + D[4 * i + 3]
    Tn[15] = 1.0
    return Tn


def face_edges(verts, faces, near):
    """ab, ac (Q, 3) of the winning faces; zeros where a pair has none"""
    v, faces = widen(verts), np.asarray(faces)
    f = np.where(near["status"] == 0, near["face"], 0)
    A = v[faces[f, 0]]
    ab, ac = v[faces[f, 1]] - A, v[faces[f, 2]] - A
    ab[near["status"] != 0] = 0.0
    ac[near["status"] != 0] = 0.0
    return ab, ac


def evaluate(verts, faces, points, T, metric, reject, cbar, closest=None):
    """one evaluation at T -> (terms (Q, 32), near, moved)"""
    pm = map_points(T, np.asarray(points, np.float64))
    near = (closest or CO.closest)(verts, faces, pm)
    ab, ac = face_edges(verts, faces, near)
    c = map_points(T, np.asarray(cbar, np.float64)[None, :])[0]
    return pair_terms(metric, pm, near, ab, ac, c, reject), near, pm


def register(verts, faces, points, T0=None, metric=PLANE, max_iter=20, reject=np.inf, tol=0.0, tree=True, closest=None):
    """the loop for one humerus -> dict(T (4, 4), rms, rms_first, min_pivot, pairs, iterations, converged, status, history
    (max_iter + 1, 2), near, sums: the joined row of every evaluation made, Ts: the transform of every evaluation)"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    Q = len(points)
    T = [float(x) for x in (np.identity(4) if T0 is None else np.asarray(T0, np.float64)).reshape(16)]
    ones = np.concatenate([np.ones((Q, 1)), points], axis=1)
    cbar = tree_sum(ones, tree)[1:] / float(Q)
    hist = np.zeros((max_iter + 1, 2))
    out = dict(rms=0.0, rms_first=0.0, min_pivot=1.0, pairs=0, iterations=0, converged=0, status=0, sums=[], Ts=[])
    for k in range(max_iter + 1):
        terms, near, pm = evaluate(verts, faces, points, T, metric, reject, cbar, closest)
        tot = tree_sum(terms, tree)
        out["sums"].append(tot)
        out["Ts"].append(np.array(T).reshape(4, 4))
        n = float(tot[0])
        rms = math.sqrt(float(tot[1]) / n) if n > 0.0 else 0.0
        prev = out["rms"]
        hist[k] = rms, n
        out.update(rms=rms, pairs=int(n), iterations=k, near=near, moved=pm)
        if k == 0:
            out["rms_first"] = rms
        if k > 0 and abs(prev - rms) <= tol:
            out["converged"] = 1
            break
        if k == max_iter:
            break
        if n < 6.0:
            out["status"] = GEOMETRY
            break
        if metric == PLANE:
            c = map_points(T, cbar[None, :])[0]
            got = plane_solve(tot, c)
            D, mp = got if got is not None else (None, 1.0)
        else:
            D, mp = horn_solve(tot), 1.0
        Tn = compose(D, T) if D is not None else None
        if Tn is None or not all(finite(x) for x in Tn):
            out["status"] = GEOMETRY
            break
        out["min_pivot"] = mp
        T = Tn
    out["T"] = np.array(T).reshape(4, 4)
    out["history"] = hist
    return out


def record(o):
    """the dict of register() as one _lib.REGISTRATION_DTYPE record"""
    from shoulder_amd import _lib
    r = np.zeros((), dtype=_lib.REGISTRATION_DTYPE)
    for k in ("T", "rms", "rms_first", "min_pivot", "pairs", "iterations", "converged", "status"):
        r[k] = o[k]
    return r


# ---- inputs the tests share --------------------------------------------------------------------------------------------------
def rigid(axis, deg, t, about=(0.0, 0.0, 0.0)):
    """rotation by deg about the axis through `about`, then the translation t: a (4, 4)"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.identity(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    M = np.identity(4)
    M[:3, :3] = R
    M[:3, 3] = np.asarray(about) - R @ np.asarray(about) + np.asarray(t)
    return M


def apply(M, p):
    return p @ M[:3, :3].T + M[:3, 3]


def box(sx=30.0, sy=20.0, sz=10.0):
    """the axis-aligned scalene box [0, sx] x [0, sy] x [0, sz]: 8 vertices, 12 faces, outward normals"""
    v = np.array([(x, y, z) for z in (0.0, sz) for y in (0.0, sy) for x in (0.0, sx)], dtype=np.float32)
    f = np.array([(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)],
                 dtype=np.int32)
    return v, f


def box_points(Q, seed=0, size=(30.0, 20.0, 10.0)):
    """Q points on the six faces of the box, dealt face after face, strictly inside each face"""
    rng = np.random.default_rng(seed)
    size = np.asarray(size)
    p = rng.uniform(0.1, 0.9, size=(Q, 3)) * size
    for i in range(Q):
        ax, side = (i % 6) // 2, i % 2
        p[i, ax] = side * size[ax]
    return p


BOX_MOVE = rigid((1.0, 2.0, 3.0), 3.0, (0.4, -0.3, 0.2))


# ---- the ctypes side of the host twins (tests/hostcheck/icp_check.cpp) ----------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("icp", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.ic_precheck.argtypes = [i, vp, i, i, vp, vp, i, i]
    L.ic_jacobi.argtypes, L.ic_jacobi.restype = [vp, vp], None
    L.ic_chol.argtypes = [vp, vp, vp, vp]
    L.ic_tree.argtypes, L.ic_tree.restype = [vp, i, vp], None
    L.ic_evaluate.argtypes, L.ic_evaluate.restype = [vp, vp, i, vp, i, vp, i, d, vp], None
    L.ic_register.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp]
    L.ic_plan.argtypes, L.ic_plan.restype = [i, i, i, ctypes.c_longlong, i, vp], None
    return L


def closest_culled(verts, faces, points):
    """closest_oracle.closest on the faces that can hold the winner: a face is kept when its bounding sphere comes at least as near as
    the nearest vertex of the mesh (plus a millimetre, far beyond every rounding involved).  Every face at the winning distance is
    kept and the winner is chosen as closest_oracle.closest chooses it, so the records are those of the full walk, bytes; the tests
    hold it to the full walk once."""
    from shoulder_amd import _lib
    v, faces = widen(verts), np.asarray(faces)
    A, ab, ac = CO.corners(v, faces)
    nrm = cross3(ab, ac)
    tri = v[faces]
    cen = tri.mean(axis=1)
    rad = np.linalg.norm(tri - cen[:, None, :], axis=2).max(axis=1)
    used = v[np.unique(faces)]
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(points), dtype=_lib.CLOSEST_DTYPE)
    for i, p in enumerate(points):
        d = used - p
        upper = math.sqrt(np.einsum("ij,ij->i", d, d).min())
        d = cen - p
        keep = np.nonzero(np.sqrt(np.einsum("ij,ij->i", d, d)) - rad <= upper + 1.0)[0]
        u, w, region, dd, q, r = CO.tri_terms(A[keep], ab[keep], ac[keep], p)
        fin = np.nonzero(np.isfinite(dd))[0]
        if len(fin) == 0:
            out[i]["face"], out[i]["status"] = -1, GEOMETRY
            continue
        k = fin[np.lexsort((keep[fin], dd[fin]))[0]]
        out[i]["dist"], out[i]["point"], out[i]["face"], out[i]["region"] = np.sqrt(dd[k]), q[k], keep[k], region[k]
        out[i]["side"] = 1 if dot3(r[k], nrm[keep[k]]) >= 0 else -1
    return out
