"""NumPy statement of sh_smooth_vertices (include/shoulder_hip.h "smoothing of the vertices of the resident batch"): the vertex -> vertex
rows, the stored weights, the pins, the neighbour mean, the Laplacian, Taubin and HC filters, the scaling that keeps the volume and the
info record, on float64 and written operation by operation in the order of sh_scalar.h smooth_*, so that it gives the bytes the
host-compiled statement gives (tests/hostcheck/smooth_check.cpp, -ffp-contract=off) and the device gives: the chain is + - x / sqrt, all
correctly rounded.  The rows come from topo_oracle.incidence, the pins from topo_oracle.adjacency, the volume sums are the terms of
mass_oracle.face_terms in the tree of icp_oracle.tree_sum.  A sum over a row runs position by position over all rows at once, which is
the row's order in every row.  Also the test meshes and the ctypes side of the host twin."""
import ctypes

import numpy as np

import host_twin
import icp_oracle as IO
import mass_oracle as MO
import topo_oracle as TO
import vert_oracle as VO
from ray_oracle import cross3, dot3, widen

ARG, STATE, GEOMETRY = -1, -3, -5
LAPLACIAN, TAUBIN, HC = 0, 1, 2
UNIFORM, INVLEN = 0, 1
PIN_BORDER, KEEP_VOLUME = 1, 2
MAX_ITER, NEWTON, BLOCK = 256, 10, 256
FILTERS = {"laplacian": LAPLACIAN, "taubin": TAUBIN, "hc": HC}


def neighbours(faces, nv):
    """-> (nrow (nv + 1,), nbr): row v the distinct u != v that share a non-degenerate face with v, ascending; from the incidence rows"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vrow, vface = TO.incidence(f, nv)
    v = np.repeat(np.arange(nv, dtype=np.int64), np.diff(vrow))
    corners = f[vface[:vrow[-1]]]                                   # (pairs, 3): the faces of every (vertex, face) pair
    vv, uu = np.repeat(v, 3), corners.ravel()
    key = np.unique((vv * max(nv, 1) + uu)[uu != vv])               # sorted by (v, u): the ascending order of every row
    nrow = np.zeros(nv + 1, dtype=np.int32)
    nrow[1:] = np.cumsum(np.bincount(key // max(nv, 1), minlength=nv))
    return nrow, (key % max(nv, 1)).astype(np.int32)


def row_of(nrow):
    return np.repeat(np.arange(len(nrow) - 1), np.diff(nrow))


def weights(verts, nrow, nbr):
    """the stored weights: 1.0 / l in the canonical order of the pair, 0.0 for a pair that is skipped (smooth_weight)"""
    p0, v, u = widen(verts).reshape(-1, 3), row_of(nrow), nbr.astype(np.int64)
    D = p0[np.maximum(v, u)] - p0[np.minimum(v, u)]
    l = np.sqrt(dot3(D, D))
    with np.errstate(all="ignore"):
        return np.where((l == 0.0) | ~np.isfinite(l), 0.0, 1.0 / l)


def border_pins(faces, nv):
    """the test behind VERT_BORDER | VERT_NONMANIFOLD: a border or non-manifold slot that touches the vertex (smooth_border)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    adj = TO.adjacency(f)[0]
    hit = (adj == TO.BORDER) | (adj == TO.NONMANIFOLD)             # slot e is the edge {f[e], f[(e + 1) % 3]}: it touches both
    pin = np.zeros(nv, dtype=bool)
    for e in range(3):
        pin[f[hit[:, e], e]] = True
        pin[f[hit[:, e], (e + 1) % 3]] = True
    return pin


def mean(x, nrow, nbr, w, pinned):
    """M(x) (smooth_mean); w None: uniform"""
    nv, deg = len(nrow) - 1, np.diff(nrow)
    S, W, added = np.zeros((nv, 3)), np.zeros(nv), np.zeros(nv, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(int(deg.max()) if nv else 0):
            rows = np.nonzero((deg > k) & ~pinned)[0]
            at = nrow[rows] + k
            wi = np.ones(len(rows)) if w is None else w[at]
            use = wi != 0.0
            rows, at, wi = rows[use], at[use], wi[use]
            S[rows] = S[rows] + wi[:, None] * x[nbr[at]]
            W[rows] = W[rows] + wi
            added[rows] += 1
        keep = pinned | (added == 0) | ~np.isfinite(W)
        return np.where(keep[:, None], x, S / W[:, None])


def volume_terms(P, faces, o):
    """terms 13 .. 16 of mass_face_terms on float64 corners P about the pivot o -> (F, 4).  (mass_oracle.face_terms rounds its vertices to
    float32 first; on P0 the two are the same bytes, which tests/test_smooth_host.py holds.)"""
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = P[f[:, 0]] - o, P[f[:, 1]] - o, P[f[:, 2]] - o
    s = (a + b) + c
    d = dot3(a, cross3(b, c))
    return np.concatenate([d[:, None], d[:, None] * s], axis=1)


def cube_root(r):
    s = 1.0
    for _ in range(NEWTON):
        s = s - ((s * s) * s - r) / (3.0 * (s * s))
    return s


def smooth(verts, faces, filter="taubin", iterations=10, lamb=0.5, mu=-0.53, alpha=0.1, beta=0.5, weight=UNIFORM, pin=None, pin_border=False,
           keep_volume=False):
    """one mesh -> dict(nrow, nbr, w, pos (V, 3), info (record), pinned (V,) bool)"""
    from shoulder_amd import _lib
    filter = FILTERS.get(filter, filter)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    p0 = widen(verts).reshape(-1, 3)
    nv = len(p0)
    nrow, nbr = neighbours(f, nv)
    wst = weights(verts, nrow, nbr)
    w = wst if weight == INVLEN else None
    pinned = np.zeros(nv, dtype=bool) if pin is None else np.asarray(pin).reshape(-1) != 0
    if pin_border:
        pinned = pinned | border_pins(f, nv)
    M = lambda x: mean(x, nrow, nbr, w, pinned)
    P = p0.copy()
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            if filter == HC:
                q = P
                p = M(q)
                b = np.where(pinned[:, None], 0.0, p - (alpha * p0 + (1.0 - alpha) * q))
                P = p - (beta * b + (1.0 - beta) * M(b))
            else:
                P = P + lamb * (M(P) - P)
                if filter == TAUBIN:
                    P = P + mu * (M(P) - P)
        info = np.zeros((), dtype=_lib.SMOOTH_INFO_DTYPE)
        o = p0[0] if nv else np.zeros(3)
        T0 = IO.tree_sum(volume_terms(p0, f, o)) if len(f) else np.zeros(4)
        T1 = IO.tree_sum(volume_terms(P, f, o)) if len(f) else np.zeros(4)
        V0, V1 = T0[0] / 6.0, T1[0] / 6.0
        info["volume_before"], info["volume_after"], info["scale"] = V0, V1, 1.0
        if keep_volume:
            r = V0 / V1 if V1 != 0.0 else np.nan
            c = T1[1:4] / (4.0 * T1[0]) + o if T1[0] != 0.0 else np.full(3, np.nan)
            if V0 == 0.0 or V1 == 0.0 or not np.isfinite(V0) or not np.isfinite(V1) or not (0.125 <= r <= 8.0) or not np.isfinite(c).all():
                info["status"] = GEOMETRY
            else:
                s = cube_root(float(r))
                info["scale"] = s
                P = c + s * (P - c)
        d = P - p0
        d2 = dot3(d, d)
        dist = np.sqrt(d2)
        info["max_disp"] = float(np.where(dist > 0.0, dist, 0.0).max()) if nv else 0.0
        info["sum_sq_disp"] = IO.tree_sum(d2) if nv else 0.0
    info["pinned"], info["isolated"] = int(pinned.sum()), int((np.diff(nrow) == 0).sum())
    return dict(nrow=nrow, nbr=nbr, w=wst, pos=P, info=info, pinned=pinned)


NAMES = ("nrow", "nbr", "w", "pos", "info")
_REFERENCE = {}


def reference(name, mesh, tag, kw):
    """smooth(*mesh, **kw), computed once per (name, tag) of a test session and shared by the test files; treat it as read-only"""
    if (name, tag) not in _REFERENCE:
        _REFERENCE[name, tag] = smooth(*mesh, **kw)
    return _REFERENCE[name, tag]


def same_bytes(got, want, tag):
    """rows, weights, positions and info of one mesh, as bytes"""
    for n in NAMES:
        assert np.ascontiguousarray(got[n]).tobytes() == np.ascontiguousarray(want[n]).tobytes(), (tag, n)


# ---- the test meshes -------------------------------------------------------------------------------------------------------------------
def unused_vertex_mesh(box):
    """the box with a vertex no face uses, in the middle of the vertex array (every later index moves up by one)"""
    v, f = box
    v = np.concatenate([v[:3], [[7.0, 8.0, 9.0]], v[3:]]).astype(np.float32)
    return np.ascontiguousarray(v), np.ascontiguousarray(np.where(f >= 3, f + 1, f).astype(np.int32))


def coincident_mesh():
    """a tetrahedron with a fifth vertex at the coordinates of vertex 1, joined to it by two faces: l = 0 under INVLEN"""
    v, f = TO.tetrahedron()
    v = np.concatenate([v, v[1:2]]).astype(np.float32)
    f = np.concatenate([f, [[1, 4, 2], [4, 1, 3]]]).astype(np.int32)
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


def noisy_icosphere(sigma=0.2, seed=7):
    """vert_oracle.icosphere at 3 subdivisions, radius 25, with seeded radial noise of sigma mm"""
    v, f = VO.icosphere(3, 25.0)
    v = v.astype(np.float64)
    r = np.linalg.norm(v, axis=1)
    n = np.random.default_rng(seed).normal(0.0, sigma, len(v))
    return np.ascontiguousarray((v * ((r + n) / r)[:, None]).astype(np.float32)), f


def small_cases(meshes):
    """the shapes at which the kernels can go wrong: name -> mesh.  meshes: topo_oracle.table's dict (box, humerus_left ...)"""
    T, further = TO.table(meshes), TO.further(meshes)
    out = {"tetrahedron": further["tetrahedron"]}
    for n in ("box", "box without face 0", "fan of 300", "strip of 600, shuffled", "humerus_left[:255]", "humerus_left[:256]", "humerus_left[:257]"):
        out[n] = T[n][0]
    for n in ("boxes sharing an edge", "degenerate faces", "degenerate faces, four faces", "only degenerate faces"):
        out[n] = further[n]
    out["loose triangles"] = TO.loose_triangles(40)
    out["unused vertex"] = unused_vertex_mesh(meshes["box"])
    out["coincident vertices"] = coincident_mesh()
    return out


def pin_mask(nv, seed=5):
    """a seeded mask: about a quarter of the vertices, bytes 0 / 1 / 200"""
    r = np.random.default_rng(seed).integers(0, 8, nv)
    return np.where(r == 0, 1, np.where(r == 1, 200, 0)).astype(np.uint8)


def variants(nv):
    """the argument sets every case runs: all three filters, both weights, 3 iterations, with and without a seeded mask, with
    pin_border, with keep_volume -> list of (tag, kwargs of smooth())"""
    out = []
    for filt in (LAPLACIAN, TAUBIN, HC):
        for weight in (UNIFORM, INVLEN):
            out.append((f"filter {filt} weight {weight}", dict(filter=filt, weight=weight, iterations=3)))
        out.append((f"filter {filt} mask", dict(filter=filt, weight=INVLEN, iterations=3, pin=pin_mask(nv))))
        out.append((f"filter {filt} pin_border", dict(filter=filt, weight=UNIFORM, iterations=3, pin_border=True)))
        out.append((f"filter {filt} keep_volume", dict(filter=filt, weight=filt % 2, iterations=3, keep_volume=True)))
    return out


# the whole meshes both test files run: (fixture, tag, kwargs of smooth())
WHOLE = [("humerus_left", "taubin, invlen, 10", dict(filter=TAUBIN, weight=INVLEN, iterations=10)),
         ("humerus_left", "hc, 10, keep_volume", dict(filter=HC, iterations=10, keep_volume=True)),
         ("humerus_left_trab", "laplacian, invlen, 3, keep_volume", dict(filter=LAPLACIAN, weight=INVLEN, iterations=3, keep_volume=True)),
         ("proximal_left_cut", "hc, invlen, 3, pin_border", dict(filter=HC, weight=INVLEN, iterations=3, pin_border=True))]


# ---- the ctypes side of the host twin (tests/hostcheck/smooth_check.cpp) ---------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("smooth", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.sc_smooth.argtypes, L.sc_smooth.restype = [vp, i, vp, i, vp, vp, vp, i, i, i, i, d, d, vp, vp, vp, vp, vp, vp], None
    L.sc_precheck.argtypes = [i, i, i, i, i, d, d, i, i, ctypes.c_longlong, i, i, vp, i]
    L.sc_plan.argtypes, L.sc_plan.restype = [i, i, i, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, vp], None
    L.sc_cbrt.argtypes, L.sc_cbrt.restype = [d], d
    return L


def params(filter, lamb=0.5, mu=-0.53, alpha=0.1, beta=0.5):
    return (alpha, beta) if filter == HC else (lamb, mu)


def host_smooth(shim, verts, faces, filter=TAUBIN, iterations=10, lamb=0.5, mu=-0.53, alpha=0.1, beta=0.5, weight=UNIFORM, pin=None, pin_border=False,
                keep_volume=False):
    """the host twin of the kernels for one mesh (incidence and adjacency from topo_oracle) -> the dict of smooth() without `pinned`"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    vrow, vface = TO.incidence(f, len(v))
    adj = np.ascontiguousarray(TO.adjacency(f)[0].ravel(), np.int32)
    out = dict(nrow=np.zeros(len(v) + 1, np.int32), nbr=np.zeros(6 * max(len(f), 1), np.int32), w=np.zeros(6 * max(len(f), 1)), pos=np.zeros((len(v), 3)),
               info=np.zeros(1, dtype=_lib.SMOOTH_INFO_DTYPE))
    mask = None if pin is None else np.ascontiguousarray(pin, np.uint8)
    p0, p1 = params(filter, lamb, mu, alpha, beta)
    flags = (PIN_BORDER if pin_border else 0) | (KEEP_VOLUME if keep_volume else 0)
    shim.sc_smooth(v.ctypes.data, len(v), f.ctypes.data, len(f), vrow.ctypes.data, vface.ctypes.data, adj.ctypes.data, int(filter), int(weight), int(iterations), flags,
                   float(p0), float(p1), None if mask is None else mask.ctypes.data, *[out[n].ctypes.data for n in NAMES])
    n = int(out["nrow"][-1])
    out["nbr"], out["w"], out["info"] = out["nbr"][:n], out["w"][:n], out["info"][0]
    return out
