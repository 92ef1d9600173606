"""NumPy statement of the rule of sh_closest_points (include/shoulder_hip.h "closest surface points of the resident batch"): the closest
point of every face of a mesh to a query point by the Voronoi-region walk of Ericson 5.1.5, every face, no cull, the winner by
np.lexsort((face, d2)) among the finite d2.  Written operation by operation like sh_common.h dot3 / cross3 and sh_scalar.h
closest_pt_tri, so that float64 NumPy gives the bits the host-compiled statement gives (tests/hostcheck/closest_check.cpp) and the
device gives (-ffp-contract=off).  Also an independent formulation of the distance (plane projection with an inside test, else the
nearest of the three edges) and the ctypes side of the host twins."""
import ctypes

import numpy as np

import host_twin
from ray_oracle import cross3, dot3, widen

ARG, STATE, GEOMETRY = -1, -3, -5


def tri_terms(A, ab, ac, p):
    """u, w, region, d2 of one point against F triangles kept as (A, ab, ac), each (F, 3)"""
    p = np.asarray(p, np.float64)
    ap = p[None, :] - A
    bp = ap - ab
    cp = ap - ac
    d1, d2, d3, d4, d5, d6 = dot3(ab, ap), dot3(ac, ap), dot3(ab, bp), dot3(ac, bp), dot3(ab, cp), dot3(ac, cp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (g >= 0)]
        w_bc = e / (e + g)
        denom = 1.0 / ((va + vb) + vc)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        u = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, 1.0 - w_bc], default=vb * denom)
        w = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w_bc], default=vc * denom)
        region = np.select(conds, [4, 5, 1, 6, 3, 2], default=0).astype(np.int32)
        q = (A + ab * u[:, None]) + ac * w[:, None]
        r = p[None, :] - q
        dd = dot3(r, r)
    return u, w, region, dd, q, r


def corners(v, faces):
    A = v[faces[:, 0]]
    return A, v[faces[:, 1]] - A, v[faces[:, 2]] - A


def closest(verts, faces, points):
    """(Q,) records of _lib.CLOSEST_DTYPE of one mesh: the layout of one humerus of sh_closest_points"""
    from shoulder_amd import _lib
    v, faces = widen(verts), np.asarray(faces)
    A, ab, ac = corners(v, faces)
    n = cross3(ab, ac)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(points), dtype=_lib.CLOSEST_DTYPE)
    ids = np.arange(len(faces))
    for i, p in enumerate(points):
        u, w, region, dd, q, r = tri_terms(A, ab, ac, p)
        fin = np.nonzero(np.isfinite(dd))[0]
        if len(fin) == 0:
            out[i]["face"], out[i]["status"] = -1, GEOMETRY
            continue
        f = fin[np.lexsort((ids[fin], dd[fin]))[0]]
        out[i]["dist"], out[i]["point"], out[i]["face"], out[i]["region"] = np.sqrt(dd[f]), q[f], f, region[f]
        out[i]["side"] = 1 if dot3(r[f], n[f]) >= 0 else -1
    return out


def ties(verts, faces, p):
    """how many faces share the winning d2 bit for bit"""
    v = widen(verts)
    dd = tri_terms(*corners(v, np.asarray(faces)), p)[3]
    dd = dd[np.isfinite(dd)]
    return int((dd == dd.min()).sum())


def distance_independent(verts, faces, points):
    """the distance by another formulation: the foot of the perpendicular where it falls inside the triangle (three edge-side tests
    against the normal), else the smallest of the three point-segment distances"""
    v, faces = widen(verts), np.asarray(faces)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    nn = np.einsum("ij,ij->i", n, n)
    out = np.empty(len(points))

    def seg(p, s0, s1):
        d = s1 - s0
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.clip(np.nan_to_num(np.einsum("ij,ij->i", p - s0, d) / np.einsum("ij,ij->i", d, d)), 0.0, 1.0)
        return np.linalg.norm(p - (s0 + d * t[:, None]), axis=1)
    for i, p in enumerate(np.asarray(points, np.float64).reshape(-1, 3)):
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.einsum("ij,ij->i", p - a, n) / nn
        foot = p - n * h[:, None]
        inside = np.ones(len(faces), bool)
        for s0, s1 in ((a, b), (b, c), (c, a)):
            inside &= np.einsum("ij,ij->i", np.cross(s1 - s0, foot - s0), n) >= 0
        inside &= nn > 0
        edge = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
        with np.errstate(invalid="ignore"):
            out[i] = np.where(inside, np.abs(h) * np.sqrt(nn), edge).min()
    return out


TETRA = (np.array([(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, 0.0, 4.0)]),
         np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], dtype=np.int32))      # outward normals


def build_shim(directory, sanitize=False):
    """tests/hostcheck/closest_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library; sanitize=True: the
    stand-alone program with -fsanitize=address,undefined instead -> its path (it is run as a program, never loaded)"""
    L = host_twin.build_shim("closest", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.cc_tri.argtypes, L.cc_tri.restype = [vp, vp, vp, vp, vp], ctypes.c_double
    L.cc_key_less.argtypes = [ctypes.c_double, i, ctypes.c_double, i]
    L.cc_mesh.argtypes, L.cc_mesh.restype = [vp, vp, i, vp, i, i, vp], None
    L.cc_precheck.argtypes = [i, vp, i, i, i, i]
    L.cc_splits.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    L.cc_split_range.argtypes, L.cc_split_range.restype = [i, i, i, vp, vp], None
    return L


def host_tri(S, p, tri):
    """(u, w, region, d2) of the host-compiled statement for the triangle with corners tri (3, 3)"""
    p, tri = np.ascontiguousarray(p, np.float64), np.ascontiguousarray(tri, np.float64)
    u, w, region = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(-1)
    d2 = S.cc_tri(p.ctypes.data, tri.ctypes.data, ctypes.addressof(u), ctypes.addressof(w), ctypes.addressof(region))
    return u.value, w.value, region.value, d2


def oracle_tri(p, tri):
    tri = np.asarray(tri, np.float64)
    u, w, region, dd, q, r = tri_terms(tri[None, 0], (tri[1] - tri[0])[None], (tri[2] - tri[0])[None], p)
    return float(u[0]), float(w[0]), int(region[0]), float(dd[0])


def host_mesh(S, verts, faces, points, splits=1, backwards=True):
    """the points against one mesh through the host-compiled device source: the faces walked in `splits` shares (backwards within a
    share when asked), the partials joined as k_cp_join joins them -> (Q,) records"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(pts), dtype=_lib.CLOSEST_DTYPE)
    for i in range(len(pts)):
        S.cc_mesh(v.ctypes.data, f.ctypes.data, len(f), pts[i].ctypes.data, splits, int(backwards), out[i:i + 1].ctypes.data)
    return out
