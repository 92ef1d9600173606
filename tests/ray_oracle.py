"""NumPy statement of the rule of sh_ray_cast / sh_anp_axis_hits (include/shoulder_hip.h "rays against the resident batch"): every hit
of a ray with a mesh, ascending by (t, face).  Written operation by operation like sh_common.h cross3 / dot3 and sh_scalar.h
ray_tri_hit, so that float64 NumPy gives the bits the host-compiled statement gives (tests/hostcheck/ray_check.cpp); against the device
the tests still ask 1e-6 mm only.  Also the ctypes side of the host twins."""
import ctypes

import numpy as np

import host_twin

ARG, STATE = -1, -3


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def widen(verts):
    """the resident vertices: float32, widened to float64"""
    return np.asarray(verts, dtype=np.float32).astype(np.float64)


def terms(v, faces, o, d):
    """det, u, w, t (F,) of one ray against every face; v: float64 corners (V, 3)"""
    A = v[faces[:, 0]]
    e1, e2 = v[faces[:, 1]] - A, v[faces[:, 2]] - A
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tv = o[None, :] - A
    qv = cross3(tv, e1)
    pv = cross3(np.broadcast_to(d, e2.shape), e2)
    det = dot3(e1, pv)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / det
        u = dot3(tv, pv) * inv
        w = dot3(np.broadcast_to(d, qv.shape), qv) * inv
        t = dot3(e2, qv) * inv
    return det, u, w, t


def ray_hits(v, faces, o, d):
    """every hit of one ray -> (t, face, side), ascending by (t, face)"""
    det, u, w, t = terms(v, faces, o, d)
    with np.errstate(invalid="ignore"):
        hit = (np.abs(det) > 1e-12) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 1e-9)
    f = np.nonzero(hit)[0]
    order = np.lexsort((f, t[f]))
    f = f[order]
    return t[f], f.astype(np.int32), np.where(det[f] > 0, 1, -1).astype(np.int32)


def in_doubt(v, faces, o, d, eps=1e-9):
    """some face lies within eps of a threshold of the rule: a ray the issue lets a comparison against NumPy set aside"""
    det, u, w, t = terms(v, faces, o, d)
    with np.errstate(invalid="ignore"):
        live = np.abs(det) > 1e-12
        near_det = np.abs(np.abs(det) - 1e-12) <= eps
        # a barycentric or t threshold matters only where the others hold (with the same slack)
        inside = (u >= -eps) & (w >= -eps) & (u + w <= 1 + eps) & (t > 1e-9 - eps)
        edge = (np.abs(u) <= eps) | (np.abs(w) <= eps) | (np.abs(u + w - 1) <= eps) | (np.abs(t - 1e-9) <= eps)
    return bool(np.any(near_det & np.isfinite(t)) or np.any(live & inside & edge))


def cast(verts, faces, origins, directions, cap):
    """(hits (R, cap) of _lib.RAY_HIT_DTYPE, counts (R,)) of one mesh, the layout of one humerus of sh_ray_cast"""
    from shoulder_amd import _lib
    v, faces = widen(verts), np.asarray(faces)
    origins, directions = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(directions, np.float64).reshape(-1, 3)
    R = len(origins)
    hits, counts = np.zeros((R, cap), dtype=_lib.RAY_HIT_DTYPE), np.zeros(R, dtype=np.int32)
    hits["face"] = -1
    for r in range(R):
        t, f, s = ray_hits(v, faces, origins[r], directions[r])
        counts[r] = len(t)
        k = min(len(t), cap)
        hits["t"][r, :k], hits["face"][r, :k], hits["side"][r, :k] = t[:k], f[:k], s[:k]
        hits["point"][r, :k] = origins[r][None, :] + directions[r][None, :] * t[:k, None]
    return hits, counts


def plates(n, gap=1.0, half=1.0):
    """n separated square plates z = gap * (k + 1), two triangles each sharing the diagonal (-half, -half) -> (half, half):
    -> (verts float64 (4 n, 3), faces int32 (2 n, 3)); normals along +z"""
    v, f = [], []
    for k in range(n):
        z = gap * (k + 1)
        v += [(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)]
        f += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int32)


TETRA = (np.array([(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (0.0, 0.0, 4.0)]),
         np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], dtype=np.int32))      # outward normals


def build_shim(directory, sanitize=False):
    """tests/hostcheck/ray_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library; sanitize=True: the
    stand-alone program with -fsanitize=address,undefined instead -> its path (it is run as a program, never loaded)"""
    L = host_twin.build_shim("ray", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.rc_hit.argtypes = [vp, vp, vp, vp, vp]
    L.rc_hit_plain.argtypes = [vp, vp, vp, vp]
    L.rc_sort.argtypes, L.rc_sort.restype = [vp, vp, vp, i, vp, vp, vp, i, vp], None
    L.rc_cast.argtypes = [vp, vp, i, vp, vp, vp, i, vp]
    L.rc_precheck.argtypes = [vp, i, i, i, i, i]
    return L


def host_hit(S, o, d, tri):
    """(hit, t, side) of the side-returning statement, and (hit, t) of canal_ray_hit"""
    o, d, tri = (np.ascontiguousarray(a, np.float64) for a in (o, d, tri))
    t, t2, side = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
    h = S.rc_hit(o.ctypes.data, d.ctypes.data, tri.ctypes.data, ctypes.addressof(t), ctypes.addressof(side))
    h2 = S.rc_hit_plain(o.ctypes.data, d.ctypes.data, tri.ctypes.data, ctypes.addressof(t2))
    return (h, t.value, side.value), (h2, t2.value)


def host_sort(S, t, face, side, o, d, cap, T=None):
    """the segment sort of k_ray_sort on the host: keys in the order given -> (cap,) records"""
    from shoulder_amd import _lib
    t, face, side = np.ascontiguousarray(t, np.float64), np.ascontiguousarray(face, np.int32), np.ascontiguousarray(side, np.int32)
    o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
    T = None if T is None else np.ascontiguousarray(T, np.float64)
    out = np.zeros(cap, dtype=_lib.RAY_HIT_DTYPE)
    S.rc_sort(t.ctypes.data, face.ctypes.data, side.ctypes.data, len(t), o.ctypes.data, d.ctypes.data, T.ctypes.data if T is not None else None, cap, out.ctypes.data)
    return out


def host_cast(S, verts, faces, o, d, cap, T=None):
    """one ray against one mesh through the host-compiled device source (the faces are walked backwards, so that the pool is not in
    face order) -> ((cap,) records, count)"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
    T = None if T is None else np.ascontiguousarray(T, np.float64)
    out = np.zeros(cap, dtype=_lib.RAY_HIT_DTYPE)
    n = S.rc_cast(v.ctypes.data, f.ctypes.data, len(f), T.ctypes.data if T is not None else None, o.ctypes.data, d.ctypes.data, cap, out.ctypes.data)
    return out, int(n)
