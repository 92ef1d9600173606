"""NumPy statement of the rule of sh_winding_numbers (include/shoulder_hip.h "generalized winding numbers of the resident batch"): the
signed solid angle of every face seen from a query point (Van Oosterom & Strackee 1983), summed in the one order the definition fixes
-- blocks of 2048 consecutive faces, each block from 0 in face order, the block sums from 0 in block order, both serially -- and
divided by 4 pi.  Written operation by operation like sh_common.h dot3 / cross3 and sh_scalar.h solid_angle_tri:
    a = A - p, b = B - p, c = C - p;  la = sqrt(a . a), lb, lc alike
    num = a . (b x c)
    den = ((la * lb) * lc + (a . b) * lc) + ((a . c) * lb + (b . c) * la)
    omega = 2.0 * atan2(num, den), and 0 when num == 0.0
so that num and den are the bits the host-compiled statement gives (tests/hostcheck/winding_check.cpp, -ffp-contract=off).  atan2 is
each math library's own: omega, and with it the sum, is compared within a bound, `bound(F, A)`, never as bytes.  Also returns
A = sum |omega_f| / 4 pi per point, which that bound needs, and the ctypes side of the host twins."""
import ctypes

import numpy as np

import host_twin
from ray_oracle import cross3, dot3, widen

ARG, STATE, GEOMETRY = -1, -3, -5
BLOCK = 2048
FOUR_PI = 4.0 * np.pi


def solid_terms(A, B, C, p):
    """num, den (F,) of one point against F triangles with float64 corners A, B, C (F, 3)"""
    p = np.asarray(p, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        a, b, c = A - p[None, :], B - p[None, :], C - p[None, :]
        la, lb, lc = np.sqrt(dot3(a, a)), np.sqrt(dot3(b, b)), np.sqrt(dot3(c, c))
        num = dot3(a, cross3(b, c))
        den = ((la * lb) * lc + dot3(a, b) * lc) + (dot3(a, c) * lb + dot3(b, c) * la)
    return num, den


def solid_angles(A, B, C, p):
    """omega (F,): 2 atan2(num, den), 0 where num == 0.0"""
    num, den = solid_terms(A, B, C, p)
    with np.errstate(invalid="ignore"):
        return np.where(num == 0.0, 0.0, 2.0 * np.arctan2(num, den))


def serial_sum(x):
    """x[0] + x[1] + ... from 0.0, left to right, one rounding per addition (np.sum adds pairwise: not this)"""
    s = 0.0
    for t in x.tolist():
        s += t
    return s


def block_sum(om):
    """the summation tree of the definition"""
    total = 0.0
    for k in range(0, len(om), BLOCK):
        total += serial_sum(om[k:k + BLOCK])
    return total


def corners(verts, faces):
    v, faces = widen(verts), np.asarray(faces)
    return v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]


def winding(verts, faces, points):
    """-> ((Q,) records of _lib.WINDING_DTYPE of one mesh: the layout of one humerus of sh_winding_numbers, A (Q,) = sum |omega| / 4 pi)"""
    from shoulder_amd import _lib
    A, B, C = corners(verts, faces)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(points), dtype=_lib.WINDING_DTYPE)
    absw = np.zeros(len(points))
    for i, p in enumerate(points):
        om = solid_angles(A, B, C, p)
        total = block_sum(om)
        if not np.isfinite(total):
            out[i]["status"] = GEOMETRY
            absw[i] = np.inf
            continue
        w = total / FOUR_PI
        out[i]["winding"], out[i]["inside"] = w, int(abs(w) >= 0.5)
        absw[i] = float(np.abs(om).sum()) / FOUR_PI
    return out, absw


def bound(F, A):
    """|w_device - w_oracle| <= (2 F + 16) 2^-53 max(1, A): (F - 1) 2^-53 A for the recursive summation of each of the two sums, the
    rest for up to 4 ulp of difference per atan2 term (an assumption about the device's atan2)"""
    return (2.0 * F + 16.0) * 2.0 ** -53 * np.maximum(1.0, A)


def compare(got, want, absw, F):
    """one humerus' records (Q,) against the oracle's: inside and status equal, winding within bound(F, A) -> (largest difference, the
    smallest bound)"""
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["inside"], want["inside"]), np.nonzero(got["inside"] != want["inside"])[0][:8]
    ok = want["status"] == 0
    assert not got["winding"][~ok].any()
    if not ok.any():
        return 0.0, 0.0
    diff, lim = np.abs(got["winding"][ok] - want["winding"][ok]), bound(F, absw[ok])
    assert np.all(diff <= lim), (float(diff.max()), float(lim.min()))
    return float(diff.max()), float(lim.min())


# the cube of edge 2 about the origin: corners (-1 | 1)^3, twelve triangles, outward normals; faces 10 and 11 are the side z = 1,
# cut along its diagonal y = x
CUBE_V = np.array([(x, y, z) for z in (-1.0, 1.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)], dtype=np.float32)
CUBE_F = np.array([(0, 2, 3), (0, 3, 1),      # z = -1
                   (0, 1, 5), (0, 5, 4),      # y = -1
                   (0, 4, 6), (0, 6, 2),      # x = -1
                   (1, 3, 7), (1, 7, 5),      # x = 1
                   (2, 6, 7), (2, 7, 3),      # y = 1
                   (4, 5, 7), (4, 7, 6)], dtype=np.int32)      # z = 1


def cube(kind="closed"):
    """closed | open (the side z = 1 removed) | doubled (every face stored twice) | reversed (stored inside-out)"""
    f = {"closed": CUBE_F, "open": CUBE_F[:10], "doubled": np.concatenate([CUBE_F, CUBE_F]), "reversed": CUBE_F[:, ::-1]}[kind]
    return CUBE_V.copy(), np.ascontiguousarray(f, np.int32)


def build_shim(directory, sanitize=False):
    """tests/hostcheck/winding_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library; sanitize=True: the
    stand-alone program with -fsanitize=address,undefined instead -> its path (it is run as a program, never loaded)"""
    L = host_twin.build_shim("winding", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.wc_solid.argtypes, L.wc_solid.restype = [vp, vp, vp, vp], ctypes.c_double
    L.wc_mesh.argtypes, L.wc_mesh.restype = [vp, vp, i, vp, i, i, vp], None
    L.wc_precheck.argtypes = [i, vp, i, i, i, i]
    L.wc_splits.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    L.wc_plan.argtypes, L.wc_plan.restype = [i, i, ctypes.c_longlong, vp], None
    L.wc_split_range.argtypes, L.wc_split_range.restype = [i, i, i, vp, vp], None
    return L


def host_solid(S, p, tri):
    """(num, den, omega) of the host-compiled statement for the triangle with corners tri (3, 3)"""
    p, tri = np.ascontiguousarray(p, np.float64), np.ascontiguousarray(tri, np.float64)
    num, den = ctypes.c_double(0.0), ctypes.c_double(0.0)
    om = S.wc_solid(p.ctypes.data, tri.ctypes.data, ctypes.addressof(num), ctypes.addressof(den))
    return num.value, den.value, om


def host_mesh(S, verts, faces, points, splits=1):
    """the points against one mesh through the host-compiled device source: the blocks dealt to `splits` shares as k_wn_walk deals
    them, the block sums joined as k_wn_join joins them (splits == 1: folded in the walk) -> (Q,) records"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(pts), dtype=_lib.WINDING_DTYPE)
    S.wc_mesh(v.ctypes.data, f.ctypes.data, len(f), pts.ctypes.data, len(pts), splits, out.ctypes.data)
    return out


def host_plan(S, B, Q, maxF):
    """(blocks of the largest humerus, chunks, splits, doubles of "wn.part" per point) that sh_winding_numbers uses for this shape"""
    r = (ctypes.c_int * 4)()
    S.wc_plan(B, Q, maxF, ctypes.addressof(r))
    return tuple(r)
