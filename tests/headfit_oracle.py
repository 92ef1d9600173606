"""CPU oracle of the head fit (include/shoulder_hip.h sh_head_fit), test infrastructure shared by tests/test_headfit_host.py and
tests/test_gpu_headfit.py.  The triangles come from oracle/clip.py slice_plane as tests/test_gpu_resect.OracleCut takes them; the
sphere is solved by np.linalg.lstsq on the sqrt(w)-scaled rows [2 q, 1] against |q|^2 -- a route that never forms the moments --
and the ellipse by np.linalg.eigh on the polygon moments of the oracle ring taken about its own centroid."""
import ctypes

import numpy as np

import host_twin
from oracle import clip

EPS = 2.0 ** -53


def basis(n):
    un = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    u = np.cross(un, [1.0, 0.0, 0.0] if abs(un[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return u, np.cross(un, u)


def samples_of(tri, o):
    """triangles (n, 3, 3) -> samples q (3 n, 3) about o and weights (3 n): a third of the triangle's area on each corner"""
    cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    w = (0.5 * np.sqrt((cr[:, 0] ** 2 + cr[:, 1] ** 2) + cr[:, 2] ** 2)) / 3.0
    return tri.reshape(-1, 3) - o, np.repeat(w, 3)


def moment_terms(q, w):
    """(n, 14) terms of S0, S1, S2 (xx xy xz yy yz zz), S3, S4"""
    r2 = (q[:, 0] ** 2 + q[:, 1] ** 2) + q[:, 2] ** 2
    cols = [w, w * q[:, 0], w * q[:, 1], w * q[:, 2]]
    cols += [w * q[:, i] * q[:, j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    cols += [w * r2 * q[:, 0], w * r2 * q[:, 1], w * r2 * q[:, 2], w * r2 * r2]
    return np.array(cols).T


def moments16(q, w):
    m = np.zeros(16)
    if len(q):
        m[:14] = moment_terms(q, w).sum(axis=0)
    return m


def sphere_lstsq(q, w):
    """-> c (about the origin of q), r, first-order rms; None without samples"""
    if len(q) == 0:
        return None
    sw = np.sqrt(w)
    A = np.c_[2.0 * q, np.ones(len(q))] * sw[:, None]
    y = ((q[:, 0] ** 2 + q[:, 1] ** 2) + q[:, 2] ** 2) * sw
    sol = np.linalg.lstsq(A, y, rcond=None)[0]
    c, t = sol[:3], sol[3]
    r = np.sqrt(t + c @ c)
    E = float(((A @ sol - y) ** 2).sum())
    return c, r, np.sqrt(max(E, 0.0) / w.sum()) / (2.0 * r)


def ring_sums(ring, o, n):
    """closed ring (k + 1, 3) -> the six shoelace sums about o in base.Section's basis (the words of "resect.fit_ring")"""
    u, w = basis(n)
    d = ring - o
    x, y = d @ u, d @ w
    x0, x1, y0, y1 = x[:-1], x[1:], y[:-1], y[1:]
    cr = x0 * y1 - x1 * y0
    return np.array([cr.sum(), ((x0 + x1) * cr).sum(), ((y0 + y1) * cr).sum(), (cr * (x0 * x0 + x0 * x1 + x1 * x1)).sum(),
                     (cr * (y0 * y0 + y0 * y1 + y1 * y1)).sum(), (cr * (x0 * y1 + 2 * x0 * y0 + 2 * x1 * y1 + x1 * y0)).sum()])


def ellipse_of_ring(ring, o, n):
    """closed ring -> semi_major, semi_minor, unit major direction in 3-D (sign rule of the header)"""
    u, w = basis(n)
    d = ring - o
    x, y = d @ u, d @ w
    cr = x[:-1] * y[1:] - x[1:] * y[:-1]
    A = 0.5 * cr.sum()
    cx, cy = ((x[:-1] + x[1:]) * cr).sum() / (6 * A), ((y[:-1] + y[1:]) * cr).sum() / (6 * A)
    x, y = x - cx, y - cy                                                            # moments about the area centroid, directly
    cr = x[:-1] * y[1:] - x[1:] * y[:-1]
    x0, x1, y0, y1 = x[:-1], x[1:], y[:-1], y[1:]
    Ixx = (cr * (x0 * x0 + x0 * x1 + x1 * x1)).sum() / 12.0
    Iyy = (cr * (y0 * y0 + y0 * y1 + y1 * y1)).sum() / 12.0
    Ixy = (cr * (x0 * y1 + 2 * x0 * y0 + 2 * x1 * y1 + x1 * y0)).sum() / 24.0
    lam, vec = np.linalg.eigh(np.array([[Ixx, Ixy], [Ixy, Iyy]]) / A)
    d3 = vec[0, 1] * u + vec[1, 1] * w
    lead = d3[np.nonzero(d3)[0][0]]
    return 2.0 * np.sqrt(lam[1]), 2.0 * np.sqrt(lam[0]), d3 if lead > 0 else -d3


class OracleFit:
    """every field of a sh_head_fit for the cut of (v64, f) by (o, n), csys: the humerus' CT -> canal / articular matrix or None"""

    def __init__(self, v64, f, o, n, csys=None):
        ov, of, oe = clip.slice_plane(v64, f, o, n)
        self.q, self.w = samples_of(ov[of], o) if len(of) else (np.zeros((0, 3)), np.zeros(0))
        self.terms = moment_terms(self.q, self.w) if len(of) else np.zeros((0, 14))
        self.moments = moments16(self.q, self.w)
        self.sphere = sphere_lstsq(self.q, self.w)
        un = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if self.sphere is not None:
            c, r, rms = self.sphere
            self.center, self.radius, self.rms, self.cap_height = o + c, r, rms, r + c @ un
            self.center_articular = None if csys is None else csys[:3, :3] @ self.center + csys[:3, 3]
        try:
            loops = clip.loops_from_edges(oe)
        except ValueError:
            loops = None
        self.ellipse = None
        if loops:
            rings = [ov[lp + lp[:1]] for lp in loops]
            best = int(np.argmax([abs(ring_sums(r, o, n)[0]) for r in rings]))
            self.ring = rings[best]
            self.ellipse = ellipse_of_ring(self.ring, o, n)


def sum_bound(terms):
    """the project's bound for one sum added in two orders (tests/test_gpu_resect.py): 4 n 2^-53 sum |t|, per column"""
    return 4.0 * len(terms) * EPS * np.abs(terms).sum(axis=0)


def build_shim(directory):
    """tests/hostcheck/headfit_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library"""
    L = host_twin.build_shim("headfit", directory)
    L.hf_sphere.argtypes = [ctypes.c_void_p] * 4
    L.hf_ellipse.argtypes = [ctypes.c_void_p] * 4
    return L


def host_sphere(L, m16):
    m = np.ascontiguousarray(m16, dtype=np.float64)
    c, r, rms = np.zeros(3), np.zeros(1), np.zeros(1)
    rc = L.hf_sphere(m.ctypes.data, c.ctypes.data, r.ctypes.data, rms.ctypes.data)
    return rc, c, float(r[0]), float(rms[0])


def host_ellipse(L, rm6):
    m = np.ascontiguousarray(rm6, dtype=np.float64)
    a, b, d = np.zeros(1), np.zeros(1), np.zeros(2)
    rc = L.hf_ellipse(m.ctypes.data, a.ctypes.data, b.ctypes.data, d.ctypes.data)
    return rc, float(a[0]), float(b[0]), d


def icosphere(levels, radius, centre):
    """20 x 4^levels faces on the sphere (radius, centre), outward windings -> (verts float32, faces int32)"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    v /= np.linalg.norm(v, axis=1)[:, None]
    for _ in range(levels):
        cache, vs, nf = {}, list(v), []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = vs[a] + vs[b]
                vs.append(m / np.linalg.norm(m)); cache[k] = len(vs) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(vs), np.array(nf)
    return np.ascontiguousarray(v * radius + np.asarray(centre), np.float32), np.ascontiguousarray(f, np.int32)
