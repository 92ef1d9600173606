"""CPU oracle of the seats of implant heads on a cut (include/shoulder_hip.h sh_seat), test infrastructure shared by
tests/test_seat_host.py and tests/test_gpu_seat.py: a NumPy float64 statement of the header's definitions, and an independent check of
the covered area -- Sutherland-Hodgman clipping of the ring by the regular N-gon inscribed in the disk (a convex clip polygon, so the
method is valid for any simple ring), whose area falls short of the exact one by at most pi rho^2 (1 - sin(2 pi / N) / (2 pi / N))."""
import ctypes
import os

import numpy as np

import headfit_oracle as H
import host_twin
from conftest import BONES

NGON = 4096


def in_plane(pts, o, n):
    """CT points -> coordinates about o in base.Section's basis"""
    u, w = H.basis(np.asarray(n, dtype=np.float64))
    d = np.asarray(pts, dtype=np.float64) - o
    return d @ u, d @ w


def _sector(x0, y0, x1, y1, rho2):
    return 0.5 * rho2 * np.arctan2(x0 * y1 - y0 * x1, x0 * x1 + y0 * y1)


def covered_area(x, y, rho):
    """area(polygon n disk(rho) about the origin): x, y the open ring; the header's edge rule, all edges at once"""
    ax, ay, bx, by = x, y, np.roll(x, -1), np.roll(y, -1)
    dx, dy = bx - ax, by - ay
    rho2 = rho * rho
    A, Bh, C = dx * dx + dy * dy, ax * dx + ay * dy, (ax * ax + ay * ay) - rho2
    disc = Bh * Bh - A * C
    pos = disc > 0.0
    sq = np.sqrt(np.where(pos, disc, 0.0))
    As = np.where(pos, A, 1.0)
    c0 = np.where(pos, np.maximum((-Bh - sq) / As, 0.0), 0.0)
    c1 = np.where(pos, np.minimum((-Bh + sq) / As, 1.0), 0.0)
    chord = c0 < c1
    px, py, qx, qy = ax + c0 * dx, ay + c0 * dy, ax + c1 * dx, ay + c1 * dy
    with_chord = (_sector(ax, ay, px, py, rho2) + 0.5 * (px * qy - py * qx)) + _sector(qx, qy, bx, by, rho2)
    return abs(float(np.where(chord, with_chord, _sector(ax, ay, bx, by, rho2)).sum()))


def rim(x, y):
    """-> rim_min, nearest point, its segment, rim_max, farthest vertex, its index (first in ring order on a tie)"""
    bx, by = np.roll(x, -1), np.roll(y, -1)
    dx, dy = bx - x, by - y
    dd = dx * dx + dy * dy
    t = np.clip(np.where(dd > 0, -(x * dx + y * dy) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
    nx, ny = x + t * dx, y + t * dy
    d2 = nx * nx + ny * ny
    i = int(np.argmin(d2))
    v2 = x * x + y * y
    j = int(np.argmax(v2))
    return np.sqrt(d2[i]), np.array([nx[i], ny[i]]), i, np.sqrt(v2[j]), np.array([x[j], y[j]]), j


def winding(x, y):
    bx, by = np.roll(x, -1), np.roll(y, -1)
    cr = x * by - y * bx
    return int(((y <= 0) & (by > 0) & (cr > 0)).sum()) - int(((y > 0) & (by <= 0) & (cr < 0)).sum())


def shoelace(x, y):
    return 0.5 * float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def ngon_bound(rho, N=NGON):
    t = 2.0 * np.pi / N
    return np.pi * rho * rho * (1.0 - np.sin(t) / t)


def clip_area_ngon(x, y, rho, N=NGON):
    """|area| of the ring clipped by the regular N-gon inscribed in the circle of radius rho about the origin (Sutherland-Hodgman,
    one half-plane after the other; a half-plane that holds every vertex is skipped)"""
    if shoelace(x, y) < 0:
        x, y = x[::-1], y[::-1]
    px, py = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
    ang = np.arange(N + 1) * (2.0 * np.pi / N)
    cx, cy = rho * np.cos(ang), rho * np.sin(ang)
    for k in range(N):
        if len(px) == 0:
            return 0.0
        ex, ey = cx[k + 1] - cx[k], cy[k + 1] - cy[k]
        side = ex * (py - cy[k]) - ey * (px - cx[k])                                  # >= 0: inside (the N-gon is counter-clockwise)
        ins = side >= 0.0
        if ins.all():
            continue
        qx, qy, qs, qi = np.roll(px, -1), np.roll(py, -1), np.roll(side, -1), np.roll(ins, -1)
        cross = ins != qi
        t = np.where(cross, side / np.where(cross, side - qs, 1.0), 0.0)
        ix, iy = px + t * (qx - px), py + t * (qy - py)
        # per edge p -> q: emit p if inside, then the crossing if the edge changes side
        ox = np.stack([px, ix], axis=1).reshape(-1)
        oy = np.stack([py, iy], axis=1).reshape(-1)
        keep = np.stack([ins, cross], axis=1).reshape(-1)
        px, py = ox[keep], oy[keep]
    return abs(shoelace(px, py)) if len(px) else 0.0


def surface_rms_direct(q, w, c, R):
    """the header's surface_rms summed over the samples themselves (q about the plane point, c too)"""
    if len(q) == 0:
        return 0.0
    d = q - c
    f = ((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2) - R * R
    return float(np.sqrt((w * f * f).sum() / w.sum()) / (2.0 * R))


def seat_record(ring, o, n, s_ct, R, h, q, w, sphere_center=None, csys=None):
    """every field of a sh_seat for the closed ring (k + 1, 3; CT) of the cut (o, n), the seat centre s_ct (CT; projected onto the
    plane), the head (R, h), the head piece's samples (q about o, w), the fitted sphere's centre and the humerus' CT -> canal /
    articular matrix (or None)"""
    o, n = np.asarray(o, dtype=np.float64), np.asarray(n, dtype=np.float64)
    u, wv = H.basis(n)
    un = n / np.linalg.norm(n)
    su, sw = in_plane(s_ct, o, n)
    x, y = in_plane(ring[:-1], o, n)
    x, y = x - su, y - sw
    rho = np.sqrt(h * (2.0 * R - h))
    cut_area = abs(shoelace(x, y))
    cov = covered_area(x, y, rho)
    rmin, near, imin, rmax, far, imax = rim(x, y)
    s3 = o + su * u + sw * wv
    ic = s3 + (h - R) * un
    r = dict(base_radius=rho, seat_center=s3, covered_area=cov, coverage=cov / cut_area, overhang_area=np.pi * rho * rho - cov,
             uncovered_area=cut_area - cov, rim_min=rmin, rim_max=rmax, max_overhang=max(0.0, rho - rmin), max_uncovered=max(0.0, rmax - rho),
             overhang_dir=(near[0] * u + near[1] * wv) / rmin if rmin > 0 else np.zeros(3),
             uncovered_dir=(far[0] * u + far[1] * wv) / rmax if rmax > 0 else np.zeros(3),
             center_inside=int(winding(x, y) != 0), implant_center=ic, surface_rms=surface_rms_direct(q, w, ic - o, R), status=0,
             xy=(x, y), cut_area=cut_area)
    r["cor_shift"] = ic - sphere_center if sphere_center is not None else np.zeros(3)
    r["cor_shift_articular"] = np.full(3, np.nan) if csys is None else csys[:3, :3] @ r["cor_shift"]
    return r


def humerus_cuts():
    """the four cuts of humerus_left of tests/test_headfit_host.py: (v64, f, [(o, n, OracleFit)])"""
    from shoulder_amd.stl import load_stl
    v, f = load_stl(os.path.join(BONES, "humerus_left.stl"))
    v64 = np.asarray(v, np.float32).astype(np.float64)
    f = np.asarray(f, np.int32)
    ctr = v64.mean(axis=0)
    ax = np.linalg.svd(v64 - ctr, full_matrices=False)[2][0]
    s = (v64 - ctr) @ ax
    cuts = []
    for frac, sign, tilt in ((0.88, 1.0, (0.0, 0.0, 0.0)), (0.80, 1.0, (0.2, -0.1, 0.0)), (0.12, -1.0, (0.0, 0.0, 0.0)), (0.2, -1.0, (-0.1, 0.15, 0.05))):
        o = ctr + ax * (s.min() + frac * (s.max() - s.min()))
        n = sign * ax + np.array(tilt)
        cuts.append((o, n, H.OracleFit(v64, f, o, n)))
    return v64, f, cuts


def build_shim(directory):
    """tests/hostcheck/seat_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library"""
    L = host_twin.build_shim("seat", directory)
    d, vp = ctypes.c_double, ctypes.c_void_p
    L.st_edge.argtypes, L.st_edge.restype = [d] * 5, d
    L.st_seg.argtypes, L.st_seg.restype = [d] * 4 + [vp], d
    L.st_wind.argtypes = [d] * 4
    L.st_rms.argtypes, L.st_rms.restype = [vp, vp, d], d
    L.st_seat.argtypes, L.st_seat.restype = [vp, vp, ctypes.c_int, d, vp, vp], None
    return L


def host_seat(L, x, y, rho):
    """the ring-dependent part of a seat through the host-compiled device source, in k_seat's order"""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out, idx = np.zeros(7), np.zeros(3, dtype=np.int32)
    L.st_seat(x.ctypes.data, y.ctypes.data, len(x), rho * rho, out.ctypes.data, idx.ctypes.data)
    return dict(covered_area=abs(out[0]), signed_area=out[0], rim_min=np.sqrt(out[1]), near=out[2:4].copy(), rim_max=np.sqrt(out[4]), far=out[5:7].copy(),
                imin=int(idx[0]), imax=int(idx[1]), winding=int(idx[2]))


def host_rms(L, m16, c, R):
    m, c = np.ascontiguousarray(m16, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    return float(L.st_rms(m.ctypes.data, c.ctypes.data, float(R)))


def spire(k, radius=20.0, height=10.0, centre=(0.0, 0.0, 0.0), phase=0.1):
    """closed pyramid over the regular k-gon (circumradius `radius`) with its apex `height` above the base centre: a horizontal cut
    at height z has a ring of exactly k points, the regular k-gon of circumradius radius (1 - z / height) (a triangulated prism would
    give 2 k) -> (verts float32, faces int32), outward windings"""
    t = phase + np.arange(k) * (2.0 * np.pi / k)
    c = np.asarray(centre, dtype=np.float64)
    base = np.c_[radius * np.cos(t), radius * np.sin(t), np.zeros(k)] + c
    v = np.concatenate([base, [c, c + [0.0, 0.0, height]]])
    f = []
    for i in range(k):
        j = (i + 1) % k
        f += [[i, j, k + 1], [k, j, i]]
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def regular_polygon_in_disk(k, r, rho):
    """area(regular k-gon of circumradius r n disk of radius rho), both about the same centre, in closed form"""
    a = r * np.cos(np.pi / k)                                                        # apothem
    if rho <= a:
        return np.pi * rho * rho
    if rho >= r:
        return 0.5 * k * r * r * np.sin(2.0 * np.pi / k)
    th = np.arccos(a / rho)                                                           # half-angle of the part of a side inside the disk
    return k * (a * np.sqrt(rho * rho - a * a) + rho * rho * (np.pi / k - th))
