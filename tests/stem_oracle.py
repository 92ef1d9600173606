"""CPU oracle of the canal profile and the stems below a cut (include/shoulder_hip.h sh_canal_profile / sh_resect_stems), test
infrastructure shared by tests/test_stem_host.py, tests/test_gpu_stem.py and tools/time_stem.py: a NumPy float64 statement of the
header's definitions -- the profile as a brute-force loop of every ray over ALL faces, without any culling -- closed forms of
prisms, and the ctypes side of tests/hostcheck/stem_check.cpp."""
import ctypes

import numpy as np

import host_twin

GEOMETRY, ARG = -5, -1


def dirs(A):
    t = (2.0 * np.pi * np.arange(A)) / A
    return np.cos(t), np.sin(t)


def rigid(rotvec=(0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0)):
    """CT -> frame matrix: rotation by |rotvec| about rotvec (Rodrigues), then the shift"""
    w = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.zeros((3, 3))
    if th > 0:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    T[:3, 3] = shift
    return T


def map_points(T, v):
    """float32 CT vertices widened and mapped, the header's order of operations"""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    return np.stack([((T[i, 0] * v[:, 0] + T[i, 1] * v[:, 1]) + T[i, 2] * v[:, 2]) + T[i, 3] for i in range(3)], axis=1)


def to_ct(T, pts):
    """frame points -> CT through the inverse of the rigid T"""
    R, t = T[:3, :3], T[:3, 3]
    return (np.asarray(pts, dtype=np.float64) - t) @ R


def profile(vf, faces, z0, dz, L, A, margins=False):
    """near, far (L, A) of the frame vertices vf by Moller-Trumbore of every ray against every face (k_rays_hit's statement).
    margins=True: also `doubtful` (L, A) -- rays the issue lets an oracle set aside: the nearest (or farthest) hit has a barycentric
    margin or |det| below 1e-6, or another hit within 1e-6 mm of it in t."""
    a0, e1, e2 = vf[faces[:, 0]], vf[faces[:, 1]] - vf[faces[:, 0]], vf[faces[:, 2]] - vf[faces[:, 0]]
    c, s = dirs(A)
    d = np.stack([c, s, np.zeros(A)], axis=1)                                        # (A, 3)
    pv = np.cross(d[None, :, :], e2[:, None, :])                                     # (F, A, 3)
    det = np.einsum("fk,fak->fa", e1, pv)
    ok_det = np.abs(det) > 1e-12
    inv = 1.0 / np.where(ok_det, det, 1.0)
    near, far = np.full((L, A), np.inf), np.zeros((L, A))
    doubt = np.zeros((L, A), dtype=bool)
    for l in range(L):
        o = np.array([0.0, 0.0, z0 - l * dz])
        tv = o - a0
        qv = np.cross(tv, e1)
        u = np.einsum("fk,fak->fa", tv, pv) * inv
        w = (qv @ d.T) * inv
        t = np.einsum("fk,fk->f", e2, qv)[:, None] * inv
        hit = ok_det & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 1e-9)
        tn, tf = np.where(hit, t, np.inf), np.where(hit, t, 0.0)
        near[l], far[l] = tn.min(axis=0), tf.max(axis=0)
        if margins:
            m = np.minimum(np.minimum(u, w), 1.0 - (u + w))
            weak = hit & ((m < 1e-6) | (np.abs(det) < 1e-6))
            i, j, cols = tn.argmin(axis=0), tf.argmax(axis=0), np.arange(A)
            second = ((hit & (np.abs(t - near[l]) <= 1e-6)).sum(axis=0) > 1) | ((hit & (np.abs(t - far[l]) <= 1e-6)).sum(axis=0) > 1)
            doubt[l] = np.isfinite(near[l]) & (weak[i, cols] | weak[j, cols] | second)
    return (near, far, doubt) if margins else (near, far)


def levels(near, far):
    """(L,) list of dicts with the fields of sh_canal_level"""
    A = near.shape[1]
    c, s = dirs(A)
    out = []
    for nr, fr in zip(near, far):
        nh = int(np.isfinite(nr).sum())
        if nh < A:
            out.append(dict(n_hit=nh, status=GEOMETRY, area=0.0))
            continue
        x, y = nr * c, nr * s
        xn, yn = np.roll(x, -1), np.roll(y, -1)
        cr = x * yn - y * xn
        out.append(dict(r_min=nr.min(), a_min=int(np.argmin(nr)), r_max=nr.max(), a_max=int(np.argmax(nr)), r_mean=nr.mean(),
                        area=0.5 * np.sin(2.0 * np.pi / A) * (nr * np.roll(nr, -1)).sum(),
                        centroid=np.array([((x + xn) * cr).sum(), ((y + yn) * cr).sum()]) / (3.0 * cr.sum()),
                        extent_x=np.array([x.min(), x.max()]), extent_y=np.array([y.min(), y.max()]), wall_min=(fr - nr).min(), n_hit=nh, status=0))
    return out


def stem_record(plane, T, near, lv, z0, dz, stem):
    """the fields of sh_stem_fit for one cut (plane: point, normal in CT), one stem (length, r_prox, r_tip) and a profile with its
    levels (dicts of levels(), or a structured array); the used levels by the header's own expression d_l = z_e - (z0 - l dz)"""
    L, A = near.shape
    c, s = dirs(A)
    R, t = T[:3, :3], T[:3, 3]
    of, un = R @ np.asarray(plane[:3], dtype=np.float64) + t, R @ np.asarray(plane[3:], dtype=np.float64)
    un = un / np.linalg.norm(un)
    if abs(un[2]) < 1e-12:
        return dict(status=GEOMETRY)
    ze = of[2] + (of[0] * un[0] + of[1] * un[1]) / un[2]
    length, rp, rt = (float(x) for x in stem)
    zl = z0 - np.arange(L) * dz
    if not (z0 >= ze and zl[-1] <= ze - length):
        return dict(status=ARG)
    d = ze - zl
    used = np.nonzero((d >= 0.0) & (d <= length))[0]
    r = rp + ((rt - rp) * d) / length
    rec = dict(status=0, z_entry=ze, entry=to_ct(T, [0.0, 0.0, ze]), n_samples=0, n_breach=0, n_open=0, min_clearance=0.0, depth=0.0, angle_index=-1,
               direction=np.zeros(3), scale_max=0.0, fill_mean=0.0, fill_max=0.0, fill_max_depth=0.0)
    best, fills = None, []
    for l in used:
        side = ((r[l] * c - of[0]) * un[0] + (r[l] * s - of[1]) * un[1]) + (zl[l] - of[2]) * un[2]
        cnt = side <= 0.0
        hit = cnt & np.isfinite(near[l])
        rec["n_samples"] += int(cnt.sum())
        rec["n_open"] += int((cnt & ~np.isfinite(near[l])).sum())
        cl = np.where(hit, near[l] - r[l], np.inf)
        rec["n_breach"] += int((cl < 0).sum())
        if hit.any():
            a = int(np.argmin(cl))
            if best is None or cl[a] < best[0]:
                best = (cl[a], l, a)
            sc = (np.where(hit, near[l], np.inf) / r[l]).min()
            rec["scale_max"] = sc if rec["scale_max"] == 0.0 else min(rec["scale_max"], sc)
        if lv[l]["status"] == 0 and lv[l]["area"] > 0:
            fills.append((np.pi * r[l] * r[l] / lv[l]["area"], d[l]))
    if best is not None:
        rec.update(min_clearance=best[0], depth=d[best[1]], angle_index=best[2], direction=np.array([c[best[2]], s[best[2]], 0.0]) @ R)
    if fills:
        f = np.array(fills)
        k = int(np.argmax(f[:, 0]))
        rec.update(fill_mean=f[:, 0].mean(), fill_max=f[k, 0], fill_max_depth=f[k, 1])
    rec["fits"] = int(rec["n_breach"] == 0 and rec["n_open"] == 0 and rec["n_samples"] > 0)
    return rec


def prism(n, radius, z_lo, z_hi, phase=0.0, reverse=False, caps=True):
    """closed prism over the regular n-gon (circumradius `radius`, first vertex at angle `phase`) about the z axis, in FRAME coordinates
    -> (verts float64 (2 n + 2, 3), faces int32): 2 n side faces, then 2 n cap faces as fans about the cap centres"""
    t = phase + np.arange(n) * (2.0 * np.pi / n)
    ring = np.c_[radius * np.cos(t), radius * np.sin(t)]
    if phase == 0.0:
        ring[0] = [radius, 0.0]
    v = np.concatenate([np.c_[ring, np.full(n, z_lo)], np.c_[ring, np.full(n, z_hi)], [[0, 0, z_lo], [0, 0, z_hi]]])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, j + n], [i, j + n, i + n]]
    if caps:
        for i in range(n):
            j = (i + 1) % n
            f += [[2 * n, j, i], [2 * n + 1, i + n, j + n]]
    f = np.asarray(f, dtype=np.int32)
    return v, (f[:, ::-1].copy() if reverse else f)


def tube(n, r_in, r_out, z_lo, z_hi, phase=0.0):
    """outer prism and reversed inner prism, both without caps (the rays never see them)"""
    vo, fo = prism(n, r_out, z_lo, z_hi, phase, caps=False)
    vi, fi = prism(n, r_in, z_lo, z_hi, phase, reverse=True, caps=False)
    return np.concatenate([vo, vi]), np.concatenate([fo, fi + len(vo)]).astype(np.int32)


def prism_near(n, radius, phase, A):
    """near of the regular n-gon prism about its own axis in closed form: apothem / cos(theta - theta_side), theta_side the direction
    of the middle of the side the ray leaves through; the circumradius for a ray through a vertex"""
    th = (2.0 * np.pi * np.arange(A)) / A
    k = np.floor((th - phase) / (2.0 * np.pi / n))
    mid = phase + (k + 0.5) * (2.0 * np.pi / n)
    return radius * np.cos(np.pi / n) / np.cos(th - mid)


def mesh_in_ct(T, v_frame, faces):
    return np.ascontiguousarray(to_ct(T, v_frame), np.float32), np.ascontiguousarray(faces, np.int32)


def build_shim(directory):
    """tests/hostcheck/stem_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library"""
    L = host_twin.build_shim("stem", directory)
    d, vp, i = ctypes.c_double, ctypes.c_void_p, ctypes.c_int
    L.sc_hit.argtypes = [vp, vp, vp, vp]
    L.sc_radius.argtypes, L.sc_radius.restype = [d] * 4, d
    L.sc_ranges.argtypes, L.sc_ranges.restype = [vp, d, d, i, i, vp], None
    L.sc_profile.argtypes, L.sc_profile.restype = [vp, vp, i, vp, d, d, i, i, i, vp, vp], ctypes.c_longlong
    L.sc_levels.argtypes, L.sc_levels.restype = [vp, vp, i, i, vp], None
    L.sc_stem.argtypes, L.sc_stem.restype = [vp, vp, vp, vp, d, d, i, i, vp, vp], None
    return L


def host_profile(S, verts, faces, T, z0, dz, L, A, cull=True):
    """near, far, levels (structured) through the host-compiled device source; also the number of (face, ray) tests made"""
    from shoulder_amd import _lib
    v, f, T = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32), np.ascontiguousarray(T, np.float64)
    near, far = np.empty((L, A)), np.empty((L, A))
    n = S.sc_profile(v.ctypes.data, f.ctypes.data, len(f), T.ctypes.data, z0, dz, L, A, int(cull), near.ctypes.data, far.ctypes.data)
    lv = np.zeros(L, dtype=_lib.CANAL_LEVEL_DTYPE)
    S.sc_levels(near.ctypes.data, far.ctypes.data, L, A, lv.ctypes.data)
    return near, far, lv, int(n)


def host_stem(S, plane, T, near, lv, z0, dz, stem):
    from shoulder_amd import _lib
    pl, T, near = np.ascontiguousarray(plane, np.float64), np.ascontiguousarray(T, np.float64), np.ascontiguousarray(near, np.float64)
    st, out = np.ascontiguousarray(stem, np.float64), np.zeros(1, dtype=_lib.STEM_FIT_DTYPE)
    lv = np.ascontiguousarray(lv)
    S.sc_stem(pl.ctypes.data, T.ctypes.data, near.ctypes.data, lv.ctypes.data, z0, dz, near.shape[0], near.shape[1], st.ctypes.data, out.ctypes.data)
    return out[0]
