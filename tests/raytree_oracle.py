"""NumPy statements about the rays through the face hierarchy (include/shoulder_hip.h sh_ray_nearest, sh_ray_cast with SH_ACCEL_BVH;
k_raytree.h): the nearest hit and the thickness, both built on ray_oracle.cast -- every ray against every face, no tree, no cull --, the
skip rule of a node (sh_scalar.h bvh_ray_box_skip) restated operation by operation, the rays of the tests, and the ctypes side of
tests/hostcheck/raytree_check.cpp."""
import ctypes

import numpy as np

import host_twin
import ray_oracle as O

ARG, STATE = -1, -3
RAY_CHUNK, TREE_CHUNK = 256, 64      # SH_RAY_CHUNK, SH_BVH_CHUNK
GUARD2 = 2.0 ** 40
N_ADVERSARIAL = 320                  # the rays of adversarial_rays with n = 16


def nearest(verts, faces, origins, directions):
    """(R,) of _lib.RAY_HIT_DTYPE: row 0 of every ray's hits in the order (t, face); a miss is zero with face = -1"""
    return np.ascontiguousarray(O.cast(verts, faces, origins, directions, 1)[0][:, 0])


def unit_normals(normals):
    n = np.asarray(normals, np.float64)
    return n / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])[..., None]


def thickness(verts, faces, points, normals, offset=1e-3):
    """-> (thickness (N,), opposite point (N, 3), opposite face (N,)): one ray per point from p - offset n along -n, n the unit outward
    normal; thickness = offset + t of the nearest hit, inf and face -1 without one"""
    p, n = np.asarray(points, np.float64).reshape(-1, 3), unit_normals(normals).reshape(-1, 3)
    hit = nearest(verts, faces, p - offset * n, -n)
    return np.where(hit["face"] < 0, np.inf, offset + hit["t"]), hit["point"].copy(), hit["face"].copy()


def box_skip(o, d, bx, tbest=np.inf):
    """sh_scalar.h bvh_ray_box_skip in float64 NumPy scalars, operation by operation -> (skip, tn)"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    bx = np.asarray(bx, np.float32).astype(np.float64)
    lo, hi = bx[:3], bx[3:]
    with np.errstate(all="ignore"):
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        dl = np.sqrt(dd)
        df = np.maximum(np.abs(lo - o), np.abs(o - hi))
        ex = hi - lo
        m1 = np.float64(0.0)
        for k in range(3):
            m1 = m1 + max(abs(lo[k]), abs(hi[k]))
        far2, ext2 = (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2], (ex[0] * ex[0] + ex[1] * ex[1]) + ex[2] * ex[2]
        if not (dd <= GUARD2 and far2 <= GUARD2):
            return False, 0.0
        pad = (2.0 ** -8 * dl) * (np.sqrt(far2) * ext2) + m1 * 2.0 ** -40
        tn, tf, beside = np.float64(0.0), np.float64(np.inf), False
        for k in range(3):
            l, h = lo[k] - pad, hi[k] + pad
            inv = np.float64(1.0) / d[k]
            if d[k] == 0.0:
                beside = beside or bool(o[k] < l or o[k] > h)
            elif abs(inv) < np.inf:
                t1, t2 = (l - o[k]) * inv, (h - o[k]) * inv
                tn, tf = max(tn, min(t1, t2)), min(tf, max(t1, t2))
        if beside or tn > tf + abs(tf) * 2.0 ** -40:
            return True, float(tn)
        return bool((tn - pad * (np.float64(1.0) / dl)) * (1.0 - 2.0 ** -40) > tbest), float(tn)


# ---- the rays of the tests -----------------------------------------------------------------------------------------------------------
def _unit(x):
    with np.errstate(all="ignore"):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)


def adversarial_rays(verts, faces, index, seed=0, n=16):
    """The rays the skip rule is written for, about one mesh and its index (the dict of bvh_oracle.build / host_build) -> (o, d, names):
    from a vertex through another vertex; along an edge (in the plane of its faces: det = 0 there); through edge midpoints; along the
    axes with two and with one zero component; an origin coordinate equal to a node box's lo or hi with the direction in that face of the
    box; grazing (a face's in-plane direction + 1e-9 x its normal); |d| of 1e-6 and 1e6; origins 2e4 mm and 1e6 mm away; an origin on a
    face.  A class the mesh cannot give (no nodes, no area) is filled with rays along z."""
    rng = np.random.default_rng(seed)
    v = O.widen(verts)
    f = np.asarray(faces)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = 0.5 * (lo + hi), (hi - lo) + 1.0
    fi = rng.integers(0, len(f), n)
    A, Bc, C = v[f[fi, 0]], v[f[fi, 1]], v[f[fi, 2]]
    nrm = _unit(np.cross(Bc - A, C - A))
    cen = (A + Bc + C) / 3.0
    out_o, out_d, names = [], [], []

    def add(name, o, d):
        o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
        out_o.append(o.reshape(-1, 3)); out_d.append(d.reshape(-1, 3)); names.extend([name] * len(o.reshape(-1, 3)))

    i, j = rng.integers(0, len(v), n), rng.integers(0, len(v), n)
    add("vertex to vertex", v[i], v[j] - v[i])
    add("outside through two vertices", v[i] - 0.5 * (v[j] - v[i]), v[j] - v[i])
    add("along an edge", A - 0.5 * (Bc - A), Bc - A)
    far = c + 3.0 * ext * _unit(rng.normal(size=(n, 3)))
    add("through an edge midpoint", far, 0.5 * (A + Bc) - far)
    inside = c + rng.uniform(-0.6, 0.6, size=(2 * n, 3)) * ext
    axes = np.eye(3)[rng.integers(0, 3, 2 * n)] * rng.choice([-1.0, 1.0, 2.5, -0.125], size=(2 * n, 1))
    add("two zero components", inside, axes)
    one = rng.normal(size=(2 * n, 3))
    one[np.arange(2 * n), rng.integers(0, 3, 2 * n)] = 0.0
    add("one zero component", np.concatenate([cen, inside[:n]]), one)
    box = np.asarray(index["box"], np.float32).astype(np.float64).reshape(-1, 6)
    if len(box):
        bi = np.concatenate([rng.integers(0, len(box), 2 * n - 4), np.arange(len(box) - 4, len(box)) % len(box)])      # the top of the tree among them
        ax, side = rng.integers(0, 3, 2 * n), rng.integers(0, 2, 2 * n)
        bo = 0.5 * (box[bi, :3] + box[bi, 3:])
        bd = rng.normal(size=(2 * n, 3))
        bo[np.arange(2 * n), ax] = box[bi, 3 * side + ax]
        bd[np.arange(2 * n), ax] = 0.0
        add("in a face plane of a node box", bo - 3.0 * bd, bd)
    else:
        add("in a face plane of a node box", np.tile(c - (0, 0, 50.0), (2 * n, 1)), (0.0, 0.0, 1.0))
    u = _unit(Bc - A)
    add("grazing", cen - 5.0 * (u + 1e-9 * nrm), u + 1e-9 * nrm)
    add("grazing from the other side", cen - 5.0 * (u - 1e-9 * nrm), u - 1e-9 * nrm)
    rd = rng.normal(size=(2 * n, 3))
    add("|d| = 1e-6", inside, 1e-6 * _unit(rd))
    add("|d| = 1e6", inside, 1e6 * _unit(rd))
    w = _unit(rng.normal(size=(2 * n, 3)))
    add("origin 2e4 mm away", c + 2e4 * w[:n], v[i] - (c + 2e4 * w[:n]))
    add("origin 1e6 mm away", c + 1e6 * w[n:], -w[n:])
    add("origin on a face, inward", cen, -nrm)
    add("origin on a face, anywhere", cen, rng.normal(size=(n, 3)))
    o, d = np.concatenate(out_o), np.concatenate(out_d)
    bad = ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0.0).any(axis=1))
    o[bad], d[bad] = c - (0.0, 0.0, 50.0), (0.0, 0.0, 1.0)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), names


def random_rays(verts, R, seed):
    """R rays about one mesh: origins inside and outside (its box blown up by a half), directions anywhere"""
    rng = np.random.default_rng(seed)
    v = O.widen(verts)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, h = 0.5 * (lo + hi), 0.75 * (hi - lo) + 0.5
    return c + rng.uniform(-1.0, 1.0, size=(R, 3)) * h, rng.normal(size=(R, 3))


def rays_for(verts, faces, index, total, seed=0):
    """the adversarial set and random rays up to `total`"""
    ao, ad, names = adversarial_rays(verts, faces, index, seed)
    ro, rd = random_rays(verts, total - len(ao), seed + 1)
    return np.concatenate([ao, ro]), np.concatenate([ad, rd]), names + ["random"] * len(ro)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
def build_shim(directory, sanitize=False):
    """tests/hostcheck/raytree_check.cpp (which holds bvh_check.cpp's build) compiled as the device compiles it -> ctypes library;
    sanitize=True: the stand-alone program with -fsanitize=address,undefined instead -> its path (run as a program, never loaded)"""
    L = host_twin.build_shim("raytree", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, ll, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    L.bc_build.argtypes, L.bc_build.restype = [vp, vp, i, i, vp, vp, vp, vp, vp, vp], None
    L.rt_box_skip.argtypes = [vp, vp, vp, d, vp]
    L.rt_brute.argtypes, L.rt_brute.restype = [vp, vp, i, vp, i, i, vp, vp], None
    L.rt_cast.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp, vp, vp]
    L.rt_near.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp]
    L.rt_plan.argtypes, L.rt_plan.restype = [i, i, i, i, ll, i, i, i, vp], None
    L.rt_precheck_nearest.argtypes = [vp, i, i, i, i, i]
    return L


def _rays(o, d):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)], axis=1))


def _index_args(index):
    arr = {k: np.ascontiguousarray(index[k]) for k in ("order", "loose", "off", "box", "tri")}
    return {k: (a if a.size else np.zeros(8, a.dtype)) for k, a in arr.items()}      # (an empty array has no address worth passing)


def host_brute(S, verts, faces, o, d, cap):
    """the twin's walk over all faces -> (hits (R, cap), counts (R,))"""
    from shoulder_amd import _lib
    v, f, rays = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32), _rays(o, d)
    hits, counts = np.zeros((len(rays), cap), dtype=_lib.RAY_HIT_DTYPE), np.zeros(len(rays), np.int32)
    S.rt_brute(v.ctypes.data, f.ctypes.data, len(f), rays.ctypes.data, len(rays), cap, hits.ctypes.data, counts.ctypes.data)
    return hits, counts


def host_cast(S, verts, faces, index, o, d, cap):
    """the twin's count, fill and sort through the index -> (hits (R, cap), counts (R,), totals: nodes popped, tree faces tested, loose
    faces tested, deepest stack)"""
    from shoulder_amd import _lib
    v, f, rays, a = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32), _rays(o, d), _index_args(index)
    hits, counts, tot = np.zeros((len(rays), cap), dtype=_lib.RAY_HIT_DTYPE), np.zeros(len(rays), np.int32), np.zeros(4, np.int64)
    rc = S.rt_cast(v.ctypes.data, f.ctypes.data, a["order"].ctypes.data, a["loose"].ctypes.data, a["off"].ctypes.data, a["box"].ctypes.data, a["tri"].ctypes.data,
                   rays.ctypes.data, len(rays), cap, hits.ctypes.data, counts.ctypes.data, tot.ctypes.data)
    assert rc == 0, "the stack went beyond SH_BVH_STACK" if rc == -1 else "count and fill disagree"
    return hits, counts, tot


def host_near(S, verts, faces, index, o, d):
    """the twin's k_ray_near -> ((R,) records, totals as host_cast's)"""
    from shoulder_amd import _lib
    v, f, rays, a = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32), _rays(o, d), _index_args(index)
    out, tot = np.zeros(len(rays), dtype=_lib.RAY_HIT_DTYPE), np.zeros(4, np.int64)
    rc = S.rt_near(v.ctypes.data, f.ctypes.data, a["order"].ctypes.data, a["loose"].ctypes.data, a["off"].ctypes.data, a["box"].ctypes.data, a["tri"].ctypes.data,
                   rays.ctypes.data, len(rays), out.ctypes.data, tot.ctypes.data)
    assert rc == 0, "the stack went beyond SH_BVH_STACK"
    return out, tot


def host_plan(S, B_, R, per, cap, maxF, with_status=False, tree=False, near=False):
    out = np.zeros(11, np.int64)
    S.rt_plan(B_, R, int(per), cap, maxF, int(with_status), int(tree), int(near), out.ctypes.data)
    return dict(zip(("tmax", "chunks", "n", "rays", "counts", "offs", "cursor", "hits", "blockhit", "near", "status"), (int(x) for x in out)))
