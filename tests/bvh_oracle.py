"""NumPy statement of the face hierarchy of sh_mesh_bvh (include/shoulder_hip.h "a face hierarchy of the resident batch"; the rules are
shoulder_amd/csrc/sh_scalar.h bvh_*): which faces are loose, the box of the tight ones, the cell and the 30-bit code of every tight
face, the order by (code, face id), the corners in that order, the implicit tree of float32 boxes level by level and the row of
"bvh.off".  float32 minima and maxima in the total order of topo_enc (-0 below +0), one float64 quantisation, integers: NumPy gives the
bytes the host twin (tests/hostcheck/bvh_check.cpp) and the device give.  LEAF and WIDTH are read from the header.  Also the ctypes
side of the twin."""
import ctypes
import os
import re

import numpy as np

import host_twin
from conftest import ROOT

ARG, STATE, NOMEM, GEOMETRY = -1, -3, -6, -5
OFF_WORDS, OFF_LEVEL = 32, 8
MAX_FACES = 0x7FFFFFFF // 3      # the faces of the largest mesh an upload admits


def _header_constant(name):
    src = open(os.path.join(ROOT, "shoulder_amd", "csrc", "sh_scalar.h")).read()
    return int(re.search(r"^#define\s+" + name + r"\s+(\d+)", src, flags=re.M).group(1))


LEAF, WIDTH = _header_constant("SH_BVH_LEAF"), _header_constant("SH_BVH_WIDTH")


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def enc(x):
    """topo_enc: float32 -> uint32 in the floats' order, -0 below +0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dec(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def loose_faces(verts, faces):
    """bvh_loose: !(g >= 2^-7), g = |ab x ac|^2 / Lmax^3 on the widened edges -> bool (F,)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    A = v[faces[:, 0]]
    ab, ac = v[faces[:, 1]] - A, v[faces[:, 2]] - A
    bc = ac - ab
    n = cross3(ab, ac)
    l2 = np.maximum(dot3(ab, ab), np.maximum(dot3(ac, ac), dot3(bc, bc)))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = dot3(n, n) / (l2 * np.sqrt(l2))
        return ~(g >= 2.0 ** -7)


def levels_of(tight):
    if tight <= 0:
        return 0
    n, k = -(-tight // LEAF), 1
    while n > 1:
        n, k = -(-n // WIDTH), k + 1
    return k


def nodes_of(tight):
    if tight <= 0:
        return 0
    n = -(-tight // LEAF)
    total = n
    while n > 1:
        n = -(-n // WIDTH)
        total += n
    return total


MAX_LEVELS = levels_of(MAX_FACES)
STACK = MAX_LEVELS * (WIDTH - 1) + 1


def off_row(tight, loose, base):
    """bvh_off_row -> int32 (32,)"""
    row = np.zeros(OFF_WORDS, np.int32)
    n = -(-tight // LEAF) if tight > 0 else 0
    leaves, levels, nodes = n, 0, 0
    while n > 0:
        row[OFF_LEVEL + levels] = nodes
        nodes += n
        levels += 1
        if n == 1:
            break
        n = -(-n // WIDTH)
    row[OFF_LEVEL + levels] = nodes
    row[:6] = (tight, loose, leaves, levels, nodes, base)
    return row


def spread(v):
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    for shift, mask in ((16, 0x030000FF), (8, 0x0300F00F), (4, 0x030C30C3), (2, 0x09249249)):
        v = (v | (v << np.uint32(shift))) & np.uint32(mask)
    return v


def build(verts, faces, base=0):
    """the index of one mesh whose first node is `base` -> dict: order, loose (int32), off (32 int32), box ((nodes, 6) float32), tri
    ((tight, 9) float32), info (one record of _lib.BVH_INFO_DTYPE), code (uint32 per tight face of the order)"""
    from shoulder_amd import _lib
    v32 = np.ascontiguousarray(verts, np.float32)
    faces = np.ascontiguousarray(faces, np.int32)
    is_loose = loose_faces(v32, faces)
    ids = np.arange(len(faces), dtype=np.int32)
    tight, loose = ids[~is_loose], ids[is_loose]
    T = len(tight)
    info = np.zeros((), dtype=_lib.BVH_INFO_DTYPE)
    row = off_row(T, len(loose), base)
    info["tight"], info["loose"], info["leaves"], info["levels"], info["nodes"] = row[:5]
    if T == 0:
        return dict(order=tight, loose=loose, off=row, box=np.zeros((0, 6), np.float32), tri=np.zeros((0, 9), np.float32), info=info, code=np.zeros(0, np.uint32))
    e = enc(v32[faces[tight]].reshape(-1)).reshape(T, 3, 3)      # (face, corner, axis) as ordered words
    lo, hi = dec(e.min(axis=(0, 1))), dec(e.max(axis=(0, 1)))
    info["lo"], info["hi"] = lo, hi
    mn, mx = dec(e.min(axis=1)).astype(np.float64), dec(e.max(axis=1)).astype(np.float64)
    s = mn + mx
    ext = 2.0 * (hi.astype(np.float64) - lo.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(ext > 0.0, np.minimum(1023.0, np.floor(((s - 2.0 * lo.astype(np.float64)) / ext) * 1024.0)), 0.0).astype(np.int64)
    code = spread(q[:, 0]) | (spread(q[:, 1]) << np.uint32(1)) | (spread(q[:, 2]) << np.uint32(2))
    perm = np.lexsort((tight, code))
    order, code = tight[perm], code[perm]
    tri = np.ascontiguousarray(v32[faces[order]].reshape(T, 9))
    eo = e[perm]
    starts = np.arange(0, T, LEAF)
    blo, bhi = np.minimum.reduceat(eo.min(axis=1), starts, axis=0), np.maximum.reduceat(eo.max(axis=1), starts, axis=0)
    los, his = [blo], [bhi]
    while len(los[-1]) > 1:
        starts = np.arange(0, len(los[-1]), WIDTH)
        los.append(np.minimum.reduceat(los[-1], starts, axis=0))
        his.append(np.maximum.reduceat(his[-1], starts, axis=0))
    box = np.concatenate([np.concatenate([dec(a), dec(b)], axis=1) for a, b in zip(los, his)]).astype(np.float32)
    assert len(box) == row[4] and len(los) == row[3]
    return dict(order=order, loose=loose, off=row, box=np.ascontiguousarray(box), tri=tri, info=info, code=code)


def bases(face_counts):
    """the first node of every mesh of a batch and, behind the last, the nodes the batch has room for"""
    out = [0]
    for nf in face_counts:
        out.append(out[-1] + nodes_of(int(nf)))
    return out


def same_index(got, want):
    """two indices (dicts of build / Engine.bvh) byte for byte -> the name of the first array that differs, or None"""
    for k in ("order", "loose", "off", "box", "tri"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            return k
    return None


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
def build_shim(directory, sanitize=False):
    """tests/hostcheck/bvh_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library; sanitize=True: the
    stand-alone program with -fsanitize=address,undefined instead -> its path (it is run as a program, never loaded)"""
    L = host_twin.build_shim("bvh", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, ll, d, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float
    L.bc_consts.argtypes, L.bc_consts.restype = [vp], None
    L.bc_max_faces.argtypes, L.bc_max_faces.restype = [], ll
    L.bc_levels_of.argtypes = [ll]
    L.bc_nodes_of.argtypes, L.bc_nodes_of.restype = [ll], ll
    L.bc_off_row.argtypes, L.bc_off_row.restype = [i, i, i, vp], None
    L.bc_loose.argtypes = [vp]
    L.bc_code.argtypes, L.bc_code.restype = [i, i, i], ctypes.c_uint
    L.bc_quant.argtypes = [f, f, f, f]
    L.bc_box_skip.argtypes = [vp, vp, d]
    L.bc_plan.argtypes = [i, vp, vp, vp, vp]
    L.bc_precheck.argtypes = [i, i, i]
    L.bc_precheck_accel.argtypes = [i, i]
    L.bc_build.argtypes, L.bc_build.restype = [vp, vp, i, i, vp, vp, vp, vp, vp, vp], None
    L.bc_walk.argtypes = [vp] * 10
    return L


def host_build(S, verts, faces, base=0):
    """the twin's index of one mesh -> the dict of build()"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    nf = len(f)
    order, loose, off = np.full(nf, -7, np.int32), np.full(nf, -7, np.int32), np.zeros(OFF_WORDS, np.int32)
    box, tri = np.zeros((nodes_of(nf) + 1, 6), np.float32), np.zeros((nf, 9), np.float32)
    info = np.zeros(1, dtype=_lib.BVH_INFO_DTYPE)
    S.bc_build(v.ctypes.data, f.ctypes.data, nf, base, order.ctypes.data, loose.ctypes.data, off.ctypes.data, box.ctypes.data, tri.ctypes.data, info.ctypes.data)
    t, nl, nodes = int(off[0]), int(off[1]), int(off[4])
    assert (order[t:] == -1).all() and (loose[nl:] == -1).all()
    return dict(order=order[:t].copy(), loose=loose[:nl].copy(), off=off, box=box[:nodes].copy(), tri=tri[:t].copy(), info=info[0])


def host_walk(S, verts, faces, index, points):
    """the points against one mesh through the twin's k_cp_tree and k_cp_join -> ((Q,) records, (Q, 4) counts: nodes popped, faces
    tested in the tree, loose faces tested, the deepest stack)"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    arr = {k: np.ascontiguousarray(index[k]) for k in ("order", "loose", "off", "box", "tri")}
    pad = {k: (a if a.size else np.zeros(8, a.dtype)) for k, a in arr.items()}      # (an empty array has no address worth passing)
    out = np.zeros(len(pts), dtype=_lib.CLOSEST_DTYPE)
    counts = np.zeros((len(pts), 4), np.int64)
    for i in range(len(pts)):
        rc = S.bc_walk(v.ctypes.data, f.ctypes.data, pad["order"].ctypes.data, pad["loose"].ctypes.data, pad["off"].ctypes.data, pad["box"].ctypes.data,
                       pad["tri"].ctypes.data, pts[i].ctypes.data, out[i:i + 1].ctypes.data, counts[i].ctypes.data)
        assert rc == 0, "the stack went beyond SH_BVH_STACK"
    return out, counts


# ---- the meshes and the points of the tests --------------------------------------------------------------------------------------------
def point_classes(verts, faces, n_each=64, far=8, seed=0, with_overflow=True):
    """the query points of the walk tests about one mesh: n_each exactly on vertices, n_each on edge midpoints, n_each inside (toward
    the centroid), points up to 50 mm outside, `far` points 2e4 mm away and one at 1e200 -> float64 (Q, 3) with Q = 512 for the defaults"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces)
    on = v[rng.integers(0, len(v), n_each)]
    fe = f[rng.integers(0, len(f), n_each)]
    mid = 0.5 * (v[fe[:, 0]] + v[fe[:, 1]])
    c = v.mean(axis=0)
    inside = c + (v[rng.integers(0, len(v), n_each)] - c) * rng.uniform(0.0, 0.9, size=(n_each, 1))
    n_out = 512 - 3 * n_each - far - (1 if with_overflow else 0) if n_each == 64 else n_each
    d = rng.normal(size=(n_out, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    outside = v[rng.integers(0, len(v), n_out)] + d * rng.uniform(0.0, 50.0, size=(n_out, 1))
    d = rng.normal(size=(far, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    parts = [on, mid, inside, outside, c + d * 2e4]
    if with_overflow:
        parts.append(np.array([[1e200, 0.0, 0.0]]))
    return np.ascontiguousarray(np.concatenate(parts))
