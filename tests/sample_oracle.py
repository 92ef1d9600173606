"""NumPy statement of sh_sample_surface (include/shoulder_hip.h "surface samples of the resident batch"): the face areas, the
sequential cumulative areas in blocks of 256, the SplitMix64 counter words in uint64 arithmetic, the face by searchsorted(side="right"),
the point, and the thinning as the sequential greedy loop AND as Jacobi rounds over the neighbour lists (the rounds are part of the
record).  Written operation by operation in the order of sh_scalar.h (samp_*), on float64, so that it gives the bytes the host-compiled
statement gives (tests/hostcheck/sample_check.cpp, -ffp-contract=off) and the device can give: + - x sqrt, all correctly rounded.
Also the ctypes side of the host twin."""
import ctypes
import math

import numpy as np

import host_twin
from ray_oracle import cross3, dot3, widen

ARG, STATE, CAPACITY, GEOMETRY = -1, -3, -4, -5
BLOCK, SAMPLE_MAX, THIN_MAX, MAX_ROUNDS, HEAD = 256, 1048576, 65536, 32, 64
GAMMA, M1, M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
KNOWN_SEED, KNOWN_WORDS = 1234567, [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
FMAX = 1.7976931348623157e308


def words(seed, n):
    """w(seed, n) for an array of counters n, mod 2^64"""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + (np.asarray(n, dtype=np.uint64) + np.uint64(1)) * GAMMA
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def unit(w):
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def area2(verts, faces):
    v, faces = widen(verts), np.asarray(faces).reshape(-1, 3)
    A, B, C = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = cross3(B - A, C - A)
    return np.sqrt(dot3(n, n))


def cdf_of(a2):
    """the cumulative areas: a Python loop in index order within each block of 256, the bases in block order"""
    a2 = [float(x) for x in a2]
    cdf, base = [], 0.0
    for b0 in range(0, len(a2), BLOCK):
        s, blk = 0.0, []
        for i, x in enumerate(a2[b0:b0 + BLOCK]):
            s = x if i == 0 else s + x
            blk.append(s)
        cdf.extend(base + x for x in blk)
        base = base + blk[-1]
    return np.array(cdf, dtype=np.float64)


def neighbours(points, radius):
    """for every j the indices i < j with d2(i, j) < radius * radius, d2 = (dx dx + dy dy) + dz dz"""
    r2 = float(radius) * float(radius)
    out = []
    for j in range(len(points)):
        d = points[j] - points[:j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out.append(np.nonzero(d2 < r2)[0])
    return out


def greedy(nbrs):
    """the definition: keep_j = 1 iff no lower neighbour is kept, in index order"""
    keep = np.zeros(len(nbrs), dtype=np.int32)
    for j, nb in enumerate(nbrs):
        keep[j] = 0 if keep[nb].any() else 1
    return keep


def jacobi(nbrs, max_rounds):
    """the rounds of the device -> (states: 1 kept, 0 removed, -1 undecided; rounds; status)"""
    st = np.full(len(nbrs), -1, dtype=np.int32)
    rounds = 0
    while (st == -1).any():
        if rounds == max_rounds:
            return st, rounds, CAPACITY
        new = st.copy()
        for j in np.nonzero(st == -1)[0]:
            s = st[nbrs[j]]
            if (s == 1).any():
                new[j] = 0
            elif not (s == -1).any():
                new[j] = 1
        st, rounds = new, rounds + 1
    return st, rounds, 0


def thin(points, radius, max_rounds=MAX_ROUNDS):
    """-> (keep, kept, rounds, status) of the points under the thinning; where the rounds finish the set is the greedy one"""
    nbrs = neighbours(np.asarray(points, np.float64), radius)
    st, rounds, status = jacobi(nbrs, max_rounds)
    if status == 0:
        assert np.array_equal(st, greedy(nbrs))
    return st, int((st == 1).sum()), rounds, status


def sample(verts, faces, N, seed, radius=0.0, max_rounds=MAX_ROUNDS):
    """one humerus -> (records (N,) of _lib.SAMPLE_DTYPE, info record of _lib.SAMPLE_INFO_DTYPE, cdf (nf,))"""
    from shoulder_amd import _lib
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    rec, info = np.zeros(N, dtype=_lib.SAMPLE_DTYPE), np.zeros((), dtype=_lib.SAMPLE_INFO_DTYPE)
    cdf = cdf_of(area2(verts, faces))
    total = float(cdf[-1]) if len(cdf) else 0.0
    if len(cdf) == 0 or total == 0.0 or not abs(total) <= FMAX:
        info["status"] = GEOMETRY
        return rec, info, cdf
    info["area"] = total / 2.0
    j = np.arange(N, dtype=np.uint64)
    target = unit(words(seed, np.uint64(3) * j)) * total
    face = np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1)
    r1, r2 = unit(words(seed, np.uint64(3) * j + np.uint64(1))), unit(words(seed, np.uint64(3) * j + np.uint64(2)))
    fold = r1 + r2 > 1.0
    r1, r2 = np.where(fold, 1.0 - r1, r1), np.where(fold, 1.0 - r2, r2)
    v = widen(verts)
    A, B, C = v[faces[face, 0]], v[faces[face, 1]], v[faces[face, 2]]
    rec["point"] = A + (r1[:, None] * (B - A) + r2[:, None] * (C - A))
    rec["u"], rec["v"], rec["face"], rec["keep"] = r1, r2, face, 1
    info["kept"] = N
    if radius > 0.0:
        rec["keep"], info["kept"], info["rounds"], info["status"] = thin(rec["point"], radius, max_rounds)
    return rec, info, cdf


def zero_area_mesh(verts, faces, where):
    """the faces with faces of zero area (a corner repeated) put in front of the given positions of the result"""
    faces = [tuple(int(x) for x in f) for f in np.asarray(faces).reshape(-1, 3)]
    out, k = [], 0
    for pos in range(len(faces) + len(where)):
        if pos in where:
            f = faces[min(k, len(faces) - 1)]
            out.append((f[0], f[1], f[1]))
        else:
            out.append(faces[k])
            k += 1
    return np.ascontiguousarray(verts, np.float32), np.array(out, dtype=np.int32)


# ---- the ctypes side of the host twin (tests/hostcheck/sample_check.cpp) -------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("sample", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, d, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    L.sc_words.argtypes, L.sc_words.restype = [u64, u64, i, vp], None
    L.sc_unit.argtypes, L.sc_unit.restype = [u64], d
    L.sc_sample.argtypes, L.sc_sample.restype = [vp, i, vp, i, i, u64, d, i, vp, vp, vp], None
    L.sc_thin.argtypes, L.sc_thin.restype = [vp, i, d, i, vp, vp], None
    L.sc_precheck.argtypes = [i, i, i, i, d, i, i, i, i, vp, i]
    L.sc_plan.argtypes, L.sc_plan.restype = [i, i, i, ctypes.c_longlong, ctypes.c_longlong, vp], None
    return L


def host_sample(shim, verts, faces, N, seed, radius=0.0, max_rounds=MAX_ROUNDS):
    """the host twin of the kernels for one humerus -> (records, info record, cdf)"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    rec, info, cdf = np.zeros(N, dtype=_lib.SAMPLE_DTYPE), np.zeros(1, dtype=_lib.SAMPLE_INFO_DTYPE), np.zeros(max(len(f), 1))
    shim.sc_sample(v.ctypes.data, len(v), f.ctypes.data, len(f), N, int(seed), float(radius), int(max_rounds), cdf.ctypes.data, rec.ctypes.data, info.ctypes.data)
    return rec, info[0], cdf[:len(f)]


def host_thin(shim, points, radius, max_rounds=MAX_ROUNDS):
    """the rounds of the host twin on given points -> (keep, kept, rounds, status)"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    keep, res = np.zeros(len(p), dtype=np.int32), np.zeros(3, dtype=np.int32)
    shim.sc_thin(p.ctypes.data, len(p), float(radius), int(max_rounds), keep.ctypes.data, res.ctypes.data)
    return keep, int(res[0]), int(res[1]), int(res[2])
