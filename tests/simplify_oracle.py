"""NumPy statement of sh_mesh_simplify (include/shoulder_hip.h "simplification of the resident batch"): vertex clustering with quadric
placement, for one mesh.  Every float64 expression is written operation by operation in the header's order; where a sum has an order
(a vertex's quadric over its row, a cluster's sums over its members) it is a loop over the POSITION in that order, vectorised across
the rows or clusters: entry j of every row is added before entry j + 1.  The clusters come from np.unique and a stable argsort, the
duplicates from np.unique over the sorted triples -- deliberately not from the rows the device walks.  Also the test meshes and the
ctypes side of the host twin.  No test functions."""
import ctypes

import numpy as np

import host_twin
import mass_oracle as MO
import topo_oracle as TO

ARG, STATE, CAPACITY, GEOMETRY, NOMEM = -1, -3, -4, -5, -6
MEAN, QUADRIC = 0, 1
MAX_CELLS, MAX_CLUSTERS = 1 << 20, 1 << 21
NO_KEY = np.uint64(0xffffffffffffffff)
INFO_DTYPE = np.dtype([(n, "<i4") for n in ("status", "verts_used", "clusters", "verts_out", "faces_out", "faces_collapsed", "faces_duplicate", "fallbacks",
                                            "largest_cluster", "reserved")] + [("cell", "<f8"), ("max_move", "<f8"), ("pad", "<i4", (2,))])


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def solve(q, m, o, h, reg, clamp):
    """the placement of every cluster (rows of q, m, o) -> (x relative to o, solved): the header's Cholesky, term by term"""
    with np.errstate(all="ignore"):
        tr = (q[:, 0] + q[:, 3]) + q[:, 5]
        bad = (tr == 0.0) | ~np.isfinite(tr)
        lam = reg * tr
        m00, m11, m22 = q[:, 0] + lam, q[:, 3] + lam, q[:, 5] + lam
        r0, r1, r2 = lam * (m[:, 0] - o[:, 0]) - q[:, 6], lam * (m[:, 1] - o[:, 1]) - q[:, 7], lam * (m[:, 2] - o[:, 2]) - q[:, 8]
        bad |= ~(m00 > 0.0) | ~np.isfinite(m00)
        l00 = np.sqrt(m00)
        l10, l20 = q[:, 1] / l00, q[:, 2] / l00
        p1 = m11 - l10 * l10
        bad |= ~(p1 > 0.0) | ~np.isfinite(p1)
        l11 = np.sqrt(p1)
        l21 = (q[:, 4] - l20 * l10) / l11
        p2 = (m22 - l20 * l20) - l21 * l21
        bad |= ~(p2 > 0.0) | ~np.isfinite(p2)
        l22 = np.sqrt(p2)
        y0 = r0 / l00
        y1 = (r1 - l10 * y0) / l11
        y2 = ((r2 - l20 * y0) - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = ((y0 - l10 * x1) - l20 * x2) / l00
        x = np.stack([x0, x1, x2], axis=1)
        lim = (0.5 * h) * clamp
        bad |= (~np.isfinite(x)).any(axis=1) | (np.abs(x) > lim).any(axis=1)
    return x, ~bad


def simplify(verts, faces, cell, place=QUADRIC, reg=1e-3, clamp=1.0):
    """-> dict: info (a record of INFO_DTYPE), verts (verts_out, 3) float32, faces (faces_out, 3) int32, map (V,) int32, and what the
    host twin is also held to: key (V,) uint64, cid (V,) int32, quad (V, 10), pos (clusters, 3) float32"""
    v32 = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, h = len(v32), float(cell)
    info = np.zeros(1, dtype=INFO_DTYPE)[0]
    info["cell"] = h
    out = dict(info=info, verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), map=np.full(nv, -1, np.int32), key=np.full(nv, NO_KEY, np.uint64),
               cid=np.full(nv, -1, np.int32), quad=np.zeros((nv, 10)), pos=np.zeros((0, 3), np.float32))
    good = np.nonzero(~TO.degenerate(f))[0]
    used = np.zeros(nv, bool)
    used[f[good].ravel()] = True
    uv = np.nonzero(used)[0]
    info["verts_used"] = len(uv)
    if len(uv) == 0:
        info["status"] = GEOMETRY
        return out
    x = v32.astype(np.float64)
    lo, hi = v32[uv].min(axis=0).astype(np.float64), v32[uv].max(axis=0).astype(np.float64)
    with np.errstate(all="ignore"):
        cells = np.floor((hi - lo) / h)
    if not ((cells >= 0.0) & (cells < float(MAX_CELLS))).all():
        info["status"] = CAPACITY
        return out
    n = cells.astype(np.int64) + 1
    idx = np.minimum(np.floor((x[uv] - lo) / h).astype(np.int64), n - 1)
    key = (idx[:, 2] * n[1] + idx[:, 1]) * n[0] + idx[:, 0]
    ukeys, cid_u = np.unique(key, return_inverse=True)
    C = len(ukeys)
    info["clusters"] = C
    if C > MAX_CLUSTERS:
        info["status"] = CAPACITY
        return out
    out["key"][uv] = key.astype(np.uint64)
    cid = out["cid"]
    cid[uv] = cid_u
    o_u = lo + (idx.astype(np.float64) + 0.5) * h              # the centre of the cell of every used vertex
    o_v = np.zeros((nv, 3))
    o_v[uv] = o_u
    # the quadric of every used vertex over its row, in row order
    vrow, vface = TO.incidence(f, nv)
    length = np.diff(vrow)
    Q = out["quad"]
    for j in range(int(length.max())):
        sel = np.nonzero(length > j)[0]
        g = vface[vrow[sel] + j]
        A, B, Cc = x[f[g, 0]], x[f[g, 1]], x[f[g, 2]]
        nrm = _cross3(B - A, Cc - A)
        d = -_dot3(nrm, A - o_v[sel])
        terms = (nrm[:, 0] * nrm[:, 0], nrm[:, 0] * nrm[:, 1], nrm[:, 0] * nrm[:, 2], nrm[:, 1] * nrm[:, 1], nrm[:, 1] * nrm[:, 2], nrm[:, 2] * nrm[:, 2],
                 nrm[:, 0] * d, nrm[:, 1] * d, nrm[:, 2] * d, d * d)
        for k, t in enumerate(terms):
            Q[sel, k] = Q[sel, k] + t
    # the sums of every cluster over its members, ascending by vertex index
    order = uv[np.argsort(cid_u, kind="stable")]
    count = np.bincount(cid_u, minlength=C)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    S, QC = np.zeros((C, 3)), np.zeros((C, 10))
    for j in range(int(count.max())):
        sel = np.nonzero(count > j)[0]
        v = order[start[sel] + j]
        S[sel] = S[sel] + x[v]
        QC[sel] = QC[sel] + Q[v]
    m = S / count.astype(np.float64)[:, None]
    o_c = np.zeros((C, 3))
    o_c[cid_u] = o_u                                            # (one value per cluster: its members share the cell)
    pos = m.astype(np.float32)
    if place == QUADRIC:
        xs, solved = solve(QC, m, o_c, h, reg, clamp)
        with np.errstate(all="ignore"):
            pos = np.where(solved[:, None], (o_c + xs).astype(np.float32), pos)
        info["fallbacks"] = int((~solved).sum())
    out["pos"] = pos
    info["largest_cluster"] = int(count.max())
    # the faces
    tri = cid[f[good]]
    collapsed = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    info["faces_collapsed"] = int(collapsed.sum())
    rest = good[~collapsed]
    _, first = np.unique(np.sort(tri[~collapsed], axis=1), axis=0, return_index=True) if len(rest) else (None, np.zeros(0, np.int64))
    kept = rest[np.sort(first)]
    info["faces_duplicate"] = len(rest) - len(kept)
    named = np.unique(cid[f[kept]].ravel()) if len(kept) else np.zeros(0, np.int64)
    number = np.full(C, -1, np.int32)
    number[named] = np.arange(len(named), dtype=np.int32)
    out["faces"] = number[cid[f[kept]]].astype(np.int32).reshape(-1, 3)
    out["verts"] = np.ascontiguousarray(pos[named]).reshape(-1, 3)
    out["map"][uv] = number[cid_u]
    info["verts_out"], info["faces_out"] = len(named), len(kept)
    with np.errstate(all="ignore"):
        d = x[uv] - pos[cid_u].astype(np.float64)
        r = np.sqrt(_dot3(d, d))
    r = np.where(np.isnan(r), 0.0, r)
    info["max_move"] = float(r.max())
    if len(kept) == 0:
        info["status"] = GEOMETRY
    return out


def same_bytes(got, want, tag, names=("info", "verts", "faces", "map")):
    for n in names:
        a, b = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, n, a.shape, b.shape)


def volume(verts, faces):
    """the volume as sh_mass_properties states it (about the mesh's own reference point)"""
    return float(MO.mass(verts, faces)[0]["volume"]) if len(faces) else 0.0


def volume_about_origin(verts, faces):
    """the sum of the signed tetrahedra about the origin of the coordinates, as trimesh's mesh.volume: the figure of the issue's table.
    A clustered mesh may have border edges, and the volume of an open mesh depends on the point it is taken about."""
    a, b, c = (np.asarray(verts, np.float64)[np.asarray(faces)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum()) / 6.0


def edges_left(verts, faces):
    """-> (border edges, non-manifold edges, euler characteristic) of a result, by the topology oracle"""
    t = TO.topology(verts, faces)["info"]
    return int(t["border_edges"]), int(t["nonmanifold_edges"]), int(t["euler"])


# ---- test meshes ---------------------------------------------------------------------------------------------------------------------
def sheet(nx, ny, z=0.0, step=1.0):
    """a flat triangulated sheet of nx x ny squares in the plane z"""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([gx.ravel() * step, gy.ravel() * step, np.full(gx.size, z)], axis=1).astype(np.float32)
    i = (gx[:-1, :-1] * (ny + 1) + gy[:-1, :-1]).ravel()
    a, b, c, d = i, i + (ny + 1), i + (ny + 1) + 1, i + 1
    f = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    return v, f


def two_sheets(nx=8, ny=8, gap=0.5):
    """two parallel sheets `gap` apart, their faces interleaved: face 2 k of the first, face 2 k + 1 its twin on the second"""
    v, f = sheet(nx, ny, 0.25)
    w = v.copy()
    w[:, 2] += np.float32(gap)
    faces = np.stack([f, f + len(v)], axis=1).reshape(-1, 3).astype(np.int32)
    return np.concatenate([v, w]).astype(np.float32), faces


def strip_of(nf):
    """a wavy sheet cut to exactly nf faces"""
    v, f = sheet(16, (nf + 31) // 32 + 1)
    v = v.copy()
    v[:, 2] = (np.sin(v[:, 0] * 0.7) + np.cos(v[:, 1] * 0.9)).astype(np.float32)
    return v, np.ascontiguousarray(f[:nf])


def awkward(box):
    """a box with unused vertices in front, behind and far outside, degenerate faces (repeated indices) and zero-area faces (three
    different vertices on a line, two of them at one position)"""
    bv, bf = box
    far = np.array([[1e4, 1e4, 1e4], [-1e4, 0, 0]], np.float32)
    v = np.concatenate([far[:1], bv, far[1:], bv[:1], (bv[:1] + bv[1:2]) * np.float32(0.5)]).astype(np.float32)
    f = bf + 1
    dup, mid = len(bv) + 2, len(bv) + 3                        # a copy of box vertex 0; the midpoint of box vertices 0 and 1
    extra = np.array([[1, 1, 2], [3, 4, 3], [1, 2, mid], [1, dup, 2]], np.int32)
    return v, np.concatenate([extra[:2], f, extra[2:]]).astype(np.int32)


# ---- the ctypes side of the host twin --------------------------------------------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("simplify", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.sc_simplify.argtypes, L.sc_simplify.restype = [vp, i, vp, i, vp, vp, d, i, d, d, vp, vp, vp, vp, vp, vp, vp, vp], None
    L.sc_precheck.argtypes = [i, i, i, i, d, d, i, vp, i, i, i, vp, i]
    L.sc_plan.argtypes, L.sc_plan.restype = [i, vp, vp, vp], i
    L.sc_sizes.argtypes, L.sc_sizes.restype = [vp], None
    return L


def host_simplify(shim, verts, faces, cell, place=QUADRIC, reg=1e-3, clamp=1.0):
    """the host twin of the kernels for one mesh, on the oracle's incidence -> the dict of simplify()"""
    v, f = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    vrow, vface = TO.incidence(f, len(v))
    vrow, vface = np.ascontiguousarray(vrow, np.int32), np.ascontiguousarray(vface, np.int32)
    out = dict(info=np.zeros(1, dtype=INFO_DTYPE), verts=np.zeros((len(v), 3), np.float32), faces=np.zeros((len(f), 3), np.int32), map=np.zeros(len(v), np.int32),
               key=np.zeros(len(v), np.uint64), cid=np.zeros(len(v), np.int32), quad=np.zeros((len(v), 10)), pos=np.zeros((len(v), 3), np.float32))
    shim.sc_simplify(v.ctypes.data, len(v), f.ctypes.data, len(f), vrow.ctypes.data, vface.ctypes.data, float(cell), int(place), float(reg), float(clamp),
                     *[out[n].ctypes.data for n in ("info", "verts", "faces", "map", "key", "cid", "quad", "pos")])
    out["info"] = out["info"][0]
    out["verts"], out["faces"] = out["verts"][:int(out["info"]["verts_out"])], out["faces"][:int(out["info"]["faces_out"])]
    out["pos"] = out["pos"][:int(out["info"]["clusters"]) if out["info"]["status"] != CAPACITY else 0]
    return out
