"""NumPy statement of sh_geodesic (include/shoulder_hip.h "geodesic distances and shortest paths on the resident batch"): the face
records, the graph, the distances twice -- Jacobi relaxation to its fixed point, and SciPy's Dijkstra over the same arcs with the sources
hung on a virtual node by arcs of d0 --, then the roots, predecessors, sources and info records from the converged distances alone.
float64, one ufunc per operation of the rule (NumPy contracts nothing).  The incidence and the adjacency come from tests/topo_oracle.py.
The relaxation PUSHES along the arcs as the rule lists them (from v to the others of its faces); the device PULLS over v's own row: the
two agree because every arc has its reverse with the same bytes, which test_geo_host.py also checks.  Also the test meshes and the ctypes
side of the host twin."""
import ctypes

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

import host_twin
import topo_oracle as TO

ARG, STATE, INTERNAL = -1, -3, -8
EDGES, UNFOLD, MAX_SETS, LDS_VERTICES, CHUNK, INFO_BYTES = 0, 1, 16, 20000, 32, 32
ROOT, NO_PRED, UNREACHED = -1, -2, -3
FACE = 6
INF = np.inf
INFO_DTYPE = np.dtype([("far_dist", "<f8"), ("reached", "<i4"), ("roots", "<i4"), ("no_pred", "<i4"), ("farthest", "<i4"), ("sweeps", "<i4"), ("status", "<i4")])
MODES = {EDGES: "edges", UNFOLD: "unfold"}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def face_records(verts, faces, adj=None):
    """-> (rec (F, 6): len[3], unf[3];  opp (F, 3): the vertex across slot e, -1 where adj[f][e] < 0;  cross (F, 3): x_c / l of the
    unfolded line on the shared edge, measured from its smaller index, NaN where there is none)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    adj = TO.adjacency(f)[0] if adj is None else np.asarray(adj).reshape(-1, 3)
    rec, opp, cross = np.full((F, FACE), INF), np.full((F, 3), -1, np.int32), np.full((F, 3), np.nan)
    deg = TO.degenerate(f)
    with np.errstate(all="ignore"):
        for e in range(3):
            a, b, p = f[:, e], f[:, (e + 1) % 3], f[:, (e + 2) % 3]
            lo, hi = np.minimum(a, b), np.maximum(a, b)
            E = v[hi] - v[lo]
            l = np.sqrt(_dot(E, E))
            rec[:, e] = l
            g = adj[:, e].astype(np.int64)
            has = g >= 0
            q = np.where(has, f[np.where(has, g, 0)].sum(axis=1) - a - b, 0)
            p1, q1 = np.minimum(p, q), np.maximum(p, q)
            xs, ys = [], []
            for r in (p1, q1):
                d = v[r] - v[lo]
                x = _dot(d, E) / l
                t = _dot(d, d) - x * x
                xs.append(x)
                ys.append(np.sqrt(np.where(t < 0, 0.0, t)))
            s = ys[0] + ys[1]
            xc = (xs[0] * ys[1] + xs[1] * ys[0]) / s
            dx = xs[0] - xs[1]
            unf = np.sqrt(dx * dx + s * s)
            valid = has & (p != q) & (s > 0) & (xc > 0) & (xc < l)
            rec[:, 3 + e] = np.where(valid, unf, INF)
            opp[:, e] = np.where(has, q, -1)
            cross[:, e] = np.where(valid, xc / l, np.nan)
    rec[deg], opp[deg], cross[deg] = INF, -1, np.nan
    return rec, opp, cross


def arcs(faces, rec, opp, mode):
    """the graph as the rule lists it -> (tail, head, w): per non-degenerate face f and corner k with v = f[k] the arcs from v to
    f[(k + 1) % 3] with len[k], to f[(k + 2) % 3] with len[(k + 2) % 3] and, unfolded, to the vertex across slot (k + 1) % 3"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    live = np.nonzero(~TO.degenerate(f))[0]
    T, H, W = [], [], []
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        T += [f[live, k], f[live, k]]
        H += [f[live, k1], f[live, k2]]
        W += [rec[live, k], rec[live, k2]]
        if mode == UNFOLD:
            has = opp[live, k1] >= 0
            T.append(f[live[has], k])
            H.append(opp[live[has], k1].astype(np.int64))
            W.append(rec[live[has], 3 + k1])
    if not T:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(T), np.concatenate(H), np.concatenate(W)


def sets_of(sources, d0=None):
    """one mesh's K sets -> list of (vertices int64, d0 float64 with -0.0 made +0.0)"""
    out = []
    for k, s in enumerate(sources):
        s = np.asarray(s, np.int64).reshape(-1)
        z = np.zeros(len(s)) if d0 is None or d0[k] is None else np.asarray(d0[k], np.float64).reshape(-1) + 0.0
        assert len(z) == len(s)
        out.append((s, z))
    return out


def seed(nv, src, d0, max_dist):
    d = np.full(nv, INF)
    keep = d0 <= max_dist
    np.minimum.at(d, src[keep], d0[keep])
    return d


def jacobi(nv, tail, head, w, src, d0, max_dist=INF):
    """-> (d, rounds: up to and including the first that changes nothing)"""
    d, rounds = seed(nv, src, d0, max_dist), 0
    while True:
        with np.errstate(all="ignore"):
            cand = d[tail] + w
        cand = np.where(cand <= max_dist, cand, INF)      # (a NaN compares false)
        new = d.copy()
        np.minimum.at(new, head, cand)
        rounds += 1
        if new.tobytes() == d.tobytes():
            return d, rounds
        d = new


def by_dijkstra(nv, tail, head, w, src, d0, max_dist=INF):
    """SciPy's Dijkstra over the same arcs; node nv is virtual and reaches source i by an arc of d0[i].  Parallel arcs are reduced to
    their minimum first (a sparse matrix would add them)."""
    keep = np.isfinite(w)
    t, h, ww = np.r_[tail[keep], np.full(len(src), nv)], np.r_[head[keep], src], np.r_[w[keep], d0]
    order = np.lexsort((ww, h, t))
    t, h, ww = t[order], h[order], ww[order]
    first = np.r_[True, (t[1:] != t[:-1]) | (h[1:] != h[:-1])] if len(t) else np.zeros(0, bool)
    g = csr_matrix((ww[first], (t[first], h[first])), shape=(nv + 1, nv + 1))      # (explicit zeros stay: arcs of length 0)
    return dijkstra(g, directed=True, indices=nv, limit=max_dist)[:nv]


def finish(nv, tail, head, w, src, d0, d, sweeps=0):
    """roots, predecessors, sources and the info record from the converged d alone"""
    label = np.full(nv, np.iinfo(np.int32).max, np.int64)
    hit = d0 == d[src]
    np.minimum.at(label, src[hit], np.nonzero(hit)[0])
    root = label != np.iinfo(np.int32).max
    reached = np.isfinite(d)
    with np.errstate(all="ignore"):
        ok = (d[tail] + w == d[head]) & (d[tail] < d[head]) & reached[head]
    best = np.full(nv, nv, np.int64)
    np.minimum.at(best, head[ok], tail[ok])
    pred = np.where(~reached, UNREACHED, np.where(root, ROOT, np.where(best < nv, best, NO_PRED))).astype(np.int32)
    top = np.where(pred >= 0, pred, np.arange(nv))
    while True:
        nxt = top[top]
        if np.array_equal(nxt, top):
            break
        top = nxt
    source = np.where(reached & root[top], label[top], -1).astype(np.int32)
    info = np.zeros((), INFO_DTYPE)
    info["reached"], info["roots"], info["no_pred"] = int(reached.sum()), int(root.sum()), int((pred == NO_PRED).sum())
    info["far_dist"], info["farthest"] = (float(d[reached].max()), int(np.argmax(np.where(reached, d, -1.0)))) if reached.any() else (0.0, -1)
    info["sweeps"], info["status"] = sweeps, 0
    return pred, source, info


def graph(verts, faces, mode=UNFOLD):
    """what every evaluation of one mesh shares -> dict(nv, face, opp, cross, arcs)"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    rec, opp, cross = face_records(v, faces)
    return dict(nv=len(v), face=rec, opp=opp, cross=cross, arcs=arcs(faces, rec, opp, mode), mode=mode)


def geodesic(verts, faces, sources, d0=None, mode=UNFOLD, max_dist=INF, g=None, check=True):
    """one mesh, K sets -> dict(face (F, 6), dist (K, V), pred (K, V) int32, source (K, V) int32, info (K,), rounds [K]).
    check: Dijkstra and the Jacobi rounds give the same bytes (the rule's claim), asserted here for every evaluation."""
    g = g or graph(verts, faces, mode)
    nv, (t, h, w) = g["nv"], g["arcs"]
    sets = sets_of(sources, d0)
    K = len(sets)
    out = dict(face=g["face"], dist=np.zeros((K, nv)), pred=np.zeros((K, nv), np.int32), source=np.zeros((K, nv), np.int32), info=np.zeros(K, INFO_DTYPE), rounds=[])
    for k, (s, z) in enumerate(sets):
        d = by_dijkstra(nv, t, h, w, s, z, max_dist)
        if check:
            dj, rounds = jacobi(nv, t, h, w, s, z, max_dist)
            assert dj.tobytes() == d.tobytes(), "Jacobi and Dijkstra differ"
            out["rounds"].append(rounds)
        out["dist"][k] = d
        out["pred"][k], out["source"][k], out["info"][k] = finish(nv, t, h, w, s, z, d)
    return out


BUFFERS = ("face", "dist", "pred", "source")
INFO_FIELDS = ("far_dist", "reached", "roots", "no_pred", "farthest", "status")      # (not sweeps: informational)


def compare(got, want, tag):
    """everything as bytes; of the info records every field but sweeps"""
    for n in BUFFERS:
        a, b = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, n, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))
    for n in INFO_FIELDS:
        assert np.asarray(got["info"][n]).tobytes() == np.asarray(want["info"][n]).tobytes(), (tag, "info", n, got["info"][n], want["info"][n])


def path(verts, faces, g, res, k, target):
    """the polyline of the rule from `target` back to its root on one mesh -> (points (n, 3) float64 from the root to the target, their
    summed length); a hop over an unfolded diagonal contributes its crossing point P_lo + (x_c / l) E on the shared edge"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d, pred = res["dist"][k], res["pred"][k]
    assert pred[target] >= 0 or pred[target] == ROOT
    pts, at = [v[target]], int(target)
    while pred[at] >= 0:
        u = int(pred[at])
        rows = np.nonzero((f == at).any(axis=1) & ~TO.degenerate(f))[0]
        edge = [(fi, kk) for fi in rows for kk in range(3) if f[fi, kk] == at and u in (f[fi, (kk + 1) % 3], f[fi, (kk + 2) % 3])]
        if not any(d[u] + g["face"][fi, kk if f[fi, (kk + 1) % 3] == u else (kk + 2) % 3] == d[at] for fi, kk in edge):
            fi, e = next((fi, (kk + 1) % 3) for fi in rows for kk in range(3)
                         if f[fi, kk] == at and g["opp"][fi, (kk + 1) % 3] == u and d[u] + g["face"][fi, 3 + (kk + 1) % 3] == d[at])
            a, b = f[fi, e], f[fi, (e + 1) % 3]
            lo, hi = min(a, b), max(a, b)
            pts.append(v[lo] + g["cross"][fi, e] * (v[hi] - v[lo]))
        pts.append(v[u])
        at = u
    pts = np.array(pts[::-1])
    return pts, float(np.linalg.norm(np.diff(pts, axis=0), axis=1).sum())


# ---- the test meshes -------------------------------------------------------------------------------------------------------------------
def twin_box(box):
    """the box with vertex 0 a second time, at the same coordinates, as vertex 8, joined to it by the face [0, 8, 1]: an arc of length 0"""
    v, f = box
    v = np.concatenate([v, v[:1]])
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(np.concatenate([f, [[0, 8, 1]]]).astype(np.int32))


def small_cases(meshes):
    """the shapes at which the kernels can go wrong: name -> (mesh, the single source vertex).  meshes: topo_oracle.table's dict"""
    T, further = TO.table(meshes), TO.further(meshes)
    out = {"tetrahedron": (further["tetrahedron"], 0)}
    for n, s in (("box", 0), ("box without face 0", 0), ("two boxes", 0), ("fan of 300", 0), ("strip of 600, shuffled", 0), ("humerus_left[:255]", None),
                 ("humerus_left[:256]", None), ("humerus_left[:257]", None)):
        mesh = T[n][0]
        out[n] = (mesh, int(mesh[1][0][0]) if s is None else s)
    out["fan of 300, from the rim"] = (T["fan of 300"][0], 150)
    for n in ("boxes sharing an edge", "degenerate faces", "degenerate faces, four faces", "only degenerate faces"):
        out[n] = (further[n], int(further[n][1][0][0]))
    out["box with a twin of vertex 0"] = (twin_box(meshes["box"]), 8)
    return out


def case_sets(mesh, single):
    """the sets every small case is asked with: one vertex; all vertices of face 0 (repeats included); nothing"""
    return [np.array([single]), np.asarray(mesh[1][0], np.int64), np.zeros(0, np.int64)]


def topmost(verts):
    return int(np.argmax(np.asarray(verts)[:, 2]))


def bottommost(verts):
    return int(np.argmin(np.asarray(verts)[:, 2]))


# ---- the ctypes side of the host twin (tests/hostcheck/geo_check.cpp) ------------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("geo", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.gc_geodesic.argtypes, L.gc_geodesic.restype = [vp, i, vp, i, vp, vp, vp, i, i, d, vp, vp, vp, i, vp, vp, vp, vp, vp], i
    L.gc_precheck.argtypes = [i, i, i, d, i, i, vp, vp, vp, vp, i, i, i, vp, i]
    L.gc_plan.argtypes, L.gc_plan.restype = [i, i] + [ctypes.c_longlong] * 6 + [vp], None
    return L


def host_geodesic(shim, verts, faces, sources, d0=None, mode=UNFOLD, max_dist=INF, lds=True):
    """the host twin of the kernels for one mesh (incidence and adjacency from topo_oracle) -> the dict of geodesic().  lds: the schedule
    of the LDS kernel (all reads of a round, then its writes, in one array); otherwise the two planes of the general path"""
    v, f = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    vrow, vface = TO.incidence(f, len(v))
    adj = np.ascontiguousarray(TO.adjacency(f)[0].ravel(), np.int32)
    sets = sets_of(sources, d0)
    K, nv = len(sets), len(v)
    off = np.cumsum([0] + [len(s) for s, _ in sets]).astype(np.int32)
    src = np.ascontiguousarray(np.concatenate([s for s, _ in sets] + [np.zeros(0, np.int64)]), np.int32)
    z = np.ascontiguousarray(np.concatenate([x for _, x in sets] + [np.zeros(0)]), np.float64)
    out = dict(face=np.zeros((len(f), FACE)), dist=np.zeros((K, nv)), pred=np.zeros((K, nv), np.int32), source=np.zeros((K, nv), np.int32), info=np.zeros(K, INFO_DTYPE))
    rc = shim.gc_geodesic(v.ctypes.data, nv, f.ctypes.data, len(f), vrow.ctypes.data, vface.ctypes.data, adj.ctypes.data, int(mode), K, float(max_dist), off.ctypes.data,
                          src.ctypes.data, z.ctypes.data, int(bool(lds)), *[out[n].ctypes.data for n in ("face", "dist", "pred", "source", "info")])
    assert rc == 0, rc
    return out
