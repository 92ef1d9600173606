"""NumPy statement of sh_mesh_topology (include/shoulder_hip.h "mesh topology of the resident batch"): the incidence rows, the face
adjacency, the shells and their counts.  The adjacency and the edge counts come from SORTING the edge keys, deliberately not from the
incidence rows the device walks; the Jacobi rounds of FastSV run with np.minimum.at (the rounds are part of the record); the labels are
computed a second way, with scipy.sparse.csgraph.connected_components, and the two are held equal.  Everything is integer except the
box corners, which are minima and maxima under the order of the float32 in which -0 < +0.  Also the test meshes and the ctypes side of
the host twin."""
import ctypes

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import host_twin

ARG, STATE, CAPACITY = -1, -3, -4
BORDER, NONMANIFOLD, DEGENERATE = -1, -2, -3
MAX_SHELLS, MAX_ROUNDS, HEAD = 65536, 32, 64
WATERTIGHT, CONSISTENT = 1, 2


def degenerate(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])


def incidence(faces, nv):
    """-> (vrow (nv + 1,), vface (3 F,)): the rows by sorting the (vertex, face) pairs of the non-degenerate faces"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.nonzero(~degenerate(f))[0]
    vert, face = f[keep].ravel(), np.repeat(keep, 3)
    order = np.lexsort((face, vert))
    vrow = np.zeros(nv + 1, dtype=np.int32)
    vrow[1:] = np.cumsum(np.bincount(vert, minlength=nv))
    vface = np.full(3 * len(f), -1, dtype=np.int32)
    vface[:len(order)] = face[order]
    return vrow, vface


def adjacency(faces):
    """-> (adj (F, 3), counts dict, same (F, 3) bool: the slot's edge is manifold and both faces traverse it in the same direction)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    adj = np.full((F, 3), DEGENERATE, dtype=np.int32)
    same = np.zeros((F, 3), dtype=bool)
    keep = np.nonzero(~degenerate(f))[0]
    face, slot = np.repeat(keep, 3), np.tile(np.arange(3), len(keep))
    a, c = f[face, slot], f[face, (slot + 1) % 3]
    key = (np.minimum(a, c) << 32) | np.maximum(a, c)
    order = np.argsort(key, kind="stable")      # (the slots come in (face, slot) order: the first of a group is the owner)
    ks = key[order]
    start = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0] if len(ks) else np.zeros(0, np.int64)
    uses = np.diff(np.r_[start, len(ks)])
    group = np.repeat(np.arange(len(start)), uses)
    n = uses[group]
    fo, so, fwd = face[order], slot[order], (a < c)[order]
    adj[fo[n == 1], so[n == 1]] = BORDER
    adj[fo[n >= 3], so[n >= 3]] = NONMANIFOLD
    two = np.nonzero(uses == 2)[0]
    i0, i1 = start[two], start[two] + 1
    adj[fo[i0], so[i0]], adj[fo[i1], so[i1]] = fo[i1], fo[i0]
    bad = fwd[i0] == fwd[i1]
    same[fo[i0], so[i0]], same[fo[i1], so[i1]] = bad, bad
    counts = dict(edges=len(start), border_edges=int((uses == 1).sum()), nonmanifold_edges=int((uses >= 3).sum()), inconsistent_edges=int(bad.sum()))
    return adj, counts, same


def fastsv(adj, max_rounds=MAX_ROUNDS):
    """the Jacobi rounds -> (p, rounds, status): rounds counts up to and including the first round that changes nothing"""
    F = len(adj)
    u, e = np.nonzero(adj >= 0)
    v = adj[u, e].astype(np.int64)
    p, rounds = np.arange(F, dtype=np.int64), 0
    while True:
        if rounds == max_rounds:
            return p, rounds, CAPACITY
        g = p[p]
        new = g.copy()
        np.minimum.at(new, u, g[v])
        np.minimum.at(new, p[u], g[v])
        rounds += 1
        changed = bool((new != p).any())
        p = new
        if not changed:
            return p, rounds, 0


def naive_rounds(adj):
    """the rounds of the plain minimum-over-neighbours propagation (why the rule is FastSV)"""
    u, e = np.nonzero(adj >= 0)
    v = adj[u, e].astype(np.int64)
    p, rounds = np.arange(len(adj), dtype=np.int64), 0
    while True:
        new = p.copy()
        np.minimum.at(new, u, p[v])
        rounds += 1
        if (new == p).all():
            return rounds
        p = new


def components(adj):
    """the labels a second way: scipy's connected components of the slot graph, renumbered by first face; -1 for a degenerate face"""
    F = len(adj)
    u, e = np.nonzero(adj >= 0)
    g = coo_matrix((np.ones(len(u), np.int8), (u, adj[u, e])), shape=(F, F))
    comp = connected_components(g, directed=False)[1]
    live = adj[:, 0] != DEGENERATE
    first = np.full(comp.max() + 1 if F else 0, F, dtype=np.int64)
    np.minimum.at(first, comp[live], np.nonzero(live)[0])
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return np.where(live, rank[comp], -1).astype(np.int32)


def enc(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dec(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def topology(verts, faces, max_shells=64, max_rounds=MAX_ROUNDS):
    """one mesh -> dict(vrow, vface, adj (3 F,), label, info (record), shells (max_shells,))"""
    from shoulder_amd import _lib
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    F, nv = len(f), len(v)
    deg = degenerate(f)
    vrow, vface = incidence(f, nv)
    adj, counts, same = adjacency(f)
    p, rounds, status = fastsv(adj, max_rounds)
    info, shells = np.zeros((), dtype=_lib.TOPOLOGY_DTYPE), np.zeros(max_shells, dtype=_lib.SHELL_DTYPE)
    valence = np.diff(vrow)
    info["status"], info["rounds"], info["faces_degenerate"] = status, rounds, int(deg.sum())
    info["vertices_used"], info["max_valence"] = int((valence > 0).sum()), int(valence.max()) if nv else 0
    for k, x in counts.items():
        info[k] = x
    info["euler"] = int(info["vertices_used"]) - counts["edges"] + int((~deg).sum())
    info["flags"] = (WATERTIGHT if counts["border_edges"] == 0 and counts["nonmanifold_edges"] == 0 and not deg.any() else 0) | \
                    (CONSISTENT if counts["inconsistent_edges"] == 0 else 0)
    label = np.full(F, -1, dtype=np.int32)
    info["largest_shell"] = -1
    if status == 0:
        root = ~deg & (p == np.arange(F))
        rank = np.cumsum(root) - 1
        label = np.where(deg, -1, rank[p]).astype(np.int32)
        assert np.array_equal(label, components(adj))      # the rounds and scipy agree
        n = int(root.sum())
        size = np.bincount(label[~deg], minlength=n)
        info["n_shells"], info["shells_written"] = n, min(n, max_shells)
        if n:
            info["largest_shell"], info["largest_faces"] = int(np.argmax(size)), int(size.max())      # (argmax: the first of equals)
        w = min(n, max_shells)
        live = ~deg & (label < w)
        lab = label[live]
        shells["first_face"][:w] = np.nonzero(root)[0][:w]
        shells["faces"][:w] = size[:w]
        a = adj[live]
        shells["border_slots"][:w] = np.bincount(lab, weights=(a == BORDER).sum(axis=1), minlength=w)
        shells["nonmanifold_slots"][:w] = np.bincount(lab, weights=(a == NONMANIFOLD).sum(axis=1), minlength=w)
        shells["manifold_edges"][:w] = np.bincount(lab, weights=(a >= 0).sum(axis=1), minlength=w).astype(np.int64) // 2
        shells["inconsistent_edges"][:w] = np.bincount(lab, weights=same[live].sum(axis=1), minlength=w).astype(np.int64) // 2
        for k in range(3):
            e = enc(v[:, k])[f[live]]
            lo, hi = np.full(w, 0xFFFFFFFF, dtype=np.uint32), np.zeros(w, dtype=np.uint32)
            np.minimum.at(lo, lab, e.min(axis=1))
            np.maximum.at(hi, lab, e.max(axis=1))
            shells["lo"][:w, k], shells["hi"][:w, k] = dec(lo), dec(hi)
    return dict(vrow=vrow, vface=vface, adj=np.ascontiguousarray(adj.ravel()), label=label, info=info, shells=shells)


NAMES = ("vrow", "vface", "adj", "label", "info", "shells")


def split(verts, faces, label, largest_only=False):
    """the meshes of the shells from the labels: vertices compacted in first-use order, faces in their order"""
    v, f, label = np.asarray(verts), np.asarray(faces).reshape(-1, 3), np.asarray(label)
    n = int(label.max()) + 1 if len(label) else 0
    ks = range(n)
    if largest_only and n:
        ks = [int(np.argmax(np.bincount(label[label >= 0], minlength=n)))]
    out = []
    for k in ks:
        fk = f[label == k]
        uniq, first, inv = np.unique(fk.ravel(), return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        out.append((np.ascontiguousarray(v[uniq[order]]), np.ascontiguousarray(rank[inv].reshape(-1, 3).astype(np.int32))))
    return out


# ---- the test meshes -------------------------------------------------------------------------------------------------------------------
def join(*meshes):
    """several meshes as one: the vertices and faces one behind the other"""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int32).reshape(-1, 3) + base)
        base += len(vs[-1])
    return np.ascontiguousarray(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(fs))


def shifted(mesh, d):
    return (np.asarray(mesh[0], np.float32) + np.asarray(d, np.float32)).astype(np.float32), mesh[1]


def two_boxes(box):
    return join(box, shifted(box, (100, 0, 0)))


def boxes_sharing(box, shared):
    """two boxes in one mesh; the second one's vertices `shared` are the first one's (its own copies stay, unused)"""
    v, f = two_boxes(box)
    nv = len(box[0])
    f = f.copy()
    for i in shared:
        f[f == nv + i] = i
    return v, f


def fan(n):
    """n faces [0, i, i + 1] around vertex 0"""
    t = np.arange(n + 1) * (2.0 * np.pi / (n + 7))
    v = np.zeros((n + 2, 3), np.float32)
    v[0] = (0, 0, 25)
    v[1:, 0], v[1:, 1] = 40 * np.cos(t), 40 * np.sin(t)
    i = np.arange(1, n + 1)
    return v, np.ascontiguousarray(np.stack([np.zeros(n, np.int64), i, i + 1], axis=1).astype(np.int32))


def strip(n, seed=None):
    """n faces [i, i + 1, i + 2] with the odd ones swapped (one winding), in order or shuffled by default_rng(seed).permutation"""
    i = np.arange(n)
    f = np.stack([i, i + 1, i + 2], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    v = np.zeros((n + 2, 3), np.float32)
    v[:, 0], v[:, 1] = np.arange(n + 2) // 2, np.arange(n + 2) % 2
    if seed is not None:
        f = f[np.random.default_rng(seed).permutation(n)]
    return v, np.ascontiguousarray(f.astype(np.int32))


def loose_triangles(n, at=(300, 300, 300)):
    v = np.zeros((3 * n, 3), np.float32)
    k = np.arange(n)
    v[0::3] = np.stack([k * 3.0, 0 * k, 0 * k], axis=1) + at
    v[1::3] = np.stack([k * 3.0 + 1, 0 * k, 0 * k], axis=1) + at
    v[2::3] = np.stack([k * 3.0, 0 * k + 1, 0 * k], axis=1) + at
    return v.astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def with_degenerate(verts, faces, where):
    """the faces with degenerate ones (a corner repeated: three forms in turn) put at the given positions of the result"""
    faces = [tuple(int(x) for x in f) for f in np.asarray(faces).reshape(-1, 3)]
    out, k = [], 0
    for pos in range(len(faces) + len(where)):
        if pos in where:
            a, b, c = faces[min(k, len(faces) - 1)]
            out.append(((a, b, b), (a, a, c), (a, b, a), (a, a, a))[len(out) % 4])
        else:
            out.append(faces[k])
            k += 1
    return np.ascontiguousarray(verts, np.float32), np.array(out, dtype=np.int32)


def tetrahedron():
    v = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


# ---- the ctypes side of the host twin (tests/hostcheck/topo_check.cpp) ----------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("topo", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.tc_topology.argtypes, L.tc_topology.restype = [vp, i, vp, i, i, i, vp, vp, vp, vp, vp, vp], None
    L.tc_precheck.argtypes = [i, i, i, i, i, i, i, vp, i]
    L.tc_plan.argtypes, L.tc_plan.restype = [i, i, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, vp], None
    return L


def host_topology(shim, verts, faces, max_shells=64, max_rounds=MAX_ROUNDS):
    """the host twin of the kernels for one mesh -> the dict of topology()"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    out = dict(vrow=np.zeros(len(v) + 1, np.int32), vface=np.zeros(3 * len(f), np.int32), adj=np.zeros(3 * len(f), np.int32), label=np.zeros(len(f), np.int32),
               info=np.zeros(1, dtype=_lib.TOPOLOGY_DTYPE), shells=np.zeros(max_shells, dtype=_lib.SHELL_DTYPE))
    shim.tc_topology(v.ctypes.data, len(v), f.ctypes.data, len(f), int(max_shells), int(max_rounds), *[out[n].ctypes.data for n in NAMES])
    out["info"] = out["info"][0]
    return out


# ---- the cases both test files walk: name -> (mesh, the figures it must show) ----------------------------------------------------------
def table(meshes, big=False):
    """meshes: dict with "box", "humerus_left", "humerus_left_flipped", "humerus_right", "humerus_left_trab", "proximal_left_cut".
    -> dict name -> ((verts, faces), dict of figures: the counts and rounds a CPU run of the rule gave, as conditions).
    big: also the shuffled strip of 20 000 faces."""
    box, left = meshes["box"], meshes["humerus_left"]
    bv, bf = box
    lv, lf = left
    flipped = bf.copy()
    flipped[5] = flipped[5][[1, 0, 2]]
    T = {}

    def row(name, mesh, **figures):
        T[name] = ((np.ascontiguousarray(mesh[0], np.float32), np.ascontiguousarray(mesh[1], np.int32)), figures)
    row("box", box, edges=18, border_edges=0, inconsistent_edges=0, n_shells=1, largest_faces=12, rounds=3, euler=2)
    row("box without face 0", (bv, bf[1:]), edges=18, border_edges=3, inconsistent_edges=0, n_shells=1, largest_faces=11, rounds=4)
    row("box, face 5 flipped", (bv, flipped), edges=18, border_edges=0, inconsistent_edges=3, n_shells=1, largest_faces=12, rounds=3)
    row("two boxes", two_boxes(box), edges=36, border_edges=0, inconsistent_edges=0, n_shells=2, largest_faces=12, rounds=3)
    row("two boxes sharing vertex 0", boxes_sharing(box, (0,)), edges=36, border_edges=0, inconsistent_edges=0, n_shells=2, largest_faces=12, rounds=3, vertices_used=15)
    row("fan of 300", fan(300), edges=601, border_edges=302, inconsistent_edges=0, n_shells=1, largest_faces=300, rounds=10, max_valence=300)
    row("strip of 600", strip(600), inconsistent_edges=0, n_shells=1, largest_faces=600, rounds=11)
    row("strip of 600, shuffled", strip(600, seed=1), inconsistent_edges=0, n_shells=1, largest_faces=600, rounds=11)
    if big:
        row("strip of 20000, shuffled", strip(20000, seed=1), inconsistent_edges=0, n_shells=1, largest_faces=20000, rounds=17)
    for n, figures in ((4, dict(edges=10, border_edges=8, n_shells=2, largest_faces=3, rounds=3)), (255, dict(edges=403, border_edges=41, n_shells=1, largest_faces=255, rounds=6)),
                       (256, dict(edges=405, border_edges=42, n_shells=1, largest_faces=256, rounds=6)), (257, dict(edges=408, border_edges=45, n_shells=2, largest_faces=256, rounds=6)),
                       (513, dict(edges=821, border_edges=103, n_shells=3, largest_faces=352, rounds=6))):
        row(f"humerus_left[:{n}]", (lv, lf[:n]), **figures)
    whole = dict(border_edges=0, inconsistent_edges=0, n_shells=1)
    row("humerus_left", left, edges=48660, largest_faces=32440, rounds=10, **whole)
    row("humerus_left_flipped", meshes["humerus_left_flipped"], edges=48660, largest_faces=32440, rounds=10, **whole)
    row("humerus_right", meshes["humerus_right"], edges=41028, largest_faces=27352, rounds=10, **whole)
    row("humerus_left_trab", meshes["humerus_left_trab"], edges=48438, largest_faces=32292, rounds=11, euler=0, **whole)
    row("proximal_left_cut", meshes["proximal_left_cut"], edges=28047, largest_faces=18698, rounds=10, max_valence=117, **whole)
    loose = loose_triangles(40)
    row("humerus_left + 40 loose triangles behind", join(left, loose), edges=48780, border_edges=120, n_shells=41, largest_faces=32440, rounds=10)
    row("humerus_left + 40 loose triangles in front", join(loose, left), edges=48780, border_edges=120, n_shells=41, largest_faces=32440, rounds=10)
    row("humerus_left + a box", join(left, box), edges=48678, border_edges=0, inconsistent_edges=0, n_shells=2, largest_faces=32440, rounds=10)
    return T


def further(meshes):
    """the further cases of both test files: name -> mesh"""
    lv, lf = meshes["humerus_left"]
    out = {"tetrahedron": tetrahedron(), "boxes sharing an edge": boxes_sharing(meshes["box"], (0, 1)),
           "degenerate faces": with_degenerate(lv, lf[:513], (0, 1, 100, 255, 256, 300, 519)),
           "degenerate faces, four faces": with_degenerate(lv, lf[:2], (0, 3)),
           "only degenerate faces": (lv, np.array([[0, 1, 1], [2, 2, 3], [4, 5, 4], [6, 6, 6]], np.int32)),
           "humerus_left, shuffled": (lv, np.ascontiguousarray(lf[np.random.default_rng(1).permutation(len(lf))]))}
    return {k: (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)) for k, (v, f) in out.items()}


def holds(info, figures, nf):
    """the record shows the figures of its row"""
    bad = {k: (int(info[k]), x) for k, x in figures.items() if int(info[k]) != x}
    assert not bad and info["status"] == 0 and int(info["euler"]) == int(info["vertices_used"]) - int(info["edges"]) + nf - int(info["faces_degenerate"]), (bad, info)
