"""NumPy statement of sh_mesh_repair (include/shoulder_hip.h "repair of the resident batch"): one winding per shell, outward shells
(optionally by nesting depth) and filled holes, on top of topo_oracle.adjacency / topology.  The parities come from a breadth-first walk
over whole levels with NumPy (the device walks with a queue and atomics); V6 is the winding sum's tree (winding_oracle.block_sum) over
the shell's ascending faces; the holes are traced with a dictionary of the directed edges of the oriented faces and walked one after
the other (the device doubles pointers).  Everything but W is integer or + - x / on float64 in the written order, so it is held to the
host twin and the device AS BYTES; W is an atan2 sum and is held within winding_oracle.bound.  Also the test meshes and the ctypes side
of the host twin (tests/hostcheck/repair_check.cpp)."""
import ctypes

import numpy as np

import host_twin
import topo_oracle as TO
import winding_oracle as WO
from ray_oracle import cross3, dot3, widen

ARG, STATE, CAPACITY, NOMEM = -1, -3, -4, -6
NONE, WINDING, OUTWARD, NESTED = 0, 1, 2, 3
FILL_NONE, FAN, CENTROID = 0, 1, 2
NONORIENTABLE, AMBIGUOUS = 1, 2
HOLE_FILLED, HOLE_TOO_LONG, HOLE_SHELL, HOLE_OPEN, HOLE_TOO_SHORT = 0, 1, 2, 3, 4
CHANGED, SHELLS_LEFT = 1, 2
MAX_HOLES, MAX_ROUNDS, LDS_FACES = 65536, 1048576, 131072
ORIENTS = {NONE: "none", WINDING: "winding", OUTWARD: "outward", NESTED: "nested"}
FILLS = {FILL_NONE: "none", FAN: "fan", CENTROID: "centroid"}


def parities(adj, same, label):
    """the walk from the first faces of all shells at once -> (parity (F,) uint8, levels: the non-empty levels of the walk)"""
    F = len(adj)
    par, seen = np.zeros(F, np.uint8), np.zeros(F, bool)
    live = label >= 0
    first = np.full(int(label.max()) + 1 if live.any() else 0, F, np.int64)
    np.minimum.at(first, label[live], np.nonzero(live)[0])
    frontier, levels = first, 0
    seen[frontier] = True
    while len(frontier):
        levels += 1
        f, e = np.repeat(frontier, 3), np.tile(np.arange(3), len(frontier))
        g = adj[f, e]
        ok = g >= 0
        f, e, g = f[ok], e[ok], g[ok]
        new = ~seen[g]
        f, e, g = f[new], e[new], g[new]
        frontier, at = np.unique(g, return_index=True)      # whichever face reaches g first: the same parity in an orientable shell
        par[frontier] = par[f[at]] ^ same[f[at], e[at]]
        seen[frontier] = True
    return par, levels


def oriented(faces, adj, flip):
    """the faces and the adjacency as the flips leave them: (a, b, c) -> (a, c, b) exchanges slots 0 and 2"""
    fo, ao = np.array(faces, np.int64).reshape(-1, 3), np.array(adj, np.int64).reshape(-1, 3)
    m = np.asarray(flip, bool)
    fo[m] = fo[m][:, [0, 2, 1]]
    ao[m] = ao[m][:, [2, 1, 0]]
    return fo, ao


def v6(verts, fo, faces_of_shell, lo, hi):
    """the sum of det[A - o, B - o, C - o] over the shell's ascending faces in the tree of the winding sum"""
    o = lo.astype(np.float64) + (hi.astype(np.float64) - lo.astype(np.float64)) * 0.5
    P = widen(verts)[fo[faces_of_shell]] - o[None, None, :]
    return WO.block_sum(dot3(P[:, 0], cross3(P[:, 1], P[:, 2])))


def nesting(verts, fo, label, k, use):
    """W of shell k: the solid angles of the faces with use[f] seen from the first corner of the shell's first face, over 4 pi, in blocks
    of 2048 face INDICES of the mesh, the faces left out skipped -> (W, sum |omega| / 4 pi)"""
    v = widen(verts)
    p = v[fo[np.nonzero(label == k)[0][0], 0]]
    total, absw = 0.0, 0.0
    for b0 in range(0, len(fo), WO.BLOCK):
        idx = b0 + np.nonzero(use[b0:b0 + WO.BLOCK])[0]
        if not len(idx):
            total += 0.0
            continue
        om = WO.solid_angles(v[fo[idx, 0]], v[fo[idx, 1]], v[fo[idx, 2]], p)
        total += WO.serial_sum(om)
        absw += float(np.abs(om).sum())
    return total / WO.FOUR_PI, absw / WO.FOUR_PI


def successors(fo, ao):
    """the border half-edges (ids ascending) and the successor of each as an index into them, -1 for a blocked one"""
    bf, be = np.nonzero(ao == TO.BORDER)
    ids = 3 * bf + be
    place = {int(x): i for i, x in enumerate(ids)}
    directed = {}
    if len(ids):
        live = np.nonzero(ao[:, 0] != TO.DEGENERATE)[0]
        for e in range(3):
            for f, a, c in zip(live.tolist(), fo[live, e].tolist(), fo[live, (e + 1) % 3].tolist()):
                directed.setdefault((a, c), []).append((f, e))
    succ = np.full(len(ids), -1, np.int64)
    for i, (f, e) in enumerate(zip(bf.tolist(), be.tolist())):
        for _ in range(3 * len(fo) + 1):
            n = (e + 1) % 3
            w, x, a = int(fo[f, n]), int(fo[f, (n + 1) % 3]), int(ao[f, n])
            if a == TO.BORDER:
                succ[i] = place[3 * f + n]
                break
            if a < 0:
                break
            into = [(g, k) for g, k in directed.get((x, w), []) if g == a]      # g's slot that runs the other way, x -> w
            if not into:
                break
            f, e = into[0]
    return ids, succ


def cycles(succ):
    """-> (the cycles as lists of places, each from its smallest place, in the order of their starts; the number of places on no cycle)"""
    n, seen, out = len(succ), np.zeros(len(succ), bool), []
    for i in range(n):
        if seen[i]:
            continue
        path, j = [], i
        while j >= 0 and not seen[j]:
            seen[j] = True
            path.append(j)
            j = int(succ[j])
        if j == i:
            out.append(path)
    return out, n - sum(len(c) for c in out)


def cut_at_repeated_vertices(ids, succ, fo):
    """a cycle that passes a vertex more than once is cut there: each of its half-edges with that head takes the successor of the one
    before it along the cycle (cyclically), which closes every stretch between two passes into a cycle of its own"""
    new = succ.copy()
    for loop in cycles(succ)[0]:
        heads = {}
        for i in loop:
            f, e = divmod(int(ids[i]), 3)
            heads.setdefault(int(fo[f, (e + 1) % 3]), []).append(i)
        for group in heads.values():
            if len(group) > 1:
                for j, i in enumerate(group):
                    new[i] = succ[group[j - 1]]
    return new


def repair(verts, faces, orient=OUTWARD, fill=CENTROID, max_hole_edges=4096, max_shells=64, max_holes=64, max_rounds=MAX_ROUNDS, topo_rounds=TO.MAX_ROUNDS, topo=None):
    """one mesh -> dict(info, shells (max_shells,), holes (max_holes,), flip (F,) uint8, faces (faces_out, 3) int32, verts (verts_out, 3)
    float32; absw (max_shells,): sum |omega| / 4 pi behind every W; levels)"""
    from shoulder_amd import _lib
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F, nv = len(f), len(v)
    t = topo if topo is not None else TO.topology(v, f, max_shells=max_shells, max_rounds=topo_rounds)
    adj, _, same = TO.adjacency(f)
    assert np.array_equal(adj.ravel(), t["adj"])
    label, tinfo, tshells = t["label"], t["info"], t["shells"]
    info = np.zeros((), dtype=_lib.REPAIR_INFO_DTYPE)
    shells, holes = np.zeros(max_shells, dtype=_lib.REPAIR_SHELL_DTYPE), np.zeros(max_holes, dtype=_lib.REPAIR_HOLE_DTYPE)
    flip, absw = np.zeros(F, np.uint8), np.zeros(max_shells)
    info["shell_records"], info["faces_out"], info["verts_out"] = max_shells, F, nv
    out = dict(info=info, shells=shells, holes=holes, flip=flip, faces=f.copy(), verts=v.copy(), absw=absw, levels=0)
    if tinfo["status"] != 0 or F > LDS_FACES:
        info["status"] = CAPACITY
        return out
    par, levels = parities(adj, same, label)
    out["levels"] = levels
    if levels > max_rounds:
        info["status"] = CAPACITY
        return out
    n_shells, written = int(tinfo["n_shells"]), int(tinfo["shells_written"])
    u, e = np.nonzero(adj >= 0)
    g = adj[u, e]
    bad = np.zeros(n_shells, bool)
    bad[label[u[(par[u] ^ par[g]) != same[u, e]]]] = True
    live = label >= 0
    if orient >= WINDING:
        flip[live] = np.where(bad[label[live]], 0, par[live])
    members = [np.nonzero(label == k)[0] for k in range(written)]
    for k in range(written):
        shells[k]["status"], shells[k]["depth"] = (NONORIENTABLE if bad[k] else 0), -1
        shells[k]["parity_flips"] = int(flip[members[k]].sum())
        if orient >= OUTWARD and not bad[k]:
            fo, _ = oriented(f, adj, flip)
            shells[k]["V6"] = v6(v, fo, members[k], tshells[k]["lo"], tshells[k]["hi"])
            if shells[k]["V6"] < 0.0:
                shells[k]["inverted"] = 1
                flip[members[k]] ^= 1
    left = n_shells > written
    if orient == NESTED and not left:
        fo, _ = oriented(f, adj, flip)      # every written shell outward
        closed = np.array([not bad[k] and tshells[k]["border_slots"] == 0 and tshells[k]["nonmanifold_slots"] == 0 for k in range(written)], bool)
        odd = []
        for k in range(written):
            if bad[k]:
                shells[k]["depth"] = 0
                continue
            use = live & (label != k)
            use[live] &= closed[label[live]]
            W, absw[k] = nesting(v, fo, label, k, use)
            depth = float(np.rint(W))
            ambiguous = not abs(W - depth) <= 0.25
            shells[k]["W"], shells[k]["depth"] = W, 0 if ambiguous else int(depth)
            if ambiguous:
                shells[k]["status"] = AMBIGUOUS
            elif int(depth) & 1:
                odd.append(k)
        for k in odd:
            flip[members[k]] ^= 1
    if left and orient == NESTED:
        info["status"] = CAPACITY
    # the holes of the oriented faces
    fo, ao = oriented(f, adj, flip)
    ids, succ = successors(fo, ao)
    loops, blocked = cycles(cut_at_repeated_vertices(ids, succ, fo))
    new_faces, new_verts = [], []
    v64 = widen(v)
    for h, loop in enumerate(loops):
        L = len(loop)
        sf, se = int(ids[loop[0]]) // 3, int(ids[loop[0]]) % 3
        lab = int(label[sf])
        status = HOLE_SHELL if bad[lab] else HOLE_TOO_SHORT if L < 3 else HOLE_TOO_LONG if L > max_hole_edges else HOLE_OPEN if fill == FILL_NONE else HOLE_FILLED
        tails = [int(fo[int(ids[i]) // 3, int(ids[i]) % 3]) for i in loop]
        rec = dict(shell=lab, start_face=sf, start_slot=se, edges=L, status=status, first_face=-1, faces_added=0, vertex=-1)
        if status == HOLE_FILLED:
            rec["first_face"] = F + len(new_faces)
            if fill == FAN:
                new_faces += [(tails[0], tails[j + 1], tails[j]) for j in range(1, L - 1)]
            else:
                c = nv + len(new_verts)
                rec["vertex"] = c
                new_faces += [(tails[(j + 1) % L], tails[j], c) for j in range(L)]
                s = np.zeros(3)
                for j in range(L):
                    s = s + v64[tails[j]]
                new_verts.append((s / float(L)).astype(np.float32))
            rec["faces_added"] = F + len(new_faces) - rec["first_face"]
            info["holes_filled"] += 1
        if lab < written:
            shells[lab]["holes"] += 1
            shells[lab]["holes_filled"] += int(status == HOLE_FILLED)
        info["largest_hole"] = max(int(info["largest_hole"]), L)
        if h < max_holes:
            for key, x in rec.items():
                holes[h][key] = x
    info["holes"], info["holes_written"], info["blocked_edges"] = len(loops), min(len(loops), max_holes), blocked
    info["shells_nonorientable"], info["shells_inverted"], info["faces_flipped"] = int(bad.sum()), int(shells["inverted"].sum()), int(flip.sum())
    info["faces_added"], info["verts_added"] = len(new_faces), len(new_verts)
    info["faces_out"], info["verts_out"] = F + len(new_faces), nv + len(new_verts)
    info["flags"] = (CHANGED if flip.any() or new_faces else 0) | (SHELLS_LEFT if left and orient >= OUTWARD else 0)
    out["faces"] = np.ascontiguousarray(np.concatenate([fo, np.array(new_faces, np.int64).reshape(-1, 3)]).astype(np.int32))
    out["verts"] = np.ascontiguousarray(np.concatenate([v, np.array(new_verts, np.float32).reshape(-1, 3)]).astype(np.float32))
    return out


BYTES = ("info", "flip", "holes", "faces", "verts")


def same_bytes(got, want, tag):
    """everything but W as bytes; W within the bound of the winding sum over the mesh's faces"""
    for n in BYTES:
        assert np.asarray(got[n]).tobytes() == np.asarray(want[n]).tobytes(), (tag, n, got[n] if n == "info" else None, want[n] if n == "info" else None)
    gs, ws = np.asarray(got["shells"]), np.asarray(want["shells"])
    for n in ws.dtype.names:
        if n != "W":
            assert gs[n].tobytes() == ws[n].tobytes(), (tag, "shells", n, gs[n][:8], ws[n][:8])
    lim = WO.bound(len(want["flip"]), want["absw"])
    assert np.all(np.abs(gs["W"] - ws["W"]) <= lim), (tag, "W", float(np.abs(gs["W"] - ws["W"]).max()), float(lim.min()))


# ---- the test meshes -------------------------------------------------------------------------------------------------------------------
def mobius(n=10):
    """a strip of n faces over n vertices in two rows that closes with a half twist: one shell, not orientable, one border loop"""
    m = n // 2
    t = np.arange(m) * (2.0 * np.pi / m)
    mid = np.stack([30.0 * np.cos(t), 30.0 * np.sin(t), 0.0 * t], axis=1)
    w = np.stack([np.cos(t / 2.0) * np.cos(t), np.cos(t / 2.0) * np.sin(t), np.sin(t / 2.0)], axis=1)
    v = np.concatenate([mid - 4.0 * w, mid + 4.0 * w]).astype(np.float32)      # vertex i and i + m: the two sides at angle t_i
    f = []
    for i in range(m):
        a, b = i, i + m
        c, d = ((i + 1, i + 1 + m) if i + 1 < m else (m, 0))                   # the last quad meets the first one twisted
        f += [(a, c, b), (c, d, b)]
    return v, np.array(f, np.int32)


def reversed_faces(faces, seed=5, share=0.3):
    f = np.array(faces, np.int32).reshape(-1, 3)
    mask = np.random.default_rng(seed).random(len(f)) < share
    f[mask] = f[mask][:, [0, 2, 1]]
    return np.ascontiguousarray(f), mask


def with_holes(verts, faces, single=(100, 20000, 20001), rings=(5000, 9000)):
    """the mesh without the faces `single` and without every face at the vertices `rings` -> (mesh, the faces taken out)"""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    gone = np.zeros(len(f), bool)
    gone[list(single)] = True
    for r in rings:
        gone |= (f == r).any(axis=1)
    return (np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(f[~gone])), f[gone]


def touching_holes(verts, faces, vertex=5000):
    """two faces of one vertex's fan that share no edge taken out: two holes that touch in that vertex"""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    fan = np.nonzero((f == vertex).any(axis=1))[0]
    a = int(fan[0])
    far = [int(g) for g in fan[1:] if len(set(f[a].tolist()) & set(f[g].tolist())) == 1]
    gone = np.zeros(len(f), bool)
    gone[[a, far[0]]] = True
    return np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(f[~gone])


def fin_on_open_box(box):
    """the box without face 0 and a third face on an inner edge at a corner of the hole: the rotation about that corner meets a
    non-manifold edge, so the hole's chain is blocked there"""
    bv, bf = box
    v = np.concatenate([bv, bv[:1] + np.float32([[7, -9, -11]])]).astype(np.float32)
    f0 = bf[0].tolist()
    a = f0[0]
    x = [int(u) for g in bf[1:] if a in g for u in g if int(u) not in f0][0]
    return v, np.ascontiguousarray(np.concatenate([bf[1:], [[a, x, len(bv)]]]).astype(np.int32))


def small_cases(meshes):
    """meshes: dict with "box" and "humerus_left" -> name -> mesh: the small shapes that can still go wrong.  An upload takes no mesh
    with fewer than four faces, so the single triangle and the tetrahedron without a face stand beside a box, as shells of their own;
    lone_cases() has them alone, for the oracle and the host twin."""
    box, (lv, lf) = meshes["box"], meshes["humerus_left"]
    tv, tf = TO.tetrahedron()
    out = {"box": box, "box inside out": (box[0], box[1][:, [0, 2, 1]]), "box, face 5 flipped": (box[0], np.concatenate([box[1][:5], box[1][5:6][:, [0, 2, 1]], box[1][6:]])),
           "box without face 0": (box[0], box[1][1:]), "single triangle": TO.join((tv, tf[:1]), box), "tetrahedron minus one face": TO.join((tv, tf[1:]), box),
           "mobius strip": mobius(10), "fin on an open box": fin_on_open_box(box), "two boxes": TO.two_boxes(box),
           "box and loose triangles": TO.join(box, TO.loose_triangles(5)), "fan of 300": TO.fan(300),
           "degenerate faces": TO.with_degenerate(lv, lf[:513], (0, 1, 100, 255, 256, 300, 519)),
           "only degenerate faces": (lv[:8], np.array([[0, 1, 1], [2, 2, 3], [4, 5, 4], [6, 6, 6]], np.int32))}
    for n in (255, 256, 257):
        out[f"humerus_left[:{n}]"] = (lv, reversed_faces(lf[:n], seed=n)[0])
    return {k: (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)) for k, (v, f) in out.items()}


def lone_cases():
    tv, tf = TO.tetrahedron()
    return {"single triangle, alone": (tv, np.ascontiguousarray(tf[:1])), "tetrahedron minus one face, alone": (tv, np.ascontiguousarray(tf[1:]))}


VARIANTS = [("outward, centroid", dict()), ("outward, fan", dict(fill=FAN)), ("winding, none", dict(orient=WINDING, fill=FILL_NONE)),
            ("none, centroid", dict(orient=NONE)), ("nested, fan, 2 holes", dict(orient=NESTED, fill=FAN, max_holes=2)),
            ("outward, centroid, short holes", dict(max_hole_edges=3))]


# ---- the ctypes side of the host twin --------------------------------------------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("repair", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.rc_repair.argtypes, L.rc_repair.restype = [vp, i, vp, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp], None
    L.rc_precheck.argtypes = [i, i, i, i, i, i, i, i, i, i, i, vp, i]
    L.rc_plan.argtypes, L.rc_plan.restype = [i, i, i, vp, vp, vp, vp], None
    L.rc_sizes.argtypes, L.rc_sizes.restype = [vp], None
    return L


def host_repair(shim, verts, faces, orient=OUTWARD, fill=CENTROID, max_hole_edges=4096, max_shells=64, max_holes=64, max_rounds=MAX_ROUNDS, topo_rounds=TO.MAX_ROUNDS):
    """the host twin of the kernels for one mesh, on the oracle's topology -> the dict of repair() (without absw)"""
    from shoulder_amd import _lib
    v, f = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    t = TO.topology(v, f, max_shells=max_shells, max_rounds=topo_rounds)
    tinfo, tshells = np.array([t["info"]]), np.ascontiguousarray(t["shells"])
    border = max(int(tinfo[0]["border_edges"]), 0)
    opt = np.array([orient, fill, max_hole_edges, max_holes, max_rounds, 0], np.int32)
    out = dict(info=np.zeros(1, dtype=_lib.REPAIR_INFO_DTYPE), shells=np.zeros(max_shells, dtype=_lib.REPAIR_SHELL_DTYPE), holes=np.zeros(max_holes, dtype=_lib.REPAIR_HOLE_DTYPE),
               flip=np.zeros(len(f), np.uint8), faces=np.zeros((len(f) + border, 3), np.int32), verts=np.zeros((len(v) + border // 3, 3), np.float32))
    shim.rc_repair(v.ctypes.data, len(v), f.ctypes.data, len(f), np.ascontiguousarray(t["adj"]).ctypes.data, np.ascontiguousarray(t["label"]).ctypes.data, tinfo.ctypes.data,
                   tshells.ctypes.data, int(max_shells), opt.ctypes.data, *[out[n].ctypes.data for n in ("info", "shells", "holes", "flip", "faces", "verts")])
    out["info"] = out["info"][0]
    out["faces"], out["verts"] = out["faces"][:int(out["info"]["faces_out"])], out["verts"][:int(out["info"]["verts_out"])]
    return out
