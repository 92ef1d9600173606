"""NumPy statement of sh_vertex_fields (include/shoulder_hip.h "vertex normals and discrete curvatures of the resident batch"): the face
records, the vertex sums in the order of the rows, the results, the flags and the Jacobi rounds of the smoothing.  float64, one ufunc
per operation of the rule (NumPy contracts nothing), the rows walked position by position so that every accumulator adds its terms in
ascending face index.  The incidence and the adjacency come from tests/topo_oracle.py.  Also the bound on the fields an atan2 enters,
the comparison both test files use, the icosphere and the ctypes side of the host twin."""
import ctypes

import numpy as np

import host_twin
import topo_oracle as TO

ARG, STATE, GEOMETRY = -1, -3, -5
AREA, ANGLE, MAX_SMOOTH, FIELDS, FACE = 0, 1, 64, 8, 10
USED, BORDER, NONMANIFOLD, FLAT = 1, 2, 4, 8
NAMES = ("area", "angle_sum", "defect", "gauss", "mean", "gauss_smooth", "mean_smooth")
U = 2.0 ** -53                 # the unit roundoff of float64
ATAN = 4 * 2.0 ** -51          # 4 ulp of an angle in [2, 4): the project's figure for atan2 between two math libraries (winding_oracle.bound)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def face_records(verts, faces):
    """-> (F, 10): n[3], A2, angle[3], cot[3]; ten zeros for a flat face"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    P = v[f]
    n = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    A2 = np.sqrt(_dot(n, n))
    rec = np.zeros((len(f), FACE))
    rec[:, :3], rec[:, 3] = n, A2
    with np.errstate(all="ignore"):
        for k in range(3):
            e1, e2 = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
            d = _dot(e1, e2)
            rec[:, 4 + k], rec[:, 7 + k] = np.arctan2(A2, d), d / A2
    flat = TO.degenerate(f) | (A2 == 0.0) | ~np.isfinite(A2)
    rec[flat] = 0.0
    return rec


def _rows(vrow, vface):
    """the rows position by position: yields (the vertices with a face at position j, that face)"""
    valence = np.diff(vrow)
    for j in range(int(valence.max()) if len(valence) else 0):
        sel = np.nonzero(valence > j)[0]
        yield sel, vface[vrow[sel] + j].astype(np.int64)


def smooth_round(f, a2, vrow, vface, s):
    """one Jacobi round of the rule on one array s (V,)"""
    den, acc = np.zeros(len(s)), np.zeros(len(s))
    for sel, fj in _rows(vrow, vface):
        live = a2[fj] != 0.0
        sel, fj = sel[live], fj[live]
        fm = ((s[f[fj, 0]] + s[f[fj, 1]]) + s[f[fj, 2]]) / 3.0
        den[sel] += a2[fj]
        acc[sel] += a2[fj] * fm
    with np.errstate(all="ignore"):
        return np.where(den == 0.0, 0.0, acc / den)


def vertex_fields(verts, faces, weight=AREA, smooth=0):
    """one mesh -> dict(face (F, 10), normals (V, 3), fields (V, 8), flags, status, the seven named fields, and what bound() reads)"""
    v32 = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    vrow, vface = TO.incidence(f, V)
    adj = TO.adjacency(f)[0]
    rec = face_records(v32, f)
    a2 = rec[:, 3]
    s, angle_sum, N, L = np.zeros(V), np.zeros(V), np.zeros((V, 3)), np.zeros((V, 3))
    flags, terms = np.where(np.diff(vrow) > 0, USED, 0).astype(np.int32), np.zeros(V, np.int64)
    for sel, fj in _rows(vrow, vface):
        k = np.argmax(f[fj] == sel[:, None], axis=1)
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        a0, a1 = adj[fj, k], adj[fj, k2]
        flags[sel[(a0 == TO.BORDER) | (a1 == TO.BORDER)]] |= BORDER
        flags[sel[(a0 == TO.NONMANIFOLD) | (a1 == TO.NONMANIFOLD)]] |= NONMANIFOLD
        live = a2[fj] != 0.0
        flags[sel[~live]] |= FLAT
        sel, fj, k, k1, k2 = sel[live], fj[live], k[live], k1[live], k2[live]
        r = rec[fj]
        i = np.arange(len(fj))
        w = r[i, 4 + k]
        s[sel] += r[:, 3]
        angle_sum[sel] += w
        N[sel] += (r[:, :3] / r[:, 3:4]) * w[:, None] if weight == ANGLE else r[:, :3]
        c1, c2 = r[i, 7 + k1], r[i, 7 + k2]
        Pv, p1, p2 = v[sel], v[f[fj, k1]], v[f[fj, k2]]
        L[sel] += c1[:, None] * (Pv - p2) + c2[:, None] * (Pv - p1)
        terms[sel] += 1
    length = np.sqrt(_dot(N, N))
    unit = (length != 0.0) & np.isfinite(length)
    area = s / 6.0
    border = (flags & BORDER) != 0
    with np.errstate(all="ignore"):
        normals = np.where(unit[:, None], N / length[:, None], 0.0)
        defect = np.where(border, 3.141592653589793, 6.283185307179586) - angle_sum
        gauss, mean = defect / area, _dot(L, normals) / (4.0 * area)
    none = area == 0.0
    defect, gauss, mean = np.where(none, 0.0, defect), np.where(none, 0.0, gauss), np.where(none, 0.0, mean)
    gs, ms = gauss, mean
    for _ in range(smooth):
        gs, ms = smooth_round(f, a2, vrow, vface, gs), smooth_round(f, a2, vrow, vface, ms)
    fields = np.zeros((V, FIELDS))
    for i, x in enumerate((area, angle_sum, defect, gauss, mean, gs, ms)):
        fields[:, i] = x
    out = dict(face=rec, normals=np.ascontiguousarray(normals), fields=fields, flags=flags, status=np.int32(0 if (a2 != 0.0).any() else GEOMETRY),
               weight=weight, smooth=smooth, terms=terms, length=length, L1=np.abs(L).sum(axis=1), mesh=(f, a2, vrow, vface))
    out.update({n: fields[:, i] for i, n in enumerate(NAMES)})
    return out


def bound(want):
    """How far two evaluations of the rule may lie apart when their atan2 differ by up to 4 ulp per term (ATAN) and every operation
    behind an atan2 rounds once in each evaluation (U each, so 2 U per operation) -> dict of bounds by field, from the oracle's values.
      angle         ATAN.
      angle_sum     n terms: n ATAN, and n additions whose partial sums are at most the sum S itself: 2 n U (S + n ATAN).
      defect        one subtraction more: 2 U (|defect| + E_sum).
      gauss         one division by the area, which is the same bytes in both: E_defect / area + 2 U (|gauss| + E_defect / area).
      normals       (angle weights) a term (n_c / A2) angle has |n_c / A2| <= 1 in both the same bytes: ATAN and the product's rounding
                    2 U 4 per term, and the additions as for angle_sum (the partial sums of a component are at most S): E_N per
                    component.  Normalising: 2 sqrt(3) E_N / |N|, and 16 U for dot3, sqrt and the division in both evaluations.
      mean          (angle weights) L is the same bytes: (|L|_1 (E_normal + 6 U)) / (4 area) for the dot product, 2 U for the division.
      *_smooth      a round is a weighted mean W: E' = W(E) + 2 (2 n + 8) U W(|s|) -- per face two additions, a division and a product,
                    then n additions into each of the two sums and the last division."""
    n, S, area = want["terms"].astype(np.float64), want["angle_sum"], want["area"]
    f, a2, vrow, vface = want["mesh"]
    with np.errstate(all="ignore"):
        e_sum = n * ATAN + 2 * n * U * (S + n * ATAN)
        e_def = e_sum + 2 * U * (np.abs(want["defect"]) + e_sum)
        e_gauss = np.where(area == 0.0, 0.0, e_def / area + 2 * U * (np.abs(want["gauss"]) + e_def / area))
        e_def = np.where(area == 0.0, 0.0, e_def)
        out = dict(angle=ATAN, angle_sum=e_sum, defect=e_def, gauss=e_gauss)
        e_mean = np.zeros(len(n))
        if want["weight"] == ANGLE:
            e_N = n * (ATAN + 8 * U) + 2 * n * U * (S + n * ATAN)
            e_normal = np.where(n == 0, 0.0, 2 * np.sqrt(3.0) * e_N / want["length"] + 16 * U)
            t = want["L1"] * (e_normal + 6 * U) / (4.0 * area)
            e_mean = np.where(area == 0.0, 0.0, t + 2 * U * (np.abs(want["mean"]) + t))
            out.update(normals=e_normal[:, None], mean=e_mean)

        def rounds(e, s):
            s = s.copy()
            for _ in range(want["smooth"]):
                e = smooth_round(f, a2, vrow, vface, e) + 2 * (2 * n + 8) * U * smooth_round(f, a2, vrow, vface, np.abs(s))
                s = smooth_round(f, a2, vrow, vface, s)
            return e
        out["gauss_smooth"] = rounds(e_gauss, want["gauss"])
        if want["weight"] == ANGLE:
            out["mean_smooth"] = rounds(e_mean, want["mean"])
    return out


def compare(got, want, tag, show=True):
    """got: dict(face, normals, fields, flags, status) of one mesh against the oracle's.  As bytes: n, A2 and cot of the face records,
    area, the last field, the flags and the status, and with area weights the normals, mean and mean_smooth.  Within bound(want):
    the angles, angle_sum, defect, gauss, gauss_smooth, and with angle weights the normals, mean and mean_smooth.  The largest
    difference of every bounded comparison is printed beside its bound.  -> dict field -> (largest difference, its bound)"""
    gf, wf = np.asarray(got["face"]).reshape(-1, FACE), want["face"]
    for cols, what in (((0, 1, 2, 3), "n, A2"), ((7, 8, 9), "cot")):
        assert np.ascontiguousarray(gf[:, cols]).tobytes() == np.ascontiguousarray(wf[:, cols]).tobytes(), (tag, "vert.face", what)
    G, W = np.asarray(got["fields"]).reshape(-1, FIELDS), want["fields"]
    exact = [0, 7] + ([4, 6] if want["weight"] == AREA else [])
    for i in exact:
        assert np.ascontiguousarray(G[:, i]).tobytes() == np.ascontiguousarray(W[:, i]).tobytes(), (tag, "vert.fields", i)
    assert np.asarray(got["flags"], np.int32).tobytes() == want["flags"].tobytes(), (tag, "vert.flags")
    assert int(got["status"]) == int(want["status"]), (tag, "vert.status", int(got["status"]))
    gn = np.asarray(got["normals"]).reshape(-1, 3)
    if want["weight"] == AREA:
        assert gn.tobytes() == want["normals"].tobytes(), (tag, "vert.normal")
    lim = bound(want)
    pairs = [("angle", gf[:, 4:7], wf[:, 4:7])] + [(n, G[:, 1 + i], W[:, 1 + i]) for i, n in enumerate(NAMES[1:]) if n in lim]
    if want["weight"] == ANGLE:
        pairs.append(("normals", gn, want["normals"]))
    seen = {}
    for name, g, w in pairs:
        diff = np.abs(g - w)
        b = np.broadcast_to(lim[name], diff.shape)
        assert np.isfinite(g).all() and np.all(diff <= b), (tag, name, float(diff.max()), float(b.ravel()[np.argmax(diff)]))
        at = int(np.argmax(diff)) if diff.size else 0
        seen[name] = (float(diff.ravel()[at]), float(b.ravel()[at])) if diff.size else (0.0, 0.0)
    if show:
        print(f"{tag} weight {want['weight']} smooth {want['smooth']}: " + ", ".join(f"{k} {d:.3g} <= {b:.3g}" for k, (d, b) in seen.items()))
    return seen


# ---- the test meshes -------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=25.0):
    """the icosahedron subdivided in its flat faces (plain midpoints) and projected onto the sphere ONCE, at the end -- the mesh the
    figures of the issue were computed on (projecting after every level gives mean R down to 0.9898 at two subdivisions); float64, then
    rounded to float32 once; outward normals"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                v.append((v[a] + v[b]) / 2.0)
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    v = np.asarray(v)
    return (v / np.linalg.norm(v, axis=1)[:, None] * radius).astype(np.float32), np.asarray(f, np.int32)


def flat_face_mesh(box):
    """the box and one face of zero area with three distinct indices: corners 0 and 1 and a new vertex half way between them"""
    v, f = box
    v = np.concatenate([v, ((v[0].astype(np.float64) + v[1]) / 2.0).astype(np.float32)[None]])
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(np.concatenate([f, [[0, 1, 8]]]).astype(np.int32))


def small_cases(meshes):
    """the shapes at which the kernels can go wrong: name -> mesh.  meshes: topo_oracle.table's dict (box, humerus_left ...)"""
    T, further = TO.table(meshes), TO.further(meshes)
    out = {"tetrahedron": further["tetrahedron"]}
    for n in ("box", "box without face 0", "box, face 5 flipped", "fan of 300", "strip of 600, shuffled", "humerus_left[:255]", "humerus_left[:256]", "humerus_left[:257]"):
        out[n] = T[n][0]
    for n in ("boxes sharing an edge", "degenerate faces", "degenerate faces, four faces", "only degenerate faces"):
        out[n] = further[n]
    out["box with a flat face"] = flat_face_mesh(meshes["box"])
    out["icosphere 2"] = icosphere(2)
    return out


# ---- the ctypes side of the host twin (tests/hostcheck/vert_check.cpp) ----------------------------------------------------------------
def build_shim(directory, sanitize=False):
    L = host_twin.build_shim("vert", directory, sanitize, std="c++17")
    if sanitize:
        return L
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.vc_fields.argtypes, L.vc_fields.restype = [vp, i, vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp], None
    L.vc_precheck.argtypes = [i, i, i, i, i, i, vp, i]
    L.vc_plan.argtypes, L.vc_plan.restype = [i, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, vp], None
    return L


def host_fields(shim, verts, faces, weight=AREA, smooth=0):
    """the host twin of the kernels for one mesh (incidence and adjacency from topo_oracle) -> dict(face, normals, fields, flags, status)"""
    v, f = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    vrow, vface = TO.incidence(f, len(v))
    adj = np.ascontiguousarray(TO.adjacency(f)[0].ravel(), np.int32)
    out = dict(face=np.zeros((len(f), FACE)), normals=np.zeros((len(v), 3)), fields=np.zeros((len(v), FIELDS)), flags=np.zeros(len(v), np.int32), status=np.zeros(1, np.int32))
    shim.vc_fields(v.ctypes.data, len(v), f.ctypes.data, len(f), vrow.ctypes.data, vface.ctypes.data, adj.ctypes.data, int(weight), int(smooth),
                   *[out[n].ctypes.data for n in ("face", "normals", "fields", "flags", "status")])
    out["status"] = out["status"][0]
    return out
