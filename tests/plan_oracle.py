"""CPU oracle of the implant plans (include/shoulder_hip.h sh_resect_plan), test infrastructure shared by tests/test_plan_host.py,
tests/test_gpu_plan.py and tools/time_plan.py: a NumPy float64 statement of the header's definitions -- the references from mesh,
frame and plane in canal_map_point's order of operations, the three parts of a cost from FETCHED records, the ranking with
np.lexsort on (i, cost) -- and the ctypes side of tests/hostcheck/plan_check.cpp.  Every expression is written operation by
operation as sh_scalar.h plan_* writes it, so that with contraction off the device's numbers are expected bit for bit."""
import ctypes

import numpy as np

import host_twin

GEOMETRY, ARG, STATE = -5, -1, -3
RULE_FIELDS = ("max_overhang", "min_coverage", "min_clearance", "max_eccentricity", "fill_target", "margin",
               "w_uncovered", "w_overhang", "w_cor", "w_height", "w_eccentricity", "w_fill")
TERM_DTYPE = np.dtype([("cost", "<f8"), ("feasible", "<i4"), ("pad", "<i4")])


def rule(**kw):
    """a full rule from the fields given: missing limits are off, everything else 0 (what Engine.plan does)"""
    r = dict(max_overhang=np.inf, min_coverage=-np.inf, min_clearance=-np.inf, max_eccentricity=np.inf, fill_target=0.0, margin=0.0,
             w_uncovered=0.0, w_overhang=0.0, w_cor=0.0, w_height=0.0, w_eccentricity=0.0, w_fill=0.0)
    assert set(kw) <= set(r), kw
    r.update({k: float(v) for k, v in kw.items()})
    return r


def norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def map_row(T, i, x, y, z):
    """row i of canal_map_point"""
    return ((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]


def reference(verts, T, plane, margin, status=0):
    """the fields of sh_plan_ref (without n_feasible) of one humerus: verts float32 (nv, 3) CT, T its frame, plane (point, normal) CT"""
    none = dict(tuberosity_top=np.zeros(3), tuberosity_z=0.0, head_apex=np.zeros(3), head_apex_z=0.0, head_height=0.0,
                tuberosity_vid=-1, head_apex_vid=-1, status=status)
    if status != 0:
        return none
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    o, n = np.asarray(plane, dtype=np.float64).reshape(6)[:3], np.asarray(plane, dtype=np.float64).reshape(6)[3:]
    s = ((v[:, 0] - o[0]) * n[0] + (v[:, 1] - o[1]) * n[1]) + (v[:, 2] - o[2]) * n[2]
    z = map_row(T, 2, v[:, 0], v[:, 1], v[:, 2])
    head, tub = s > 0.0, s <= -(margin * norm3(n[0], n[1], n[2]))
    if not head.any() or not tub.any():
        return dict(none, status=GEOMETRY)
    hv = int(np.argmax(np.where(head, z, -np.inf)))      # (argmax takes the first of equals: the smaller id)
    tv = int(np.argmax(np.where(tub, z, -np.inf)))
    return dict(tuberosity_top=v[tv], tuberosity_z=z[tv], head_apex=v[hv], head_apex_z=z[hv], head_height=z[hv] - z[tv],
                tuberosity_vid=tv, head_apex_vid=hv, status=0)


def entries(T, o, n):
    """stem_entry for planes (P, 3) + (P, 3): exists (P,), entry in CT (P, 3)"""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    of = [map_row(T, i, o[:, 0], o[:, 1], o[:, 2]) for i in range(3)]
    un = [(T[i, 0] * n[:, 0] + T[i, 1] * n[:, 1]) + T[i, 2] * n[:, 2] for i in range(3)]
    ln = norm3(*un)
    with np.errstate(all="ignore"):
        ok = (ln > 0.0) & (ln < 1e300)
        un = [u / ln for u in un]
        ok &= np.abs(un[2]) >= 1e-12
        z = of[2] + (of[0] * un[0] + of[1] * un[1]) / un[2]
        ok &= np.abs(z) < 1e300
    back = [0.0 - T[0, 3], 0.0 - T[1, 3], z - T[2, 3]]
    entry = np.stack([(T[0, j] * back[0] + T[1, j] * back[1]) + T[2, j] * back[2] for j in range(3)], axis=-1)
    return ok, entry


def terms(r, rec, fit, seat, stem, heads, T, ref):
    """The three parts of one humerus from its fetched records: rec, fit (P,), seat (P, K_h), stem (P, K_s), heads (K_h, 2) as (radius,
    thickness), T its frame, ref its reference (a dict of reference() or a PLAN_REF_DTYPE row).
    -> dict of cut / head / stem cost and feasible arrays and the unweighted terms"""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    heads = np.asarray(heads, dtype=np.float64).reshape(-1, 2)
    o, n = rec["plane_point"], rec["plane_normal"]
    with np.errstate(all="ignore"):
        has_entry, entry = entries(T, o, n)
        sc0 = seat[:, 0]["seat_center"]
        d = sc0 - entry
        exists = (int(ref["status"]) == 0) & (rec["status"] == 0) & (rec["n_loops"] >= 1) & (seat[:, 0]["status"] == 0) & has_entry
        ecc = np.where(exists, norm3(d[:, 0], d[:, 1], d[:, 2]), 0.0)
        cut_cost = r["w_eccentricity"] * ecc
        cut_ok = exists & ((not r["w_cor"] > 0.0) | (fit["sphere_status"] == 0)) & (ecc <= r["max_eccentricity"])
        cov, ovh, cs, sc = seat["coverage"], seat["max_overhang"], seat["cor_shift"], seat["seat_center"]
        unc, cor = 1.0 - cov, norm3(cs[..., 0], cs[..., 1], cs[..., 2])
        nl = norm3(n[:, 0], n[:, 1], n[:, 2])
        apex = np.stack([sc[..., i] + (heads[None, :, 1] * n[:, None, i]) / nl[:, None] for i in range(3)], axis=-1)
        apex_z = map_row(T, 2, apex[..., 0], apex[..., 1], apex[..., 2])
        height = np.abs(apex_z - float(ref["head_apex_z"]))
        head_cost = ((r["w_uncovered"] * unc + r["w_overhang"] * ovh) + r["w_cor"] * cor) + r["w_height"] * height
        head_ok = (ovh <= r["max_overhang"]) & (cov >= r["min_coverage"])
        fill = np.abs(stem["fill_mean"] - r["fill_target"])
        stem_cost = r["w_fill"] * fill
        stem_ok = (stem["status"] == 0) & (stem["fits"] == 1) & (stem["min_clearance"] >= r["min_clearance"])
    return dict(cut_cost=cut_cost, cut_ok=cut_ok, ecc=ecc, head_cost=head_cost, head_ok=head_ok, uncovered=unc, overhang=ovh, cor=cor, height=height,
                apex=apex, apex_z=apex_z, head_height=apex_z - float(ref["tuberosity_z"]), stem_cost=stem_cost, stem_ok=stem_ok, fill=fill)


def rank(cut_cost, cut_ok, head_cost, head_ok, stem_cost, stem_ok, compat, N):
    """cut (P,), head (P, K_h), stem (P, K_s) parts -> (indices i of the first N feasible candidates in (cost, i) order, their costs,
    n_feasible); compat (K_h, K_s) booleans or None"""
    P, Kh = head_cost.shape
    Ks = stem_cost.shape[1]
    with np.errstate(all="ignore"):
        cost = (head_cost[:, :, None] + stem_cost[:, None, :]) + cut_cost[:, None, None]
    ok = np.asarray(cut_ok, bool)[:, None, None] & np.asarray(head_ok, bool)[:, :, None] & np.asarray(stem_ok, bool)[:, None, :] & ~np.isnan(cost)
    if compat is not None:
        ok = ok & np.asarray(compat, bool)[None, :Kh, :Ks]
    idx = np.nonzero(ok.reshape(-1))[0]
    c = cost.reshape(-1)[idx]
    order = np.lexsort((idx, c))[:N]
    return idx[order], c[order], len(idx)


def plans(r, rec, fit, seat, stem, heads, T, ref, compat, N):
    """what sh_resect_plan returns for one humerus, from its fetched records: (N,) PLAN_DTYPE rows and n_feasible"""
    from shoulder_amd import _lib
    out = np.zeros(N, dtype=_lib.PLAN_DTYPE)
    out["cut"] = out["head"] = out["stem"] = -1
    out["status"] = int(ref["status"]) if int(ref["status"]) != 0 else GEOMETRY
    if int(ref["status"]) != 0:
        return out, 0
    t = terms(r, rec, fit, seat, stem, heads, T, ref)
    idx, cost, nf = rank(t["cut_cost"], t["cut_ok"], t["head_cost"], t["head_ok"], t["stem_cost"], t["stem_ok"], compat, N)
    Kh, Ks = seat.shape[1], stem.shape[1]
    for k, (i, c) in enumerate(zip(idx, cost)):
        q, ks = divmod(int(i), Ks)
        p, kh = divmod(q, Kh)
        o = out[k]
        o["cost"], o["uncovered"], o["overhang"], o["cor"], o["height"] = c, t["uncovered"][p, kh], t["overhang"][p, kh], t["cor"][p, kh], t["height"][p, kh]
        o["eccentricity"], o["fill"], o["apex"], o["apex_z"], o["head_height"] = t["ecc"][p], t["fill"][p, ks], t["apex"][p, kh], t["apex_z"][p, kh], t["head_height"][p, kh]
        o["cut"], o["head"], o["stem"], o["status"] = p, kh, ks, 0
    return out, nf


def rank_fetched(cut_terms, head_terms, stem_terms, compat, N):
    """rank() on the three compact arrays of one humerus as fetched ("plan.*_terms": TERM_DTYPE of shapes (P,), (P, K_h), (P, K_s))"""
    return rank(cut_terms["cost"], cut_terms["feasible"] != 0, head_terms["cost"], head_terms["feasible"] != 0, stem_terms["cost"],
                stem_terms["feasible"] != 0, compat, N)


def compat_words(compat, Kh):
    """(K_h, K_s) booleans -> the K_h uint64 words of the C call"""
    cm = np.asarray(compat, dtype=bool)
    return np.ascontiguousarray((cm.astype(np.uint64) << np.arange(cm.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)[:Kh])


def build_shim(directory, sanitize=False):
    """tests/hostcheck/plan_check.cpp compiled as the device compiles it (-ffp-contract=off) -> ctypes library; sanitize=True: the
    stand-alone program with -fsanitize=address,undefined instead -> its path (it is run as a program, never loaded)"""
    L = host_twin.build_shim("plan", directory, sanitize)
    if sanitize:
        return L
    d, vp, i = ctypes.c_double, ctypes.c_void_p, ctypes.c_int
    L.pc_ref.argtypes, L.pc_ref.restype = [vp, i, vp, vp, d, i, vp], None
    L.pc_cut_term.argtypes, L.pc_cut_term.restype = [vp, i, i, i, i, i, vp, vp, vp, vp], None
    L.pc_head_term.argtypes, L.pc_head_term.restype = [vp, d, d, vp, vp, vp, d, vp, d, vp, vp], None
    L.pc_stem_term.argtypes, L.pc_stem_term.restype = [vp, i, i, d, d, vp], None
    L.pc_candidate.argtypes, L.pc_candidate.restype = [vp, vp, vp, ctypes.c_uint64, i, vp], i
    L.pc_select.argtypes, L.pc_select.restype = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp, vp], None
    return L


def rule_array(r):
    return np.array([r[k] for k in RULE_FIELDS], dtype=np.float64)


def host_ref(S, verts, T, plane, margin, status=0):
    from shoulder_amd import _lib
    v, T, pl = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(T, np.float64), np.ascontiguousarray(plane, np.float64)
    out = np.zeros(1, dtype=_lib.PLAN_REF_DTYPE)
    S.pc_ref(v.ctypes.data, len(v), T.ctypes.data, pl.ctypes.data, float(margin), int(status), out.ctypes.data)
    return out[0]


def host_select(S, cut_terms, head_terms, stem_terms, compat, N, tuberosity_z=0.0):
    """the host twin of k_plan_select on TERM_DTYPE arrays (P,), (P, K_h), (P, K_s): -> (N,) PLAN_DTYPE rows, n_feasible.  The
    unweighted terms it copies are the costs themselves here (what is under test is the selection)."""
    from shoulder_amd import _lib
    P, Kh = head_terms.shape
    Ks = stem_terms.shape[1]
    ct, ht, st = (np.ascontiguousarray(a, dtype=TERM_DTYPE) for a in (cut_terms, head_terms, stem_terms))
    cv, sv = np.ascontiguousarray(ct["cost"]), np.ascontiguousarray(st["cost"])
    hv = np.zeros((P, Kh, 8))
    hv[..., 0] = ht["cost"]
    words = np.full(64, ~np.uint64(0), dtype=np.uint64)
    if compat is not None:
        words[:Kh] = compat_words(compat, Kh)
    ref = np.zeros(1, dtype=_lib.PLAN_REF_DTYPE)
    ref["tuberosity_z"] = tuberosity_z
    out = np.zeros(N, dtype=_lib.PLAN_DTYPE)
    S.pc_select(ct.ctypes.data, ht.ctypes.data, st.ctypes.data, cv.ctypes.data, hv.ctypes.data, sv.ctypes.data, words.ctypes.data, P, Kh, Ks, N,
                ref.ctypes.data, out.ctypes.data)
    return out, int(ref[0]["n_feasible"])
