"""`HumeralHeadOsteotomy` -- resection of the humeral head at, or offset from, the anatomic-neck plane.

Same public surface as reference `src/shoulder/arthroplasty.py:13-175` (`plane`, `neckshaft_rel`, `retroversion_rel`,
`points()`, `resect_mesh()`, `offset_retroversion`, `offest_neckshaft` [sic], `offset_depth`, `offset_anterior_posterior`,
`offset_medial_lateral`), with its own bookkeeping: the resection plane is a (point, normal) pair of arrays kept in the
canal / articular coordinate system, where retroversion and neck-shaft angle are the two spherical angles of the normal;
every offset is one of two primitives (turn the normal by spherical-angle increments, shift the point), and `plane` maps
the pair into whatever coordinate system the humerus currently has.  The two mesh operations run on the device through
`sh_slice_mesh_planes` (k_clip.h): a resection sends the plane and its mirror image in one pass.

Results are pinned against the reference's own class (tests/golden/make_osteotomy_golden.py, tests/test_osteotomy_golden.py),
including its quirk that reading `retroversion_rel` flips the sign of the stored normal's x component.
"""
from typing import Tuple

import numpy as np

from .base import Mesh, Plane
from .csys import inv_transform, spherical_to_unitxyz, transform_plane_pn, unitxyz_to_spherical

_DEPTH_DIRECTIONS = ("canal", "anp", "resection")


class HumeralHeadOsteotomy:
    def __init__(self, humerus) -> None:
        self._humerus = humerus
        caller_csys = np.array(humerus._tfrm.matrix, dtype=np.float64)
        # visit the canal / articular csys once to read the anatomic-neck plane there, then hand the caller's csys back
        # (through CT: every matrix of the facade is CT-based) -- arthroplasty.py:18-31
        humerus.apply_csys_canal_articular()
        self._to_anp = np.array(humerus._tfrm.matrix, dtype=np.float64)
        native = humerus.anatomic_neck.plane()
        self._native_point = np.array(native.point, dtype=np.float64)
        self._native_normal = np.array(native.normal, dtype=np.float64)
        self._point = self._native_point.copy()
        self._normal = self._native_normal.copy()
        humerus.apply_csys_ct()
        humerus.apply_csys_custom(caller_csys)

    # ---- state ---------------------------------------------------------------------------------------
    def _side_sign(self) -> float:
        """+1 for a right humerus, -1 for a left one: the sense in which retroversion / anterior count (arthroplasty.py:97-100, :155-158)."""
        return 1.0 if self._humerus.side() == "right" else -1.0

    def _turn(self, d_theta=0.0, d_phi=0.0) -> None:
        r, theta, phi = unitxyz_to_spherical(self._normal)
        self._normal = spherical_to_unitxyz(np.array([r, theta + d_theta, phi + d_phi]))

    def _shift(self, vec) -> None:
        self._point = self._point + np.asarray(vec, dtype=np.float64)

    @property
    def plane(self) -> Plane:
        """the resection plane in the humerus's current csys (arthroplasty.py:33-40): anp csys -> CT -> current"""
        p, n = transform_plane_pn(self._point, self._normal, inv_transform(self._to_anp))
        return Plane(*transform_plane_pn(p, n, self._humerus._tfrm.matrix))

    @property
    def neckshaft_rel(self):
        """neck-shaft angle of the cut minus the native one, degrees (arthroplasty.py:42-54)"""
        phi_cut = unitxyz_to_spherical(self._normal)[2]
        phi_native = unitxyz_to_spherical(self._native_normal)[2]
        return (180 - phi_cut) - (180 - phi_native)

    @property
    def retroversion_rel(self):
        """retroversion of the cut, degrees, measured from -x (arthroplasty.py:56-67).  As in the reference the mirrored x
        stays in the stored normal, so two consecutive reads differ in sign and the second restores the state."""
        self._normal[0] = -self._normal[0]
        theta = unitxyz_to_spherical(self._normal)[1]
        return theta * (-1.0 if self._humerus.side() == "right" else 1.0)

    # ---- mesh operations (device) -----------------------------------------------------------------------
    def points(self):
        """closed polyline where the resection plane meets the bone: the loop of largest area (arthroplasty.py:69-78)"""
        cut = self.plane
        section = self._humerus.mesh.section(cut.normal, cut.point)
        if not section.discrete:
            raise ValueError("the resection plane does not cut the mesh")
        areas = [poly.area for poly in section.polygons_closed]
        return section.discrete[int(np.argmax(areas)) if len(section.entities) > 1 else 0]

    def resect_mesh(self) -> Tuple[Mesh, Mesh]:
        """(head, resected humerus) in the current csys (arthroplasty.py:80-87)"""
        cut = self.plane
        bone = self._humerus.mesh
        if bone._engine is None:
            raise RuntimeError("resect_mesh needs the HIP engine (no CPU fallback)")
        halves = bone._engine.slice_mesh_planes(bone.vertices, bone.faces, [cut.point, cut.point], [cut.normal, -cut.normal])
        return tuple(Mesh(v, f, bone._engine) for v, f in halves)

    def measure(self) -> dict:
        """What a planning sweep reads off the current cut, from the mesh resident on the device (sh_resect_planes with
        B = P = 1; nothing is uploaded, no mesh comes back): `head_volume`, `head_area`, `head_height`, `cut_area`,
        `cut_perimeter`, `cut_centroid`, `cap_area`, `n_loops`, `n_ring`, `n_cut_faces`, `status` and the plane that was cut,
        all in CT (the plane is mapped there through the inverse of the humerus' current matrix).  The reference has no
        accessor for these; its users call trimesh on `resect_mesh()`'s result."""
        cut = self.plane
        bone = self._humerus
        p, n = transform_plane_pn(cut.point, cut.normal, inv_transform(np.array(bone._tfrm.matrix, dtype=np.float64)))
        bone._ensure_loaded()
        rec = bone._engine.resect(planes=np.concatenate([p, n]).reshape(1, 1, 6))[0, 0]
        return {k: (rec[k].copy() if rec[k].ndim else rec[k].item()) for k in rec.dtype.names}

    def _plane_ct(self):
        cut = self.plane
        return transform_plane_pn(cut.point, cut.normal, inv_transform(np.array(self._humerus._tfrm.matrix, dtype=np.float64)))

    def head_fit(self) -> dict:
        """The sphere of the current cut's head piece and the ellipse of its cut (sh_resect_planes_fit with B = P = 1, the
        counterpart of `measure()`): the fields of sh_head_fit as a dict, in CT.  `center_articular` needs the humerus' landmarks on
        the device (NaN otherwise)."""
        p, n = self._plane_ct()
        bone = self._humerus
        bone._ensure_loaded()
        fit = bone._engine.resect(planes=np.concatenate([p, n]).reshape(1, 1, 6), fit=True)[1][0, 0]
        return {k: (fit[k].copy() if fit[k].ndim else fit[k].item()) for k in fit.dtype.names}

    def implant_head(self, catalogue=None) -> dict:
        """The planned spherical cap for the current cut, from `head_fit()` (the step the reference leaves open, arthroplasty.py:178-182)."""
        return implant_from_fit(self.head_fit(), self._humerus.side(), catalogue)

    def seat(self, catalogue, center="centroid") -> list:
        """How each head of `catalogue` -- (diameter, thickness) pairs, as `implant_from_fit` takes them -- sits on the current cut
        (sh_resect_planes_seat with B = P = 1): K dicts with the fields of sh_seat, in CT.  center: "centroid" (the cut's area
        centroid) or "sphere" (the foot of the fitted sphere's centre)."""
        cat = np.asarray(catalogue, dtype=np.float64).reshape(-1, 2)
        p, n = self._plane_ct()
        bone = self._humerus
        bone._ensure_loaded()
        heads = np.c_[0.5 * cat[:, 0], cat[:, 1]]
        seats = bone._engine.resect(planes=np.concatenate([p, n]).reshape(1, 1, 6), fit=True, heads=heads, seat_center=center)[2][0, 0]
        return [{k: (s[k].copy() if s[k].ndim else s[k].item()) for k in s.dtype.names} for s in seats]

    def _entry_height(self) -> float:
        """height, in the canal / articular frame, at which the canal axis pierces the current plane"""
        n = self._normal / np.linalg.norm(self._normal)
        return float(self._point[2] + (self._point[0] * n[0] + self._point[1] * n[1]) / n[2])

    def canal_profile(self, z0=None, dz=1.0, L=None, A=64, fetch=("levels",)):
        """The polar profile of the humerus about its canal axis in the canal / articular frame (sh_canal_profile with the frame this
        object read the anatomic-neck plane in): by default the grid starts 5 mm above the point where the axis enters the current
        plane, has dz = 1 mm and spans 160 mm.  Returns what Engine.canal_profile returns, for this humerus alone; the profile stays on
        the device for `stem_fit`."""
        z0 = self._entry_height() + 5.0 if z0 is None else float(z0)
        L = int(round(160.0 / dz)) + 1 if L is None else int(L)
        bone = self._humerus
        bone._ensure_loaded()
        got = bone._engine.canal_profile(z0, dz, L, A, frames=self._to_anp.reshape(1, 4, 4), fetch=fetch)
        self._profiled = bone._engine
        return tuple(g[0] for g in got) if isinstance(got, tuple) else got[0]

    def stem_fit(self, stems) -> list:
        """How each stem of `stems` -- (length, r_prox, r_tip) rows -- sits in the canal below the current cut (sh_resect_planes with
        B = P = 1, then sh_resect_stems against the last `canal_profile()`, which is taken with its defaults when there is none): K dicts
        with the fields of sh_stem_fit, in CT."""
        bone = self._humerus
        bone._ensure_loaded()
        if getattr(self, "_profiled", None) is not bone._engine:
            self.canal_profile()
        p, n = self._plane_ct()
        bone._engine.resect(planes=np.concatenate([p, n]).reshape(1, 1, 6))
        fits = bone._engine.resect_stems(stems)[0, 0]
        return [{k: (s[k].copy() if s[k].ndim else s[k].item()) for k in s.dtype.names} for s in fits]

    # ---- offsets (arthroplasty.py:89-175) ------------------------------------------------------------------
    def offset_retroversion(self, deg: float) -> None:
        """more retroversion for positive `deg` (the azimuth decreases on a left humerus, increases on a right one)"""
        self._turn(d_theta=self._side_sign() * deg)

    def offest_neckshaft(self, deg: float) -> None:
        """larger neck-shaft angle for positive `deg` (the polar angle of the normal decreases)"""
        self._turn(d_phi=-deg)

    def offset_depth(self, mm, direction="canal") -> None:
        """move the plane by `mm` along the canal (z of the anp csys), the native neck normal, or the current cut normal"""
        if direction not in _DEPTH_DIRECTIONS:
            raise ValueError("Invalid direction. Choose from: 'canal', 'anp', or 'resection'")
        along = {"canal": np.array([0.0, 0.0, 1.0]), "anp": self._native_normal, "resection": self._normal}[direction]
        self._shift(mm * along)

    def offset_anterior_posterior(self, mm):
        """anterior (+) / posterior (-): x of the anp csys, mirrored for a left humerus"""
        self._shift([self._side_sign() * mm, 0.0, 0.0])

    def offset_medial_lateral(self, mm):
        """medial (+) / lateral (-): -y of the anp csys"""
        self._shift([0.0, -mm, 0.0])


class HumeralImplantation:
    """The implant below and on a `HumeralHeadOsteotomy`: the ranked (head, stem) pairs of its current cut.

    The reference names this class and leaves it commented out (arthroplasty.py:178-182: it "continues from the humeral head
    osteotomy and places the implant").  Here it drives the engine's chain for the osteotomy's current plane -- seated resection,
    canal profile, stems, plan (sh_resect_planes_seat, sh_canal_profile, sh_resect_stems, sh_resect_plan with B = P = 1) -- in the
    frame the osteotomy read the anatomic-neck plane in, with the native anatomic-neck plane as the plan's reference plane.
    heads: (diameter, thickness) pairs, as `HumeralHeadOsteotomy.seat` takes them; stems: (length, r_prox, r_tip) rows; rule: a dict
    with sh_plan_rule's field names (Engine.plan); seat_center: "centroid" or "sphere"; compat: (K_h, K_s) booleans or None."""

    def __init__(self, osteotomy, heads, stems, rule=None, seat_center="centroid", compat=None) -> None:
        self._ost = osteotomy
        self._heads = [tuple(float(x) for x in h) for h in np.asarray(heads, dtype=np.float64).reshape(-1, 2)]
        self._stems = [tuple(float(x) for x in s) for s in np.asarray(stems, dtype=np.float64).reshape(-1, 3)]
        self._rule = dict(rule or {})
        self._center = seat_center
        self._compat = compat
        self._last = None      # (the cut's plane, n, plans, refs) of the last chain

    def _run(self, n):
        """(plans (1, >= n), refs (1,)) of the current cut.  The chain -- profile, seated resection, stems, plan -- runs once per
        plane: a call for the same plane with the same or a smaller n is answered from the last result, of which plan r is the same
        record whatever n is; another plane, or a larger n, runs the chain again.  The result is a SNAPSHOT taken when the chain ran: it
        is not refreshed when the engine's resident batch is replaced (another bone on the same engine) or the humerus is reloaded,
        and the device buffers it was copied from may be gone by then; make a new HumeralImplantation after either."""
        ost = self._ost
        key = np.concatenate(ost._plane_ct()).tobytes()
        if self._last is not None and self._last[0] == key and self._last[1] >= n:
            return self._last[2][:, :n], self._last[3]
        plans, refs = self._chain(n)
        self._last = (key, n, plans, refs)
        return plans, refs

    def _chain(self, n):
        ost = self._ost
        bone = ost._humerus
        bone._ensure_loaded()
        eng = bone._engine
        dz = 1.0      # the grid of HumeralHeadOsteotomy.canal_profile, long enough for the longest stem
        L = min(1024, max(int(round(160.0 / dz)) + 1, int(np.ceil((max(s[0] for s in self._stems) + 5.0) / dz)) + 2))
        ost.canal_profile(dz=dz, L=L)
        p, nrm = ost._plane_ct()
        heads = np.array([(0.5 * d, h) for d, h in self._heads])
        eng.resect(planes=np.concatenate([p, nrm]).reshape(1, 1, 6), fit=True, heads=heads, seat_center=self._center)
        eng.resect_stems(self._stems)
        ref = np.concatenate(transform_plane_pn(ost._native_point, ost._native_normal, inv_transform(ost._to_anp))).reshape(1, 6)
        return eng.plan(n=n, rule=self._rule, compat=self._compat, ref_planes=ref)

    def plans(self, n=8) -> list:
        """The n best (head, stem) pairs of the current cut, best first: dicts with the fields of sh_plan and the chosen `head_tuple`
        (diameter, thickness) and `stem_tuple` (length, r_prox, r_tip).  Fewer than n when fewer are feasible.  `best()` and
        `reference()` after it, on the same plane, cost no further engine call: they read the snapshot of that chain (`_run`)."""
        got = self._run(n)[0][0]
        out = []
        for r in got[got["status"] == 0]:
            d = {k: (r[k].copy() if r[k].ndim else r[k].item()) for k in r.dtype.names}
            d["head_tuple"], d["stem_tuple"] = self._heads[d["head"]], self._stems[d["stem"]]
            out.append(d)
        return out

    def best(self):
        """the first of `plans()`, or None"""
        got = self.plans(1)
        return got[0] if got else None

    def reference(self) -> dict:
        """The height reference of the humerus (sh_plan_ref) as a dict: native head apex and tuberosity top, in CT and in the frame."""
        r = self._run(1)[1][0]
        return {k: (r[k].copy() if r[k].ndim else r[k].item()) for k in r.dtype.names if k != "pad"}


def implant_from_fit(fit, side, catalogue=None) -> dict:
    """A head-fit record (dict or structured scalar with sh_head_fit's fields) -> the cap a planner picks: `radius` of curvature,
    `thickness` (= cap_height), `base_diameters` (2 x the cut's semi-axes, major first), `center` (CT), and the centre's offsets from
    the canal axis in the canal / articular frame signed as offset_medial_lateral / offset_anterior_posterior count them
    (`medial_offset` = -y; `posterior_offset` = -x on a right humerus, +x on a left one).  catalogue: (diameter, thickness) pairs;
    `catalogue_index` is the pair nearest in (2 radius, thickness).  Pure NumPy."""
    if fit["sphere_status"] != 0 or not fit["sphere_radius"] > 0:
        raise ValueError("the cut has no head sphere (sphere_status %d)" % fit["sphere_status"])
    ca = np.asarray(fit["center_articular"], dtype=np.float64)
    sign = 1.0 if side == "right" else -1.0
    out = dict(radius=float(fit["sphere_radius"]), thickness=float(fit["cap_height"]),
               base_diameters=(2.0 * float(fit["cut_semi_major"]), 2.0 * float(fit["cut_semi_minor"])),
               medial_offset=float(-ca[1]), posterior_offset=float(-sign * ca[0]), center=np.array(fit["sphere_center"], dtype=np.float64))
    if catalogue is not None:
        cat = np.asarray(catalogue, dtype=np.float64).reshape(-1, 2)
        d = (cat[:, 0] - 2.0 * out["radius"]) ** 2 + (cat[:, 1] - out["thickness"]) ** 2
        out["catalogue_index"] = int(np.argmin(d))
    return out


def best_seat(seats, max_overhang_mm):
    """Index of the seat with the largest `coverage` among those with `status` == 0 and `max_overhang` <= max_overhang_mm (the first
    of equals), or None.  seats: a 1-D structured array of _lib.SEAT_DTYPE or a list of dicts with its fields.  Pure NumPy."""
    if isinstance(seats, np.ndarray) and seats.dtype.names:
        st, ov, cov = seats["status"].reshape(-1), seats["max_overhang"].reshape(-1), seats["coverage"].reshape(-1)
    else:
        st, ov, cov = (np.array([s[k] for s in seats]) for k in ("status", "max_overhang", "coverage"))
    ok = np.nonzero((st == 0) & (ov <= max_overhang_mm))[0]
    return int(ok[np.argmax(cov[ok])]) if len(ok) else None


def best_stem(fits, stems):
    """Index of the stem with the largest `r_prox`, then the largest `length` (the first of equals), among those with `status` == 0 and
    `fits` == 1, or None.  fits: a 1-D structured array of _lib.STEM_FIT_DTYPE or a list of dicts with its fields; stems: the catalogue
    they were fitted from, (length, r_prox, r_tip) rows.  Pure NumPy."""
    if isinstance(fits, np.ndarray) and fits.dtype.names:
        st, ok = fits["status"].reshape(-1), fits["fits"].reshape(-1)
    else:
        st, ok = (np.array([f[k] for f in fits]) for k in ("status", "fits"))
    cat = np.asarray(stems)
    cat = np.stack([cat[k] for k in ("length", "r_prox", "r_tip")], axis=-1) if cat.dtype.names else cat
    cat = np.asarray(cat, dtype=np.float64).reshape(-1, 3)
    idx = np.nonzero((st == 0) & (ok == 1))[0]
    if len(idx) == 0:
        return None
    return int(min(idx, key=lambda i: (-cat[i, 1], -cat[i, 0], i)))
