"""`shoulder.Humerus` drop-in facade (reference src/shoulder/bone.py:109-157 and the accessor API
of humerus/{canal,bicipital_groove,anatomic_neck,epicondyle,surgical_neck}.py).

Same names (incl. `trans_epiconylar`, `apply_csys_canal_transepiconylar`), argument meaning,
return shapes, float64 NumPy arrays, lazy + memoised evaluation, landmarks cached in CT and
re-expressed through one shared `Transform`.  Every number comes from libshoulder_hip.so through
`Engine` (one sh_run over a batch of one); nothing here falls back to the CPU.
"""
import contextlib
import os
import pathlib
import threading
import warnings

import numpy as np

from . import _lib, unet_spec
from .base import Bone, Landmark, Mesh, Plane, Transform
from .engine import Engine, ShoulderHipError
from .stl import load_stl

_DEFAULT_ENGINE = None
_DEFAULT_LOCK = threading.Lock()

EARLY = _lib.STAGE_OBB | _lib.STAGE_FULL | _lib.STAGE_NECK | _lib.STAGE_CANAL
LATE = _lib.STAGE_PROXIMAL | _lib.STAGE_GROOVE | _lib.STAGE_ANP | _lib.STAGE_DISTAL | _lib.STAGE_TE | _lib.STAGE_CSYS | _lib.STAGE_APPLY


def default_engine(device=0, unet_weights=None, unet_onnx=None):
    """Process-wide engine on `device` (created once, under a lock; an Engine itself is single-threaded like the
    reference's objects -- give threads their own engines).

    The anatomic-neck network: `unet_onnx` (or the environment variable SHOULDER_UNET_ONNX) names an ONNX file of the
    supported UNet family -- the reference opens its packaged `humerus/models/unetcrf_anp.onnx` (anatomic_neck.py:62-66),
    which is not part of this tree; `unet_weights` takes a parameter dict.  With neither, the seeded TEACHER weights of
    `unet_spec` are loaded and a RuntimeWarning says so: they make every stage computable and testable, but anatomic-neck
    dependent values (anatomic_neck.*, neckshaft, retroversion, radius_curvature, side, apply_csys_canal_articular) are then
    NOT those of a trained model."""
    global _DEFAULT_ENGINE
    with _DEFAULT_LOCK:
        if _DEFAULT_ENGINE is None:
            e = Engine(device)
            e.load_rfc()
            onnx_path = unet_onnx or os.environ.get("SHOULDER_UNET_ONNX")
            if onnx_path:
                e.load_unet_onnx(onnx_path)
            elif unet_weights is not None:
                e.load_unet(unet_weights, unet_spec.BASE, unet_spec.DEPTH)
            else:
                warnings.warn("shoulder_amd: no anatomic-neck model given (SHOULDER_UNET_ONNX / default_engine(unet_onnx=...)): loading the "
                              "seeded TEACHER stand-in -- anatomic-neck dependent landmarks and metrics are not those of a trained model",
                              RuntimeWarning, stacklevel=3)
                e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
            _DEFAULT_ENGINE = e
    return _DEFAULT_ENGINE


def _inv(T):
    # utils.inv_transform (utils.py:227-256) on the host for a single 4x4 (glue; the device
    # computes the same inside every stage that maps OBB -> CT)
    R = np.identity(4)
    R[:3, :3] = T[:3, :3]
    t = np.identity(4)
    t[:3, 3] = T[:3, 3]
    return np.linalg.inv(R) @ np.linalg.inv(t)


def _registration_info(rec):
    """what Bone.register reports of one _lib.REGISTRATION_DTYPE record beside the matrix"""
    return dict(rms=float(rec["rms"]), rms_first=float(rec["rms_first"]), pairs=int(rec["pairs"]), iterations=int(rec["iterations"]),
                converged=bool(rec["converged"]), min_pivot=float(rec["min_pivot"]))


def _scatter(pts, name, **kw):
    """One plotly trace per landmark, as the reference's `_graph_obj` methods build them (e.g. canal.py:132-142)."""
    import plotly.graph_objects as go
    return go.Scatter3d(x=pts[:, 0], y=pts[:, 1], z=pts[:, 2], name=name, **kw)


class _Lm(Landmark):
    def __init__(self, bone):
        self._b = bone
        self._tfrm = bone._tfrm

    def _t(self, pts_ct):
        return self._b._engine.transform_points(pts_ct, self._tfrm.matrix)


class Canal(_Lm):
    """canal.py"""

    def __init__(self, bone):
        super().__init__(bone)
        self._points_ct = None
        self._axis_ct = None

    def points(self, cutoff_pcts=(0.35, 0.75)) -> np.ndarray:
        if self._points_ct is None:
            # DeepGroove.__init__ calls canal.axis() in the reference (bicipital_groove.py:21), so the
            # default cutoff is already fixed when user code first gets here (canal.py:60-62)
            e = self._b._engine
            self._b._ensure_loaded()
            c0, c1 = self._b._canal_cutoff
            n = int((1 - c0) * 200) - int((1 - c1) * 200)                 # Slices._cutoff (slice.py:157-164) on the 200 full slices
            obb = e.fetch("canal.points_obb", np.float64, (1, 200, 3))[0][:n]
            self._points_obb = obb
            self._points_ct = e.transform_points(obb, _inv(self._b._obb_transform))
        self._points = self._t(self._points_ct)
        return self._points

    def axis(self, cutoff_pcts=(0.35, 0.75)) -> np.ndarray:
        if self._axis_ct is None:
            self._axis_ct = np.array(self._b._early["canal_axis"], dtype=np.float64)
        self._axis = self._t(self._axis_ct)
        return self._axis

    def get_transform(self) -> np.ndarray:
        """canal.py:88-124 (CT -> canal csys, x from the OBB frame)."""
        ax = self.axis()
        z_hat = (ax[0] - ax[1]) / np.linalg.norm(ax[0] - ax[1])
        x_hat = self._b._obb_transform[:3, :1].flatten().copy()
        x_hat -= z_hat * np.dot(x_hat, z_hat) / np.dot(z_hat, z_hat)
        x_hat /= np.linalg.norm(x_hat)
        y_hat = np.cross(z_hat, x_hat)
        y_hat /= np.linalg.norm(y_hat)
        T = np.r_[np.c_[x_hat, y_hat, z_hat, np.average(ax, axis=0)], np.array([[0, 0, 0, 1.0]])]
        return _inv(T)

    def transform_landmark(self) -> None:
        if self._axis_ct is not None:
            self.axis()
        if self._points_ct is not None:
            self.points()

    def _graph_obj(self):                                  # canal.py:132-142
        return None if self._points_ct is None else _scatter(self._points, "Canal Axis")


class SurgicalNeck(_Lm):
    """surgical_neck.py"""

    def __init__(self, bone):
        super().__init__(bone)
        e = bone._engine
        self.neck_z = float(bone._early["neck_z"])
        ring = e.ring("neckc", 0, 0)
        pts_obb = np.c_[ring, np.full(len(ring), self.neck_z)]
        self.points_ct = e.transform_points(pts_obb, _inv(bone._obb_transform))
        self.points = self.points_ct.copy()

    def cutoff_zs(self, bottom_pct=0.35, top_pct=0.85):
        z_max = self._b._z_bounds[1]
        span = z_max - self.neck_z
        return [self.neck_z + span * bottom_pct, self.neck_z + span * top_pct]

    def z_percent(self):
        z_min, z_max = self._b._z_bounds
        return (self.neck_z - z_min) / (abs(z_max) + abs(z_min))

    def transform_landmark(self) -> None:
        if self.points is not None:
            self.points = self._t(self.points_ct)

    def _graph_obj(self):                                  # surgical_neck.py:82-93
        return None if self.points is None else _scatter(self.points, "Surgical Neck")


class DeepGroove(_Lm):
    """bicipital_groove.py"""

    def __init__(self, bone):
        super().__init__(bone)
        self._points_ct = None
        self._axis_ct = None

    def points(self, cutoff_pcts=(0.2, 0.75), deg_window=7) -> np.ndarray:
        if self._points_ct is None:
            lm = self._b._all(groove_cutoff=cutoff_pcts, deg_window=deg_window)
            self.bg_theta = float(lm["bg_theta"])
            self._points_ct = np.array(lm["groove_points"], dtype=np.float64)
        self._points = self._t(self._points_ct)
        return self._points

    def axis(self) -> np.ndarray:
        if self._axis_ct is None:
            if self._points_ct is None:
                self.points()
            self._axis_ct = np.array(self._b._all()["groove_axis"], dtype=np.float64)
        self._axis = self._t(self._axis_ct)
        return self._axis

    def transform_landmark(self) -> None:
        if self._axis_ct is not None:
            self.axis()
        if self._points_ct is not None:
            self.points()

    def _graph_obj(self):                                  # bicipital_groove.py:273-284
        return None if self._points_ct is None else _scatter(self._points, "Bicipital Groove")


class AnatomicNeck(_Lm):
    """anatomic_neck.py"""

    def __init__(self, bone):
        super().__init__(bone)
        self._points_ct = self._plane_ct = self._plane_points_ct = None
        self._central_axis_ct = self._normal_axis_ct = None
        self._axis_hits_ct = None      # every hit of the four rays (CT), for hits="all" / "outermost"

    def points(self) -> np.ndarray:
        if self._points_ct is None:
            self._b.bicipital_groove.axis()               # anatomic_neck.py:47 forces the groove
            lm = self._b._all()
            k = int(lm["n_anp"])
            if k > _lib.ANP_MAX_PTS:                       # the record is padded to 4096 rows; fetch the rest
                self._b._ensure_loaded()
                obb =self._b._engine.fetch("anp.points_obb", np.float64, (65536, 3))[:k]
                self._points_ct = self._b._engine.transform_points(obb, _inv(self._b._obb_transform))
            else:
                self._points_ct = np.array(lm["anp_points"][:k], dtype=np.float64)
        self._points = self._t(self._points_ct)
        return self._points

    def plane(self) -> Plane:
        if self._plane_ct is None:
            self.points()
            lm = self._b._all()
            self._plane_ct = Plane(lm["anp_plane_point"], lm["anp_plane_normal"])
        T = self._tfrm.matrix
        self._plane = Plane(self._t(self._plane_ct.point.reshape(1, 3))[0], T[:3, :3] @ self._plane_ct.normal)   # utils.py:191-206
        return self._plane

    def plane_points(self) -> np.ndarray:
        if self._plane_points_ct is None:
            self.plane()
            self._b._ensure_loaded()
            self._plane_points_ct = self._b._engine.section_plane(0, self._plane_ct.point, self._plane_ct.normal)
        self._plane_points = self._t(self._plane_points_ct)
        return self._plane_points

    def _axis_hits(self, first, hits):
        """The rays `first` (upper) and `first + 1` (lower) with every hit (Engine.anp_axis_hits): hits="all" is the reference's
        `np.r_[upper_loc, bottom_loc]` (anatomic_neck.py:184-192, 217-224) with each direction ascending by (t, face), "outermost"
        the last hit of each direction.  Neither touches the cached nearest-hit axes, so metrics and coordinate systems stay."""
        if hits not in ("all", "outermost"):
            raise ValueError(f'hits is "nearest", "all" or "outermost", not {hits!r}')
        if self._axis_hits_ct is None:
            self.plane()
            b, e = self._b, self._b._engine
            b._ensure_loaded()
            cap = 16
            while True:
                try:
                    h, n, st = e.anp_axis_hits(cap)
                except ShoulderHipError as ex:
                    if ex.code != -3:
                        raise
                    e.set_params(groove_cutoff=b._groove_params[0], groove_deg_window=b._groove_params[1])      # the engine's last run was not this bone's late one
                    b._run(b._LATE, fetch=False)
                    h, n, st = e.anp_axis_hits(cap)
                if int(n.max()) <= cap or cap >= _lib.RAY_MAX_HITS:
                    break
                cap = min(int(n.max()), _lib.RAY_MAX_HITS)
            if int(st[0]) != 0:
                raise ValueError(f"landmark stage failed with status {int(st[0])}")
            self._axis_hits_ct = [np.array(h[0, r, :min(int(n[0, r]), cap)]["point"], dtype=np.float64) for r in range(4)]
        up, lo = self._axis_hits_ct[first], self._axis_hits_ct[first + 1]
        return self._t(np.r_[up, lo] if hits == "all" else np.r_[up[-1:], lo[-1:]])

    def axis_normal(self, hits="nearest") -> np.ndarray:
        if hits != "nearest":
            return self._axis_hits(0, hits)
        if self._normal_axis_ct is None:
            self.plane()
            self._normal_axis_ct = np.array(self._b._all()["anp_axis_normal"], dtype=np.float64)
        self._normal_axis = self._t(self._normal_axis_ct)
        return self._normal_axis

    def axis_central(self, hits="nearest") -> np.ndarray:
        if hits != "nearest":
            return self._axis_hits(2, hits)
        if self._central_axis_ct is None:
            self.plane()
            self._central_axis_ct = np.array(self._b._all()["anp_axis_central"], dtype=np.float64)
        self._central_axis = self._t(self._central_axis_ct)
        return self._central_axis

    def transform_landmark(self) -> None:
        if self._points_ct is not None:
            self.points()
        if self._plane_ct is not None:
            self.plane()
        if self._plane_points_ct is not None:
            self.plane_points()
        if self._normal_axis_ct is not None:
            self.axis_normal()
        if self._central_axis_ct is not None:
            self.axis_central()

    def _graph_obj(self):                                  # anatomic_neck.py:250-273
        if self._points_ct is None:
            return None
        pp = self.plane_points()
        return [_scatter(self._points, "Anatomic Neck", mode="markers", showlegend=True),
                _scatter(pp, "Anatomic Neck Plane", mode="markers", showlegend=True)]


class TransEpicondylar(_Lm):
    """epicondyle.py"""

    def __init__(self, bone):
        super().__init__(bone)
        self._axis_ct = None

    def axis(self, num_slices: int = 50) -> np.ndarray:       # num_slices is ignored by the reference too
        if self._axis_ct is None:
            self._b.anatomic_neck.axis_central()              # epicondyle.py:90 forces groove + neck
            self._axis_ct = np.array(self._b._all()["te_axis"], dtype=np.float64)
        self._axis = self._t(self._axis_ct)
        return self._axis

    def transform_landmark(self) -> None:
        if self._axis_ct is not None:
            self.axis()

    def _graph_obj(self):                                  # epicondyle.py:107-117
        return None if self._axis_ct is None else _scatter(self._axis, "Transverse Epicondylar Axis")


class ProximalHumerus(Bone):
    """bone.py:24-105 -- a humerus whose scan ends in the shaft (and, as in the reference, the base class of `Humerus`:
    `isinstance(Humerus(...), ProximalHumerus)` holds).  The device runs the ProxObb head-end rule and canal range
    (mesh.py:128-192), the (0.2, 0.99) neck cut-off (surgical_neck.py:25-26) and the canal cut-offs taken from the box
    (canal.py:33-38); there is no trans-epicondylar axis and no retroversion, and the coordinate system is
    `apply_csys_canal_articular` (bone.py:53-62)."""
    _BONE_KIND = _lib.BONE_PROXIMAL
    _EARLY = EARLY
    _LATE = _lib.STAGE_PROXIMAL | _lib.STAGE_GROOVE | _lib.STAGE_ANP | _lib.STAGE_CSYS | _lib.STAGE_APPLY

    def __init__(self, stl_file, engine=None, open_contours="error", max_gap=_lib.OPEN_GAP_DEFAULT):
        """open_contours="bridge": a mesh that is not watertight is measured with its section gaps up to max_gap mm bridged
        (Engine.set_open_contours, include/shoulder_hip.h) and warns as the reference does (mesh.py:24-27); "error" (the
        default): an open section fails the humerus."""
        if open_contours not in ("error", "bridge"):
            raise ValueError(f'open_contours is "error" or "bridge", not {open_contours!r}')
        gap = float(max_gap)
        if not np.isfinite(gap) or gap < 0:
            raise ValueError(f"max_gap must be finite and >= 0, not {max_gap!r}")
        self._open = (open_contours, gap)
        self._tfrm = Transform()
        self.transform = self._tfrm.matrix
        self.stl_file = stl_file if isinstance(stl_file, pathlib.Path) else pathlib.Path(stl_file)
        self._engine = engine if engine is not None else default_engine()
        verts, faces = load_stl(self.stl_file)
        self._verts, self._faces = verts, faces
        self._engine.upload([(verts, faces)])
        self._engine._resident_bone = id(self)      # (two bones with the same vertices have the same box: _ensure_loaded tells them apart by this)
        self._engine.set_params(bone_kind=self._BONE_KIND)      # (read-modify-write: the engine's UNet dtype and cut-offs stay as configured)
        if open_contours == "bridge" and int(self._engine.open_edges()[0]) > 0:
            warnings.warn(f"{self.stl_file.name} is not watertight!", UserWarning)      # mesh.py:26
        self._lm_all = None
        self._groove_params = None      # (cutoff_pcts, deg_window) this bone's late stages ran with
        # eager part of the reference constructor: OBB, full slices, surgical neck, canal axis
        self._early = self._run(self._EARLY)[0].copy()
        self._canal_cutoff = tuple(float(x) for x in self._early["canal_cutoff"])
        self._obb_transform = np.array(self._early["obb_transform"], dtype=np.float64)
        self._z_bounds = tuple(self._engine.fetch("z_bounds", np.float64, (1, 2))[0])
        self._mesh_ct = Mesh(verts, faces, self._engine)
        self.mesh = self._mesh_ct.copy()
        self.surgical_neck = SurgicalNeck(self)
        self.canal = Canal(self)
        self.bicipital_groove = DeepGroove(self)
        self.anatomic_neck = AnatomicNeck(self)
        self._init_kind_specific()

    def _init_kind_specific(self):
        # metrics (bone.py:46-51 -> bone_props.py); values come from the device record (k_metrics)
        self.side = self._side
        self.neckshaft = self._neckshaft
        self.radius_curvature = self._radius_curvature
        e = self._engine
        self.cutoff_pcts = [float(x) for x in self._canal_cutoff]           # ProxObb.cutoff_pcts (mesh.py:190)
        self.cutoff_bot = int(e.fetch("pobb.cutoff_idx", np.int32, (1, 2))[0][0])      # mesh.py:187

    def _run(self, stages, fetch=True):
        """Every run of this bone on the (possibly shared) engine takes this bone's open-contour setting."""
        self._engine.set_open_contours(*self._open)
        return self._engine.run(stages, fetch=fetch)

    def _ensure_loaded(self):
        """The shared engine may have been used for another bone since: bring this one back."""
        e = self._engine
        if e.B != 1 or getattr(e, "_resident_bone", id(self)) != id(self) or not np.array_equal(e.fetch("obb_transform", np.float64, (1, 4, 4))[0], self._obb_transform):
            e.upload([(self._verts, self._faces)])
            e._resident_bone = id(self)
            e.set_params(bone_kind=self._BONE_KIND, canal_cutoff=self._canal_cutoff if self._BONE_KIND == _lib.BONE_HUMERUS else None)
            self._run(self._EARLY, fetch=False)
            if self._lm_all is not None:      # device buffers fetched later (e.g. anp.points_obb beyond 4096 rows) must match the cached record
                e.set_params(groove_cutoff=self._groove_params[0], groove_deg_window=self._groove_params[1])
                self._run(self._LATE, fetch=False)

    # -- the late stages, once ------------------------------------------------------------------------
    def _all(self, groove_cutoff=(0.2, 0.75), deg_window=7):
        if self._lm_all is None:
            e = self._engine
            self._ensure_loaded()
            try:
                e.set_params(groove_cutoff=tuple(groove_cutoff), groove_deg_window=float(deg_window), bone_kind=self._BONE_KIND)
            except Exception as ex:
                raise ValueError(f"bicipital_groove cutoff_pcts {groove_cutoff} is not supported: {ex}") from ex
            self._groove_params = (tuple(float(x) for x in groove_cutoff), float(deg_window))
            self._lm_all = self._run(self._LATE)[0].copy()
            if int(self._lm_all["status"]) != 0:
                raise ValueError(f"landmark stage failed with status {int(self._lm_all['status'])}")
        return self._lm_all

    # -- metrics (bone_props.py) ---------------------------------------------------------------------------
    def _side(self) -> str:
        """bone_props.py:23-47"""
        self.canal.axis(); self.anatomic_neck.axis_central(); self.bicipital_groove.points()
        return "right" if int(self._all()["side"]) == 1 else "left"

    def _neckshaft(self) -> float:
        """bone_props.py:93-112"""
        self.canal.axis(); self.anatomic_neck.axis_normal()
        return float(self._all()["neckshaft"])

    def _radius_curvature(self) -> float:
        """bone_props.py:119-125"""
        self.anatomic_neck.points()
        return float(self._all()["radius_curvature"])

    def _retroversion(self) -> float:
        """bone_props.py:64-85.  The reference transforms `axis_normal()` as returned in the CURRENT coordinate
        system (:72-73); with the identity Transform that is the device value, otherwise the same two-point
        arithmetic is redone here on the re-expressed axis (2 points, host glue)."""
        self.canal.axis(); self.trans_epiconylar.axis()
        an = self.anatomic_neck.axis_normal()
        lm = self._all()
        if np.array_equal(self._tfrm.matrix, np.identity(4)):
            return float(lm["retroversion"])
        q = self._engine.transform_points(an, np.array(lm["csys"], dtype=np.float64))
        v = (q[0] - q[1]) / np.linalg.norm(q[0] - q[1])
        theta = float(np.rad2deg(np.arctan2(v[1], -1 * v[0])))
        return -theta if int(lm["side"]) == 1 else theta

    # -- rays against the mesh --------------------------------------------------------------------------------
    def _rays_ct(self, origins, directions):
        """rays given in the CURRENT coordinate system -> (origins and directions in CT, the current matrix); the bone is resident
        afterwards.  Points go through the inverse of the current transform by the full matrix, directions by its linear part."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if len(o) != len(d) or len(o) < 1:
            raise ValueError("origins and directions must both have shape (n, 3), n >= 1")
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        Ti = np.linalg.inv(T)
        self._ensure_loaded()
        return self._engine.transform_points(o, Ti), d @ Ti[:3, :3].T, T

    def ray_hits(self, origins, directions, accel=None):
        """`mesh.ray.intersects_location(origins, directions)` in the CURRENT coordinate system on the device (Engine.ray_cast):
        -> (locations (n, 3), index_ray (n,), index_tri (n,)), sorted by ray and then by (t, face).  The rays go to CT through the
        inverse of the current transform (points by the full matrix, directions by its linear part), the locations come back through it.
        accel="bvh": through the face hierarchy (Engine.query_accel), the same results."""
        o, d, T = self._rays_ct(origins, directions)
        with self._accel(accel):
            hits, counts = self._engine.ray_cast(o, d, cap=None)
        keep = np.arange(hits.shape[2])[None, :] < counts[0][:, None]
        loc_ct = np.ascontiguousarray(hits[0]["point"][keep])
        loc = self._engine.transform_points(loc_ct, T) if len(loc_ct) else np.zeros((0, 3))
        return loc, np.nonzero(keep)[0], np.array(hits[0]["face"][keep], dtype=np.int64)

    def ray_first(self, origins, directions, accel=None):
        """`mesh.ray.intersects_location(origins, directions, multiple_hits=False)` / `intersects_first` in the CURRENT coordinate
        system on the device (Engine.ray_nearest): the nearest hit of every ray that has one -> (locations (m, 3), index_ray (m,),
        index_tri (m,)), by ray: the first location per ray of ray_hits.  accel as in ray_hits."""
        o, d, T = self._rays_ct(origins, directions)
        with self._accel(accel):
            hit = self._engine.ray_nearest(o, d)[0]
        keep = hit["face"] >= 0
        loc_ct = np.ascontiguousarray(hit["point"][keep])
        loc = self._engine.transform_points(loc_ct, T) if len(loc_ct) else np.zeros((0, 3))
        return loc, np.nonzero(keep)[0], np.array(hit["face"][keep], dtype=np.int64)

    def thickness(self, points=None, sample=None, seed=0, offset=1e-3, accel=None):
        """`trimesh.proximity.thickness(mesh, points, method="ray")` in the CURRENT coordinate system on the device (Engine.thickness):
        how much bone lies under a surface point along the inward normal -> (thickness (n,), opposite points (n, 3), opposite faces
        (n,)); inf, a point of nan and face -1 where the ray meets nothing.  points (n, 3): each is snapped to the surface (closest_point) and takes the
        unit normal of the winning face; or sample=n: the points and faces of sample_surface(n, seed).  offset (mm) starts the ray that
        far under the point (Engine.thickness).  The normals follow the mesh's winding, as trimesh's do: on an inward-wound mesh the
        rays leave the bone and the thickness is inf.  accel as in ray_hits (the snap of `points` goes the same way)."""
        if (points is None) == (sample is None):
            raise ValueError("give either points or sample=n")
        self._ensure_loaded()
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        with self._accel(accel):
            if points is not None:
                rec, _ = self._closest_ct(points)
                if np.any(rec["status"] != 0):
                    raise ValueError("thickness: a point could not be snapped to the surface")
                p_ct, face = np.ascontiguousarray(rec["point"]), np.array(rec["face"], dtype=np.int64)
            else:
                rec, info = self._engine.sample_surface(int(sample), seed=seed)
                if info[0]["status"] != 0:
                    raise ValueError(f"thickness: sample_surface failed with status {int(info[0]['status'])}")
                p_ct, face = np.ascontiguousarray(rec[0]["point"]), np.array(rec[0]["face"], dtype=np.int64)
            if not self._engine._has_buffer("vert.face"):
                self._engine.vertex_fields()
            normals = self._engine.face_normals(0)[0][face]
            out = self._engine.thickness(p_ct, normals, offset=offset)[0]
        hit = out["face"] >= 0
        opp = np.full((len(out), 3), np.nan)
        if hit.any():
            opp[hit] = self._engine.transform_points(np.ascontiguousarray(out["point"][hit]), T)
        return np.array(out["thickness"]), opp, np.array(out["face"], dtype=np.int64)

    # -- closest surface points ---------------------------------------------------------------------------------
    def _points_ct(self, points):
        """points given in the CURRENT coordinate system -> (the points in CT, the current matrix); the bone is resident afterwards"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        if len(p) < 1:
            raise ValueError("points must have shape (n, 3), n >= 1")
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        self._ensure_loaded()
        return self._engine.transform_points(p, np.linalg.inv(T)), T

    @contextlib.contextmanager
    def _accel(self, accel):
        """accel=None: the engine as it is configured; "off" | "bvh": its closest-point step and its rays switched for this call (Engine.query_accel:
        the same results either way) and put back afterwards"""
        if accel is None:
            yield
            return
        before = self._engine.query_accel
        self._engine.query_accel = accel
        try:
            yield
        finally:
            self._engine.query_accel = before

    def _closest_ct(self, points, accel=None):
        """the records of Engine.closest_points for points given in the CURRENT coordinate system, and the current matrix"""
        p, T = self._points_ct(points)
        with self._accel(accel):
            return self._engine.closest_points(p)[0], T

    def closest_point(self, points, accel=None):
        """`trimesh.proximity.closest_point(mesh, points)` in the CURRENT coordinate system on the device (Engine.closest_points):
        -> (closest (n, 3), distance (n,), triangle_id (n,)).  The points go to CT through the inverse of the current transform, the
        closest points come back through it (the transforms are rigid: the distance is CT's).  Among triangles at the same distance
        the smallest id is returned.  accel="bvh": through the face hierarchy (Engine.query_accel), the same results."""
        rec, T = self._closest_ct(points, accel)
        if np.any(rec["status"] != 0):
            raise ValueError(f"closest_point failed with status {int(rec['status'][rec['status'] != 0][0])}: no face of the mesh gave a finite distance")
        return self._engine.transform_points(np.ascontiguousarray(rec["point"]), T), np.array(rec["dist"]), np.array(rec["face"], dtype=np.int64)

    def _other_points(self, other, sample, seed):
        """the points of `other` that register / surface_distance use: an (n, 3) array, `.vertices`, or with sample=n and a bone n
        area-weighted surface samples of it (`other.sample_surface(n, seed)`), read in the CURRENT coordinate system like the others"""
        if sample is not None:
            if not hasattr(other, "sample_surface"):
                raise ValueError("sample=n needs a bone (something with sample_surface) as `other`")
            return other.sample_surface(int(sample), seed=seed)[0]
        return other.vertices if hasattr(other, "vertices") else other

    def surface_distance(self, other, sample=None, seed=0, symmetric=False, accel=None):
        """How far `other` lies from this bone's surface: `other` is an (n, 3) array of points or anything with `.vertices` (a Mesh,
        another bone's mesh, a half from `resect_mesh()`), in the CURRENT coordinate system.  -> dict with `mean`, `rms`, `max` (the
        one-sided Hausdorff distance), `p95`, `n` and `argmax` (the index of the farthest point), from one closest_point call.
        ONE-SIDED by design: the distances run from the points of `other` to this surface.  For the symmetric figures call
        `b.surface_distance(a.mesh)` on the other bone as well and take the larger `max` (Hausdorff) or pool the two sets of distances.

        Vertices follow the mesher's density, not the surface.  With `sample=n` and a bone as `other` the points are n area-weighted
        samples of its surface instead (`other.sample_surface(n, seed)`); `symmetric=True` (needs `sample`) also measures n samples of
        this bone against `other` and adds `max_back`, `rms_back` and `hausdorff`, the larger of the two `max`.  accel as in closest_point."""
        if symmetric and sample is None:
            raise ValueError("symmetric=True needs sample=n and a bone as `other`")
        d = self.closest_point(self._other_points(other, sample, seed), accel=accel)[1]
        out = dict(mean=float(d.mean()), rms=float(np.sqrt(np.mean(d * d))), max=float(d.max()), p95=float(np.percentile(d, 95)),
                   n=int(len(d)), argmax=int(np.argmax(d)))
        if symmetric:
            back = other.closest_point(self.sample_surface(int(sample), seed=seed)[0], accel=accel)[1]
            out.update(max_back=float(back.max()), rms_back=float(np.sqrt(np.mean(back * back))), hausdorff=max(out["max"], float(back.max())))
        return out

    # -- surface samples ------------------------------------------------------------------------------------------
    def sample_surface(self, n, seed=0, radius=None):
        """`trimesh.sample.sample_surface(mesh, n)` in the CURRENT coordinate system on the device (Engine.sample_surface): n points
        on the surface, every face drawn in proportion to its area -> (points (n, 3), face_index (n,)).  With `radius` (mm) it is
        `sample_surface_even`: only the samples that keep that spacing are returned (m <= n of them; n at most 65 536).  The same seed
        gives the same points.  Raises ValueError for a mesh without area or a thinning that did not finish."""
        self._ensure_loaded()
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        rec, info = self._engine.sample_surface(n, seed=seed, radius=radius)
        if info[0]["status"] != 0:
            raise ValueError(f"sample_surface failed with status {int(info[0]['status'])}: the mesh has no area, or the thinning was not decided "
                             f"within its rounds (rounds {int(info[0]['rounds'])})")
        rec = rec[0][rec[0]["keep"] == 1]
        return self._engine.transform_points(np.ascontiguousarray(rec["point"]), T), np.array(rec["face"], dtype=np.int64)

    # -- topology: adjacency, shells, counts -------------------------------------------------------------------------
    def topology(self, max_shells=64, max_rounds=32):
        """How this bone's triangles hang together, on the device (Engine.topology) -> dict of the mesh's record: faces_degenerate,
        vertices_used, edges, border_edges, nonmanifold_edges, inconsistent_edges, euler, max_valence, n_shells, shells_written,
        largest_shell, largest_faces, rounds, plus watertight and winding_consistent (the two flags), shells (the first max_shells
        shell records; their boxes are CT's) and, for a watertight mesh, genus = (2 n_shells - euler) / 2: the handles of all shells
        together (1: one tunnel).  Raises ValueError when the labelling did not finish within max_rounds."""
        self._ensure_loaded()
        info, shells = self._engine.topology(max_shells=max_shells, max_rounds=max_rounds)
        r = info[0]
        if r["status"] != 0:
            raise ValueError(f"topology failed with status {int(r['status'])}: the shells were not labelled within {int(r['rounds'])} rounds")
        out = {n: int(r[n]) for n in r.dtype.names if n not in ("status", "flags", "reserved")}
        out["watertight"], out["winding_consistent"] = bool(r["flags"] & _lib.TOPO_WATERTIGHT), bool(r["flags"] & _lib.TOPO_CONSISTENT)
        out["shells"] = shells[0][:out["shells_written"]].copy()
        if out["watertight"]:
            out["genus"] = (2 * out["n_shells"] - out["euler"]) // 2
        return out

    def shells(self, largest_only=False):
        """`mesh.split(only_watertight=False)` of this bone (Engine.split) -> a list of (verts, faces) in CT, one per shell in shell
        order (the largest alone with largest_only): the standard first step on a segmentation with islands of noise.  Each is ready
        for Engine.upload."""
        self._ensure_loaded()
        info = self._engine.topology()[0][0]
        if info["status"] != 0:
            raise ValueError(f"shells failed with status {int(info['status'])}: the shells were not labelled within {int(info['rounds'])} rounds")
        return self._engine.split(0, largest_only=largest_only)

    # -- vertex normals and discrete curvatures ------------------------------------------------------------------
    def vertex_normals(self, weight="angle"):
        """`mesh.vertex_normals` of this bone on the device (Engine.vertex_fields) -> (V, 3) unit normals in CT, weighted by the corners'
        angles (trimesh's default) or by the faces' areas ("area"); zeros at a vertex no face of non-zero area uses."""
        self._ensure_loaded()
        return self._engine.vertex_fields(weight=weight)["normals"]

    def curvature(self, smooth=0):
        """The discrete curvatures of this bone's vertices (Engine.vertex_fields, area-weighted normals) -> dict: gauss and mean (after
        `smooth` rounds of averaging when smooth > 0), k1 >= k2 = mean +- sqrt(max(mean^2 - gauss, 0)) the principal curvatures in
        1/mm (computed here with NumPy), area, defect, normals, and border, the mask of the vertices on an open edge.  With outward
        normals the head is where k1 and k2 are positive and about equal, the bicipital groove where k2 is negative along a line.
        Raises ValueError for a mesh without a face of non-zero area."""
        self._ensure_loaded()
        r = self._engine.vertex_fields(weight="area", smooth=smooth)
        if r["status"][0] != 0:
            raise ValueError(f"curvature failed with status {int(r['status'][0])}: the mesh has no face of non-zero area")
        gauss, mean = (r["gauss_smooth"], r["mean_smooth"]) if smooth > 0 else (r["gauss"], r["mean"])
        root = np.sqrt(np.maximum(mean * mean - gauss, 0.0))
        return dict(gauss=gauss, mean=mean, k1=mean + root, k2=mean - root, area=r["area"], defect=r["defect"], normals=r["normals"],
                    border=(r["flags"] & _lib.VERT_BORDER) != 0)

    # -- smoothing of the vertices ---------------------------------------------------------------------------------------
    def smoothed_mesh(self, **options):
        """This bone with its vertices smoothed on the device (Engine.smooth_vertices, whose options these are: filter, iterations,
        lamb, mu, alpha, beta, weight, pin, pin_border, keep_volume; default ten Taubin iterations) -> (verts (V, 3) float64, faces) in
        the CURRENT coordinate system, ready for Engine.upload: what `trimesh.smoothing.filter_taubin(mesh)` leaves in the mesh, before
        the staircase of the CT voxels enters curvatures, thickness or a registration.  The resident mesh is not changed.  Two ways on:
            engine.upload([(verts.astype(np.float32), faces)])            # a new batch of the float32-rounded vertices (from CT: call
                                                                          # it while the bone is in CT)
            engine.store("verts", verts_ct.astype(np.float32))            # or new vertices for the resident faces: the queries that
                                                                          # follow (vertex_fields, mass_properties ...) measure them
        Raises ValueError when keep_volume could not restore the volume."""
        self._ensure_loaded()
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        r = self._engine.smooth_vertices(**options)
        if r["info"][0]["status"] != 0:
            raise ValueError(f"smoothed_mesh failed with status {int(r['info'][0]['status'])}: the volume could not be restored")
        return self._engine.transform_points(np.ascontiguousarray(r["vertices"]), T), np.array(self._faces, dtype=np.int32)

    # -- repair ---------------------------------------------------------------------------------------------------------
    def repaired_mesh(self, **options):
        """This bone with one winding, outward shells and filled holes (Engine.repair, whose options these are: orient, fill,
        max_hole_edges, max_shells, max_holes, max_rounds) -> (verts (V', 3) float64, faces (F', 3) int32) in the CURRENT coordinate
        system, ready for Engine.upload as smoothed_mesh's result is: what trimesh.repair's fix_winding, fix_inversion and fill_holes
        leave in the mesh, before a volume, a winding number or a thickness is asked of it.  The resident mesh is not changed.
        Raises ValueError when the mesh could not be repaired (a status in its info record)."""
        self._ensure_loaded()
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        r = self._engine.repair(**options)
        if r["info"][0]["status"] != 0:
            raise ValueError(f"repaired_mesh failed with status {int(r['info'][0]['status'])}: the mesh was not repaired")
        verts, faces = r["meshes"][0]
        return self._engine.transform_points(np.ascontiguousarray(verts, dtype=np.float64), T), faces

    # -- simplification --------------------------------------------------------------------------------------------------
    def simplified_mesh(self, cell=None, target_faces=None, place="quadric"):
        """This bone made smaller by vertex clustering (Engine.simplify with `cell` in mm, or Engine.simplify_to with `target_faces`:
        exactly one of the two) -> (verts (V', 3) float64, faces (F', 3) int32) in the CURRENT coordinate system, ready for
        Engine.upload as repaired_mesh's result is.  The resident mesh is not changed.  Clustering does not preserve topology.
        Raises ValueError when the mesh could not be simplified (a status in its info record: every face collapsed, or the cell is too
        small for the grid)."""
        if (cell is None) == (target_faces is None):
            raise ValueError("simplified_mesh needs cell or target_faces, not both")
        self._ensure_loaded()
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        meshes, info, _ = self._engine.simplify(cell, place=place) if cell is not None else self._engine.simplify_to(target_faces, place=place)
        if info[0]["status"] != 0:
            raise ValueError(f"simplified_mesh failed with status {int(info[0]['status'])}: the mesh was not simplified")
        verts, faces = meshes[0]
        return self._engine.transform_points(np.ascontiguousarray(verts, dtype=np.float64), T), faces

    # -- distances along the surface -------------------------------------------------------------------------------
    def _geodesic_seeds(self, where):
        """a vertex index, or a 3-D point in the CURRENT coordinate system -> (vertices, d0): the vertex itself with 0.0, or the point
        snapped with closest_point -- the three vertices of its closest face with their Euclidean distances from the snapped point"""
        if isinstance(where, (int, np.integer)):
            if not 0 <= int(where) < len(self._verts):
                raise ValueError("vertex index out of range")
            return np.array([int(where)], np.int64), np.zeros(1)
        p = np.asarray(where, dtype=np.float64)
        if p.shape != (3,):
            raise ValueError("a source is a vertex index or one 3-D point")
        rec, _ = self._closest_ct(p[None])
        if int(rec["status"][0]) != 0:
            raise ValueError(f"closest_point failed with status {int(rec['status'][0])}")
        tri = np.asarray(self._faces[int(rec["face"][0])], np.int64)
        return tri, np.linalg.norm(np.asarray(self._verts, np.float64)[tri] - np.asarray(rec["point"][0], np.float64), axis=1)

    def geodesic_distance(self, points_or_vertices, mode="unfold", max_dist=None):
        """How far every vertex lies from a vertex (an integer) or from a 3-D point in the CURRENT coordinate system, ALONG the bone
        (Engine.geodesic) -> (V,) float64, +inf where nothing within max_dist leads.  A point is snapped to the surface and enters as
        the three vertices of its closest face, each with its straight distance from the snapped point.  mode "edges": along mesh
        edges, as networkx on trimesh's vertex_adjacency_graph; "unfold": also across pairs of faces unfolded into a plane, which
        stays within a few per cent of the true geodesic."""
        v, d0 = self._geodesic_seeds(points_or_vertices)
        self._ensure_loaded()
        out = self._engine.geodesic([[v]], d0=[[d0]], mode=mode, max_dist=max_dist)
        return self._engine.geodesic_field(out, 0, 0)[0].copy()

    def geodesic_path(self, a, b, mode="unfold"):
        """The line on the bone from vertex a to vertex b -> (polyline (n, 3) in the CURRENT coordinate system, its length).  The
        distances come from the device, the walk from b back along the predecessors runs on the host; where the path crosses a pair of
        unfolded faces the polyline gets the crossing point on their shared edge, so it stays on the surface.  Raises ValueError when b
        cannot be reached from a, or is reached only over an arc of length 0."""
        for x in (a, b):
            if not isinstance(x, (int, np.integer)) or not 0 <= int(x) < len(self._verts):
                raise ValueError("geodesic_path runs between two vertex indices")
        self._ensure_loaded()
        pts, length = self._engine.geodesic_path(0, int(a), int(b), mode=mode)
        return self._engine.transform_points(pts, np.array(self._tfrm.matrix, dtype=np.float64)), length

    def surface_patch(self, center, radius):
        """The faces around `center` (a vertex or a 3-D point) within `radius` mm along the surface -> bool mask (F,): the faces whose
        three vertices all lie within it (one geodesic_distance call with max_dist = radius): the cap around the head apex, not
        everything a sphere of that radius cuts out of the bone."""
        if not float(radius) > 0.0:
            raise ValueError("radius must be > 0")
        d = self.geodesic_distance(center, max_dist=float(radius))
        return np.isfinite(d)[np.asarray(self._faces)].all(axis=1)

    # -- inside tests: generalized winding numbers -------------------------------------------------------------
    def winding_number(self, points):
        """The generalized winding number of the mesh about `points` (n, 3) in the CURRENT coordinate system -> float64 (n,), on the
        device (Engine.winding_numbers).  1 inside and 0 outside a closed bone; an OPEN mesh (a half from `resect_mesh()` has no cap)
        returns a fraction; a CAVITY whose wall faces inward returns 0; on the surface itself the value is about 0.5."""
        rec = self._engine.winding_numbers(self._points_ct(points)[0])[0]
        if np.any(rec["status"] != 0):
            raise ValueError(f"winding_number failed with status {int(rec['status'][rec['status'] != 0][0])}: a sum is not finite")
        return np.array(rec["winding"])

    def contains(self, points):
        """`mesh.contains(points)` in the CURRENT coordinate system -> bool (n,): |winding_number| >= 0.5.  An open mesh answers by its
        thresholded fraction, a cavity whose wall faces inward is outside, and a point on the surface itself is undefined."""
        return self._engine.contains(self._points_ct(points)[0])[0]

    def signed_distance(self, points, accel=None):
        """`trimesh.proximity.signed_distance(mesh, points)` in the CURRENT coordinate system -> float64 (n,): the distance to the
        surface, POSITIVE INSIDE and negative outside (the transforms are rigid: the distance is CT's).  Open meshes, cavities and
        the surface itself as in `contains`.  accel as in closest_point (the winding numbers do not read the hierarchy)."""
        p = self._points_ct(points)[0]
        with self._accel(accel):
            return self._engine.signed_distance(p)[0]

    # -- mass properties ----------------------------------------------------------------------------------------
    def mass_properties(self):
        """`mesh.area`, `volume`, `center_mass`, `moment_inertia`, `principal_inertia_components`, `principal_inertia_vectors` and the
        frame of the surface itself, in the CURRENT coordinate system, on the device (Engine.mass_properties) -> dict: the scalars
        (area, volume, closure, principal, shell_eig, faces, degenerate, vstatus) are CT's, unchanged by a rigid transform;
        center_mass and shell_centroid are mapped as points, principal_axes and shell_axes (rows) as directions, inertia and shell_cov
        (3, 3) as tensors.  Raises ValueError for a mesh without a surface; a mesh that encloses no volume has vstatus set and zeros
        in the volume fields."""
        self._ensure_loaded()
        T = np.array(self._tfrm.matrix, dtype=np.float64)
        R = T[:3, :3]
        m = self._engine.mass_properties()[0]
        if m["status"] != 0:
            raise ValueError(f"mass_properties failed with status {int(m['status'])}: the mesh has no faces or no area")
        C = np.zeros((3, 3))
        C[np.triu_indices(3)] = m["shell_cov"]
        C = C + np.triu(C, 1).T
        pts = self._engine.transform_points(np.ascontiguousarray(np.stack([m["center_mass"], m["shell_centroid"]])), T)
        has_volume = m["vstatus"] == 0
        return dict(area=float(m["area"]), volume=float(m["volume"]), closure=float(m["closure"]), center_mass=pts[0] if has_volume else np.zeros(3),
                    inertia=R @ m["inertia"] @ R.T, principal=np.array(m["principal"]), principal_axes=m["principal_axes"] @ R.T,
                    shell_centroid=pts[1], shell_cov=R @ C @ R.T, shell_eig=np.array(m["shell_eig"]), shell_axes=m["shell_axes"] @ R.T,
                    faces=int(m["faces"]), degenerate=int(m["degenerate"]), vstatus=int(m["vstatus"]))

    # -- rigid registration (ICP) -------------------------------------------------------------------------------
    def register(self, other, initial=None, mirror=None, sample=None, seed=0, accel=None, **options):
        """`trimesh.registration.icp(other, mesh)` / `mesh.register(other)` on the device (Engine.register): the rigid matrix that
        moves `other` onto this bone's surface.  `other` is an (n, 3) array of points or anything with `.vertices`, in the CURRENT
        coordinate system; `initial` a rigid (4, 4) starting matrix in that system (default: the identity); `mirror` = "x" | "y" | "z"
        reflects the points in that coordinate plane FIRST (a contralateral bone) -- the reflection is the caller's and is not part of
        the returned matrix.  options: metric ("plane" | "point"), max_iter, reject (mm), tol as in Engine.register.
        -> (matrix (4, 4) in the current system, info) with info = dict(rms, rms_first, pairs, iterations, converged, min_pivot);
        raises ValueError where the registration set a status (fewer than six accepted pairs, a singular system).

        ICP IS LOCAL: it finds the nearest minimum and needs an initial pose within its basin, whose size has not been measured (the
        tests start 3 and 4 degrees and a few millimetres off).  The bone's own coordinate system is the intended common ground: call
        `apply_csys_canal_transepiconylar()` on both bones first.  The point metric converges linearly (many iterations, each a small
        step), the plane metric quadratically near the solution but lets the points slide where the surface does not hold them
        (see `min_pivot`: near 0 on a plane, a sphere, a cylinder).

        `initial="principal"` makes the GLOBAL search of `trimesh.registration.mesh_other` instead (Engine.register_global): starts
        from the principal frames of the bone and of the points -- both directions of the long axis times `rolls` turns about it --,
        a short registration of a subsample from each and the full one from the best; for a scan, a contralateral bone or a second
        segmentation in an unknown pose.  options then also take rolls, coarse_points, coarse_iter and min_pairs, and info also holds
        winner, coarse_rms (one per start), mesh_ratio and points_ratio (the two largest shell eigenvalues' ratio: near 1 the shape
        has no long axis and the starts are arbitrary).

        THE POINTS MUST COVER THE BONE.  Vertices follow the mesher's density; with `sample=n` and a bone as `other` the points are n
        area-weighted samples of its surface instead (`other.sample_surface(n, seed)`).  accel="bvh": the pair step of every
        evaluation goes through the face hierarchy (Engine.query_accel), the same results."""
        with self._accel(accel):
            return self._register(other, initial, mirror, sample, seed, options)

    def _register(self, other, initial, mirror, sample, seed, options):
        pts = np.array(self._other_points(other, sample, seed), dtype=np.float64).reshape(-1, 3)
        if mirror is not None:
            if mirror not in ("x", "y", "z"):
                raise ValueError('mirror must be "x", "y", "z" or None')
            pts[:, "xyz".index(mirror)] *= -1.0
        p_ct, M = self._points_ct(pts)
        Mi = np.linalg.inv(M)
        if isinstance(initial, str):
            if initial != "principal":
                raise ValueError('initial must be a (4, 4) matrix, None or "principal"')
            rec, more = self._engine.register_global(p_ct, **options)
            rec = rec[0]
            if rec["status"] != 0:
                raise ValueError(f"register failed with status {int(rec['status'])}: no start qualified (winner {int(more['winner'][0])}), fewer than six "
                                 f"accepted pairs or a singular system (pairs {int(rec['pairs'])}, iterations {int(rec['iterations'])})")
            info = dict(_registration_info(rec), winner=int(more["winner"][0]), coarse_rms=np.array(more["coarse"][0]["rms"]),
                        mesh_ratio=float(more["mesh_ratio"][0]), points_ratio=float(more["points_ratio"][0]))
            return M @ np.array(rec["T"]) @ Mi, info
        T0 = None
        if initial is not None:
            initial = np.asarray(initial, dtype=np.float64).reshape(4, 4)
            if not np.array_equal(initial[3], (0.0, 0.0, 0.0, 1.0)):
                raise ValueError("initial must be a rigid matrix with the last row (0, 0, 0, 1)")
            T0 = (Mi @ initial @ M)[None]
            T0[0, 3] = (0.0, 0.0, 0.0, 1.0)      # (the product of three such rows, free of the inverse's rounding)
        rec = self._engine.register(p_ct, T0=T0, **options)[0]
        if rec["status"] != 0:
            raise ValueError(f"register failed with status {int(rec['status'])}: fewer than six accepted pairs or a singular system "
                             f"(pairs {int(rec['pairs'])}, iterations {int(rec['iterations'])})")
        return M @ np.array(rec["T"]) @ Mi, _registration_info(rec)

    # -- coordinate systems (bone.py:53-105, :146-157) --------------------------------------------------
    def _mesh_in(self, T):
        """`mesh_ct.copy().apply_transform(T)` (bone.py:155) on the device."""
        self._ensure_loaded()
        return Mesh(self._engine.mesh_transformed(0, T), self._faces, self._engine)

    def _apply(self, matrix, mesh):
        self._tfrm.matrix = matrix
        self._update_landmark_data()
        self.mesh = mesh
        self.transform = self._tfrm.matrix
        return self.transform

    def _mesh_in_record_csys(self, T):
        """The mesh in the record's own csys: the batch path's device buffer (SH_STAGE_APPLY, k_apply_csys) rather than a
        second transform pass, when this bone's late stages are what the engine holds."""
        e = self._engine
        self._ensure_loaded()
        V = len(self._verts)
        return Mesh(e.fetch("verts_csys", np.float64, (V, 3)), self._faces, e)

    def apply_csys_canal_articular(self) -> np.ndarray:
        self.canal.axis()
        self.anatomic_neck.axis_central()
        self.anatomic_neck.axis_normal()
        T = np.array(self._all()["csys_articular"], dtype=np.float64)     # construct_csys(canal, neck-normal axis) on the device (k_pack)
        mesh = self._mesh_in_record_csys(T) if self._BONE_KIND == _lib.BONE_PROXIMAL else self._mesh_in(T)
        return self._apply(T, mesh)

    def apply_csys_obb(self) -> np.ndarray:
        T = self._obb_transform.copy()
        return self._apply(T, self._mesh_in(T))

    def apply_csys_ct(self) -> np.ndarray:
        self._tfrm.reset()
        self._update_landmark_data()
        self.mesh = self._mesh_ct.copy()
        self.transform = self._tfrm.matrix
        return self.transform

    def apply_csys_custom(self, transform, from_ct=True) -> np.ndarray:
        if from_ct:
            self._tfrm.matrix = transform
            self._update_landmark_data()
            self.mesh = self._mesh_ct.copy().apply_transform(self._tfrm.matrix)
        else:   # reference quirk kept: the cumulative matrix is applied to the already moved mesh (bone.py:92-94)
            self._tfrm.matrix = np.dot(transform, self._tfrm.matrix)
            self._update_landmark_data()
            self.mesh = self.mesh.apply_transform(self._tfrm.matrix)
        self.transform = self._tfrm.matrix
        return self.transform

    def apply_translation(self, translation) -> np.ndarray:
        T = np.identity(4)
        T[:3, 3] = np.asarray(translation, dtype=np.float64).reshape(3)        # utils.py:259-264
        self._tfrm.matrix = np.dot(T, self._tfrm.matrix)
        self._update_landmark_data()
        self.mesh = self.mesh.apply_transform(self._tfrm.matrix)               # same quirk (bone.py:101-103)
        self.transform = self._tfrm.matrix
        return self.transform


# we are inheriting the functions but the init will be unique (bone.py:108-109)
class Humerus(ProximalHumerus):
    """bone.py:109-157"""
    _BONE_KIND = _lib.BONE_HUMERUS
    _LATE = LATE

    def _init_kind_specific(self):
        self.trans_epiconylar = TransEpicondylar(self)
        # metrics (bone.py:134-144 -> bone_props.py); values come from the device record (k_metrics)
        self.side = self._side
        self.retroversion = self._retroversion
        self.neckshaft = self._neckshaft
        self.radius_curvature = self._radius_curvature

    def apply_csys_canal_transepiconylar(self) -> np.ndarray:
        self.canal.axis()
        self.trans_epiconylar.axis()
        T = np.array(self._all()["csys"], dtype=np.float64)           # construct_csys on the device (k_pack)
        return self._apply(T, self._mesh_in_record_csys(T))
