"""Engine: one HIP context (device + stream) behind the C-ABI, NumPy in / NumPy out.

Host-side glue only -- every numeric stage runs in libshoulder_hip.so.  A missing library or a
failing call raises; nothing falls back to the CPU.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import LANDMARKS_DTYPE


class ShoulderHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libshoulder_hip error {code}: {msg}")
        self.code = code


_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models")

UNET_ORDER = None

# one answer of Engine.thickness: formed on the host from a sh_ray_hit, no record of the C side
THICKNESS_DTYPE = np.dtype([("thickness", "<f8"), ("point", "<f8", (3,)), ("face", "<i4")])


def unet_pack_order(depth):
    names = []
    for i in range(depth):
        names += [f"enc{i}a_w", f"enc{i}a_b", f"enc{i}b_w", f"enc{i}b_b"]
    names += ["bota_w", "bota_b", "botb_w", "botb_b"]
    for i in reversed(range(depth)):
        names += [f"up{i}_w", f"up{i}_b", f"dec{i}a_w", f"dec{i}a_b", f"dec{i}b_w", f"dec{i}b_b"]
    names += ["head_w", "head_b"]
    return names


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _is_index_array(s):
    """one set of source vertices (an integer array, or a list of integers, possibly empty), as opposed to a list of sets"""
    if isinstance(s, np.ndarray):
        return s.dtype != object and s.ndim <= 1
    return isinstance(s, (list, tuple)) and all(isinstance(x, (int, np.integer)) for x in s)


def geodesic_polyline(verts, faces, rec, opp, d, pred, end):
    """The walk back along pred from vertex `end` to its root on one mesh, on the host -> (points (n, 3) float64 from the root to `end`,
    the summed length of the polyline).  verts (V, 3) float64, faces (F, 3); rec and opp are the mesh's "geo.face" (len[3], unf[3]) and
    "geo.opp"; d and pred the planes of one set.  A hop that is no mesh edge runs over an unfolded diagonal and contributes the point
    P_lo + (x_c / l) E where it crosses the edge the two faces share (the rule of include/shoulder_hip.h, restated here in NumPy)."""
    if not 0 <= end < len(d):
        raise ValueError("vertex index out of range")
    if pred[end] == _lib.GEO_UNREACHED:
        raise ValueError(f"vertex {end} is not reached")
    pts, at = [verts[end]], int(end)
    while pred[at] != _lib.GEO_ROOT:
        u = int(pred[at])
        if u == _lib.GEO_NO_PRED:
            raise ValueError(f"vertex {at} is reached over an arc of length 0 and has no predecessor")
        rows = np.nonzero((faces == at).any(axis=1) & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]))[0]
        hop = None
        for fi in rows:      # a mesh edge first: slot k is the edge to the next corner, slot (k + 2) % 3 the one to the previous
            k = int(np.nonzero(faces[fi] == at)[0][0])
            for other, slot in ((faces[fi, (k + 1) % 3], k), (faces[fi, (k + 2) % 3], (k + 2) % 3)):
                if other == u and d[u] + rec[fi, slot] == d[at]:
                    hop = ()
        if hop is None:
            for fi in rows:
                e = (int(np.nonzero(faces[fi] == at)[0][0]) + 1) % 3
                if opp[fi, e] == u and d[u] + rec[fi, 3 + e] == d[at]:
                    a, b = int(faces[fi, e]), int(faces[fi, (e + 1) % 3])
                    lo, hi, p, q = min(a, b), max(a, b), min(at, u), max(at, u)
                    E = verts[hi] - verts[lo]
                    l = np.sqrt(E @ E)
                    x, y = [], []
                    for r in (p, q):
                        dr = verts[r] - verts[lo]
                        x.append((dr @ E) / l)
                        y.append(np.sqrt(max(dr @ dr - x[-1] * x[-1], 0.0)))
                    hop = (verts[lo] + (((x[0] * y[1] + x[1] * y[0]) / (y[0] + y[1])) / l) * E,)
                    break
        if hop is None:
            raise RuntimeError(f"no arc from {u} to {at} carries the distance")
        pts.extend(hop)
        pts.append(verts[u])
        at = u
    pts = np.array(pts[::-1])
    return pts, float(np.linalg.norm(np.diff(pts, axis=0), axis=1).sum())


def _mat4(T):
    """a C-contiguous float64 4x4 (the C side reads 16 doubles); anything else is the reference's ValueError (base.py:57-58)"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("Invalid transformation matrix shape")
    return T


def _icp_options(metric="plane", max_iter=20, reject=np.inf, tol=0.0, **_):
    """the options of a registration as the C struct; the defaults are register's (other keys of an options dict are not looked at)"""
    if metric not in ("point", "plane"):
        raise ValueError('metric must be "point" or "plane"')
    return _lib.IcpOptions(_lib.ICP_PLANE if metric == "plane" else _lib.ICP_POINT, int(max_iter), float(reject), float(tol))


def principal_start_matrices(cm, axes, points, rolls=8):
    """The starts of Engine.principal_starts for one humerus -> ((2 * rolls, 4, 4), the ratio of the two largest covariance
    eigenvalues of the points).  cm, axes: the centroid and the frame of the mesh (rows are axes, the long one first, right-handed)."""
    cm, Xm = np.asarray(cm, np.float64), np.asarray(axes, np.float64).reshape(3, 3).T
    p = np.asarray(points, np.float64).reshape(-1, 3)
    cp = p.mean(axis=0)
    d = p - cp
    w, V = np.linalg.eigh(d.T @ d / float(len(p)))
    Xp = np.ascontiguousarray(V[:, ::-1])
    Xp[:, 2] = np.cross(Xp[:, 0], Xp[:, 1])
    T = np.zeros((2 * rolls, 4, 4))
    for phi, F in enumerate((np.identity(3), np.diag([-1.0, 1.0, -1.0]))):
        for r in range(rolls):
            a = 2.0 * np.pi * r / rolls
            Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
            R = Xm @ Rx @ F @ Xp.T
            k = phi * rolls + r
            T[k, :3, :3], T[k, :3, 3], T[k, 3, 3] = R, cm - R @ cp, 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(w[2] / w[1])
    return T, ratio


class Engine:
    def __init__(self, device=0, stream=None):
        self.L = _lib.load()
        h = ctypes.c_void_p()
        rc = self.L.sh_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h))
        if rc != 0:
            raise ShoulderHipError(rc, f"sh_ctx_create(device={device}) failed (is a HIP device visible?)")
        self.h = h
        self.device = device
        self._inflight, self._pin_slot = [], 0
        self._resect_P = None      # planes per humerus of the last resect() (resect_stems sizes its output by it)

    def close(self):
        if getattr(self, "h", None):
            self._free_pinned()
            self.L.sh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise ShoulderHipError(rc, self.L.sh_last_error(self.h).decode())

    def _chk_records(self, rc, out, strict):
        """strict=False: a return code that some record's `status` carries is that humerus' failure, not the batch's -- the
        records come back and `status` says which humeri failed.  Anything else (context-level errors) raises."""
        if rc == 0 or strict or out is None or "status" not in (out.dtype.names or ()) or not np.any(out["status"] == rc):
            self._chk(rc)

    # ---- open contours (include/shoulder_hip.h sh_set_open_contours) ------------------------------------------------
    _OPEN_MODES = {"error": _lib.OPEN_ERROR, "bridge": _lib.OPEN_BRIDGE}

    def set_open_contours(self, mode="error", max_gap=_lib.OPEN_GAP_DEFAULT):
        """mode "error" (default): an open section fails its humerus (SH_ERR_GEOMETRY); "bridge": chain gaps up to max_gap mm
        are bridged, segments on no loop dropped."""
        if mode not in self._OPEN_MODES:
            raise ValueError(f'open contour mode is "error" or "bridge", not {mode!r}')
        gap = float(max_gap)
        if not np.isfinite(gap) or gap < 0:
            raise ValueError(f"max_gap must be finite and >= 0, not {max_gap!r}")
        self._chk(self.L.sh_set_open_contours(self.h, self._OPEN_MODES[mode], gap))

    def get_open_contours(self):
        """(mode, max_gap) of the next run."""
        m, g = ctypes.c_int(), ctypes.c_double()
        self._chk(self.L.sh_get_open_contours(self.h, ctypes.byref(m), ctypes.byref(g)))
        return {v: k for k, v in self._OPEN_MODES.items()}[m.value], g.value

    def open_contour_stats(self):
        """Per humerus of the last run: (bridged, dropped) open chains, two int32 arrays (zeros after an "error"-mode run)."""
        br, dr = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
        self._chk(self.L.sh_open_contour_stats(self.h, _ptr(br), _ptr(dr)))
        return br, dr

    def open_edges(self):
        """Per resident mesh: undirected edges used by a number of faces other than two (0: watertight), int64."""
        out = np.zeros(self.B, np.int64)
        self._chk(self.L.sh_mesh_open_edges(self.h, _ptr(out)))
        return out

    # ---- parameters ----------------------------------------------------------------------------
    def load_rfc(self, npz_path=None):
        z = np.load(npz_path or os.path.join(_MODELS, "rfc_bg3.npz"))
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        feat, thr = c(z["feat"], np.int32), c(z["thr"], np.float32)
        ti, fi = c(z["true_idx"], np.int32), c(z["false_idx"], np.int32)
        lw, roots = c(z["leaf_weight"], np.float32), c(z["roots"], np.int32)
        self._chk(self.L.sh_load_rfc(self.h, _ptr(feat), _ptr(thr), _ptr(ti), _ptr(fi), _ptr(lw), len(feat), _ptr(roots), len(roots)))

    def load_unet(self, weights, base, depth):
        packed = np.concatenate([np.asarray(weights[k], dtype=np.float32).ravel() for k in unet_pack_order(depth)])
        packed = np.ascontiguousarray(packed)
        self._chk(self.L.sh_load_unet(self.h, int(base), int(depth), _ptr(packed), packed.size))

    def load_unet_onnx(self, path_or_bytes):
        """Parameters of the anatomic-neck network from an ONNX file of the supported UNet family (onnx_import.py; the
        reference opens `humerus/models/unetcrf_anp.onnx` at anatomic_neck.py:62-69).  Returns (base, depth)."""
        from .onnx_import import unet_from_onnx
        w, base, depth = unet_from_onnx(path_or_bytes)
        self.load_unet(w, base, depth)
        return base, depth

    def set_params(self, canal_cutoff=None, groove_cutoff=None, groove_deg_window=None, unet_dtype=None, bone_kind=None):
        """Read-modify-write of sh_params: fields left at None keep the value in force (an engine configured for a bf16
        UNet stays so when a facade object only sets its bone kind)."""
        p = _lib.Params()
        self._chk(self.L.sh_get_params(self.h, ctypes.byref(p)))
        if canal_cutoff is not None:
            p.canal_cutoff[0], p.canal_cutoff[1] = canal_cutoff
        if groove_cutoff is not None:
            p.groove_cutoff[0], p.groove_cutoff[1] = groove_cutoff
        if groove_deg_window is not None:
            p.groove_deg_window = groove_deg_window
        if unet_dtype is not None:
            p.unet_dtype = unet_dtype
        if bone_kind is not None:
            p.bone_kind = bone_kind
        self._chk(self.L.sh_set_params(self.h, ctypes.byref(p)))

    def get_params(self):
        p = _lib.Params()
        self._chk(self.L.sh_get_params(self.h, ctypes.byref(p)))
        return dict(canal_cutoff=tuple(p.canal_cutoff), groove_cutoff=tuple(p.groove_cutoff), groove_deg_window=p.groove_deg_window,
                    unet_dtype=p.unet_dtype, bone_kind=p.bone_kind)

    def reset_params(self):
        p = _lib.Params()
        self.L.sh_default_params(ctypes.byref(p))
        self._chk(self.L.sh_set_params(self.h, ctypes.byref(p)))

    def param_block(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._chk(self.L.sh_param_block(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def param_block_commit(self):
        """The device parameter block was overwritten from outside (a broadcast): refresh the host mirrors (sh_param_block_commit)."""
        self._chk(self.L.sh_param_block_commit(self.h))

    # ---- meshes ----------------------------------------------------------------------------------
    def upload(self, meshes):
        """meshes: list of (verts float32 (V,3), faces int32 (F,3))."""
        if len(meshes) == 0:
            raise ValueError("upload() needs at least one mesh")
        verts, faces, voff, foff = self.pack_meshes(meshes)
        self._chk(self.L.sh_upload_meshes(self.h, _ptr(verts), _ptr(faces), _ptr(voff), _ptr(foff), len(meshes)))
        self.voff, self.foff = voff, foff

    def upload_packed(self, packed):
        """sh_upload_meshes from the 4-tuple of pack_meshes()."""
        verts, faces, voff, foff = packed
        self._chk(self.L.sh_upload_meshes(self.h, _ptr(verts), _ptr(faces), _ptr(voff), _ptr(foff), len(voff) - 1))
        self.voff, self.foff = voff, foff

    def upload_stl(self, files):
        """files: list of paths or bytes objects, each one binary STL; parsed and merged on the device (sh_upload_stl)."""
        import pathlib
        blobs = [f if isinstance(f, (bytes, bytearray)) else pathlib.Path(f).read_bytes() for f in files]
        n = len(blobs)
        keep = [bytes(b) for b in blobs]      # the buffers must outlive the call
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(k), ctypes.c_void_p) for k in keep])
        sizes = (ctypes.c_size_t * n)(*[len(k) for k in keep])
        voff = np.zeros(n + 1, dtype=np.int64)
        foff = np.zeros(n + 1, dtype=np.int64)
        self._chk(self.L.sh_upload_stl(self.h, ptrs, sizes, n, _ptr(voff), _ptr(foff)))
        self.voff, self.foff = voff, foff

    # ---- the staging side: the NEXT batch is handed over while a run of the resident one executes -----------------------------
    @staticmethod
    def pack_meshes(meshes):
        """list of (verts, faces) -> (verts float32 (sumV,3), faces int32 (sumF,3), voff int64 (B+1), foff int64 (B+1)): the arrays
        sh_upload_meshes / sh_stage_meshes take.  A caller that streams batches packs each one once, outside its hot loop."""
        if len(meshes) == 0:
            raise ValueError("at least one mesh")
        verts = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1, 3) for v, _ in meshes]))
        faces = np.ascontiguousarray(np.concatenate([np.asarray(f, dtype=np.int32).reshape(-1, 3) for _, f in meshes]))
        voff = np.zeros(len(meshes) + 1, dtype=np.int64)
        foff = np.zeros(len(meshes) + 1, dtype=np.int64)
        voff[1:] = np.cumsum([len(v) for v, _ in meshes])
        foff[1:] = np.cumsum([len(f) for _, f in meshes])
        return verts, faces, voff, foff

    def stage(self, meshes):
        """sh_stage_meshes: `meshes` = list of (verts, faces) or the 4-tuple of pack_meshes().  Returns at once; commit_staged()
        makes the batch the resident one."""
        packed = meshes if (isinstance(meshes, tuple) and len(meshes) == 4 and getattr(meshes[2], "dtype", None) == np.int64) else self.pack_meshes(meshes)
        verts, faces, voff, foff = packed
        self._chk(self.L.sh_stage_meshes(self.h, _ptr(verts), _ptr(faces), _ptr(voff), _ptr(foff), len(voff) - 1))
        self._staged_off = (voff, foff)
        self._staged_keep = packed      # the library reads the arrays from a background thread until the commit

    def stage_stl(self, files):
        """sh_stage_stl: list of paths or bytes objects (binary STL); parse + vertex merge on the device, beside the run in flight."""
        import pathlib
        keep = [bytes(f) if isinstance(f, (bytes, bytearray)) else pathlib.Path(f).read_bytes() for f in files]
        n = len(keep)
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(k), ctypes.c_void_p) for k in keep])
        sizes = (ctypes.c_size_t * n)(*[len(k) for k in keep])
        self._chk(self.L.sh_stage_stl(self.h, ptrs, sizes, n))
        self._staged_off = None
        self._staged_keep = keep        # the library reads the files from a background thread until the commit

    def commit_staged(self):
        """sh_commit_staged: the staged batch becomes the resident one (needs every submitted run collected)."""
        try:
            self._chk(self.L.sh_commit_staged(self.h, None, None))
        finally:
            # the arrays / file images stay referenced while the batch is STILL staged (a refused commit -- runs in flight -- leaves it
            # staged, and the library's background thread may still be copying from them)
            if not self.staged:
                self._staged_keep = None
        B = self.L.sh_batch_size(self.h)
        if getattr(self, "_staged_off", None) is not None:
            self.voff, self.foff = self._staged_off
        else:      # STL: the offsets were made on the device
            self.voff = self.fetch("voff", np.int64, (B + 1,)).copy()
            self.foff = self.fetch("foff", np.int64, (B + 1,)).copy()
        self._staged_off = None

    @property
    def staged(self):
        return self.L.sh_staged(self.h) == 1

    def synth_batch(self, T):
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 16)
        V, F = int(self.voff[1] - self.voff[0]), int(self.foff[1] - self.foff[0])
        self._chk(self.L.sh_synth_batch(self.h, _ptr(T), len(T)))
        self.voff = np.arange(len(T) + 1, dtype=np.int64) * V
        self.foff = np.arange(len(T) + 1, dtype=np.int64) * F

    @property
    def B(self):
        return self.L.sh_batch_size(self.h)

    def set_keep_products(self, on=True):
        """Every proximal plane's resampled contour and polar rows are written (sh_set_keep_products): for fetch("prox.ixy") etc.;
        off (the default) a run writes the rows its later stages read."""
        self._chk(self.L.sh_set_keep_products(self.h, int(bool(on))))

    # ---- record format ------------------------------------------------------------------------------
    def set_record_rows(self, anp_rows=0):
        """sh_set_record_rows: 0 = full 104 KB records, R > 0 = packed records carrying R anatomic-neck rows (n_anp keeps the
        true count; anp_points(b) fetches every row).  run / submit / collect then return arrays of _lib.record_dtype(R)."""
        self._chk(self.L.sh_set_record_rows(self.h, int(anp_rows)))
        if int(anp_rows) != getattr(self, "_rec_rows", 0):
            self._free_pinned()
        self._rec_rows = int(anp_rows)

    @property
    def record_dtype(self):
        return _lib.record_dtype(getattr(self, "_rec_rows", 0))

    def anp_points(self, b):
        """Every anatomic-neck point (CT) of humerus b of the last run (sh_anp_points)."""
        n = ctypes.c_int()
        self._chk(self.L.sh_anp_points(self.h, int(b), None, 0, ctypes.byref(n)))
        out = np.empty((max(1, n.value), 3), dtype=np.float64)
        self._chk(self.L.sh_anp_points(self.h, int(b), _ptr(out), len(out), ctypes.byref(n)))
        return out[: n.value]

    # ---- run ---------------------------------------------------------------------------------------
    def run(self, stages=_lib.STAGE_ALL, fetch=True, strict=True):
        """One sh_run over the resident batch.  fetch=True: a fresh record array; fetch="view": the engine's page-locked
        record buffer (no allocation, direct D2H), valid until the next run; fetch=False: records stay on the device.
        strict=False: humeri that failed do not raise, their records' `status` says so (needs fetched records)."""
        if fetch == "view":
            out = self._pinned_records()
        else:
            out = np.zeros(self.B, dtype=self.record_dtype) if fetch else None
        self._chk_records(self.L.sh_run(self.h, int(stages), _ptr(out) if out is not None else None), out, strict)
        return out

    def submit(self, stages=_lib.STAGE_ALL, fetch="view", out_ptr=None):
        """Enqueue one run and return at once (sh_submit); at most two may be in flight.  `collect()` hands back the records of
        the oldest one.  fetch="view": records go to one of the engine's two page-locked buffers; False: they stay on the
        device; out_ptr: raw address of B records of page-locked host or DEVICE memory (e.g. a gather's send buffer)."""
        if fetch not in ("view", False):
            raise ValueError('submit(fetch=...) takes "view" or False')
        out = None
        if out_ptr is not None:
            ptr = ctypes.c_void_p(int(out_ptr))
        elif fetch == "view":
            out = self._pinned_records(self._pin_slot)
            self._pin_slot ^= 1
            ptr = _ptr(out)
        else:
            ptr = None
        self._inflight.append(out)
        try:
            self._chk(self.L.sh_submit(self.h, int(stages), ptr))
        except Exception:
            self._inflight.pop()
            raise

    def collect(self, strict=True):
        out = self._inflight.pop(0) if self._inflight else None      # (nothing in flight: sh_collect reports it)
        self._chk_records(self.L.sh_collect(self.h), out, strict)
        return out

    def _pinned_records(self, slot=0):
        pins = self.__dict__.setdefault("_pins", {})
        ent = pins.get(slot)
        if ent is None or ent[1] < self.B:
            if ent is not None:
                self.L.sh_host_free(self.h, ent[0])
            p = ctypes.c_void_p()
            dt = self.record_dtype
            nbytes = self.B * dt.itemsize
            self._chk(self.L.sh_host_alloc(self.h, nbytes, ctypes.byref(p)))
            arr = np.frombuffer((ctypes.c_char * nbytes).from_address(p.value), dtype=dt)
            ent = pins[slot] = (p, self.B, arr)
        return ent[2][: self.B]

    def _free_pinned(self):
        for p, _, _ in self.__dict__.get("_pins", {}).values():
            self.L.sh_host_free(self.h, p)
        self.__dict__["_pins"] = {}

    def landmarks_device(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._chk(self.L.sh_landmarks_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def buffer_device(self, name):
        """(device address, bytes) of a named buffer (sh_buffer_device)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._chk(self.L.sh_buffer_device(self.h, name.encode(), ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def affine_apply(self, T, dev_in, dev_out, off):
        """utils.transform_pts for B point sets resident on the device (sh_affine_apply): out[off[b]:off[b+1]] = T[b] * in[...];
        dev_in / dev_out are device addresses of float64 xyz arrays, T (B,4,4), off (B+1,) point offsets."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise ValueError("Invalid transformation matrix shape")
        off = np.ascontiguousarray(off, dtype=np.int64)
        if off.shape != (len(T) + 1,):
            raise ValueError("off must hold B + 1 offsets")
        self._chk(self.L.sh_affine_apply(self.h, _ptr(T), ctypes.c_void_p(int(dev_in)), ctypes.c_void_p(int(dev_out)), _ptr(off), len(T)))

    def mesh_transformed(self, b, T):
        T = _mat4(T)
        if not 0 <= int(b) < len(self.voff) - 1:
            raise IndexError("mesh index out of range")
        out = np.empty((int(self.voff[b + 1] - self.voff[b]), 3), dtype=np.float64)
        self._chk(self.L.sh_mesh_transformed(self.h, int(b), _ptr(T), _ptr(out)))
        return out

    def transform_points(self, pts, T):
        """utils.transform_pts on the device: (n,3) float64 host points -> (n,3)."""
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        T = _mat4(T)
        out = np.empty_like(pts)
        self._chk(self.L.sh_transform_points(self.h, _ptr(T), _ptr(pts), len(pts), _ptr(out)))
        return out

    def ring(self, set_name, b, k):
        """Closed largest loop of plane k of slice set `set_name` ("distal", "prox", "neckc") of humerus b: (n + 1, 2) float64 in
        the box frame (sh_ring; also for planes whose ring lives in the overflow pool)."""
        n = ctypes.c_int()
        self._chk(self.L.sh_ring(self.h, set_name.encode(), int(b), int(k), None, 0, ctypes.byref(n)))
        out = np.empty((max(1, n.value), 2), dtype=np.float64)
        self._chk(self.L.sh_ring(self.h, set_name.encode(), int(b), int(k), _ptr(out), len(out), ctypes.byref(n)))
        return out[: n.value]

    def section_plane(self, b, origin, normal, cap=8192):
        """Unique crossing points (CT) of mesh b with one plane: `mesh_ct.section(...).vertices`."""
        o = np.ascontiguousarray(origin, dtype=np.float64)
        n = np.ascontiguousarray(normal, dtype=np.float64)
        while True:      # (a dense mesh crosses a plane more often than the default capacity: ask again with room)
            out = np.empty((cap, 3), dtype=np.float64)
            k = ctypes.c_int()
            rc = self.L.sh_section_plane(self.h, int(b), _ptr(o), _ptr(n), _ptr(out), cap, ctypes.byref(k))
            if rc == -4 and cap < (1 << 24):
                cap *= 8
                continue
            self._chk(rc)
            return out[:k.value].copy()

    def slice_mesh_planes(self, verts, faces, origins, normals, edges=False):
        """`Trimesh.slice_plane(origin, normal)` of one mesh for P planes in one device pass (sh_slice_mesh_planes;
        arthroplasty.py:80-87).  -> list of (verts (n,3) f64, faces (m,3) i32[, cut edges (k,2) i32]) per plane."""
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        n = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        if len(o) != len(n):
            raise ValueError("one origin per normal")
        P = len(o)
        cnt = np.zeros((P, 3), dtype=np.int32)
        self._chk(self.L.sh_slice_mesh_planes(self.h, _ptr(v), len(v), _ptr(f), len(f), _ptr(o), _ptr(n), P, None, 0, None, 0, None, 0, _ptr(cnt)))
        cv, cf, ce = (max(1, int(x)) for x in cnt.max(axis=0))
        ov = np.empty((P, cv, 3), dtype=np.float64)
        of = np.empty((P, cf, 3), dtype=np.int32)
        oe = np.empty((P, ce, 2), dtype=np.int32) if edges else None
        self._chk(self.L.sh_slice_mesh_planes(self.h, _ptr(v), len(v), _ptr(f), len(f), _ptr(o), _ptr(n), P, _ptr(ov), cv, _ptr(of), cf,
                                              _ptr(oe) if edges else None, ce if edges else 0, _ptr(cnt)))
        out = []
        for p in range(P):
            nv_, nf_, ne_ = (int(x) for x in cnt[p])
            out.append((ov[p, :nv_].copy(), of[p, :nf_].copy()) + ((oe[p, :ne_].copy(),) if edges else ()))
        return out

    # ---- batched head resection (include/shoulder_hip.h sh_resect_*) -------------------------------------------------
    def resect(self, planes=None, offsets=None, fit=False, heads=None, seat_center="centroid"):
        """B resident humeri x P resection planes in one device pass -> structured array (B, P) of _lib.RESECTION_DTYPE.
        planes: (B, P, 6) or (B, P, 2, 3) float64, (point, normal) in CT per humerus (sh_resect_planes; needs no run).
        offsets: P cuts relative to every humerus' own anatomic-neck plane -- a list of dicts or a structured array with the
        sh_cut_offset field names (_lib.CUT_OFFSET_DTYPE; missing keys are 0) -- planes built on the device from the records of
        the last run (sh_resect_offsets; needs a run with STAGE_ANP and STAGE_CSYS).  A cut's `status` tells its own failure.
        fit=True: -> (records, fits), fits a structured array (B, P) of _lib.HEAD_FIT_DTYPE -- the sphere of every cut's head piece and
        the ellipse of its cut (sh_resect_*_fit; the records are the same bytes).
        fit=True, heads=[(R, h), ...]: -> (records, fits, seats), seats a structured array (B, P, K) of _lib.SEAT_DTYPE -- how each of
        the K implant heads (radius of curvature, thickness) sits on each cut, about the cut's area centroid (seat_center="centroid")
        or the foot of the fitted sphere's centre ("sphere") (sh_resect_*_seat; records and fits are the same bytes)."""
        if (planes is None) == (offsets is None):
            raise ValueError("resect() takes planes or offsets")
        B = self.B
        hd = None
        if heads is not None:
            if not fit:
                raise ValueError("heads needs fit=True")
            if seat_center not in ("centroid", "sphere"):
                raise ValueError("seat_center must be 'centroid' or 'sphere'")
            hd = np.ascontiguousarray(np.asarray(heads, dtype=np.float64).reshape(-1, 2))
            mode = _lib.SEAT_SPHERE_AXIS if seat_center == "sphere" else _lib.SEAT_CUT_CENTROID
        if planes is not None:
            src = np.ascontiguousarray(planes, dtype=np.float64)
            if src.ndim < 2 or src.shape[0] != B or src.size % (6 * max(B, 1)) or src.size == 0:
                raise ValueError("planes must have shape (B, P, 6)")
            P = src.size // (6 * B)
        else:
            if isinstance(offsets, np.ndarray) and offsets.dtype.names:
                src = np.zeros(offsets.shape, dtype=_lib.CUT_OFFSET_DTYPE).reshape(-1)
                for n in offsets.dtype.names:
                    src[n] = offsets[n].reshape(-1)      # (an unknown field name raises)
            else:
                offsets = list(offsets)
                src = np.zeros(len(offsets), dtype=_lib.CUT_OFFSET_DTYPE)
                for i, d in enumerate(offsets):
                    for k, v in dict(d).items():
                        src[k][i] = v
            P = len(src)
            if P == 0:
                raise ValueError("at least one offset")
        level = "seat" if hd is not None else ("fit" if fit else "records")
        res = [np.zeros((B, P), dtype=_lib.RESECTION_DTYPE)]
        if level != "records":
            res.append(np.zeros((B, P), dtype=_lib.HEAD_FIT_DTYPE))
        if level == "seat":
            res.append(np.zeros((B, P, len(hd)), dtype=_lib.SEAT_DTYPE))
        fn = {("planes", "records"): self.L.sh_resect_planes, ("offsets", "records"): self.L.sh_resect_offsets,
              ("planes", "fit"): self.L.sh_resect_planes_fit, ("offsets", "fit"): self.L.sh_resect_offsets_fit,
              ("planes", "seat"): self.L.sh_resect_planes_seat, ("offsets", "seat"): self.L.sh_resect_offsets_seat}
        catalogue = (_ptr(hd), len(hd), mode) if level == "seat" else ()
        self._chk(fn["planes" if planes is not None else "offsets", level](self.h, _ptr(src), P, *catalogue, *(_ptr(a) for a in res)))
        self._resect_P = P
        return res[0] if level == "records" else tuple(res)

    def resect_ring(self, b, p):
        """The largest loop of cut p of humerus b of the last resect(): (n + 1, 3) float64 in CT, closed, counter-clockwise seen
        from the tip of the normal, canonical start (sh_resect_ring); (0, 3) for a cut without a ring."""
        n = ctypes.c_int()
        self._chk(self.L.sh_resect_ring(self.h, int(b), int(p), None, 0, ctypes.byref(n)))
        out = np.empty((max(1, n.value), 3), dtype=np.float64)
        if n.value:
            self._chk(self.L.sh_resect_ring(self.h, int(b), int(p), _ptr(out), len(out), ctypes.byref(n)))
        return out[: n.value]

    # ---- canal profiles and stems (include/shoulder_hip.h sh_canal_profile / sh_resect_stems) ------------------------------
    def canal_profile(self, z0, dz, L, A, frames=None, fetch=("levels",)):
        """The polar profile of every resident humerus about its canal axis: L levels z_l = z0 - l dz of the humerus' canal frame, A rays
        per level.  frames: (B, 4, 4) or (B, 16) float64 rigid CT -> frame matrices, or None for every record's csys_articular (needs a
        run with STAGE_ANP and STAGE_CSYS).  fetch: which of "levels" (structured (B, L) of _lib.CANAL_LEVEL_DTYPE), "near", "far"
        ((B, L, A) float64; +inf / 0 where a ray hits nothing) come back -- one of them alone, or a tuple in the order asked for.  The
        profile stays on the device for resect_stems() until the next upload."""
        names = (fetch,) if isinstance(fetch, str) else tuple(fetch)
        if any(n not in ("levels", "near", "far") for n in names):
            raise ValueError("fetch takes 'levels', 'near' and 'far'")
        B, L, A = self.B, int(L), int(A)
        grid = _lib.CanalGrid(float(z0), float(dz), L, A)
        fr = None
        if frames is not None:
            fr = np.ascontiguousarray(frames, dtype=np.float64)
            if fr.size != 16 * B:
                raise ValueError("frames must have shape (B, 4, 4)")
        out = {}
        if 1 <= L <= 1024 and 3 <= A <= 256:      # (the library reports a bad grid; nothing is sized by it here)
            if "levels" in names:
                out["levels"] = np.zeros((B, L), dtype=_lib.CANAL_LEVEL_DTYPE)
            for n in ("near", "far"):
                if n in names:
                    out[n] = np.zeros((B, L, A), dtype=np.float64)
        ptr = lambda n: _ptr(out[n]) if n in out else None
        self._chk(self.L.sh_canal_profile(self.h, ctypes.byref(grid), _ptr(fr) if fr is not None else None, ptr("near"), ptr("far"), ptr("levels")))
        return out[names[0]] if isinstance(fetch, str) or len(names) == 1 else tuple(out[n] for n in names)

    def resect_stems(self, stems):
        """K stems -- (length, r_prox, r_tip) rows or a structured array of _lib.STEM_DTYPE -- below every cut of the last resect()
        against the last canal_profile() -> structured array (B, P, K) of _lib.STEM_FIT_DTYPE (sh_resect_stems)."""
        st = np.asarray(stems)
        st = np.ascontiguousarray(st, dtype=_lib.STEM_DTYPE).view(np.float64).reshape(-1, 3) if st.dtype.names else np.ascontiguousarray(st, dtype=np.float64).reshape(-1, 3)
        K = len(st)
        if K < 1 or K > _lib.STEM_MAX:
            raise ValueError("1..%d stems" % _lib.STEM_MAX)
        P = self._resect_P or 1      # (the planes per humerus of the last resect(); without one the library reports the state)
        out = np.zeros((self.B, P, K), dtype=_lib.STEM_FIT_DTYPE)
        self._chk(self.L.sh_resect_stems(self.h, _ptr(st), K, _ptr(out)))
        return out

    # ---- implant plans (include/shoulder_hip.h sh_resect_plan) --------------------------------------------------------------
    def plan(self, n=8, rule=None, compat=None, ref_planes=None):
        """The n best (cut, head, stem) triples of every humerus from the last seated resect() and the last resect_stems(), ranked on
        the device under one rule -> (plans, refs): structured arrays (B, n) of _lib.PLAN_DTYPE and (B,) of _lib.PLAN_REF_DTYPE
        (sh_resect_plan).  rule: a dict with sh_plan_rule's field names; a missing limit is off (+-inf), missing weights, `fill_target`
        and `margin` are 0.  compat: (K_h, K_s) booleans, which stems each head goes with, or None for all.  ref_planes: (B, 6) or
        (B, 2, 3) float64 (point, normal) in CT, the plane that parts head from tuberosity, or None for every record's anatomic-neck
        plane (needs a run with STAGE_ANP and STAGE_CSYS)."""
        r = _lib.PlanRule(max_overhang=np.inf, min_coverage=-np.inf, min_clearance=-np.inf, max_eccentricity=np.inf)
        for k, v in dict(rule or {}).items():
            if k not in _lib.PLAN_RULE_DTYPE.names:
                raise ValueError("unknown rule field %r" % (k,))
            setattr(r, k, float(v))
        words = None
        if compat is not None:
            cm = np.asarray(compat, dtype=bool)
            if cm.ndim != 2 or cm.shape[0] > _lib.SEAT_MAX_HEADS or cm.shape[1] > _lib.STEM_MAX:
                raise ValueError("compat must have shape (K_h, K_s)")
            words = np.zeros(_lib.SEAT_MAX_HEADS, dtype=np.uint64)
            words[: cm.shape[0]] = (cm.astype(np.uint64) << np.arange(cm.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        rp = None
        if ref_planes is not None:
            rp = np.ascontiguousarray(ref_planes, dtype=np.float64)
            if rp.size != 6 * self.B:
                raise ValueError("ref_planes must have shape (B, 6)")
        n = int(n)
        plans = np.zeros((self.B, max(n, 0)), dtype=_lib.PLAN_DTYPE)
        refs = np.zeros(self.B, dtype=_lib.PLAN_REF_DTYPE)
        self._chk(self.L.sh_resect_plan(self.h, ctypes.byref(r), _ptr(words) if words is not None else None, _ptr(rp) if rp is not None else None,
                                        n, _ptr(plans), _ptr(refs)))
        return plans, refs

    # ---- rays against the resident batch, every hit (include/shoulder_hip.h sh_ray_cast / sh_anp_axis_hits) ----------------------
    def _rays_arg(self, origins, directions):
        """the rays of a call as the C side reads them -> (records of _lib.RAY_DTYPE, R, per_humerus)"""
        o = np.ascontiguousarray(origins, dtype=np.float64)
        d = np.ascontiguousarray(directions, dtype=np.float64)
        if o.shape != d.shape or o.ndim not in (2, 3) or o.shape[-1] != 3 or (o.ndim == 3 and o.shape[0] != self.B):
            raise ValueError("origins and directions must both have shape (R, 3) or (B, R, 3)")
        rays = np.empty(o.shape[:-1], dtype=_lib.RAY_DTYPE)
        rays["origin"], rays["dir"] = o, d
        return rays, o.shape[-2], int(o.ndim == 3)

    def ray_cast(self, origins, directions, cap=16):
        """Every hit of R rays with every resident humerus, ascending by (t, face) -> (hits, counts): a structured array (B, R, cap)
        of _lib.RAY_HIT_DTYPE and the exact counts (B, R) int32, whatever cap is; slots behind a ray's count are zero with face = -1.
        origins / directions: (R, 3), shared by all humeri, or (B, R, 3), in CT; a direction need not be a unit vector (t counts in
        units of its length).  cap=None: room for 16 hits, and the call is made again with the largest count when that is more.
        With query_accel "bvh" the rays descend the face hierarchy: the same bytes."""
        rays, R, per = self._rays_arg(origins, directions)
        grow, cap = cap is None, 16 if cap is None else int(cap)
        while True:
            ok = 1 <= R <= _lib.RAY_MAX and 1 <= cap <= _lib.RAY_MAX_HITS      # (the library reports the rest; nothing is sized by it here)
            hits = np.zeros((self.B, R, cap) if ok else (0,), dtype=_lib.RAY_HIT_DTYPE)
            counts = np.zeros((self.B, R) if ok else (0,), dtype=np.int32)
            self._chk(self.L.sh_ray_cast(self.h, _ptr(rays), R, per, cap, _ptr(hits), _ptr(counts)))
            most = int(counts.max()) if counts.size else 0
            if grow and most > cap and cap < _lib.RAY_MAX_HITS:
                cap = min(most, _lib.RAY_MAX_HITS)
                continue
            return hits, counts

    def anp_axis_hits(self, cap=16):
        """Every hit of the four anatomic-neck rays (0 = +normal, 1 = -normal, 2 = +central, 3 = -central) of every humerus of the last
        run with STAGE_ANP -> (hits (B, 4, cap) of _lib.RAY_HIT_DTYPE, counts (B, 4) int32, status (B,) int32).  t is the box-frame
        parameter, the points are in CT; the first hit of a ray is the record's anp_axis_normal / anp_axis_central row, bit for bit.
        A humerus whose record failed has its status and zero counts."""
        cap = int(cap)
        ok = 1 <= cap <= _lib.RAY_MAX_HITS
        hits = np.zeros((self.B, 4, cap) if ok else (0,), dtype=_lib.RAY_HIT_DTYPE)
        counts = np.zeros((self.B, 4), dtype=np.int32)
        status = np.zeros(max(self.B, 1), dtype=np.int32)
        self._chk(self.L.sh_anp_axis_hits(self.h, cap, _ptr(hits), _ptr(counts), _ptr(status)))
        return hits, counts, status[: self.B]

    def ray_nearest(self, origins, directions):
        """The nearest hit of R rays with every resident humerus (`ray.intersects_first`) -> (B, R) of _lib.RAY_HIT_DTYPE: the least
        hit under (t, face), the bytes of ray_cast(...)[0][:, :, 0]; a ray that hits nothing has zeros and face = -1.  origins /
        directions as ray_cast's.  With query_accel "bvh" it is one launch through the face hierarchy, pruned by t; "off": the chain of
        ray_cast with cap = 1.  Resident afterwards: "ray.near"."""
        rays, R, per = self._rays_arg(origins, directions)
        ok = 1 <= R <= _lib.RAY_MAX      # (the library reports the rest; nothing is sized by it here)
        hit = np.zeros((self.B, R) if ok else (0,), dtype=_lib.RAY_HIT_DTYPE)
        self._chk(self.L.sh_ray_nearest(self.h, _ptr(rays), R, per, _ptr(hit)))
        return hit

    def thickness(self, points, normals, offset=1e-3):
        """`trimesh.proximity.thickness(mesh, points, method="ray")` for every resident humerus: how much bone lies under a surface
        point along the inward normal -> (B, N) of THICKNESS_DTYPE: thickness (mm; +inf where the ray leaves the mesh without a hit),
        point (CT) and face (humerus-local; -1 without a hit) of the opposite wall.  points / normals: (N, 3), shared by all humeri, or
        (B, N, 3), in CT; a normal is the OUTWARD direction at its point and is normalised here in float64 (a zero or non-finite one
        raises ValueError).  One ray per point from p - offset n along -n through ray_nearest; thickness = offset + t.  offset (mm) is
        part of the definition: it moves the origin off the point's own face, so that the answer does not hang on the rule's t > 1e-9
        at a rounded surface point."""
        p = self._points_arg(points)
        n = np.ascontiguousarray(normals, dtype=np.float64)
        if n.shape != p.shape:
            raise ValueError("points and normals must have the same shape, (N, 3) or (B, N, 3)")
        with np.errstate(all="ignore"):
            nn = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
            unit = n / nn[..., None]
        if not (np.isfinite(unit).all() and (nn > 0.0).all()):
            raise ValueError("a normal is zero or not finite")
        offset = float(offset)
        hit = self.ray_nearest(p - offset * unit, -unit)
        out = np.zeros(hit.shape, dtype=THICKNESS_DTYPE)
        miss = hit["face"] < 0
        out["thickness"] = np.where(miss, np.inf, offset + hit["t"])
        out["point"], out["face"] = hit["point"], hit["face"]
        return out

    # ---- closest surface points of the resident batch (include/shoulder_hip.h sh_closest_points) -------------------------------
    def _points_arg(self, points):
        """the query points of a call as the C side reads them: (Q, 3), shared by all humeri, or (B, Q, 3)"""
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim not in (2, 3) or p.shape[-1] != 3 or (p.ndim == 3 and p.shape[0] != self.B):
            raise ValueError("points must have shape (Q, 3) or (B, Q, 3)")
        return p

    def closest_points(self, points):
        """The closest point of every resident humerus to every query point -> a structured array (B, Q) of _lib.CLOSEST_DTYPE: dist,
        point (CT), face (humerus-local), region (0 interior, 1 / 2 / 3 edge AB / BC / CA, 4 / 5 / 6 vertex A / B / C of that face), side
        (+1 on the side the winning face's normal points to) and status.  points: (Q, 3), shared by all humeri, or (B, Q, 3), in CT.
        Among faces at the same distance the smallest face id wins.  A call costs what a multiple of 256 points costs."""
        p = self._points_arg(points)
        Q, per = p.shape[-2], int(p.ndim == 3)
        ok = 1 <= Q <= _lib.CLOSEST_MAX      # (the library reports the rest; nothing is sized by it here)
        out = np.zeros((self.B, Q) if ok else (0,), dtype=_lib.CLOSEST_DTYPE)
        self._chk(self.L.sh_closest_points(self.h, _ptr(p), Q, per, _ptr(out)))
        return out

    # ---- the face hierarchy of the resident batch (include/shoulder_hip.h sh_mesh_bvh, sh_set_query_accel) ------------------------
    def build_bvh(self):
        """Build the bounding-box hierarchy over the faces of every resident mesh -> (B,) of _lib.BVH_INFO_DTYPE: tight (the faces in
        the tree), loose (slivers, collinear and point triangles: every query tests them), leaves, levels, nodes and the box lo, hi of
        the tight faces.  Resident afterwards: "bvh.*" (bvh()); a new batch removes them.  Needs no run."""
        info = np.zeros(max(self.B, 0), dtype=_lib.BVH_INFO_DTYPE)
        self._chk(self.L.sh_mesh_bvh(self.h, _ptr(info)))
        return info

    def bvh(self):
        """The resident hierarchy after build_bvh() (or a query in "bvh" mode) -> a list with one dict per mesh: `order` (the tight
        faces ascending by (code, id)), `loose` (ascending), `off` (the mesh's 32 int32 of "bvh.off"), `box` ((nodes, 6) float32: lo,
        hi; level k is box[off[8 + k]:off[8 + k + 1]]) and `tri` ((tight, 9) float32: the corners in the order)."""
        F = int(self.foff[-1])
        order, loose = self.fetch("bvh.order", np.int32, (F,)), self.fetch("bvh.loose", np.int32, (F,))
        off = self.fetch("bvh.off", np.int32, (self.B, 32))
        box, tri = self.fetch("bvh.box", np.float32).reshape(-1, 6), self.fetch("bvh.tri", np.float32, (F, 9))
        out = []
        for b in range(self.B):
            f0 = int(self.foff[b])
            t, nl, nodes, base = (int(off[b, i]) for i in (0, 1, 4, 5))
            out.append(dict(order=order[f0:f0 + t].copy(), loose=loose[f0:f0 + nl].copy(), off=off[b].copy(), box=box[base:base + nodes].copy(),
                            tri=tri[f0:f0 + t].copy()))
        return out

    @property
    def query_accel(self):
        """"off" (the default): the closest-point step of closest_points, register and register_multistart and the rays of ray_cast,
        ray_nearest and thickness walk all faces; "bvh": they descend the face hierarchy, which is built when it is not resident.  The
        results are the same bytes either way.  (anp_axis_hits always walks all faces.)  For points the hierarchy is five to seven times
        faster; for rays it was measured slower than the walk over all faces."""
        return "bvh" if self.L.sh_get_query_accel(self.h) == _lib.ACCEL_BVH else "off"

    @query_accel.setter
    def query_accel(self, mode):
        if mode not in ("off", "bvh"):
            raise ValueError('query_accel must be "off" or "bvh"')
        self._chk(self.L.sh_set_query_accel(self.h, _lib.ACCEL_BVH if mode == "bvh" else _lib.ACCEL_OFF))

    # ---- generalized winding numbers of the resident batch (include/shoulder_hip.h sh_winding_numbers) --------------------------
    def winding_numbers(self, points):
        """The generalized winding number of every resident humerus about every query point -> a structured array (B, Q) of
        _lib.WINDING_DTYPE: winding, inside (1 when |winding| >= 0.5) and status.  points: (Q, 3), shared by all humeri, or (B, Q, 3),
        in CT.  A closed mesh with outward normals gives 1 inside and 0 outside (up to rounding), one stored inside-out -1 inside; an
        OPEN mesh gives a fraction (a cube without one of its six sides: 5/6 at its centre); a CAVITY whose wall faces inward gives 0.
        ON THE SURFACE ITSELF the winding number is about 0.5 and `inside` is undefined.  Every face contributes (no approximation);
        a call costs what a multiple of 256 points costs."""
        p = self._points_arg(points)
        Q, per = p.shape[-2], int(p.ndim == 3)
        ok = 1 <= Q <= _lib.WINDING_MAX      # (the library reports the rest; nothing is sized by it here)
        out = np.zeros((self.B, Q) if ok else (0,), dtype=_lib.WINDING_DTYPE)
        self._chk(self.L.sh_winding_numbers(self.h, _ptr(p), Q, per, _ptr(out)))
        return out

    def contains(self, points):
        """`mesh.contains(points)` for every resident humerus -> bool (B, Q): |winding number| >= 0.5 (Engine.winding_numbers).  True
        in the solid of a closed mesh whichever way it is oriented, False outside it and in a cavity whose wall faces inward; for an
        open mesh the threshold cuts a graded answer; undefined for a point on the surface itself.  Raises when a sum was not finite."""
        rec = self.winding_numbers(points)
        if np.any(rec["status"] != 0):
            raise ShoulderHipError(int(rec["status"][rec["status"] != 0][0]), "contains: a winding number is not finite (a point too far away)")
        return rec["inside"] != 0

    def signed_distance(self, points):
        """`trimesh.proximity.signed_distance(mesh, points)` for every resident humerus -> float64 (B, Q): the distance to the surface
        (Engine.closest_points), POSITIVE INSIDE and negative outside (Engine.contains).  Two device calls joined here.  For an open
        mesh the sign is the thresholded fraction, in a cavity whose wall faces inward it is negative, and on the surface itself the
        value is 0 up to rounding with an undefined sign."""
        inside = self.contains(points)
        rec = self.closest_points(points)
        if np.any(rec["status"] != 0):
            raise ShoulderHipError(int(rec["status"][rec["status"] != 0][0]), "signed_distance: no face of a mesh gave a finite distance")
        return np.where(inside, rec["dist"], -rec["dist"])

    # ---- rigid registration of point sets onto the resident batch (include/shoulder_hip.h sh_register_points) -------------------
    def register(self, points, T0=None, metric="plane", max_iter=20, reject=np.inf, tol=0.0, history=False):
        """Rigid ICP of a point set onto every resident humerus, the whole loop on the device -> a structured array (B,) of
        _lib.REGISTRATION_DTYPE: T (4, 4), CT -> CT, moving the points onto the bone; rms and pairs at T; rms_first; min_pivot;
        iterations (updates applied); converged; status.  With history=True also a (B, max_iter + 1, 2) array of (rms, pairs) per
        evaluation made, zeros behind.  points: (Q, 3), shared by all humeri, or (B, Q, 3), in CT -- the convention of closest_points.
        T0: (B, 4, 4) rigid starting transforms (default: identity).  metric "plane" (point-to-plane, converges quadratically near
        the solution; `min_pivot` near 0 tells of a surface that lets the points slide) or "point" (Horn's closed form, converges
        linearly).  reject: pairs farther apart than this many mm are left out; tol: stop once the rms changes by no more than this.
        tol ends a humerus' updates, NOT the call's work: the host enqueues all max_iter + 1 closest-point walks and does not look at the
        flags in between, so a batch that converges early still pays for max_iter (about 10 ms per walk for 64 bones x 4 096 points).
        ICP is local: the start must lie within its basin of convergence.  The pairs of the last evaluation stay in "icp.near"."""
        p = self._points_arg(points)
        opt = _icp_options(metric, max_iter, reject, tol)
        Q, per = p.shape[-2], int(p.ndim == 3)
        t0 = None
        if T0 is not None:
            t0 = np.ascontiguousarray(T0, dtype=np.float64)
            if t0.shape != (self.B, 4, 4):
                raise ValueError("T0 must have shape (B, 4, 4)")
        rows = int(max_iter) + 1 if 1 <= int(max_iter) <= _lib.ICP_MAX_ITER else 0      # (the library reports the rest)
        out = np.zeros(self.B, dtype=_lib.REGISTRATION_DTYPE)
        hist = np.zeros((self.B, rows, 2)) if history else None
        self._chk(self.L.sh_register_points(self.h, _ptr(p), Q, per, _ptr(t0) if t0 is not None else None, ctypes.byref(opt), _ptr(out),
                                            _ptr(hist) if hist is not None else None))
        return (out, hist) if history else out

    # ---- mass properties of the resident batch (include/shoulder_hip.h sh_mass_properties) -------------------------------------
    def mass_properties(self):
        """`mesh.area`, `volume`, `center_mass`, `moment_inertia`, `principal_inertia_components` and `principal_inertia_vectors` of
        every resident humerus in one device pass -> a structured array (B,) of _lib.MASS_DTYPE: area, volume (signed: negative for a
        mesh stored inside-out), closure (0 on a closed mesh, about cap area / area on an open one), shell_centroid / shell_cov /
        shell_eig (descending) / shell_axes (rows, long axis first) of the surface itself, center_mass / inertia (density 1, about the
        centre of mass) / principal (ascending) / principal_axes (rows) of the solid, faces, degenerate (faces of zero area), status
        (shell) and vstatus (volume: set, with zeros, for a mesh that encloses nothing).  Points in CT.  Needs no run."""
        out = np.zeros(max(self.B, 0), dtype=_lib.MASS_DTYPE)
        self._chk(self.L.sh_mass_properties(self.h, _ptr(out)))
        return out

    # ---- surface samples of the resident batch (include/shoulder_hip.h sh_sample_surface) ---------------------------------------
    def sample_surface(self, n, seed=0, radius=None, max_rounds=32):
        """`trimesh.sample.sample_surface` / `sample_surface_even` for every resident humerus in one device pass -> (samples, info):
        a structured array (B, n) of _lib.SAMPLE_DTYPE -- point (CT), u, v (the barycentric weights of corners B and C), face
        (humerus-local), keep -- and (B,) of _lib.SAMPLE_INFO_DTYPE: area, kept, rounds, status.  Every face is drawn in proportion to
        its area.  seed: an int for all humeri or a sequence of B ints; a sample depends on its mesh, its seed and its index alone, so
        the first n samples of a larger call are these.  radius (mm): the greedy thinning of `remove_close` on top -- keep is 1 for a
        sample with no kept sample of lower index nearer than radius, else 0; n at most 65 536 then, and a humerus not decided within
        max_rounds has status SH_ERR_CAPACITY and keep = -1 where undecided.  A mesh without area has status SH_ERR_GEOMETRY and zero
        records.  Needs no run."""
        nb = max(self.B, 1)      # (without a batch the library refuses; it still gets a pointer)
        seeds = np.full(nb, seed, dtype=np.uint64) if np.ndim(seed) == 0 else np.ascontiguousarray(seed, dtype=np.uint64)
        if seeds.shape != (nb,):
            raise ValueError("seed must be an int or a sequence of B ints")
        opt = _lib.SampleOptions(0.0 if radius is None else float(radius), int(max_rounds), 0)
        n = int(n)
        ok = 1 <= n <= _lib.SAMPLE_MAX      # (the library reports the rest; nothing is sized by it here)
        out = np.zeros((self.B, n) if ok else (0,), dtype=_lib.SAMPLE_DTYPE)
        info = np.zeros(max(self.B, 0), dtype=_lib.SAMPLE_INFO_DTYPE)
        self._chk(self.L.sh_sample_surface(self.h, n, _ptr(seeds), ctypes.byref(opt), _ptr(out), _ptr(info)))
        return out, info

    # ---- mesh topology of the resident batch (include/shoulder_hip.h sh_mesh_topology) -------------------------------------------
    def topology(self, max_shells=64, max_rounds=32):
        """How the triangles of every resident mesh hang together, in one device pass -> (info, shells): (B,) of _lib.TOPOLOGY_DTYPE --
        status, rounds, faces_degenerate, vertices_used, edges, border_edges, nonmanifold_edges, inconsistent_edges, euler,
        max_valence, n_shells (exact whatever max_shells), shells_written, largest_shell, largest_faces, flags (bit 0 watertight,
        bit 1 winding-consistent) -- and (B, max_shells) of _lib.SHELL_DTYPE, the first max_shells shells of each mesh (the records
        behind shells_written are zero).  A shell is a connected component over manifold edges, as `mesh.split(only_watertight=False)`
        has them.  A mesh whose labelling did not finish within max_rounds has status SH_ERR_CAPACITY, n_shells 0 and labels -1; its
        adjacency and counts stay valid.  Resident afterwards: "topo.vrow", "topo.vface", "topo.adj", "topo.label" (face_adjacency,
        face_labels).  Needs no run."""
        opt = _lib.TopologyOptions(int(max_shells), int(max_rounds), 0)
        ok = 1 <= int(max_shells) <= _lib.TOPO_MAX_SHELLS      # (the library reports the rest; nothing is sized by it here)
        info = np.zeros(max(self.B, 0), dtype=_lib.TOPOLOGY_DTYPE)
        shells = np.zeros((self.B, int(max_shells)) if ok else (0,), dtype=_lib.SHELL_DTYPE)
        self._chk(self.L.sh_mesh_topology(self.h, ctypes.byref(opt), _ptr(info), _ptr(shells)))
        return info, shells

    def _face_range(self, b):
        if not 0 <= int(b) < self.B:
            raise ValueError("mesh index out of range")
        return int(self.foff[int(b)]), int(self.foff[int(b) + 1])

    def face_adjacency(self, b):
        """The resident adjacency of mesh b after topology() -> (F, 3) int32: per slot e the other face on the edge {f[e], f[(e+1)%3]},
        or _lib.ADJ_BORDER / ADJ_NONMANIFOLD / ADJ_DEGENERATE."""
        f0, f1 = self._face_range(b)
        return self.fetch("topo.adj", np.int32, (int(self.foff[-1]), 3))[f0:f1].copy()

    def face_labels(self, b):
        """The resident shell index of every face of mesh b after topology() -> (F,) int32, -1 for a degenerate face."""
        f0, f1 = self._face_range(b)
        return self.fetch("topo.label", np.int32, (int(self.foff[-1]),))[f0:f1].copy()

    def split(self, b, largest_only=False):
        """`mesh.split(only_watertight=False)` of resident mesh b from the resident labels (topology() first) -> a list of (verts, faces),
        one per shell in shell order, or the largest shell alone: vertices compacted in first-use order, faces in their order, each
        ready for upload().  The gather runs on the host."""
        label = self.face_labels(b)
        v0, v1 = int(self.voff[int(b)]), int(self.voff[int(b) + 1])
        f0, f1 = self._face_range(b)
        verts = self.fetch("verts", np.float32, (int(self.voff[-1]), 3))[v0:v1]
        faces = self.fetch("faces", np.int32, (int(self.foff[-1]), 3))[f0:f1]
        n = int(label.max()) + 1 if len(label) else 0
        ks = list(range(n))
        if largest_only and n:
            ks = [int(np.argmax(np.bincount(label[label >= 0], minlength=n)))]      # (argmax: ties to the smaller index)
        out = []
        for k in ks:
            fk = faces[label == k]
            uniq, first, inv = np.unique(fk.ravel(), return_index=True, return_inverse=True)
            order = np.argsort(first, kind="stable")
            rank = np.empty_like(order)
            rank[order] = np.arange(len(order))
            out.append((np.ascontiguousarray(verts[uniq[order]]), np.ascontiguousarray(rank[np.ravel(inv)].reshape(-1, 3).astype(np.int32))))
        return out

    # ---- vertex normals and discrete curvatures of the resident batch (include/shoulder_hip.h sh_vertex_fields) -------------------
    def _has_buffer(self, name):
        n, e = ctypes.c_size_t(), ctypes.c_int()
        return self.L.sh_buffer_info(self.h, name.encode(), ctypes.byref(n), ctypes.byref(e)) == 0

    def vertex_fields(self, weight="area", smooth=0):
        """Per vertex of every resident mesh, in one device pass over the incidence of topology() (run first when it is not resident
        for this batch) -> dict: normals (sumV, 3) unit, weighted by the faces' areas or by the corners' angles (weight "area" /
        "angle": trimesh's default), zeros where undefined; area (a third of the incident faces'), angle_sum, defect (2 pi, or pi on a
        border, minus angle_sum: trimesh's vertex_defects), gauss = defect / area, mean (cotangent Laplacian along the normal: +1/R on
        a sphere with outward normals), gauss_smooth and mean_smooth after `smooth` (0..64) Jacobi rounds of area-weighted averaging
        (the raw fields without a round), flags (int32: _lib.VERT_USED, VERT_BORDER, VERT_NONMANIFOLD, VERT_FLAT), status (B,): 0 or
        SH_ERR_GEOMETRY for a mesh without a face of non-zero area, and voff (B + 1,), the vertex offsets of the meshes in all of these.
        Resident afterwards: "vert.face" (face_normals), "vert.normal", "vert.fields", "vert.flags", "vert.status"."""
        weights = {"area": _lib.VERT_WEIGHT_AREA, "angle": _lib.VERT_WEIGHT_ANGLE}
        w = weights.get(weight, weight)
        if not isinstance(w, (int, np.integer)):
            raise ValueError("weight must be 'area' or 'angle'")
        if self.B >= 1 and not self._has_buffer("topo.vrow"):
            self.topology()
        V = int(self.voff[-1]) if self.B >= 1 else 0
        normals, fields = np.zeros((V, 3)), np.zeros((V, _lib.VERT_FIELDS))
        flags, status = np.zeros(V, np.int32), np.zeros(max(self.B, 0), np.int32)
        self._chk(self.L.sh_vertex_fields(self.h, int(w), int(smooth), _ptr(normals), _ptr(fields), _ptr(flags), _ptr(status)))
        out = dict(normals=normals, flags=flags, status=status, voff=np.array(self.voff, dtype=np.int64))
        for i, n in enumerate(("area", "angle_sum", "defect", "gauss", "mean", "gauss_smooth", "mean_smooth")):
            out[n] = np.ascontiguousarray(fields[:, i])
        return out

    def face_normals(self, b):
        """The resident face records of mesh b after vertex_fields() -> (unit normals (F, 3), areas (F,), angles (F, 3)): trimesh's
        face_normals, area_faces and face_angles; zeros for a face of no area."""
        f0, f1 = self._face_range(b)
        rec = self.fetch("vert.face", np.float64, (int(self.foff[-1]), 10))[f0:f1]
        a2 = rec[:, 3]
        with np.errstate(all="ignore"):
            unit = np.where(a2[:, None] != 0.0, rec[:, :3] / a2[:, None], 0.0)
        return unit, a2 / 2.0, rec[:, 4:7].copy()

    # ---- smoothing of the vertices of the resident batch (include/shoulder_hip.h sh_smooth_vertices) ------------------------------
    _SMOOTH_FILTERS = {"laplacian": _lib.SMOOTH_LAPLACIAN, "taubin": _lib.SMOOTH_TAUBIN, "hc": _lib.SMOOTH_HC, "humphrey": _lib.SMOOTH_HC}
    _SMOOTH_WEIGHTS = {"uniform": _lib.SMOOTH_UNIFORM, "invlen": _lib.SMOOTH_INVLEN}

    def smooth_vertices(self, filter="taubin", iterations=10, lamb=0.5, mu=-0.53, alpha=0.1, beta=0.5, weight="uniform", pin=None, pin_border=False,
                        keep_volume=False):
        """The vertices of every resident mesh smoothed over their one-rings, on the device (the incidence of topology() is made first
        when it is not resident for this batch): trimesh.smoothing's filter_laplacian ("laplacian": `iterations` steps of lamb towards
        the neighbours' mean), filter_taubin ("taubin": a step of lamb, then one of mu <= 0, which keeps the volume nearly) and
        filter_humphrey ("hc": alpha pulls back to the start, beta spreads the correction).  weight "uniform" or "invlen" (one over the
        edge's length in the start); pin: an optional (sumV,) mask of vertices that stay; pin_border: the vertices on an open or
        non-manifold edge stay; keep_volume: one scaling about the centre of mass at the end restores each mesh's volume (not together
        with a pin).  -> dict: vertices (sumV, 3) float64, info (B,) of _lib.SMOOTH_INFO_DTYPE (volume_before, volume_after, scale,
        max_disp, sum_sq_disp, pinned, isolated, status: SH_ERR_GEOMETRY for a mesh whose volume could not be restored, which is
        then not scaled) and voff (B + 1,).  The same bytes wherever the rule runs.  "verts" is not written: upload the result, or
        store("verts", vertices.astype(np.float32)) for the resident faces.  Resident afterwards: "smooth.pos", "smooth.nrow",
        "smooth.nbr" (vertex_neighbors), "smooth.w", "smooth.info"."""
        f = self._SMOOTH_FILTERS.get(filter, filter)
        w = self._SMOOTH_WEIGHTS.get(weight, weight)
        if not isinstance(f, (int, np.integer)):
            raise ValueError("filter must be 'laplacian', 'taubin' or 'hc'")
        if not isinstance(w, (int, np.integer)):
            raise ValueError("weight must be 'uniform' or 'invlen'")
        if self.B >= 1 and not self._has_buffer("topo.vrow"):
            self.topology()
        V = int(self.voff[-1]) if self.B >= 1 else 0
        mask = None
        if pin is not None:
            mask = np.ascontiguousarray(np.asarray(pin).reshape(-1) != 0, dtype=np.uint8)
            if len(mask) != V:
                raise ValueError("pin must have one entry per vertex of the batch")
        p0, p1 = (alpha, beta) if f == _lib.SMOOTH_HC else (lamb, mu)
        flags = (_lib.SMOOTH_PIN_BORDER if pin_border else 0) | (_lib.SMOOTH_KEEP_VOLUME if keep_volume else 0)
        vertices, info = np.zeros((V, 3)), np.zeros(max(self.B, 0), dtype=_lib.SMOOTH_INFO_DTYPE)
        self._chk(self.L.sh_smooth_vertices(self.h, int(f), int(w), int(iterations), flags, float(p0), float(p1), None if mask is None else _ptr(mask), _ptr(vertices),
                                            _ptr(info)))
        return dict(vertices=vertices, info=info, voff=np.array(self.voff, dtype=np.int64))

    def vertex_neighbors(self, b=None):
        """trimesh's `vertex_neighbors` of resident mesh b from the resident rows (made by a smooth_vertices call without an iteration
        when they are missing) -> (nrow (V + 1,), nbr): the neighbours of vertex v are nbr[nrow[v]:nrow[v + 1]], distinct and ascending.
        b=None: a list of these pairs for all meshes, from ONE copy of the two buffers (each call copies the whole batch's rows)."""
        if b is not None and not 0 <= int(b) < self.B:
            raise ValueError("mesh index out of range")
        if not self._has_buffer("smooth.nrow"):
            self.smooth_vertices(iterations=0)
        rows = self.fetch("smooth.nrow", np.int32, (int(self.voff[-1]) + self.B,))
        places = self.fetch("smooth.nbr", np.int32, (6 * max(int(self.foff[-1]), 1),))

        def one(k):
            v0, v1, f0 = int(self.voff[k]), int(self.voff[k + 1]), int(self.foff[k])
            nrow = rows[v0 + k:v1 + k + 1].copy()
            return nrow, places[6 * f0:6 * f0 + int(nrow[-1])].copy()
        return [one(k) for k in range(self.B)] if b is None else one(int(b))

    # ---- repair of the resident batch (include/shoulder_hip.h sh_mesh_repair) -----------------------------------------------------
    _REPAIR_ORIENTS = {"none": _lib.REPAIR_NONE, "winding": _lib.REPAIR_WINDING, "outward": _lib.REPAIR_OUTWARD, "nested": _lib.REPAIR_NESTED}
    _REPAIR_FILLS = {"none": _lib.REPAIR_FILL_NONE, "fan": _lib.REPAIR_FAN, "centroid": _lib.REPAIR_CENTROID}

    def repair(self, orient="outward", fill="centroid", max_hole_edges=4096, max_shells=64, max_holes=64, max_rounds=_lib.REPAIR_MAX_ROUNDS):
        """Every resident mesh with one winding per shell, its shells outward and its holes filled, on the device: trimesh.repair's
        fix_winding ("winding"), fix_inversion ("outward"; "nested": by nesting depth, so that the wall of a cavity stays inward) and
        fill_holes for loops of any length up to max_hole_edges ("fan": faces about the loop's first vertex, "centroid": one new
        vertex per hole, "none": the holes are reported).  The topology() of this batch is made first, with max_shells, when it is not
        resident.  -> dict: info (B,) of _lib.REPAIR_INFO_DTYPE, shells (B, shell records) of _lib.REPAIR_SHELL_DTYPE, holes
        (B, max_holes) of _lib.REPAIR_HOLE_DTYPE, flip (sumF,) uint8, the final flip of every face, and meshes: a list of (verts
        float32, faces int32), one per resident mesh, each ready for upload().  A mesh with a status (SH_ERR_CAPACITY: its labelling
        did not finish, it has more than REPAIR_LDS_FACES faces or its face graph is deeper than max_rounds) comes back unchanged.
        "verts" and "faces" are not written.  The same bytes wherever the rule runs."""
        o, f = self._REPAIR_ORIENTS.get(orient, orient), self._REPAIR_FILLS.get(fill, fill)
        if not isinstance(o, (int, np.integer)):
            raise ValueError("orient must be 'none', 'winding', 'outward' or 'nested'")
        if not isinstance(f, (int, np.integer)):
            raise ValueError("fill must be 'none', 'fan' or 'centroid'")
        if self.B >= 1 and not self._has_buffer("topo.adj"):
            self.topology(max_shells=max_shells)
        B = max(self.B, 0)
        opt = np.array([int(o), int(f), int(max_hole_edges), int(max_holes), int(max_rounds), 0], dtype=np.int32)
        ok = 1 <= int(max_holes) <= _lib.REPAIR_MAX_HOLES      # (the library reports the rest; nothing else is sized by the options here)
        info = np.zeros(B, dtype=_lib.REPAIR_INFO_DTYPE)
        holes = np.zeros((B, int(max_holes)) if ok else (0,), dtype=_lib.REPAIR_HOLE_DTYPE)
        flip = np.zeros(int(self.foff[-1]) if B else 0, dtype=np.uint8)
        self._chk(self.L.sh_mesh_repair(self.h, _ptr(opt), _ptr(info), None, _ptr(holes), _ptr(flip)))
        S = int(info[0]["shell_records"])
        shells = self.fetch("repair.shells", _lib.REPAIR_SHELL_DTYPE)[:B * S].reshape(B, S).copy()
        off = self.fetch("repair.off", np.int64)[:3 * (B + 1)].reshape(3, B + 1)
        faces, verts = self.fetch("repair.faces", np.int32), self.fetch("repair.verts", np.float32)
        meshes = []
        for b in range(B):
            f0, v0 = int(off[0, b]), int(off[1, b])
            meshes.append((verts[3 * v0:3 * (v0 + int(info[b]["verts_out"]))].reshape(-1, 3).copy(), faces[3 * f0:3 * (f0 + int(info[b]["faces_out"]))].reshape(-1, 3).copy()))
        return dict(info=info, shells=shells, holes=holes, flip=flip, meshes=meshes)

    # ---- simplification of the resident batch (include/shoulder_hip.h sh_mesh_simplify) -------------------------------------------
    _SIMPLIFY_PLACES = {"mean": _lib.SIMPLIFY_MEAN, "quadric": _lib.SIMPLIFY_QUADRIC}

    def simplify(self, cell, place="quadric", reg=1e-3, clamp=1.0):
        """Every resident mesh made smaller by vertex clustering, on the device: the used vertices in one cell of a grid of `cell` mm
        (a scalar, or (B,): one per mesh) become one vertex -- at their mean ("mean") or where the quadric of their faces is smallest,
        clamped to the cell and regularised towards the mean by reg ("quadric") -- collapsed and duplicate faces are dropped and the
        rest renumbered.  What trimesh's simplify_vertex_clustering / simplify_quadric_decimation are reached for: the mesh at the
        density the question needs.  The topology() of this batch is made first when it is not resident.  -> (meshes, info, map):
        meshes a list of (verts float32, faces int32), one per resident mesh, each ready for upload(); info (B,) of
        _lib.SIMPLIFY_INFO_DTYPE; map (sumV,) int32, the output vertex of every input vertex at voff[b], or -1.  A mesh with a status
        (SH_ERR_CAPACITY: more than SIMPLIFY_MAX_CELLS cells on an axis or SIMPLIFY_MAX_CLUSTERS clusters; SH_ERR_GEOMETRY: every face
        collapsed) comes back empty.  Clustering does not preserve topology: topology() of the re-upload says what it left.  "verts"
        and "faces" are not written.  The same bytes wherever the rule runs."""
        p = self._SIMPLIFY_PLACES.get(place, place)
        if not isinstance(p, (int, np.integer)):
            raise ValueError("place must be 'mean' or 'quadric'")
        B = max(self.B, 0)
        cells = np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float64), (B,)) if np.ndim(cell) == 0 else np.asarray(cell, dtype=np.float64))
        if cells.shape != (B,):
            raise ValueError("cell must be a scalar or one value per resident mesh")
        if B >= 1 and not self._has_buffer("topo.vrow"):
            self.topology()
        opt = np.zeros(1, dtype=_lib.SIMPLIFY_OPTIONS_DTYPE)
        opt["place"], opt["reg"], opt["clamp"] = int(p), float(reg), float(clamp)
        nv, nf = (int(self.voff[-1]), int(self.foff[-1])) if B else (0, 0)
        info = np.zeros(B, dtype=_lib.SIMPLIFY_INFO_DTYPE)
        verts, faces, vmap = np.zeros((nv, 3), np.float32), np.zeros((nf, 3), np.int32), np.zeros(nv, np.int32)
        # (without a batch there is no cell to read: the library gets a placeholder and reports the state)
        self._chk(self.L.sh_mesh_simplify(self.h, _ptr(opt), _ptr(cells if B else np.ones(1)), _ptr(info), _ptr(verts), _ptr(faces), _ptr(vmap)))
        meshes = []
        for b in range(B):
            v0, f0 = int(self.voff[b]), int(self.foff[b])
            meshes.append((verts[v0:v0 + int(info[b]["verts_out"])].copy(), faces[f0:f0 + int(info[b]["faces_out"])].copy()))
        return meshes, info, vmap

    def simplify_to(self, target_faces, place="quadric", reg=1e-3, clamp=1.0, steps=16):
        """simplify() at, per mesh, the smallest cell tried whose result has at most target_faces faces (a scalar or (B,)): `steps`
        rounds of bisection on the cell per mesh, all meshes in every call, from [box diagonal / 2^20 raised to the cell limit, box
        diagonal].  -> (meshes, info, map) as simplify(): per mesh exactly the bytes simplify gives for info[b]["cell"].  At the box
        diagonal a mesh is one cluster and comes back empty (SH_ERR_GEOMETRY): that is the answer when no cell tried fits."""
        B = max(self.B, 0)
        target = np.broadcast_to(np.asarray(target_faces, dtype=np.int64), (B,))
        verts = self.fetch("verts", np.float32)
        lo, hi = np.ones(B), np.ones(B)
        for b in range(B):
            v = verts[3 * int(self.voff[b]):3 * int(self.voff[b + 1])].reshape(-1, 3).astype(np.float64)
            ext = v.max(axis=0) - v.min(axis=0)
            diag = float(np.sqrt((ext * ext).sum()))
            if diag > 0.0:
                hi[b], lo[b] = diag, max(diag / 2.0 ** 20, float(ext.max()) / (_lib.SIMPLIFY_MAX_CELLS - 2))
        meshes, info, vmap = self.simplify(hi, place, reg, clamp)      # (one cluster per mesh: it fits every target)
        vmap = vmap.copy()
        done = np.zeros(B, dtype=bool)

        def trial(cells):
            """-> per mesh: does the result at this cell fit?  A result that fits at a smaller cell than the best so far is taken."""
            r = self.simplify(cells, place, reg, clamp)
            fits = (r[1]["status"] != -4) & (r[1]["faces_out"] <= target)      # (SH_ERR_CAPACITY: no result)
            for b in np.nonzero(fits & (cells < info["cell"]))[0]:
                meshes[b], info[b] = r[0][b], r[1][b]
                vmap[int(self.voff[b]):int(self.voff[b + 1])] = r[2][int(self.voff[b]):int(self.voff[b + 1])]
            return fits
        done = trial(lo)
        hi[done] = lo[done]
        for _ in range(int(steps)):
            if done.all():
                break
            mid = np.where(done, hi, 0.5 * (lo + hi))
            fits = trial(mid)
            hi = np.where(fits, mid, hi)
            lo = np.where(fits | done, lo, mid)
        return meshes, info, vmap

    # ---- geodesic distances and shortest paths on the resident batch (include/shoulder_hip.h sh_geodesic) ------------------------
    _GEO_MODES = {"edges": _lib.GEO_EDGES, "unfold": _lib.GEO_UNFOLD}

    def geodesic(self, sources, d0=None, mode="unfold", max_dist=None, _lds_vertices=None):
        """Distances ALONG the surface of every resident mesh from K sets of source vertices per mesh, on the device (the incidence of
        topology() is made first when it is not resident for this batch).  sources[b][k] is an index array (vertices of mesh b; an
        empty one reaches nothing); a flat list of B arrays means K = 1.  d0, shaped like sources, gives every source a start offset
        >= 0 (None: zeros).  mode "edges" walks the mesh edges (trimesh's vertex_adjacency_graph), "unfold" also the diagonals of two
        neighbouring faces unfolded into a plane; max_dist cuts off: what lies farther is +inf and unreached.  -> dict: dist (K sumV,)
        float64, pred and source (K sumV,) int32 -- per mesh b K planes of V_b values at K voff[b] + k V_b (geodesic_field cuts one
        out); pred is the vertex before v on a shortest path, _lib.GEO_ROOT at a source that starts one, GEO_NO_PRED behind an arc of
        length 0, GEO_UNREACHED; source is the position in the set's list of the source v's path starts from, or -1 --, info (B, K) of
        _lib.GEO_INFO_DTYPE (far_dist, reached, roots, no_pred, farthest, sweeps, status), voff (B + 1,) and K.  The result is the
        fixed point of the relaxation: the same bytes whatever path the library takes.  Resident afterwards: "geo.face", "geo.dist",
        "geo.pred", "geo.source", "geo.info"."""
        m = self._GEO_MODES.get(mode, mode)
        if not isinstance(m, (int, np.integer)):
            raise ValueError("mode must be 'edges' or 'unfold'")
        B = max(self.B, 0)
        sets = list(sources)
        if len(sets) != B:
            raise ValueError("sources needs one entry per resident mesh")
        flat = B > 0 and all(_is_index_array(s) for s in sets)
        if flat:
            sets = [[s] for s in sets]
            d0 = None if d0 is None else [[z] for z in d0]
        K = len(sets[0]) if B else 1
        if any(len(s) != K for s in sets):
            raise ValueError("every mesh needs the same number of sets")
        src = [np.asarray(s, dtype=np.int64).reshape(-1) for per in sets for s in per]
        if any(len(s) and (s.min() < -2**31 or s.max() >= 2**31) for s in src):
            raise ValueError("a source index does not fit int32")
        off = np.zeros(B * K + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in src])
        idx = np.ascontiguousarray(np.concatenate(src + [np.zeros(0, np.int64)]), np.int32)
        z = None
        if d0 is not None:
            per = [[None] * K if row is None else list(row) for row in d0]
            if len(per) != B or any(len(row) != K for row in per):
                raise ValueError("d0 must be shaped like sources")
            zs = [np.zeros(len(src[b * K + k])) if per[b][k] is None else np.asarray(per[b][k], np.float64).reshape(-1) for b in range(B) for k in range(K)]
            if [len(x) for x in zs] != [len(s) for s in src]:
                raise ValueError("d0 must be shaped like sources")
            z = np.ascontiguousarray(np.concatenate(zs + [np.zeros(0)]), np.float64)
        if B >= 1 and not self._has_buffer("topo.vrow"):
            self.topology()
        V = int(self.voff[-1]) if B >= 1 else 0
        ok = 1 <= K <= _lib.GEO_MAX_SETS      # (the library reports the rest; nothing is sized by it here)
        n = K * V if ok else 0
        dist, pred, source = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        info = np.zeros((B, K) if ok else (0,), dtype=_lib.GEO_INFO_DTYPE)
        limit = np.inf if max_dist is None else float(max_dist)
        args = (int(m), int(K), limit, _ptr(off), _ptr(idx), _ptr(z) if z is not None else None, _ptr(dist), _ptr(pred), _ptr(source), _ptr(info))
        if _lds_vertices is None:
            self._chk(self.L.sh_geodesic(self.h, *args))
        else:      # the lab entry point: the threshold between the LDS path and the general path lowered (tools/time_geodesic.py, the tests)
            fn = self.L.sh_lab_geodesic
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int] + _lib.SIGNATURES["sh_geodesic"][0][1:], ctypes.c_int
            self._chk(fn(self.h, int(_lds_vertices), *args))
        return dict(dist=dist, pred=pred, source=source, info=info, voff=np.array(self.voff, dtype=np.int64), K=K)

    def geodesic_field(self, out, b, k=0):
        """The (V_b,) views of dist, pred and source of set k of mesh b in what geodesic() returned."""
        K, voff = int(out["K"]), out["voff"]
        if not 0 <= int(b) < len(voff) - 1 or not 0 <= int(k) < K:
            raise ValueError("mesh or set index out of range")
        nv = int(voff[b + 1] - voff[b])
        at = K * int(voff[b]) + int(k) * nv
        return out["dist"][at:at + nv], out["pred"][at:at + nv], out["source"][at:at + nv]

    def geodesic_path(self, b, start, end, mode="unfold"):
        """The shortest path on mesh b from vertex `start` to vertex `end` along the graph of geodesic() -> (polyline (n, 3) float64 in
        CT from start to end, its length = the distance).  The distances come from the device; the walk back along pred runs here.  A
        hop over an unfolded diagonal contributes the point where the unfolded line crosses the edge the two faces share, so the
        polyline stays on the surface.  Raises ValueError when `end` is not reached or lies behind an arc of length 0 (GEO_NO_PRED)."""
        f0, f1 = self._face_range(b)
        v0, v1 = int(self.voff[b]), int(self.voff[b + 1])
        out = self.geodesic([[[int(start)]] if i == int(b) else [[]] for i in range(self.B)], mode=mode)
        d, pred, _ = self.geodesic_field(out, b, 0)
        verts = self.fetch("verts", np.float32, (int(self.voff[-1]), 3))[v0:v1].astype(np.float64)
        faces = self.fetch("faces", np.int32, (int(self.foff[-1]), 3))[f0:f1]
        rec = self.fetch("geo.face", np.float64, (int(self.foff[-1]), 6))[f0:f1]
        opp = self.fetch("geo.opp", np.int32, (int(self.foff[-1]), 3))[f0:f1]
        return geodesic_polyline(verts, faces, rec, opp, d, pred, int(end))

    # ---- multi-start registration (include/shoulder_hip.h sh_register_multistart) -----------------------------------------------
    def principal_starts(self, points, rolls=8, with_ratios=False):
        """Starting transforms for register_multistart from principal frames -> (B, 2 * rolls, 4, 4).  The mesh frame is shell_centroid
        and shell_axes of mass_properties (device); the point frame is the mean and the covariance eigenvectors of the points,
        descending, the third set to the cross product.  Start k = phi * rolls + r is R = Xm Rx(2 pi r / rolls) F_phi Xp^T,
        t = cm - R cp, with F_0 the identity and F_1 = diag(-1, 1, -1), which reverses the long axis and stays proper: both directions
        of the long axis times a sweep of rolls about it, because a humerus' long axis is sharp and its transverse axes are not.
        Ordinary NumPy.  with_ratios=True also returns the ratio of the two largest shell eigenvalues of every mesh (B,) and of its
        points (B,): near 1 the shape has no long axis and the starts are arbitrary."""
        p = self._points_arg(points)
        if int(rolls) < 1 or 2 * int(rolls) > _lib.MS_MAX_STARTS:
            raise ValueError("rolls must be in 1..32")
        m = self.mass_properties()
        if np.any(m["status"] != 0):
            raise ShoulderHipError(int(m["status"][m["status"] != 0][0]), "principal_starts: a mesh has no surface frame (no faces, no area)")
        T, rp = np.zeros((self.B, 2 * int(rolls), 4, 4)), np.zeros(self.B)
        for b in range(self.B):
            T[b], rp[b] = principal_start_matrices(m[b]["shell_centroid"], m[b]["shell_axes"], p[b] if p.ndim == 3 else p, int(rolls))
        with np.errstate(divide="ignore", invalid="ignore"):
            rm = m["shell_eig"][:, 0] / m["shell_eig"][:, 1]
        return (T, rm, rp) if with_ratios else T

    def register_multistart(self, points, T0s, coarse=None, coarse_points=0, min_pairs=6, fine=None):
        """sh_register_multistart: K starts per humerus (T0s: (B, K, 4, 4)), a coarse registration of the subsampled points from each, the
        fine registration of all points from the best -> (records (B,), coarse records (B, K), winner (B,) int32, -1 where no start
        qualified: that record has status SH_ERR_GEOMETRY and T = T0s[b][0]).  coarse / fine: dicts of metric, max_iter, reject, tol as
        in register.  Every record is what register returns for those points, that start and those options, byte for byte."""
        p = self._points_arg(points)
        t0 = np.ascontiguousarray(T0s, dtype=np.float64)
        if t0.ndim != 4 or t0.shape[0] != self.B or t0.shape[2:] != (4, 4):
            raise ValueError("T0s must have shape (B, K, 4, 4)")
        co, fo = _icp_options(**(coarse or {})), _icp_options(**(fine or {}))
        K = t0.shape[1]
        out = np.zeros(self.B, dtype=_lib.REGISTRATION_DTYPE)
        cand = np.zeros((self.B, K) if 1 <= K <= _lib.MS_MAX_STARTS else (0,), dtype=_lib.REGISTRATION_DTYPE)
        winner = np.zeros(self.B, dtype=np.int32)
        self._chk(self.L.sh_register_multistart(self.h, _ptr(p), p.shape[-2], int(p.ndim == 3), _ptr(t0), K, ctypes.byref(co), int(coarse_points),
                                                int(min_pairs), ctypes.byref(fo), _ptr(out), _ptr(cand), _ptr(winner)))
        return out, cand, winner

    def register_global(self, points, rolls=8, coarse_points=512, coarse_iter=4, min_pairs=None, **fine_options):
        """`trimesh.registration.mesh_other` for points in an UNKNOWN pose: principal_starts (2 * rolls starts per humerus), coarse_iter
        plane-metric updates on coarse_points of the points from each, the registration of all points from the best (fine_options:
        metric, max_iter, reject, tol as in register; the coarse stage shares `reject`) -> (records (B,) of _lib.REGISTRATION_DTYPE,
        info) with info = dict(winner (B,), coarse (B, 2 * rolls) records, mesh_ratio (B,), points_ratio (B,): the ratio of the two
        largest shell eigenvalues of each mesh and of its points).  min_pairs=None: half the coarse set, at least 6; a start with
        fewer accepted pairs cannot win.  A humerus none of whose starts qualified has status SH_ERR_GEOMETRY and winner -1.
        The starts rest on the long axis: A NEAR-ROUND SHAPE (a ratio near 1: a resected head, a sphere) HAS NO LONG AXIS AND ITS
        STARTS ARE ARBITRARY -- the call then is a multi-start from 2 * rolls unrelated poses and nothing more."""
        p = self._points_arg(points)
        T0s, rm, rp = self.principal_starts(p, rolls, with_ratios=True)
        Q = p.shape[-2]
        Qc = Q if coarse_points == 0 or coarse_points > Q else int(coarse_points)
        if min_pairs is None:
            min_pairs = max(6, Qc // 2)
        coarse = dict(metric="plane", max_iter=int(coarse_iter), reject=fine_options.get("reject", np.inf), tol=0.0)
        out, cand, winner = self.register_multistart(p, T0s, coarse=coarse, coarse_points=coarse_points, min_pairs=min_pairs, fine=fine_options)
        return out, dict(winner=winner, coarse=cand, mesh_ratio=rm, points_ratio=rp, starts=T0s)

    # ---- named buffers -----------------------------------------------------------------------------
    def fetch(self, name, dtype, shape=None):
        n, e = ctypes.c_size_t(), ctypes.c_int()
        self._chk(self.L.sh_buffer_info(self.h, name.encode(), ctypes.byref(n), ctypes.byref(e)))
        dtype = np.dtype(dtype)
        count = int(np.prod(shape)) if shape is not None else n.value // dtype.itemsize
        out = np.empty(count, dtype=dtype)
        self._chk(self.L.sh_fetch(self.h, name.encode(), _ptr(out), out.nbytes))
        return out.reshape(shape) if shape is not None else out

    def store(self, name, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.sh_store(self.h, name.encode(), _ptr(arr), arr.nbytes))

    def unet_infer(self, images):
        """The anatomic-neck network alone: images (n, H, W) float32 -> logits (n, H, W) float32 (anatomic_neck.py:67-76)."""
        x = np.ascontiguousarray(images, dtype=np.float32)
        if x.ndim != 3:
            raise ValueError("images must have shape (n, H, W)")
        out = np.empty_like(x)
        self._chk(self.L.sh_unet_infer(self.h, _ptr(x), x.shape[0], x.shape[1], x.shape[2], _ptr(out)))
        return out

    # ---- timing --------------------------------------------------------------------------------------
    def enable_timing(self, on=True):
        self._chk(self.L.sh_enable_timing(self.h, int(on)))      # 0 off, 1 every launch, 2 UNet layers only

    def set_hull_mode(self, mode):
        """"host" | "device" | "auto": where the convex hull of the OBB stage is computed (sh_set_hull_mode); same results."""
        self._chk(self.L.sh_set_hull_mode(self.h, str(mode).encode()))

    @property
    def hull_mode(self):
        return "device" if self.L.sh_get_hull_mode(self.h) == 1 else "host"

    def set_overlap(self, on=True):
        """Streaming runs on the resident batch: compute the host hulls of the next run while the device works on this one."""
        self._chk(self.L.sh_set_overlap(self.h, 1 if on else 0))

    def set_unet_turns(self, on=True):
        """Several engines on one device: their UNet passes run one after another, geometry overlaps (sh_set_unet_turns)."""
        self._chk(self.L.sh_set_unet_turns(self.h, 1 if on else 0))

    def discard_prepared(self):
        self._chk(self.L.sh_discard_prepared(self.h))

    def reset_timers(self):
        self._chk(self.L.sh_kernel_time_ms(self.h, None, None, None))

    def kernel_time_ms(self, name):
        ms, n = ctypes.c_double(), ctypes.c_int()
        self._chk(self.L.sh_kernel_time_ms(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value
