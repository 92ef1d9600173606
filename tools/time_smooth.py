#!/usr/bin/env python3
"""Timing of the vertex smoothing on the bench batch (64 similarity copies of humerus_left), in the manner of
tools/time_vertex_fields.py.  The topology and the neighbour rows are resident before the clock starts.  One run gives, for the
Laplacian, Taubin and HC filters at 10 iterations in both weights:
  (a) Engine.smooth_vertices: host clock around the synchronous call (the vertices and the info records come back to the host inside
      it), median and span of 5 after 1 warm-up;
  (b) the same through the C entry point with null outputs: the device pass without the copies back;
  (c) the kernels of one call (HIP events inside the library: sh_enable_timing; averages per launch);
and, once, the build of the rows alone: a call without an iteration on a batch whose rows were removed (outside the clock: the vertices
stored again and a topology), with its kernels;
  (d) beside them, for ONE humerus and ten Taubin iterations, the NumPy oracle (tests/smooth_oracle.py) and a scipy.sparse version (the
      row-normalised adjacency matrix applied twenty times).
One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shoulder_amd import _lib, synth      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

B, ITER = 64, 10
KERNELS = ("k_smooth_count", "k_smooth_scan", "k_smooth_fill", "k_smooth_init", "k_smooth_step", "k_smooth_hc_b", "k_smooth_hc_p", "k_smooth_vol", "k_smooth_scale",
           "k_smooth_apply", "k_smooth_info")
PARAMS = {"laplacian": (_lib.SMOOTH_LAPLACIAN, 0.5, 0.0), "taubin": (_lib.SMOOTH_TAUBIN, 0.5, -0.53), "hc": (_lib.SMOOTH_HC, 0.1, 0.5)}


def spread(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def timed(fn, runs, warm, before=None):
    t = []
    for i in range(warm + runs):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
    return spread(t)


def kernels_of(e, call):
    e.enable_timing(1)
    e.reset_timers()
    call()
    out = {}
    for k in KERNELS:
        ms, n = e.kernel_time_ms(k)
        if n:
            out[k] = dict(avg_ms=ms, launches=n)
    e.enable_timing(0)
    return out


def sparse_taubin(v, f, iterations, lamb, mu):
    """ten Taubin iterations with a row-normalised scipy.sparse adjacency matrix (uniform weights): the usual host version"""
    from scipy.sparse import coo_matrix, diags
    n = len(v)
    i = np.concatenate([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
    j = np.concatenate([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
    A = coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)).tocsr()
    A.data[:] = 1.0
    M = diags(1.0 / np.maximum(np.asarray(A.sum(axis=1)).ravel(), 1.0)) @ A
    P = v.astype(np.float64)
    for _ in range(iterations):
        P = P + lamb * (M @ P - P)
        P = P + mu * (M @ P - P)
    return P


def main():
    import smooth_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    e.topology()
    e.smooth_vertices(iterations=0)
    out = dict(B=B, faces=int(len(f)), vertices=int(len(v)), iterations=ITER)
    for name, (filt, p0, p1) in PARAMS.items():
        for wname, weight in (("uniform", _lib.SMOOTH_UNIFORM), ("invlen", _lib.SMOOTH_INVLEN)):
            kw = dict(filter=name, weight=wname, iterations=ITER, **(dict(alpha=p0, beta=p1) if name == "hc" else dict(lamb=p0, mu=p1)))
            call = lambda: e.smooth_vertices(**kw)
            r = timed(call, 5, 1)
            r["device_only"] = timed(lambda: e._chk(e.L.sh_smooth_vertices(e.h, filt, weight, ITER, 0, p0, p1, None, None, None)), 5, 1)
            r["kernels"] = kernels_of(e, call)
            info = call()["info"]
            r["status_nonzero"], r["max_disp_mm"] = int((info["status"] != 0).sum()), float(info["max_disp"].max())
            out[f"{name}_{wname}"] = r
    verts = e.fetch("verts", np.float32)

    def drop_rows():
        e.store("verts", verts)
        e.topology()
    build = lambda: e._chk(e.L.sh_smooth_vertices(e.h, _lib.SMOOTH_TAUBIN, 0, 0, 0, 0.5, -0.53, None, None, None))
    out["rows"] = timed(build, 5, 1, before=drop_rows)
    drop_rows()
    out["rows"]["kernels"] = kernels_of(e, build)
    e.close()
    t0 = time.perf_counter()
    ref = O.smooth(v, f, filter=O.TAUBIN, iterations=ITER)["pos"]
    out["oracle_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sp = sparse_taubin(v, f, ITER, 0.5, -0.53)
    out["scipy_sparse_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
    out["scipy_sparse_max_abs_diff_mm"] = float(np.abs(sp - ref).max())      # (another order of the sums: rounding only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
