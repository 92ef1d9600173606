#!/usr/bin/env python3
"""Timing of the head fit of a batched resection on the bench batch (64 similarity copies of humerus_left, landmarks resident), in
the manner of tools/time_resect.py.
  python tools/time_head_fit.py new      (a) Engine.resect(offsets=<27-grid>, fit=True), (b) Engine.resect(offsets=<27-grid>), (d) the
                                         kernels of (a) alone (HIP events inside the library: sh_enable_timing)
  python tools/time_head_fit.py parent   (b) on a build without the fit (SHOULDER_LIB=<the parent commit's library>) and (c) the only
                                         way to these numbers there: HumeralHeadOsteotomy.resect_mesh() per cut + NumPy (the lstsq
                                         sphere of the head mesh), on N_CUTS cuts of one humerus, EXTRAPOLATED to 64 x 27 cuts
Every call is synchronous (it returns host data): host clock around it, median of 10 runs after 2 warm-ups, one JSON line.
Interleave the two modes on one box."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shoulder_amd import _lib, synth, unet_spec      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

GRID27 = [dict(retroversion_deg=r, neckshaft_deg=n, depth_canal_mm=d) for r in (-10.0, 0.0, 10.0) for n in (-10.0, 0.0, 10.0) for d in (-6.0, 0.0, 6.0)]
B, RUNS, WARM, N_CUTS = 64, 10, 2, 4


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def sphere_of_mesh(v, f):
    tri = v[f]
    cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    w = np.repeat(np.linalg.norm(cr, axis=1) / 6.0, 3)
    q = tri.reshape(-1, 3)
    o = q.mean(axis=0)
    q = q - o
    sw = np.sqrt(w)
    sol = np.linalg.lstsq(np.c_[2 * q, np.ones(len(q))] * sw[:, None], (q * q).sum(axis=1) * sw, rcond=None)[0]
    return o + sol[:3], np.sqrt(sol[3] + sol[:3] @ sol[:3])


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "new"
    path = os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl")
    v, f = load_stl(path)
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.set_params(unet_dtype=_lib.UNET_BF16)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    e.run(_lib.STAGE_ALL)
    out = dict(mode=mode, B=B, P=len(GRID27), faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    out["b_resect_P27"] = timed(lambda: e.resect(offsets=GRID27))
    if mode == "new":
        out["a_resect_fit_P27"] = timed(lambda: e.resect(offsets=GRID27, fit=True))
        out["b_resect_P27_again"] = timed(lambda: e.resect(offsets=GRID27))
        e.enable_timing(1)
        e.reset_timers()
        for _ in range(RUNS):
            e.resect(offsets=GRID27, fit=True)
        for k in ("k_resect_faces", "k_headfit_faces", "k_resect_join_fit", "k_headfit_solve", "k_resect_make_planes"):
            out[k + "_ms"] = e.kernel_time_ms(k)[0]
        e.enable_timing(0)
        recs, fits = e.resect(offsets=GRID27, fit=True)
        out["status_ok"] = bool(np.all(recs["status"] == 0) and np.all(fits["sphere_status"] == 0))
        out["radius_mm_b0_native"] = float(fits[0, 13]["sphere_radius"])
        out["records_equal_unfitted"] = bool(recs.tobytes() == e.resect(offsets=GRID27).tobytes())
    else:
        import shoulder_amd as shoulder
        hum = shoulder.Humerus(path, engine=e)
        ost = shoulder.HumeralHeadOsteotomy(hum)

        def one_cut():
            ost.offset_depth(0.5)
            head = ost.resect_mesh()[0]
            return sphere_of_mesh(np.asarray(head.vertices), np.asarray(head.faces))
        t = timed(lambda: [one_cut() for _ in range(N_CUTS)], runs=3, warm=1)
        out["c_resect_mesh_plus_numpy_%d_cuts" % N_CUTS] = t
        out["c_extrapolated_ms_for_%d_cuts" % (B * len(GRID27))] = t["median_ms"] / N_CUTS * B * len(GRID27)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
