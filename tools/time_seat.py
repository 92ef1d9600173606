#!/usr/bin/env python3
"""Timing of the seats of a head catalogue on a batched resection on the bench batch (64 similarity copies of humerus_left, landmarks
resident, the 27-offset grid, K = 16 heads), in the manner of tools/time_head_fit.py.
  python tools/time_seat.py new      (a) Engine.resect(offsets=<27-grid>, fit=True, heads=<16>), (b) Engine.resect(offsets=<27-grid>, fit=True),
                                     (d) the kernels of (a) alone (HIP events inside the library: sh_enable_timing), and k_seat again with
                                     K = 1 and K = 64: what grows with K is the per-head arithmetic and its reduction, what stays is the
                                     ring load and the head-independent rim pass
  python tools/time_seat.py parent   (b) on a build without the seats (SHOULDER_LIB=<the parent commit's library>) and (c) the only way to
                                     these numbers there: Engine.resect_ring per cut + the NumPy statement of tests/seat_oracle.py per
                                     head, on N_CUTS cuts, EXTRAPOLATED to 64 x 27 cuts
Every call is synchronous (it returns host data): host clock around it, median of 10 runs after 2 warm-ups, one JSON line.
Interleave the two modes on one box."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shoulder_amd import _lib, synth, unet_spec      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

GRID27 = [dict(retroversion_deg=r, neckshaft_deg=n, depth_canal_mm=d) for r in (-10.0, 0.0, 10.0) for n in (-10.0, 0.0, 10.0) for d in (-6.0, 0.0, 6.0)]
HEADS16 = [(0.5 * d, t) for d in (40.0, 44.0, 48.0, 52.0) for t in (14.0, 16.0, 18.0, 20.0)]
B, RUNS, WARM, N_CUTS = 64, 10, 2, 8
KERNELS = ("k_resect_faces", "k_headfit_faces", "k_resect_join_seat", "k_headfit_solve", "k_seat", "k_resect_make_planes")


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


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
    out = dict(mode=mode, B=B, P=len(GRID27), K=len(HEADS16), faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    out["b_resect_fit_P27"] = timed(lambda: e.resect(offsets=GRID27, fit=True))
    if mode == "new":
        out["a_resect_seat_P27_K16"] = timed(lambda: e.resect(offsets=GRID27, fit=True, heads=HEADS16))
        out["b_resect_fit_P27_again"] = timed(lambda: e.resect(offsets=GRID27, fit=True))
        e.enable_timing(1)
        for name, heads in (("K16", HEADS16), ("K1", HEADS16[5:6]), ("K64", HEADS16 * 4)):
            e.reset_timers()
            for _ in range(RUNS):
                e.resect(offsets=GRID27, fit=True, heads=heads)
            for k in (KERNELS if name == "K16" else ("k_seat",)):
                out["%s_ms_%s" % (k, name)] = e.kernel_time_ms(k)[0]
        e.enable_timing(0)
        recs, fits, seats = e.resect(offsets=GRID27, fit=True, heads=HEADS16)
        r2, f2 = e.resect(offsets=GRID27, fit=True)
        out["status_ok"] = bool(np.all(recs["status"] == 0) and np.all(seats["status"] == 0))
        out["records_and_fits_equal_fitted_call"] = bool(recs.tobytes() == r2.tobytes() and fits.tobytes() == f2.tobytes())
        out["coverage_b0_native"] = [float(x) for x in seats[0, 13]["coverage"]]
        out["n_ring_min_max"] = [int(recs["n_ring"].min()), int(recs["n_ring"].max())]
    else:
        import seat_oracle as S
        recs, fits = e.resect(offsets=GRID27, fit=True)

        def one_cut(b, p):
            ring = e.resect_ring(b, p)
            rec, fit = recs[b, p], fits[b, p]
            q, w = np.zeros((0, 3)), np.zeros(0)      # (surface_rms needs the samples: not available on this route at all)
            return [S.seat_record(ring, rec["plane_point"], rec["plane_normal"], rec["cut_centroid"], R, h, q, w, sphere_center=fit["sphere_center"])
                    for R, h in HEADS16]
        cuts = [(b, p) for b in (0, 1) for p in (0, 9, 13, 26)][:N_CUTS]
        t = timed(lambda: [one_cut(b, p) for b, p in cuts], runs=3, warm=1)
        out["c_resect_ring_plus_numpy_%d_cuts" % N_CUTS] = t
        out["c_extrapolated_ms_for_%d_cuts" % (B * len(GRID27))] = t["median_ms"] / N_CUTS * B * len(GRID27)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
