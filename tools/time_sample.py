#!/usr/bin/env python3
"""Timing of the surface samples on the bench batch (64 similarity copies of humerus_left), in the manner of
tools/time_register_global.py.  One run gives:
  (a) Engine.sample_surface without thinning at N = 4 096 and 65 536: host clock around the synchronous call (the records come back to
      the host inside it), median of 5 after 1 warm-up, and the kernels of one call (HIP events inside the library: sh_enable_timing;
      averages per launch);
  (b) the same with radius 2 mm at N = 4 096 and 16 384 (max_rounds 32: the host enqueues all 32 launches of k_samp_thin), the kernels,
      the rounds used and the samples kept;
  (c) beside them the NumPy oracle (tests/sample_oracle.py) for ONE humerus at the same N (the thinned one at N = 4 096 only: its
      neighbour lists are a Python loop);
  (d) with --register: the multi-start registration of tools/time_register_global.py with its points chosen by Engine.sample_surface
      (4 096 samples of every humerus) instead of vertices spread over the bone -- host clock, winners, distance from the truth.
One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shoulder_amd import synth, unet_spec      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

B, SEED, RADIUS = 64, 7, 2.0
KERNELS = ("k_samp_scan", "k_samp_base", "k_samp_draw", "k_samp_thin", "k_samp_finish")


def timed(fn, runs, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


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


def main():
    import sample_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    out = dict(B=B, faces=int(len(f)), seed=SEED, radius=RADIUS)
    for N in (4096, 65536):
        call = lambda: e.sample_surface(N, seed=SEED)
        r = timed(call, 5, 1)
        r["kernels"] = kernels_of(e, call)
        t0 = time.perf_counter()
        O.sample(v, f, N, SEED)
        r["oracle_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
        out["a_plain_N%d" % N] = r
    for N in (4096, 16384):
        call = lambda: e.sample_surface(N, seed=SEED, radius=RADIUS)
        r = timed(call, 3, 1)
        r["kernels"] = kernels_of(e, call)
        info = call()[1]
        r["rounds"], r["kept_min_max"], r["status_nonzero"] = sorted(set(int(x) for x in info["rounds"])), [int(info["kept"].min()), int(info["kept"].max())], int((info["status"] != 0).sum())
        if N == 4096:
            t0 = time.perf_counter()
            o = O.sample(v, f, N, SEED, RADIUS)
            r["oracle_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
            r["oracle_kept_rounds"] = [int(o[1]["kept"]), int(o[1]["rounds"])]
        out["b_thinned_N%d" % N] = r
    if "--register" in sys.argv:
        import icp_oracle as IO
        Q, ROLLS, QC = 4096, 8, 512
        truth = np.ascontiguousarray(e.sample_surface(Q, seed=SEED)[0]["point"])
        pts = np.stack([IO.apply(IO.rigid((1.0, 2.0, 3.0), 140.0, (40.0, -25.0, 60.0), about=truth[b].mean(axis=0)), truth[b]) for b in range(B)])
        T0s = e.principal_starts(pts, rolls=ROLLS)
        coarse, fine = dict(metric="plane", max_iter=4), dict(metric="plane", max_iter=8)
        call = lambda: e.register_multistart(pts, T0s, coarse=coarse, coarse_points=QC, min_pairs=QC // 2, fine=fine)
        r = timed(call, 3, 1)
        rec, cand, winner = call()
        r["status_nonzero"], r["winners"], r["rms_median"] = int((rec["status"] != 0).sum()), sorted(set(int(w) for w in winner)), float(np.median(rec["rms"]))
        r["max_distance_from_truth_mm"] = float(max(np.abs(IO.apply(rec[b]["T"], pts[b]) - truth[b]).max() for b in range(B)))
        out["d_register_multistart_on_samples"] = r
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
