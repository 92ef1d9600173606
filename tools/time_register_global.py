#!/usr/bin/env python3
"""Timing of the multi-start registration and of the mass properties on the bench batch (64 similarity copies of humerus_left), in the
manner of tools/time_register.py.  Q = 4 096 points per humerus (per_humerus): 4 096 of each humerus' own vertices, spread over the whole
bone (vertex floor(j V / Q): a patch of the bone has another principal frame than the bone and is no input for these starts), moved by 140
degrees about (1, 2, 3) through their centroid and (40, -25, 60) mm; 2 x 8 = 16 starts from Engine.principal_starts, 4 plane updates
on 512 coarse points from each, then the fine stage, plane, max_iter = 8.  One run gives:
  (a) Engine.register_multistart (the starts made once, outside the clock): host clock around the synchronous call, median of 5 after
      1 warm-up, the kernels of it alone (HIP events inside the library: sh_enable_timing; averages per launch), the winners and how
      far the registered points end from where they came from;
  (b) the same work as a build without the call has to do it: a Python loop of 16 Engine.register calls on the gathered coarse points,
      the argmin under the rule on the host, and one Engine.register from the best; median of 3 after 1 warm-up; and whether its
      records are the call's bytes;
  (c) Engine.mass_properties for B = 64: host clock, median of 10 after 2 warm-ups, and its two kernels.
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

B, Q, ROLLS, QC, COARSE_ITER, FINE_ITER = 64, 4096, 8, 512, 4, 8
KERNELS = ("k_ms_seed", "k_ms_pick", "k_icp_move", "k_cp_walk", "k_cp_join", "k_icp_sum", "k_icp_step")


def timed(fn, runs, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def main():
    import icp_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    verts = e.fetch("verts", np.float32).reshape(-1, 3)
    voff = np.asarray(e.voff)
    spread = (np.arange(Q) * len(v)) // Q                                              # Q vertices spread over the WHOLE bone: the starts rest on its frame
    truth = np.stack([verts[voff[b] + spread].astype(np.float64) for b in range(B)])
    pts = np.stack([O.apply(O.rigid((1.0, 2.0, 3.0), 140.0, (40.0, -25.0, 60.0), about=truth[b].mean(axis=0)), truth[b]) for b in range(B)])
    out = dict(B=B, Q=Q, starts=2 * ROLLS, coarse_points=QC, coarse_iter=COARSE_ITER, fine_iter=FINE_ITER, faces=int(len(f)))
    out["c_mass_properties_B64"] = timed(e.mass_properties, 10, 2)
    t0 = time.perf_counter()
    T0s = e.principal_starts(pts, rolls=ROLLS)
    out["principal_starts_ms"] = (time.perf_counter() - t0) * 1e3
    coarse, fine = dict(metric="plane", max_iter=COARSE_ITER), dict(metric="plane", max_iter=FINE_ITER)
    call = lambda: e.register_multistart(pts, T0s, coarse=coarse, coarse_points=QC, min_pairs=QC // 2, fine=fine)
    out["a_register_multistart"] = timed(call, 5, 1)
    rec, cand, winner = call()
    out["a_status_nonzero"], out["a_winners"] = int((rec["status"] != 0).sum()), sorted(set(int(w) for w in winner))
    out["a_rms_median"] = float(np.median(rec["rms"]))
    out["a_max_distance_from_truth_mm"] = float(max(np.abs(O.apply(rec[b]["T"], pts[b]) - truth[b]).max() for b in range(B)))
    e.enable_timing(1)
    e.reset_timers()
    call()
    e.mass_properties()
    for k in KERNELS + ("k_mass_sum", "k_mass_join"):
        ms, n = e.kernel_time_ms(k)
        out["%s_ms" % k], out["%s_launches" % k] = ms, n
    e.enable_timing(0)
    gathered = np.ascontiguousarray(pts[:, [j * Q // QC for j in range(QC)]])

    def python_loop():
        c = np.stack([e.register(gathered, T0=np.ascontiguousarray(T0s[:, k]), **coarse) for k in range(2 * ROLLS)], axis=1)
        ok = (c["status"] == 0) & (c["pairs"] >= QC // 2)
        w = np.argmin(np.where(ok, c["rms"], np.inf), axis=1)      # (the first among equals, as the rule)
        return e.register(pts, T0=np.ascontiguousarray(c[np.arange(B), w]["T"]), **fine), c, np.where(ok.any(axis=1), w, -1)
    out["b_python_loop_of_register_calls"] = timed(python_loop, 3, 1)
    r2, c2, w2 = python_loop()
    out["b_bytes_equal_to_the_call"] = bool(r2.tobytes() == rec.tobytes() and c2.tobytes() == cand.tobytes() and np.array_equal(w2, winner))
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
