#!/usr/bin/env python3
"""Timing of the rigid registration on the bench batch (64 similarity copies of humerus_left), in the manner of tools/time_closest.py.
Q = 4 096 points per humerus (per_humerus): each humerus' own first 4 096 vertices moved by 4 degrees about (1, 2, 3) through their
centroid and (1.5, -1.0, 0.8) mm, plane metric, max_iter = 8 (nine evaluations, tol = 0).  One run gives:
  (a) Engine.register(points (B, Q, 3)): host clock around the synchronous call, median of 10 after 2 warm-ups, the kernels of it
      alone (HIP events inside the library: sh_enable_timing; averages per launch, 9 launches of each per call, 10 of k_icp_sum and
      k_icp_step with the centroid pass), and how far the registered points end from where they came from;
  (b) the only way a build without the call has: a Python loop of Engine.closest_points, the fetched pairs, the sums and the solve in
      NumPy (tests/icp_oracle.py: pair_terms, tree_sum, plane_solve), the same nine evaluations on the same inputs, median of 3
      after 1 warm-up; and whether its transforms are the device's bytes.
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

B, Q, K, RUNS, WARM = 64, 4096, 8, 10, 2
KERNELS = ("k_icp_move", "k_cp_walk", "k_cp_join", "k_icp_sum", "k_icp_step")


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
    truth = np.stack([verts[voff[b]:voff[b] + Q].astype(np.float64) for b in range(B)])
    pts = np.stack([O.apply(O.rigid((1.0, 2.0, 3.0), 4.0, (1.5, -1.0, 0.8), about=truth[b].mean(axis=0)), truth[b]) for b in range(B)])
    out = dict(B=B, Q=Q, max_iter=K, metric="plane", faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    out["a_register_B64_Q4096"] = timed(lambda: e.register(pts, metric="plane", max_iter=K))
    rec, hist = e.register(pts, metric="plane", max_iter=K, history=True)
    out["a_status_nonzero"], out["a_iterations"] = int((rec["status"] != 0).sum()), [int(rec["iterations"].min()), int(rec["iterations"].max())]
    out["a_rms_first_median"], out["a_rms_median"], out["a_min_pivot_min"] = float(np.median(rec["rms_first"])), float(np.median(rec["rms"])), float(rec["min_pivot"].min())
    out["a_max_distance_from_truth_mm"] = float(max(np.abs(O.apply(rec[b]["T"], pts[b]) - truth[b]).max() for b in range(B)))
    e.enable_timing(1)
    e.reset_timers()
    for _ in range(RUNS):
        e.register(pts, metric="plane", max_iter=K)
    for k in KERNELS:
        ms, n = e.kernel_time_ms(k)
        out["a_%s_ms" % k], out["a_%s_launches_per_call" % k] = ms, n / RUNS
    e.enable_timing(0)
    meshes = [(verts[voff[b]:voff[b + 1]], f) for b in range(B)]

    def python_loop():
        T = [list(np.identity(4).reshape(16)) for _ in range(B)]
        cbar = [O.tree_sum(np.concatenate([np.ones((Q, 1)), pts[b]], axis=1))[1:] / float(Q) for b in range(B)]
        for k in range(K + 1):
            moved = np.stack([O.map_points(T[b], pts[b]) for b in range(B)])
            near = e.closest_points(moved)                                             # one host round trip per evaluation
            if k == K:
                break
            for b in range(B):
                ab, ac = O.face_edges(*meshes[b], near[b])
                c = O.map_points(T[b], cbar[b][None, :])[0]
                tot = O.tree_sum(O.pair_terms(O.PLANE, moved[b], near[b], ab, ac, c, np.inf))
                T[b] = O.compose(O.plane_solve(tot, c)[0], T[b])
        return np.array(T).reshape(B, 4, 4)
    out["b_python_loop_closest_points_numpy_solve"] = timed(python_loop, runs=3, warm=1)
    out["b_transforms_bytes_equal_to_register"] = bool(python_loop().tobytes() == np.ascontiguousarray(rec["T"]).tobytes())
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
