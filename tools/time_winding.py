#!/usr/bin/env python3
"""Timing of the generalized winding numbers on the bench batch (64 similarity copies of humerus_left), in the manner of
tools/time_closest.py and with its points: Q = 4 096 points per humerus (per_humerus), each humerus' own first 4 096 vertices moved
2 mm along a seeded random direction.  One run gives:
  (a) Engine.winding_numbers(points (B, Q, 3)): host clock around the synchronous call, median of 10 after 2 warm-ups, and the kernels
      of it alone (HIP events inside the library: sh_enable_timing);
  (b) the NumPy statement of tests/winding_oracle.py on the fetched meshes -- the only way to these numbers on a build without the
      call -- on N_HUMERI humeri x N_POINTS points, EXTRAPOLATED to 64 x 4 096, and how far the device is from it on those rows
      against the bound (2 F + 16) 2^-53 max(1, A);
  (c) Q = 4 points shared by all humeri: the small call, which costs what 256 points cost, walked in splits.
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

B, Q, RUNS, WARM, N_HUMERI, N_POINTS = 64, 4096, 10, 2, 2, 16
KERNELS = ("k_wn_walk", "k_wn_join")


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def kernel_times(e, fn):
    e.enable_timing(1)
    e.reset_timers()
    for _ in range(RUNS):
        fn()
    out = {"%s_ms" % k: e.kernel_time_ms(k)[0] for k in KERNELS}
    e.enable_timing(0)
    return out


def main():
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    verts = e.fetch("verts", np.float32).reshape(-1, 3)
    voff = np.asarray(e.voff)
    rng = np.random.default_rng(7)
    d = rng.normal(size=(B, Q, 3))
    pts = np.stack([verts[voff[b]:voff[b] + Q].astype(np.float64) for b in range(B)]) + 2.0 * d / np.linalg.norm(d, axis=2, keepdims=True)
    out = dict(B=B, Q=Q, faces=int(len(f)), pairs=int(B) * Q * int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    out["a_winding_numbers_B64_Q4096"] = timed(lambda: e.winding_numbers(pts))
    got = e.winding_numbers(pts)
    out["inside_share"], out["status_nonzero"] = float(got["inside"].mean()), int((got["status"] != 0).sum())
    out["max_off_integer"] = float(np.abs(got["winding"] - np.round(got["winding"])).max())
    out.update({"a_" + k: t for k, t in kernel_times(e, lambda: e.winding_numbers(pts)).items()})
    small = pts[0, :4]
    out["c_winding_numbers_Q4_shared"] = timed(lambda: e.winding_numbers(small))
    out.update({"c_" + k: t for k, t in kernel_times(e, lambda: e.winding_numbers(small)).items()})
    import winding_oracle as O

    def numpy_rows():
        return [O.winding(verts[voff[b]:voff[b + 1]], f, pts[b, :N_POINTS]) for b in range(N_HUMERI)]
    t = timed(numpy_rows, runs=3, warm=1)
    out["b_numpy_%d_humeri_%d_points" % (N_HUMERI, N_POINTS)] = t
    out["b_extrapolated_ms_for_%d_points" % (B * Q)] = t["median_ms"] / (N_HUMERI * N_POINTS) * B * Q
    want = numpy_rows()
    diff = max(float(np.abs(got[b, :N_POINTS]["winding"] - want[b][0]["winding"]).max()) for b in range(N_HUMERI))
    out["max_abs_diff_to_numpy_on_the_timed_rows"] = diff
    out["bound_on_the_timed_rows"] = float(min(O.bound(len(f), want[b][1]).min() for b in range(N_HUMERI)))
    out["inside_equal_to_numpy_on_the_timed_rows"] = bool(all(np.array_equal(got[b, :N_POINTS]["inside"], want[b][0]["inside"]) for b in range(N_HUMERI)))
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
