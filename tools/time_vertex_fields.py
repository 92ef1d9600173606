#!/usr/bin/env python3
"""Timing of the vertex fields on the bench batch (64 similarity copies of humerus_left), in the manner of tools/time_topology.py.  One
run gives, with smooth 0 and 8 (area weights; the topology is resident before the clock starts):
  (a) Engine.vertex_fields: host clock around the synchronous call (normals, fields, flags and status come back to the host inside
      it), median and span of 5 after 1 warm-up;
  (b) the same through the C entry point with null outputs: the device pass without the copies back;
  (c) the kernels of one call (HIP events inside the library: sh_enable_timing; averages per launch -- k_vert_smooth is launched
      `smooth` times);
  (d) beside them the NumPy oracle (tests/vert_oracle.py) for ONE humerus.
One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shoulder_amd import synth      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

B = 64
KERNELS = ("k_vert_face", "k_vert_gather", "k_vert_smooth", "k_vert_pack")


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
    import vert_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    e.topology()
    out = dict(B=B, faces=int(len(f)), vertices=int(len(v)))
    for smooth in (0, 8):
        call = lambda: e.vertex_fields(weight="area", smooth=smooth)
        r = timed(call, 5, 1)
        r["device_only"] = timed(lambda: e._chk(e.L.sh_vertex_fields(e.h, 0, smooth, None, None, None, None)), 5, 1)
        r["kernels"] = kernels_of(e, call)
        r["status_nonzero"] = int((call()["status"] != 0).sum())
        t0 = time.perf_counter()
        O.vertex_fields(v, f, smooth=smooth)
        r["oracle_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
        out[f"smooth_{smooth}"] = r
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
