#!/usr/bin/env python3
"""Timing of the repair on the bench batch (64 similarity copies of humerus_left), in the manner of tools/time_smooth.py.  The topology
is resident before the clock starts.  Three batches: the clean bone, the bone with 30 % of its faces reversed, and the bone with 20
single faces taken out (20 holes of three edges each).  One run gives, for each, orient = outward and fill = centroid:
  (a) Engine.repair: host clock around the synchronous call with the records, the flips and the repaired meshes copied back, median and
      span of 5 after 1 warm-up;
  (b) the same through the C entry point with null outputs: the read of "topo.info" and the device pass without the copies back;
  (c) the kernels of one call (HIP events inside the library: sh_enable_timing; averages per launch);
and beside them the project's own yardstick, one sh_mesh_topology of the same batch, and for ONE clean bone the NumPy oracle
(tests/repair_oracle.py).  One JSON line."""
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
KERNELS = ("k_repair_seed", "k_repair_parity", "k_repair_shell", "k_repair_nest", "k_repair_emit", "k_repair_holes")


def spread(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def timed(fn, runs, warm):
    t = []
    for i in range(warm + runs):
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


def main():
    import repair_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    gone = np.zeros(len(f), bool)
    gone[np.arange(500, 500 + 20 * 1500, 1500)] = True
    batches = {"clean": f, "reversed_30pct": O.reversed_faces(f)[0], "holes_20": np.ascontiguousarray(f[~gone])}
    e = Engine(0)
    out = dict(B=B, faces=int(len(f)), vertices=int(len(v)))
    opt = np.array([O.OUTWARD, O.CENTROID, 4096, 64, O.MAX_ROUNDS, 0], np.int32)
    for name, faces in batches.items():
        e.upload([(v, faces)])
        e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
        out.setdefault("topology", timed(lambda: e.topology(), 5, 1))
        e.topology()
        call = lambda: e.repair()
        r = timed(call, 5, 1)
        r["device_only"] = timed(lambda: e._chk(e.L.sh_mesh_repair(e.h, opt.ctypes.data, None, None, None, None)), 5, 1)
        r["kernels"] = kernels_of(e, call)
        info = call()["info"]
        r["status_nonzero"], r["faces_flipped"], r["holes"], r["holes_filled"] = int((info["status"] != 0).sum()), int(info["faces_flipped"][0]), int(info["holes"][0]), \
            int(info["holes_filled"][0])
        out[name] = r
    e.close()
    t0 = time.perf_counter()
    O.repair(v, f)
    out["oracle_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
