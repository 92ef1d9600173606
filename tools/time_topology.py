#!/usr/bin/env python3
"""Timing of the mesh topology on the bench batch (64 similarity copies of humerus_left), in the manner of tools/time_sample.py.  One
run gives, for the faces in the file's order and once more with the faces shuffled (default_rng(1).permutation):
  (a) Engine.topology(max_shells=64, max_rounds=32): host clock around the synchronous call (info and shell records come back to the
      host inside it), median and span of 5 after 1 warm-up;
  (b) the kernels of one call (HIP events inside the library: sh_enable_timing; averages per launch -- k_topo_round is launched
      max_rounds times, and the launches behind the last round return at once), the rounds used and the shells found;
  (c) the same call with max_rounds set to the rounds (b) used, which leaves the launches that return at once out;
  (d) beside them the NumPy oracle (tests/topo_oracle.py) for ONE humerus.
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
KERNELS = ("k_topo_count", "k_topo_scan", "k_topo_fill", "k_topo_rows", "k_topo_adj", "k_topo_round", "k_topo_rank", "k_topo_label", "k_topo_finish")


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
    import topo_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    out = dict(B=B, faces=int(len(f)))
    for tag, faces in (("in_order", f), ("shuffled", np.ascontiguousarray(f[np.random.default_rng(1).permutation(len(f))]))):
        e.upload([(v, faces)])
        e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
        call = lambda: e.topology(max_shells=64, max_rounds=32)
        r = timed(call, 5, 1)
        r["kernels"] = kernels_of(e, call)
        info = call()[0]
        r["rounds"], r["n_shells"], r["status_nonzero"] = sorted(set(int(x) for x in info["rounds"])), sorted(set(int(x) for x in info["n_shells"])), int((info["status"] != 0).sum())
        used = int(info["rounds"].max())
        r["max_rounds_as_used"] = timed(lambda: e.topology(max_shells=64, max_rounds=used), 5, 1)
        t0 = time.perf_counter()
        o = O.topology(v, faces)
        r["oracle_one_humerus_ms"] = (time.perf_counter() - t0) * 1e3
        r["oracle_rounds"] = int(o["info"]["rounds"])
        out[tag] = r
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
