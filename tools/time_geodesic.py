#!/usr/bin/env python3
"""Timing of the geodesics on the bench batch (64 similarity copies of humerus_left), in the manner of tools/time_vertex_fields.py.  One
run gives, for K = 1 (from the topmost vertex) and K = 4 (top, bottom and two more) in both modes (the topology is resident before the
clock starts):
  (a) the C entry point with null outputs: the device pass without the copies back; host clock, median and span of 5 after 1 warm-up;
  (b) the kernels of one call (HIP events inside the library: sh_enable_timing; averages per launch);
  (c) with --general the same through the lab entry point with the threshold between the two paths at 0, so that the batch takes the
      general path: what the LDS residency buys;
  (d) beside them SciPy's Dijkstra of the oracle (tests/geo_oracle.py) for ONE humerus and one set.
One JSON line."""
import argparse
import ctypes
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

B = 64
KERNELS = ("k_geo_face", "k_geo_init", "k_geo_seed", "k_geo_lds", "k_geo_round", "k_geo_root", "k_geo_pred", "k_geo_jump", "k_geo_info")


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--general", action="store_true", help="also time the batch down the general path (lab entry point, threshold 0)")
    args = ap.parse_args()
    import geo_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    e.topology()
    top, bot = O.topmost(v), O.bottommost(v)
    others = [int(np.argmax(v[:, 0])), int(np.argmin(v[:, 0]))]
    lab = e.L.sh_lab_geodesic
    lab.argtypes, lab.restype = [ctypes.c_void_p, ctypes.c_int] + _lib.SIGNATURES["sh_geodesic"][0][1:], ctypes.c_int
    out = dict(B=B, faces=int(len(f)), vertices=int(len(v)))
    for K, verts in ((1, [top]), (4, [top, bot] + others)):
        off = np.arange(B * K + 1, dtype=np.int32)
        src = np.ascontiguousarray(np.tile(np.array(verts, np.int32), B))
        for mode in (O.EDGES, O.UNFOLD):
            def call(lds=None):
                tail = (int(mode), K, float("inf"), off.ctypes.data, src.ctypes.data, None, None, None, None, None)
                e._chk(e.L.sh_geodesic(e.h, *tail) if lds is None else lab(e.h, lds, *tail))
            r = dict(device_only=timed(call, 5, 1), kernels=kernels_of(e, call))
            info = e.fetch("geo.info", _lib.GEO_INFO_DTYPE, (B, K))
            r["sweeps"] = [int(info["sweeps"].min()), int(info["sweeps"].max())]
            r["reached_all"] = bool((info["reached"] == len(v)).all())
            if args.general:
                r["general"] = dict(device_only=timed(lambda: call(0), 3, 1), kernels=kernels_of(e, lambda: call(0)))
                r["general"]["sweeps_max"] = int(e.fetch("geo.info", _lib.GEO_INFO_DTYPE, (B, K))["sweeps"].max())
            out[f"K{K}_{O.MODES[mode]}"] = r
    e.close()
    for mode in (O.EDGES, O.UNFOLD):
        g = O.graph(v, f, mode)
        t, h, w = g["arcs"]
        t0 = time.perf_counter()
        O.by_dijkstra(len(v), t, h, w, np.array([top]), np.zeros(1))
        out[f"scipy_dijkstra_one_humerus_{O.MODES[mode]}_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
