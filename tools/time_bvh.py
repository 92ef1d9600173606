#!/usr/bin/env python3
"""Timing of the face hierarchy (sh_mesh_bvh, sh_set_query_accel) against the brute-force closest-point walk on the same inputs, in the
same process, interleaved, in the manner of tools/time_geodesic.py.  The batch is the bench batch (64 similarity copies of
humerus_left); the points of a humerus are vertices of its own copy lifted by up to 2 mm, once in spatial order (ascending along the
bone, then across it) and once shuffled.  One run gives
  (a) the build: the C entry point with a null output, host clock, and its kernels (HIP events inside the library);
  (b) sh_closest_points with null outputs, switch off and on alternately, for 64 x 4 096 points in both orders, Q = 4 and Q = 262 144;
      median and span, and the two walk kernels by HIP events;
  (c) nine ICP evaluations (sh_register_points, max_iter 8) on 64 x 4 096 points, off and on;
  (d) with --highres the 2 076 160-triangle humerus of tests/test_gpu_highres.py alone: its build, and 4 096 points off and on;
  (e) with --counts the nodes popped and faces tested per point, from the host twin of the walk (tests/hostcheck/bvh_check.cpp runs the
      function the kernel runs, so the counts are the device's) on humerus_left and 4 096 points.
--quick: (b) for 64 x 4 096 alone -- what a lab build with another LEAF x WIDTH is asked (compile shoulder_hip.hip with
-DSH_BVH_LEAF=.. -DSH_BVH_WIDTH=.. and name the library in SHOULDER_LIB).  One JSON line."""
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
BUILD_KERNELS = ("k_bvh_class", "k_bvh_key", "k_bvh_emit", "k_bvh_leaves", "k_bvh_level")
WALK_KERNELS = ("k_cp_walk", "k_cp_tree", "k_cp_join")


def stats(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)), runs=len(t))


def interleaved(e, call, runs, warm=1):
    """call() with the switch off and on alternately -> {"off": .., "bvh": .., "ratio": off / bvh of the medians}"""
    t = {"off": [], "bvh": []}
    for i in range(warm + runs):
        for mode in ("off", "bvh"):
            e.query_accel = mode
            t0 = time.perf_counter()
            call()
            if i >= warm:
                t[mode].append((time.perf_counter() - t0) * 1e3)
    e.query_accel = "off"
    out = {m: stats(v) for m, v in t.items()}
    out["ratio"] = out["off"]["median_ms"] / out["bvh"]["median_ms"]
    return out


def kernels_of(e, call, names):
    e.enable_timing(1)
    e.reset_timers()
    call()
    out = {}
    for k in names:
        ms, n = e.kernel_time_ms(k)
        if n:
            out[k] = dict(avg_ms=ms, launches=n)
    e.enable_timing(0)
    return out


def points_about(verts, Q, seed, ordered):
    """Q points per mesh: vertices of the mesh lifted by up to 2 mm; ordered: ascending along the longest axis of the mesh in slabs of
    4 mm and across it within a slab, else shuffled.  verts: (B, V, 3) -> (B, Q, 3) float64"""
    rng = np.random.default_rng(seed)
    out = np.empty((len(verts), Q, 3))
    for b, v in enumerate(verts):
        p = v[rng.integers(0, len(v), Q)].astype(np.float64) + rng.uniform(-2.0, 2.0, size=(Q, 3))
        if ordered:
            ax = int(np.argmax(p.max(axis=0) - p.min(axis=0)))
            other = [k for k in range(3) if k != ax]
            p = p[np.lexsort((p[:, other[1]], p[:, other[0]], np.floor(p[:, ax] / 4.0)))]
        out[b] = p
    return out


def closest_call(e, pts):
    p = np.ascontiguousarray(pts, np.float64)
    Q, per = p.shape[-2], int(p.ndim == 3)
    return lambda: e._chk(e.L.sh_closest_points(e.h, p.ctypes.data, Q, per, None))


def time_build(e, runs=5):
    call = lambda: e._chk(e.L.sh_mesh_bvh(e.h, None))      # noqa: E731
    call()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(host=stats(t), kernels=kernels_of(e, call, BUILD_KERNELS))


def walk_entry(e, pts, runs):
    call = closest_call(e, pts)
    r = interleaved(e, call, runs)
    for mode in ("off", "bvh"):
        e.query_accel = mode
        r[mode]["kernels"] = kernels_of(e, call, WALK_KERNELS)
    e.query_accel = "off"
    if pts.shape[-2] <= 4096:      # (and the contract, once per shape: the same bytes in both modes)
        rec = {}
        for mode in ("off", "bvh"):
            e.query_accel = mode
            call()
            rec[mode] = e.fetch("cp.out", np.uint8).tobytes()
        e.query_accel = "off"
        r["same_bytes"] = rec["off"] == rec["bvh"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 x 4 096 points in both orders only")
    ap.add_argument("--highres", action="store_true", help="also the 2 076 160-triangle humerus alone")
    ap.add_argument("--counts", action="store_true", help="also nodes and faces per point from the host twin (needs g++)")
    ap.add_argument("--no-device", action="store_true", help="nothing that needs a GPU: with --counts, the counts alone")
    args = ap.parse_args()
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    out = dict(B=B, faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    if not args.no_device:
        device_part(args, v, f, out)
    if args.counts:
        import tempfile
        import bvh_oracle as O
        with tempfile.TemporaryDirectory() as tmp:
            S = O.build_shim(tmp)
            index = O.host_build(S, v, f)
            pts = points_about(v[None], 4096, 1, False)[0]
            _, c = O.host_walk(S, v, f, index, pts)
        out["per_point_humerus_left"] = dict(nodes_mean=float(c[:, 0].mean()), nodes_max=int(c[:, 0].max()), faces_mean=float(c[:, 1].mean()),
                                             faces_max=int(c[:, 1].max()), loose=int(c[0, 2]), deepest_stack=int(c[:, 3].max()), leaf=O.LEAF, width=O.WIDTH)
    print(json.dumps(out))


def device_part(args, v, f, out):
    e = Engine(0)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    verts = e.fetch("verts", np.float32, (B, len(v), 3))
    out["build_64"] = time_build(e)
    info = e.fetch("bvh.info", _lib.BVH_INFO_DTYPE, (B,))
    out["index_64"] = dict(tight=[int(info["tight"].min()), int(info["tight"].max())], loose=[int(info["loose"].min()), int(info["loose"].max())],
                           levels=int(info["levels"].max()), nodes=int(info["nodes"].max()))
    for name, ordered in (("ordered", True), ("shuffled", False)):
        out["Q4096_" + name] = walk_entry(e, points_about(verts, 4096, 1, ordered), 7)
    if not args.quick:
        out["Q4_shuffled"] = walk_entry(e, points_about(verts, 4, 2, False), 7)
        out["Q262144_ordered"] = walk_entry(e, points_about(verts, 262144, 3, True), 3)
        pts = points_about(verts, 4096, 4, False)
        opt = _lib.IcpOptions(_lib.ICP_PLANE, 8, float("inf"), 0.0)
        p = np.ascontiguousarray(pts)
        icp = lambda: e._chk(e.L.sh_register_points(e.h, p.ctypes.data, 4096, 1, None, ctypes.byref(opt), None, None))      # noqa: E731
        out["icp_9_evaluations_Q4096"] = interleaved(e, icp, 5)
    if args.highres:
        from test_gpu_highres import subdivide
        v3, f3 = subdivide(*subdivide(*subdivide(v, f)))
        e.upload([(v3, f3)])
        out["highres"] = dict(faces=int(len(f3)), build=time_build(e, runs=3))
        i3 = e.fetch("bvh.info", _lib.BVH_INFO_DTYPE, (1,))[0]
        out["highres"]["index"] = dict(tight=int(i3["tight"]), loose=int(i3["loose"]), levels=int(i3["levels"]), nodes=int(i3["nodes"]))
        for name, ordered in (("ordered", True), ("shuffled", False)):
            out["highres"]["Q4096_" + name] = walk_entry(e, points_about(v3[None], 4096, 5, ordered)[0], 5)
    e.close()


if __name__ == "__main__":
    main()
