#!/usr/bin/env python3
"""Timing of the rays through the face hierarchy (sh_ray_cast with SH_ACCEL_BVH, sh_ray_nearest) against the walk over all faces on the
same inputs, in the same process, interleaved, in the manner of tools/time_bvh.py.  The batch is the bench batch (64 similarity copies
of humerus_left); the rays of a humerus are the thickness workload: origins are surface samples of its own copy moved 1e-3 mm inwards,
directions the inward unit normals of their faces -- in sample order (independent draws: spatially random), shuffled, and sorted along
the bone.  One run gives, for R in {4, 256, 4 096} rays per humerus,
  (a) sh_ray_cast (cap = 8, null outputs) with the switch off and on alternately: median and span, and the kernels by HIP events;
  (b) sh_ray_nearest with the switch on against sh_ray_cast(cap = 1) with the switch off (the parent's way to the nearest hit), and
      sh_ray_nearest with the switch off;
  (c) the contract once per shape: "ray.hits", "ray.counts" and "ray.near" are the same bytes in both modes;
  (d) with --highres the 2 076 160-triangle humerus of tests/test_gpu_highres.py alone, the same;
  (e) with --counts the nodes popped and faces tested per ray, all hits and nearest, from the host twin (tests/hostcheck/raytree_check.cpp
      runs the function the kernels run, so the counts are the device's) on humerus_left and 4 096 rays.
A call that takes long is repeated less often (at least twice).  One JSON line."""
import argparse
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
KERNELS = ("k_ray_count", "k_ray_fill", "k_ray_tree", "k_ray_near", "k_ray_scan", "k_ray_sort")


def stats(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)), runs=len(t))


def alternately(e, calls, budget_s=12.0):
    """calls: name -> (mode, call).  Every call once to warm up and to see what it costs, then all of them alternately"""
    cost = {}
    for name, (mode, call) in calls.items():
        e.query_accel = mode
        t0 = time.perf_counter()
        call()
        cost[name] = time.perf_counter() - t0
    runs = int(min(7, max(2, budget_s / max(sum(cost.values()), 1e-9))))
    t = {name: [] for name in calls}
    for _ in range(runs):
        for name, (mode, call) in calls.items():
            e.query_accel = mode
            t0 = time.perf_counter()
            call()
            t[name].append((time.perf_counter() - t0) * 1e3)
    e.query_accel = "off"
    return {name: stats(v) for name, v in t.items()}


def kernels_of(e, mode, call):
    e.query_accel = mode
    e.enable_timing(1)
    e.reset_timers()
    call()
    out = {}
    for k in KERNELS:
        ms, n = e.kernel_time_ms(k)
        if n:
            out[k] = dict(avg_ms=ms, launches=n)
    e.enable_timing(0)
    e.query_accel = "off"
    return out


def thickness_rays(e, verts, faces, R, seed, order):
    """(B, R) rays of _lib.RAY_DTYPE: surface samples of every resident mesh and the inward normals of their faces"""
    rec, info = e.sample_surface(R, seed=seed)
    assert not info["status"].any()
    rays = np.zeros((len(verts), R), dtype=_lib.RAY_DTYPE)
    rng = np.random.default_rng(seed)
    for b, v in enumerate(verts):
        v = v.astype(np.float64)
        fc = faces[rec[b]["face"]]
        n = np.cross(v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        o, d = rec[b]["point"] - 1e-3 * n, -n
        if order == "shuffled":
            perm = rng.permutation(R)
        elif order == "sorted":
            ax = int(np.argmax(o.max(axis=0) - o.min(axis=0)))
            other = [k for k in range(3) if k != ax]
            perm = np.lexsort((o[:, other[1]], o[:, other[0]], np.floor(o[:, ax] / 4.0)))
        else:
            perm = np.arange(R)
        rays[b]["origin"], rays[b]["dir"] = o[perm], d[perm]
    return rays


def entry(e, rays):
    R = rays.shape[1]
    cast8 = lambda: e._chk(e.L.sh_ray_cast(e.h, rays.ctypes.data, R, 1, 8, None, None))      # noqa: E731
    cast1 = lambda: e._chk(e.L.sh_ray_cast(e.h, rays.ctypes.data, R, 1, 1, None, None))      # noqa: E731
    near = lambda: e._chk(e.L.sh_ray_nearest(e.h, rays.ctypes.data, R, 1, None))             # noqa: E731
    r = alternately(e, {"cast8_off": ("off", cast8), "cast8_bvh": ("bvh", cast8), "cast1_off": ("off", cast1), "nearest_off": ("off", near),
                        "nearest_bvh": ("bvh", near)})
    r["cast8_ratio"] = r["cast8_off"]["median_ms"] / r["cast8_bvh"]["median_ms"]
    r["nearest_ratio"] = r["cast1_off"]["median_ms"] / r["nearest_bvh"]["median_ms"]
    r["kernels"] = {"cast8_off": kernels_of(e, "off", cast8), "cast8_bvh": kernels_of(e, "bvh", cast8), "nearest_bvh": kernels_of(e, "bvh", near)}
    got = {}
    for mode in ("off", "bvh"):
        e.query_accel = mode
        cast8()
        got[mode] = [e.fetch(n, np.uint8).tobytes() for n in ("ray.hits", "ray.counts")]      # (before the nearest: with the switch off it rewrites both at cap = 1)
        near()
        got[mode].append(e.fetch("ray.near", np.uint8).tobytes())
    e.query_accel = "off"
    r["same_bytes"] = got["off"] == got["bvh"]
    cnt = e.fetch("ray.counts", np.int32)
    r["hits_per_ray"] = float(cnt.mean())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="R = 256 in sample order only")
    ap.add_argument("--highres", action="store_true", help="also the 2 076 160-triangle humerus alone")
    ap.add_argument("--counts", action="store_true", help="also nodes and faces per ray from the host twin (needs g++)")
    ap.add_argument("--no-device", action="store_true", help="nothing that needs a GPU: with --counts, the counts alone")
    args = ap.parse_args()
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    out = dict(B=B, faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    if not args.no_device:
        e = Engine(0)
        e.upload([(v, f)])
        e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
        verts = e.fetch("verts", np.float32, (B, len(v), 3))
        shapes = [(256, "sample")] if args.quick else [(4, "sample"), (256, "sample"), (256, "shuffled"), (256, "sorted"), (4096, "sample"), (4096, "sorted")]
        for R, order in shapes:
            out[f"R{R}_{order}"] = entry(e, thickness_rays(e, verts, f, R, 1, order))
            print(f"R{R}_{order}", json.dumps(out[f"R{R}_{order}"]), file=sys.stderr, flush=True)
        if args.highres:
            from test_gpu_highres import subdivide
            v3, f3 = subdivide(*subdivide(*subdivide(v, f)))
            e.upload([(v3, f3)])
            info = e.build_bvh()[0]
            out["highres"] = dict(faces=int(len(f3)), tight=int(info["tight"]), loose=int(info["loose"]), levels=int(info["levels"]))
            for R, order in [(4, "sample"), (256, "sample"), (4096, "sample"), (4096, "sorted")]:
                out["highres"][f"R{R}_{order}"] = entry(e, thickness_rays(e, v3[None], f3, R, 2, order))
                print(f"highres R{R}_{order}", json.dumps(out["highres"][f"R{R}_{order}"]), file=sys.stderr, flush=True)
        e.close()
    if args.counts:
        import tempfile
        import bvh_oracle as BO
        import raytree_oracle as RT
        with tempfile.TemporaryDirectory() as tmp:
            S = RT.build_shim(tmp)
            index = BO.host_build(S, v, f)
            rng = np.random.default_rng(1)
            fc = f[rng.integers(0, len(f), 4096)]
            v64 = v.astype(np.float64)
            n = np.cross(v64[fc[:, 1]] - v64[fc[:, 0]], v64[fc[:, 2]] - v64[fc[:, 0]])
            ok = np.linalg.norm(n, axis=1) > 0
            n, fc = n[ok] / np.linalg.norm(n[ok], axis=1, keepdims=True), fc[ok]
            p = v64[fc].mean(axis=1)                                   # (face centroids: the twin has no sampler)
            _, counts, tot = RT.host_cast(S, v, f, index, p - 1e-3 * n, -n, 8)
            _, ntot = RT.host_near(S, v, f, index, p - 1e-3 * n, -n)
            R = len(p)
        out["per_ray_humerus_left"] = dict(rays=R, tight=int(index["off"][0]), loose=int(index["off"][1]), hits_mean=float(counts.mean()),
                                           all_hits=dict(nodes_mean=tot[0] / R, faces_mean=tot[1] / R, deepest_stack=int(tot[3])),
                                           nearest=dict(nodes_mean=ntot[0] / R, faces_mean=ntot[1] / R, deepest_stack=int(ntot[3])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
