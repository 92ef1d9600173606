#!/usr/bin/env python3
"""Timing of the general ray cast on the bench batch (64 similarity copies of humerus_left, R = 256 rays shared by all humeri, cap 16),
in the manner of tools/time_stem.py.  One run gives:
  (a) Engine.ray_cast(origins, directions, cap=16): host clock around the synchronous call, median of 10 after 2 warm-ups, and the
      kernels of it alone (HIP events inside the library: sh_enable_timing);
  (b) Engine.canal_profile with L x A = 4 x 64 = 256 rays per humerus on the same batch -- the parent's device ray caster, which culls
      faces by level and angle before the full test, where the general caster has no grid to cull by;
  (c) the NumPy statement of tests/ray_oracle.py on the fetched meshes -- the only way to every hit on a build without the call --
      on N_HUMERI humeri x N_RAYS rays, EXTRAPOLATED to 64 x 256.
The rays start at the mean of the first humerus' vertices and at points 400 mm outside it, aimed at jittered vertices: each copy of
the batch sees them from somewhere else, so hits and misses are mixed.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shoulder_amd import _lib, synth, unet_spec      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

B, R, CAP, RUNS, WARM, N_HUMERI, N_RAYS = 64, 256, 16, 10, 2, 2, 16
KERNELS = ("k_ray_count", "k_ray_scan", "k_ray_fill", "k_ray_sort", "k_canal_clear", "k_canal_rays", "k_canal_levels")


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
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.set_params(unet_dtype=_lib.UNET_BF16)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    e.run(_lib.STAGE_ALL)
    verts = e.fetch("verts", np.float32).reshape(-1, 3)
    voff = np.asarray(e.voff)
    v0 = verts[voff[0]:voff[1]].astype(np.float64)
    rng = np.random.default_rng(7)
    c = v0.mean(axis=0)
    D = rng.normal(size=(R // 2, 3))
    org = c + 400.0 * D / np.linalg.norm(D, axis=1, keepdims=True)
    tgt = v0[rng.integers(0, len(v0), R // 2)] + rng.normal(size=(R // 2, 3))
    o = np.concatenate([np.broadcast_to(c, (R // 2, 3)), org])
    d = np.concatenate([rng.normal(size=(R // 2, 3)), tgt - org])
    out = dict(B=B, R=R, cap=CAP, faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    out["a_ray_cast_R256_cap16"] = timed(lambda: e.ray_cast(o, d, cap=CAP))
    hits, counts = e.ray_cast(o, d, cap=CAP)
    out["hits_total"], out["count_max"], out["rays_with_a_hit_share"] = int(counts.sum()), int(counts.max()), float((counts > 0).mean())
    out["b_canal_profile_L4_A64"] = timed(lambda: e.canal_profile(40.0, 10.0, 4, 64, fetch=("near", "far")))
    e.enable_timing(1)
    e.reset_timers()
    for _ in range(RUNS):
        e.ray_cast(o, d, cap=CAP)
        e.canal_profile(40.0, 10.0, 4, 64, fetch=("near", "far"))
    for k in KERNELS:
        out["%s_ms" % k] = e.kernel_time_ms(k)[0]
    e.enable_timing(0)
    out["ratio_ray_cast_to_canal_profile"] = out["a_ray_cast_R256_cap16"]["median_ms"] / out["b_canal_profile_L4_A64"]["median_ms"]
    import ray_oracle as O

    def numpy_rows():
        for b in range(N_HUMERI):
            vb = verts[voff[b]:voff[b + 1]]
            O.cast(vb, f, o[:N_RAYS], d[:N_RAYS], CAP)
    t = timed(numpy_rows, runs=3, warm=1)
    out["c_numpy_%d_humeri_%d_rays" % (N_HUMERI, N_RAYS)] = t
    out["c_extrapolated_ms_for_%d_rays" % (B * R)] = t["median_ms"] / (N_HUMERI * N_RAYS) * B * R
    want, wn = O.cast(verts[voff[0]:voff[1]], f, o[:N_RAYS], d[:N_RAYS], CAP)
    out["agrees_with_numpy_on_the_timed_rows"] = bool(np.array_equal(wn, counts[0, :N_RAYS]) and np.array_equal(want["face"], hits[0, :N_RAYS]["face"])
                                                      and np.abs(want["t"] - hits[0, :N_RAYS]["t"]).max() <= 1e-6)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
