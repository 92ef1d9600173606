#!/usr/bin/env python3
"""Timing of the implant plans on the bench batch (64 similarity copies of humerus_left, landmarks resident, the 27-offset grid, 16
heads, 16 stems, N = 8), in the manner of tools/time_stem.py.  The profile grid starts 2 mm above the HIGHEST entry point of the
sweep's cuts and reaches below the longest stem of the lowest one, so that the stems are really fitted.
  (a) Engine.plan(8, rule) on the resident seats and stems: host clock around the synchronous call
  (b) the only way a build without it has: the vectorised NumPy ranking of tests/plan_oracle.py on the ALREADY FETCHED records of the
      same batch (the fetch itself is not counted)
  (c) the four kernels of (a) alone (HIP events inside the library: sh_enable_timing)
  (d) the share of candidates that are feasible, so that (a) is not the figure of an early-out path
Median of 10 runs after 2 warm-ups ((b): 3 after 1), one JSON line."""
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

GRID27 = [dict(retroversion_deg=r, neckshaft_deg=n, depth_canal_mm=d) for r in (-10.0, 0.0, 10.0) for n in (-10.0, 0.0, 10.0) for d in (-6.0, 0.0, 6.0)]
HEADS16 = [(r, h) for r in (20.0, 22.0, 24.0, 26.0) for h in (14.0, 16.0, 18.0, 20.0)]
STEMS16 = [(length, r, 0.6 * r) for length in (80.0, 100.0) for r in (4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0)]
RULE = dict(max_overhang=6.0, min_clearance=0.0, margin=2.0, fill_target=0.6, w_uncovered=10.0, w_overhang=1.0, w_cor=0.5, w_height=0.25,
            w_eccentricity=0.2, w_fill=3.0)
B, RUNS, WARM, A, N = 64, 10, 2, 64, 8
KERNELS = ("k_plan_ref", "k_plan_ref_join", "k_plan_terms", "k_plan_select")


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
    import plan_oracle as O
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.set_params(unet_dtype=_lib.UNET_BF16)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    lm = e.run(_lib.STAGE_ALL)
    out = dict(B=B, P=len(GRID27), K_h=len(HEADS16), K_s=len(STEMS16), N=N, vertices=int(len(v)))
    rec, fit, seat = e.resect(offsets=GRID27, fit=True, heads=HEADS16)
    T = lm["csys_articular"].reshape(B, 4, 4)
    o = np.einsum("bij,bpj->bpi", T[:, :3, :3], rec["plane_point"]) + T[:, None, :3, 3]
    n = np.einsum("bij,bpj->bpi", T[:, :3, :3], rec["plane_normal"])
    ze = o[..., 2] + (o[..., 0] * n[..., 0] + o[..., 1] * n[..., 1]) / n[..., 2]      # where each cut meets its humerus' canal axis
    z0, dz = float(ze.max()) + 2.0, 1.25
    L = int(np.ceil((z0 - (float(ze.min()) - max(s[0] for s in STEMS16))) / dz)) + 2
    out["grid"] = dict(z0=z0, dz=dz, L=L, entry_min=float(ze.min()), entry_max=float(ze.max()))
    e.canal_profile(z0, dz, L, A)
    stems = e.resect_stems(STEMS16)
    out["stem_status_counts"] = {str(k): int(c) for k, c in zip(*np.unique(stems["status"], return_counts=True))}
    out["stems_fit_share"] = float(stems["fits"].mean())
    out["a_engine_plan"] = timed(lambda: e.plan(N, RULE))
    plans, refs = e.plan(N, RULE)
    out["d_feasible_share"] = float(refs["n_feasible"].sum()) / (B * len(GRID27) * len(HEADS16) * len(STEMS16))
    out["humeri_with_a_plan"] = int((plans[:, 0]["status"] == 0).sum())
    heads = np.asarray(HEADS16)
    r = O.rule(**RULE)

    def numpy_ranking():
        return [O.plans(r, rec[b], fit[b], seat[b], stems[b], heads, T[b], refs[b], None, N) for b in range(B)]
    out["b_numpy_ranking_of_fetched_records"] = timed(numpy_ranking, runs=3, warm=1)
    want = numpy_ranking()
    out["numpy_agrees"] = bool(all(np.array_equal(w[0][k], plans[b][k]) for b, w in enumerate(want) for k in ("cut", "head", "stem", "status"))
                               and all(w[1] == refs[b]["n_feasible"] for b, w in enumerate(want)))
    e.enable_timing(1)
    e.reset_timers()
    for _ in range(RUNS):
        e.plan(N, RULE)
    for k in KERNELS:
        out["%s_ms" % k] = e.kernel_time_ms(k)[0]
    e.enable_timing(0)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
