#!/usr/bin/env python3
"""Timing of the canal profile and of the stems below a batched resection on the bench batch (64 similarity copies of humerus_left,
landmarks resident, L = 128 levels of 1.25 mm from 2 mm above the highest entry point of the sweep's cuts, A = 64 rays, the 27-offset grid, K = 16 stems),
in the manner of tools/time_seat.py.
  python tools/time_stem.py new      (a) Engine.canal_profile(...), (b) Engine.resect(offsets=<27-grid>) + Engine.resect_stems(<16>),
                                     (c) Engine.resect(offsets=<27-grid>) alone, (d) the kernels of (a) and (b) alone (HIP events inside
                                     the library: sh_enable_timing), and the bytes k_canal_rays has to move
  python tools/time_stem.py parent   the only way to a profile on a build without it (SHOULDER_LIB=<the parent commit's library>): one
                                     section_plane per level and humerus (Engine.slice_mesh_planes, the call behind Mesh.section /
                                     resect_mesh) plus the NumPy polar statement of tests/stem_oracle.py on the humerus' vertices, on
                                     N_LEVELS levels of N_HUMERI humeri (1 mm apart from z = 40 mm; the cost does not hang on the spacing), EXTRAPOLATED to 64 x 128 levels
Every call is synchronous (it returns host data): host clock around it, median of 10 runs after 2 warm-ups, one JSON line.
Interleave the two modes on one box."""
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
STEMS16 = [(length, r, 0.6 * r) for length in (80.0, 100.0) for r in (4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0)]
B, RUNS, WARM, L, A, N_HUMERI, N_LEVELS = 64, 10, 2, 128, 64, 2, 8
KERNELS = ("k_canal_frames", "k_canal_clear", "k_canal_rays", "k_canal_levels", "k_stem_fit")


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
    mode = sys.argv[1] if len(sys.argv) > 1 else "new"
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    e = Engine(0)
    e.load_rfc()
    e.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    e.set_params(unet_dtype=_lib.UNET_BF16)
    e.upload([(v, f)])
    e.synth_batch(synth.similarity_transforms(B, v, seed=1234))
    lm = e.run(_lib.STAGE_ALL)
    out = dict(mode=mode, B=B, L=L, A=A, P=len(GRID27), K=len(STEMS16), faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    out["c_resect_P27"] = timed(lambda: e.resect(offsets=GRID27))
    if mode == "new":
        recs = e.resect(offsets=GRID27)
        R, t = lm["csys_articular"].reshape(B, 4, 4)[:, :3, :3], lm["csys_articular"].reshape(B, 4, 4)[:, :3, 3]
        o = np.einsum("bij,bpj->bpi", R, recs["plane_point"]) + t[:, None, :]
        n = np.einsum("bij,bpj->bpi", R, recs["plane_normal"])
        ze = o[..., 2] + (o[..., 0] * n[..., 0] + o[..., 1] * n[..., 1]) / n[..., 2]      # where each cut meets its humerus' canal axis
        z0, dz = float(ze.max()) + 2.0, 1.25
        out["grid"] = dict(z0=z0, dz=dz, entry_min=float(ze.min()), entry_max=float(ze.max()))
        out["a_canal_profile_L128_A64"] = timed(lambda: e.canal_profile(z0, dz, L, A))
        out["a_canal_profile_with_rows"] = timed(lambda: e.canal_profile(z0, dz, L, A, fetch=("levels", "near", "far")))

        def stems():
            e.resect(offsets=GRID27)
            return e.resect_stems(STEMS16)
        out["b_resect_plus_stems_P27_K16"] = timed(stems)
        e.enable_timing(1)
        e.reset_timers()
        for _ in range(RUNS):
            e.canal_profile(z0, dz, L, A)
            stems()
        for k in KERNELS:
            out["%s_ms" % k] = e.kernel_time_ms(k)[0]
        e.enable_timing(0)
        lv, near = e.canal_profile(z0, dz, L, A, fetch=("levels", "near"))
        fits = stems()
        # what k_canal_rays has to move: every face index and its three gathered float32 vertices once, one 8-byte atomic pair per hit
        hits = int(2 * np.isfinite(near).sum())
        out["k_canal_rays_min_bytes"] = int(B * len(f) * (12 + 36) + hits * 16)
        out["levels_ok_share"] = float((lv["status"] == 0).mean())
        out["stem_status_counts"] = {str(k): int(n) for k, n in zip(*np.unique(fits["status"], return_counts=True))}
        out["fits_share"] = float(fits["fits"].mean())
    else:
        import stem_oracle as S
        verts = e.fetch("verts", np.float32).reshape(-1, 3)
        voff = np.asarray(e.voff)

        def one_level(b, l):
            T = lm[b]["csys_articular"].reshape(4, 4)
            vb = verts[voff[b]:voff[b + 1]]
            z = 40.0 - l * 1.0
            o, n = S.to_ct(T, [0.0, 0.0, z]), T[2, :3]
            e.slice_mesh_planes(vb.astype(np.float64), f, [o], [n])                  # the section of this level: what Mesh.section sends
            return S.profile(S.map_points(T, vb), f, z, 1.0, 1, A)                   # and the polar rows of it in NumPy
        jobs = [(b, l) for b in range(N_HUMERI) for l in range(0, L, L // (N_LEVELS // N_HUMERI))][:N_LEVELS]
        t = timed(lambda: [one_level(b, l) for b, l in jobs], runs=3, warm=1)
        out["d_section_plus_numpy_%d_levels" % N_LEVELS] = t
        out["d_extrapolated_ms_for_%d_levels" % (B * L)] = t["median_ms"] / N_LEVELS * B * L
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
