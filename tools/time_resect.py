#!/usr/bin/env python3
"""Timing of the batched head resection on the bench batch (64 similarity copies of humerus_left, landmarks resident).
  python tools/time_resect.py new      (a) Engine.resect(offsets=<27-grid>), (d) the same with P = 1, (c) Engine.run() for scale, and the
                                       face pass alone (HIP events inside the library: sh_enable_timing) with its achieved bytes/s
  python tools/time_resect.py parent   (b) the same 64 x 27 cuts through what the library offered before: Engine.slice_mesh_planes(verts,
                                       faces, origins, normals, edges=True) per humerus with P = 27 plus base.Section for the loops.
                                       Works with a build that lacks sh_resect_* (SHOULDER_LIB=<the parent commit's library>); the
                                       planes are made on the host from the run's records (not timed).
Every call is synchronous (it returns host data), so a call is timed on the host clock around it: 10 runs after 2 warm-ups, one
JSON line.  Interleave the two modes A/B on one box as tools/probes/lib_ab.sh does."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.osteotomy import OracleOsteotomy      # noqa: E402
from shoulder_amd import _lib, synth, unet_spec      # noqa: E402
from shoulder_amd.base import Section      # noqa: E402
from shoulder_amd.engine import Engine      # noqa: E402
from shoulder_amd.stl import load_stl      # noqa: E402

GRID27 = [dict(retroversion_deg=r, neckshaft_deg=n, depth_canal_mm=d) for r in (-10.0, 0.0, 10.0) for n in (-10.0, 0.0, 10.0) for d in (-6.0, 0.0, 6.0)]
B, RUNS, WARM = 64, 10, 2


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
    out = dict(mode=mode, B=B, P=len(GRID27), faces=int(len(f)), lib=os.environ.get("SHOULDER_LIB", "in-tree"))
    if mode == "new":
        out["a_resect_P27"] = timed(lambda: e.resect(offsets=GRID27))
        out["d_resect_P1"] = timed(lambda: e.resect(offsets=GRID27[13:14]))
        out["c_run"] = timed(lambda: e.run(_lib.STAGE_ALL, fetch="view"))
        e.enable_timing(1)
        e.reset_timers()
        for _ in range(RUNS):
            e.resect(offsets=GRID27)
        for k in ("k_resect_faces", "k_resect_join", "k_resect_make_planes"):
            ms, n = e.kernel_time_ms(k)
            out[k + "_ms"] = ms
        e.enable_timing(0)
        # the face pass reads every face (12 B) and its three float32 vertices (36 B gathered) once, writes 32 B per (plane, tile)
        byts = B * (len(f) * 48 + len(GRID27) * ((len(f) + 255) // 256) * 32)
        out["face_pass_GBps"] = byts / (out["k_resect_faces_ms"] * 1e-3) / 1e9
        recs = e.resect(offsets=GRID27)
        out["status_ok"] = bool(np.all(recs["status"] == 0))
        out["volume_mm3_b0_native"] = float(recs[0, 13]["head_volume"])
    else:
        verts = e.fetch("verts", np.float32).reshape(B, len(v), 3).astype(np.float64)
        planes = []
        for b in range(B):
            pl = []
            for g in GRID27:
                O = OracleOsteotomy(lm[b]["csys_articular"], lm[b]["anp_plane_point"], lm[b]["anp_plane_normal"], "right" if lm[b]["side"] == 1 else "left")
                if g["retroversion_deg"]:
                    O.offset_retroversion(g["retroversion_deg"])
                if g["neckshaft_deg"]:
                    O.offest_neckshaft(g["neckshaft_deg"])
                if g["depth_canal_mm"]:
                    O.offset_depth(g["depth_canal_mm"])
                pl.append(np.concatenate(O.plane(np.identity(4))))
            planes.append(np.array(pl))

        def one_at_a_time():
            n = 0
            for b in range(B):
                for (cv, cf, ce), pl in zip(e.slice_mesh_planes(verts[b], f, planes[b][:, :3], planes[b][:, 3:], edges=True), planes[b]):
                    n += len(Section(cv, ce, pl[3:]).discrete)
            return n
        out["b_slice_mesh_planes_plus_section"] = timed(one_at_a_time, runs=3, warm=1)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
