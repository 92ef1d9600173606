"""Join-kernel times of the open-contour modes on the bench batch (64 similarity copies of humerus_left.stl,
seed 1234, bf16 UNet) and on the same batch made from a copy with single-triangle holes:
    python tools/time_open_contours.py [--modes error,bridge] [--reps 10] [--root CHECKOUT]      (on the GPU box)
--root: import the package from another checkout (an A/B against an older commit, mode "error" only there).
One JSON line per (batch, mode): mean ms per run of k_slice_link, k_slice_link_large, k_slice_link_huge over the reps."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from shoulder_amd import _lib, synth, unet_spec
from shoulder_amd.engine import Engine
from shoulder_amd.stl import load_stl

KERNELS = ("k_slice_link", "k_slice_link_large", "k_slice_link_huge")


def holes(v, f, n=12, gap=4.0):
    """isolated single-triangle holes at evenly spaced heights (longest edge < gap, > 4 gap apart)"""
    c = v[f].astype(np.float64).mean(axis=1)
    L = np.linalg.norm(v[f] - v[np.roll(f, -1, axis=1)], axis=2).max(axis=1)
    z0, z1 = c[:, 2].min(), c[:, 2].max()
    taken = []
    for q in np.linspace(0.03, 0.97, n):
        for i in np.argsort(np.abs(c[:, 2] - (z0 + q * (z1 - z0))), kind="stable")[:4000]:
            if L[i] < gap and (not taken or np.min(np.linalg.norm(c[taken] - c[i], axis=1)) > 4 * gap):
                taken.append(int(i)); break
    return np.array(taken)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="error,bridge")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-gap", type=float, default=4.0)
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    v, f = load_stl(os.path.join(ROOT, "tests", "golden", "bones", "humerus_left.stl"))
    eng = Engine(0); eng.load_rfc(); eng.load_unet(unet_spec.make_teacher_weights(), unet_spec.BASE, unet_spec.DEPTH)
    eng.set_params(unet_dtype=_lib.UNET_BF16)
    T = synth.similarity_transforms(64, v, seed=1234)
    for batch, faces in (("watertight", f), ("holed", np.delete(f, holes(v, f), axis=0))):
        eng.upload([(v, faces)]); eng.synth_batch(T)
        for mode in a.modes.split(","):
            if mode == "bridge":
                eng.set_open_contours("bridge", a.max_gap)
            elif hasattr(eng, "set_open_contours"):
                eng.set_open_contours("error")
            status = "ok"
            try:
                eng.run(_lib.STAGE_ALL)
            except Exception as e:
                status = str(e)[:80]
            eng.enable_timing(1); eng.reset_timers()
            for _ in range(a.reps):
                try:
                    eng.run(_lib.STAGE_ALL)
                except Exception:
                    pass
            out = {"batch": batch, "mode": mode, "status": status, "reps": a.reps, "root": ROOT}
            for k in KERNELS:
                ms, n = eng.kernel_time_ms(k)
                out[k + "_ms_per_run"] = round(ms * n / a.reps, 4)
            eng.enable_timing(0)
            print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
