"""The host side of the arthroplasty chain (shoulder_amd/csrc/sh_arthro_host.h) on the engine: how many times each kernel is launched
by one call, and that the pass a plane falls into does not change its records.  Nothing here is measured: every count is read off the
entry points' code (one launch per kernel and pass; the pass split of sh_arthro.h resect_plan), and the file passes unchanged on the
library of the commit before the host side moved.

The batches are the prisms of tests/test_gpu_plan.py (5 mm across): its three-prism batch for one seated chain, and 64 copies of the
130-gon prism (520 faces: three tiles of 256) for the sweeps that need more than one pass -- with B = 64 a fitted pass takes
4 096 / 64 = 64 planes and an un-fitted one 8 192 / 64 = 128 (the slabs are far below their 128 MB)."""
import ctypes

import numpy as np
import pytest

import stem_oracle as SO
from test_gpu_plan import HEADS4, RULE, STEMS8, T_TILT, chain, synth_batch

pytestmark = pytest.mark.gpu
TIMERS = ("k_resect_make_planes", "k_resect_faces", "k_headfit_faces", "k_resect_join", "k_resect_join_fit", "k_resect_join_seat", "k_headfit_solve", "k_seat",
          "k_canal_frames", "k_canal_clear", "k_canal_rays", "k_canal_levels", "k_stem_fit", "k_plan_ref", "k_plan_ref_join", "k_plan_terms", "k_plan_select")


def launches(engine):
    return {k: engine.kernel_time_ms(k)[1] for k in TIMERS}


def only(**counts):
    return dict({k: 0 for k in TIMERS}, **counts)


def copies(P, B=64):
    """B copies of the 130-gon prism and P distinct planes through each, tilted a little more from one to the next"""
    mesh = SO.mesh_in_ct(T_TILT, *SO.prism(130, 5.0, -2.5, 2.5, 0.011))
    planes = np.array([np.concatenate([SO.to_ct(T_TILT, [0.0, 0.0, -2.0 + 4.0 * k / (P - 1)]), T_TILT[2, :3] + (0.0005 * k) * T_TILT[0, :3]]) for k in range(P)])
    return [mesh] * B, np.ascontiguousarray(np.broadcast_to(planes, (B, P, 6)))


@pytest.fixture
def timed(engine):
    engine.enable_timing(1)
    try:
        yield engine
    finally:
        engine.enable_timing(0)
        engine.reset_timers()


def test_launches_per_call(timed):
    engine = timed
    meshes, frames, planes, ref_planes = synth_batch()
    engine.upload(meshes)
    engine.reset_timers()
    chain(engine, meshes, frames, planes, HEADS4, STEMS8, upload=False)      # 3 prisms x 4 planes, 4 heads, 8 stems, explicit frames
    engine.plan(8, RULE, ref_planes=ref_planes)
    one_chain = only(k_resect_faces=1, k_headfit_faces=1, k_resect_join_seat=1, k_headfit_solve=1, k_seat=1, k_canal_clear=1, k_canal_rays=1, k_canal_levels=1,
                     k_stem_fit=1, k_plan_ref=1, k_plan_ref_join=1, k_plan_terms=1, k_plan_select=1)
    assert launches(engine) == one_chain
    n = ctypes.c_int()
    engine._chk(engine.L.sh_resect_ring(engine.h, 1, 2, None, 0, ctypes.byref(n)))      # one sh_resect_ring: one cut's face pass and join again
    assert n.value > 1
    assert launches(engine) == dict(one_chain, k_resect_faces=2, k_resect_join=1)
    assert len(engine.resect_ring(1, 2)) == n.value                                     # the engine's: one call for the length, one for the points
    assert launches(engine) == dict(one_chain, k_resect_faces=4, k_resect_join=3)

    meshes, planes = copies(65)
    engine.upload(meshes)
    engine.reset_timers()
    engine.resect(planes=planes, fit=True, heads=HEADS4)                                 # seat level, 65 planes: passes of 64 and 1
    assert launches(engine) == only(k_resect_faces=2, k_headfit_faces=2, k_resect_join_seat=2, k_headfit_solve=2, k_seat=2)
    engine.reset_timers()
    engine.resect(planes=planes, fit=True)                                               # fit level: the same passes, one solve over the batch
    assert launches(engine) == only(k_resect_faces=2, k_headfit_faces=2, k_resect_join_fit=2, k_headfit_solve=1)
    engine.reset_timers()
    engine.resect(planes=copies(129)[1])                                                 # records level, 129 planes: passes of 128 and 1
    assert launches(engine) == only(k_resect_faces=2, k_resect_join=2)


def test_the_pass_of_a_plane_does_not_change_its_records(engine):
    meshes, planes = copies(65)
    engine.upload(meshes)
    rec, fit, seat = engine.resect(planes=planes, fit=True, heads=HEADS4)                # two passes: planes 0..63, plane 64
    assert np.all(rec["status"] == 0) and np.all(rec["n_loops"] >= 1) and np.all(seat["status"] == 0)      # (centroid seats carry the cut's status)
    for sl in (slice(0, 64), slice(64, 65)):                                             # the same planes, each range in a single pass
        r1, f1, s1 = engine.resect(planes=np.ascontiguousarray(planes[:, sl]), fit=True, heads=HEADS4)
        assert np.ascontiguousarray(rec[:, sl]).tobytes() == r1.tobytes()
        assert np.ascontiguousarray(fit[:, sl]).tobytes() == f1.tobytes()
        assert np.ascontiguousarray(seat[:, sl]).tobytes() == s1.tobytes()
    assert rec[0].tobytes() == rec[63].tobytes()                                          # (and a copy's records do not depend on its place in the batch)
