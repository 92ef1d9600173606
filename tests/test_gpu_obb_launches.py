"""The OBB stage (run_obb of shoulder_amd/csrc/shoulder_hip.hip: obb_hulls -> obb_plan -> obb_candidates -> obb_frame) on the engine:
how many times one run launches each of its kernels, with the hulls from the host and from the device, and with the pruning bound
off.  Nothing here is measured: every count is read off the stage's code (one fill, one face-area and one bounds launch, two passes
of select + candidates of which the first is timed as "k_obb_seed", one pick, and for a whole humerus the two end-section kernels),
and the file passes unchanged on the library of the commit before the stage was split into its steps.

Two fixture humeri, so every grid has one row of eight and the small tier of k_obb_candidates (2 732 hull faces)."""
import numpy as np
import pytest

from conftest import engine_with_env
from shoulder_amd import _lib

pytestmark = pytest.mark.gpu
OBB = ("k_obb_face_area2", "k_obb_bounds", "k_obb_select", "k_obb_seed", "k_obb_candidates", "k_obb_pick", "k_obb_end_points", "k_obb_ends")
TIMERS = OBB + ("k_hull_rounds", "k_hull_flag")
ONE_RUN = dict(k_obb_face_area2=1, k_obb_bounds=1, k_obb_select=2, k_obb_seed=1, k_obb_candidates=1, k_obb_pick=1, k_obb_end_points=1, k_obb_ends=1)


def census(e, meshes, mode):
    """one run of all stages on `meshes` with the hulls from `mode` -> (launches per kernel, records)"""
    before = e.hull_mode
    e.reset_params()      # (the session's engine: a whole humerus, whatever the test before left)
    e.set_hull_mode(mode)
    e.enable_timing(1)
    try:
        e.upload(meshes)
        e.reset_timers()
        rec = e.run(_lib.STAGE_ALL)
        return {k: e.kernel_time_ms(k)[1] for k in TIMERS}, rec
    finally:
        e.enable_timing(0)
        e.reset_timers()
        e.set_hull_mode(before)


@pytest.fixture(scope="module")
def two_humeri(oracle_bones):
    return [(b.verts, b.faces) for b in (oracle_bones("humerus_left"), oracle_bones("humerus_right"))]


def test_launches_with_host_hulls(engine, two_humeri):
    n, rec = census(engine, two_humeri, "host")
    assert n == dict(ONE_RUN, k_hull_rounds=0, k_hull_flag=0)
    assert np.all(rec["status"] == 0)


def test_launches_with_device_hulls(engine, two_humeri):
    n, rec = census(engine, two_humeri, "device")
    assert n == dict(ONE_RUN, k_hull_rounds=1, k_hull_flag=1)
    assert np.all(rec["status"] == 0)


def test_launches_and_records_without_the_pruning_bound(two_humeri):
    """two engines of their own (the switch is the context's, read when it is created), alike in everything else"""
    with engine_with_env() as e_pruned:
        n_pruned, rec_pruned = census(e_pruned, two_humeri, "host")
    with engine_with_env(SHOULDER_OBB_PRUNE=0) as e_all:
        n_all, rec_all = census(e_all, two_humeri, "host")
    assert n_all == n_pruned == dict(ONE_RUN, k_hull_rounds=0, k_hull_flag=0)
    assert rec_all.tobytes() == rec_pruned.tobytes()
