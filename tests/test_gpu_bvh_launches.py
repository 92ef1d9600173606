"""Which kernels the closest-point step launches with the switch of sh_set_query_accel on and off, and that a run launches what it
launched before the hierarchy existed.  Nothing here is measured: the counts are read off sh_query_host.h (one k_cp_tree or one
k_cp_walk and one k_cp_join per call; a build is class, key, emit, leaves and a k_bvh_level per level above the leaves that the largest
mesh could have), and the names of a run's kernels are every name the library launches under (the LAUNCH statements of its sources)."""
import glob
import os
import re

import numpy as np
import pytest

import bvh_oracle as B
from conftest import ROOT
from shoulder_amd import _lib
from test_bvh_host import bone

pytestmark = pytest.mark.gpu
NEW = ("k_bvh_class", "k_bvh_key", "k_bvh_emit", "k_bvh_leaves", "k_bvh_level", "k_cp_tree")


def launch_names():
    """every name a launch of the library is timed under: the string literal of each LAUNCH / LAUNCH_FN statement"""
    names = set()
    for path in glob.glob(os.path.join(ROOT, "shoulder_amd", "csrc", "*")):
        names.update(re.findall(r"\bLAUNCH(?:_FN)?\(\s*\w+\s*,\s*\"([^\"]+)\"", open(path).read()))
    return sorted(names)


@pytest.fixture
def timed(engine):
    engine.enable_timing(1)
    try:
        yield engine
    finally:
        engine.enable_timing(0)
        engine.reset_timers()
        engine.query_accel = "off"


def counts(engine, names):
    return {k: engine.kernel_time_ms(k)[1] for k in names if engine.kernel_time_ms(k)[1]}


def test_launches_of_the_closest_point_step(timed):
    engine = timed
    names = launch_names()
    assert set(NEW) <= set(names) and "k_cp_walk" in names and len(names) > 100
    v, f = bone("humerus_left")
    pts = v[:300].astype(np.float64) + (0.0, 0.25, 0.5)
    engine.upload([(v, f)])
    levels = B.levels_of(len(f))                                                        # were every face tight: what the host launches for
    build = dict(k_bvh_class=1, k_bvh_key=1, k_bvh_emit=1, k_bvh_leaves=1, k_bvh_level=levels - 1)
    engine.reset_timers()
    engine.query_accel = "off"
    want = engine.closest_points(pts)
    assert counts(engine, names) == dict(k_cp_walk=1, k_cp_join=1)                      # off: the walk over all faces, no k_bvh_* kernel
    engine.reset_timers()
    engine.query_accel = "bvh"
    got = engine.closest_points(pts)
    assert counts(engine, names) == dict(build, k_cp_tree=1, k_cp_join=1)               # the first call builds the index; k_cp_walk not at all
    engine.reset_timers()
    assert engine.closest_points(pts).tobytes() == got.tobytes() == want.tobytes()
    assert counts(engine, names) == dict(k_cp_tree=1, k_cp_join=1)                      # the index is resident
    engine.reset_timers()
    engine.build_bvh()
    assert counts(engine, names) == build
    engine.reset_timers()
    engine.register(pts, max_iter=3)                                                    # four evaluations
    got_icp = counts(engine, names)
    assert got_icp["k_cp_tree"] == 4 and got_icp["k_cp_join"] == 4 and "k_cp_walk" not in got_icp and not set(got_icp) & set(build)
    engine.reset_timers()
    engine.query_accel = "off"
    engine.register(pts, max_iter=3)
    off_icp = counts(engine, names)
    assert off_icp == {("k_cp_walk" if k == "k_cp_tree" else k): n for k, n in got_icp.items()}


def test_a_run_launches_what_it_launched(timed):
    """sh_run with the switch off, with it on, and with the index resident: the same launches, none of them new.  (That they are the
    launches of the library before the hierarchy is shown by DESIGN 10.15's run of both libraries; sh_run's code is unchanged.)"""
    engine = timed
    names = launch_names()
    v, f = bone("humerus_left")
    engine.reset_params()
    engine.upload([(v, f)])
    engine.run(_lib.STAGE_ALL)                                                          # (the first run of a batch may grow capacities)
    seen = []
    for mode, build in (("off", False), ("bvh", False), ("bvh", True), ("off", True)):
        engine.query_accel = mode
        if build:
            engine.build_bvh()
        engine.reset_timers()
        lm = engine.run(_lib.STAGE_ALL)
        assert lm["status"][0] == 0
        seen.append(counts(engine, names))
    assert seen[0] == seen[1] == seen[2] == seen[3] and not set(seen[0]) & set(NEW) and "k_cp_walk" not in seen[0]
    assert {"fill", "k_anp_plane"} <= set(seen[0])                                      # (the counting sees the run: two of its names)
    print("a run launches", sum(seen[0].values()), "kernels under", len(seen[0]), "names")
