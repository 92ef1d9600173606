"""Which kernels the ray calls launch with the switch of sh_set_query_accel on and off, that the anatomic-neck rays and a run launch what
they launched before the rays read the hierarchy, and what a new batch removes.  Nothing here is measured: the counts are read off
sh_query_host.h (off: count, scan, fill, sort; on: k_ray_tree twice, the same scan and sort; the nearest with the switch on: k_ray_near
alone; a build is class, key, emit, leaves and a k_bvh_level per level above the leaves that the largest mesh could have)."""
import numpy as np
import pytest

import bvh_oracle as B
import raytree_oracle as RT
from shoulder_amd import _lib
from test_bvh_host import bone
from test_gpu_bvh_launches import counts, launch_names

pytestmark = pytest.mark.gpu
TREE = ("k_ray_tree", "k_ray_near")
BUILD = ("k_bvh_class", "k_bvh_key", "k_bvh_emit", "k_bvh_leaves", "k_bvh_level")


@pytest.fixture
def timed(engine):
    engine.enable_timing(1)
    engine.query_accel = "off"
    try:
        yield engine
    finally:
        engine.enable_timing(0)
        engine.reset_timers()
        engine.query_accel = "off"


def test_launches_of_the_ray_calls(timed):
    engine = timed
    names = launch_names()
    assert set(TREE) <= set(names) and {"k_ray_count", "k_ray_fill", "k_ray_scan", "k_ray_sort"} <= set(names)
    v, f = bone("humerus_left")
    o, d = RT.random_rays(v, 100, 1)
    engine.upload([(v, f)])
    build = dict(k_bvh_class=1, k_bvh_key=1, k_bvh_emit=1, k_bvh_leaves=1, k_bvh_level=B.levels_of(len(f)) - 1)
    brute = dict(k_ray_count=1, k_ray_scan=1, k_ray_fill=1, k_ray_sort=1)
    tree = dict(k_ray_tree=2, k_ray_scan=1, k_ray_sort=1)
    engine.reset_timers()
    want = engine.ray_cast(o, d, cap=4)
    assert counts(engine, names) == brute                                               # off: no k_ray_tree, no k_ray_near, no k_bvh_*
    engine.reset_timers()
    want_near = engine.ray_nearest(o, d)
    assert counts(engine, names) == brute                                               # off: the chain with cap = 1 and a copy, no new kernel
    assert not engine._has_buffer("bvh.order")
    engine.query_accel = "bvh"
    engine.reset_timers()
    got = engine.ray_cast(o, d, cap=4)
    assert counts(engine, names) == dict(build, **tree)                                 # the first ray call builds the index; no count, no fill
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    engine.reset_timers()
    assert engine.ray_cast(o, d, cap=4)[0].tobytes() == want[0].tobytes()
    assert counts(engine, names) == tree                                                # the index is resident
    engine.reset_timers()
    got_near = engine.ray_nearest(o, d)
    assert counts(engine, names) == dict(k_ray_near=1)                                  # one kernel: no scan, no sort
    assert got_near.tobytes() == want_near.tobytes() and engine._has_buffer("ray.near")
    # a new batch removes "ray.near" and the index; the first nearest call in "bvh" mode builds it again
    engine.upload([(v, f)])
    assert not engine._has_buffer("ray.near") and not engine._has_buffer("bvh.order")
    engine.reset_timers()
    assert engine.ray_nearest(o, d).tobytes() == want_near.tobytes()
    assert counts(engine, names) == dict(build, k_ray_near=1)
    engine.store("verts", v)                                                            # so does a store of the vertices
    assert not engine._has_buffer("ray.near") and not engine._has_buffer("bvh.order")


def test_the_anatomic_neck_rays_and_a_run_do_not_read_the_switch(timed):
    """anp_axis_hits after a run: the same bytes and the same launches (the brute chain) with the switch on as off; sh_run's launches
    are equal in both modes and none of them is a ray-tree or a build kernel"""
    engine = timed
    names = launch_names()
    v, f = bone("humerus_left")
    engine.reset_params()
    engine.upload([(v, f)])
    engine.run(_lib.STAGE_ALL)                                                          # (the first run of a batch may grow capacities)
    seen, hits = {}, {}
    for mode in ("off", "bvh"):
        engine.query_accel = mode
        engine.reset_timers()
        lm = engine.run(_lib.STAGE_ALL)
        assert lm["status"][0] == 0
        seen[mode] = counts(engine, names)
        engine.reset_timers()
        hits[mode] = engine.anp_axis_hits(cap=4)
        seen[mode + " anp"] = counts(engine, names)
    assert seen["off"] == seen["bvh"] and not set(seen["off"]) & set(TREE + BUILD) and len(seen["off"]) > 20
    assert seen["off anp"] == seen["bvh anp"] == dict(k_ray_anp_rays=1, k_ray_count=1, k_ray_scan=1, k_ray_fill=1, k_ray_sort=1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hits["off"], hits["bvh"])) and np.all(hits["off"][1] >= 1)
    assert not engine._has_buffer("bvh.order")                                          # nothing built an index
