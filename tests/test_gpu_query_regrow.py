"""The views of the queries of the resident batch behind a re-allocation (shoulder_amd/csrc/sh_ctx.h ensure_bytes / view_of,
sh_query_host.h): every query is called with Q = 1, then Q = 257, then Q = 1 again, so that its buffers grow between the first two calls
(and, for the rays, "ray.pool" and "ray.hits" inside the second), and then on a batch of two meshes.  A pointer resolved before a
buffer grew would read or write the freed one.

Bounds.  Every result is held, as bytes, to the same call made FIRST on a fresh Engine with the same upload.  The closest points are
held to tests/closest_oracle.py as tests/test_gpu_closest.py holds them (face, region, side and status equal, dist and point within
1e-9 mm), the mass properties to tests/mass_oracle.py as tests/test_gpu_mass.py holds them (the record as bytes)."""
import numpy as np
import pytest

import closest_oracle as CO
import mass_oracle as MO
import stem_oracle as SO
from shoulder_amd.engine import Engine

pytestmark = pytest.mark.gpu
TOL = 1e-9                                                                            # tests/test_gpu_closest.py
T_TILT = SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75))                                 # tests/test_gpu_closest.py: CT -> frame of its prism


def f32(vf):
    return np.ascontiguousarray(vf[0], np.float32), np.ascontiguousarray(vf[1], np.int32)


def prism_cut():
    """the first 257 faces of the tilted 130-gon prism of tests/test_gpu_closest.py: one tile of faces and one more"""
    v, f = f32(SO.mesh_in_ct(T_TILT, *SO.prism(130, 5.0, -2.5, 2.5, 0.011)))
    return v, np.ascontiguousarray(f[:257])


def inputs(B):
    """257 points about the tetrahedron, 257 rays through it (from below, upwards), two rigid starts per humerus"""
    rng = np.random.default_rng(257)
    pts = rng.uniform(-1.0, 5.0, size=(257, 3))
    origins = np.column_stack([rng.uniform(0.2, 1.5, size=(257, 2)), np.full(257, -3.0)])
    directions = np.tile((0.0, 0.0, 1.0), (257, 1))
    c, s = np.cos(0.05), np.sin(0.05)
    turn = np.array([(c, -s, 0.0, 0.0), (s, c, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)])
    return pts, origins, directions, np.tile(np.stack([np.identity(4), turn]), (B, 1, 1, 1))


def calls(B):
    """name -> the call with its first n points (rays): engine, n -> result"""
    pts, origins, directions, T0s = inputs(B)
    return {
        "closest_points": lambda e, n: e.closest_points(pts[:n]),
        "winding_numbers": lambda e, n: e.winding_numbers(pts[:n]),
        "register": lambda e, n: e.register(pts[:n], max_iter=1),
        "register_multistart": lambda e, n: e.register_multistart(pts[:n], T0s, coarse_points=1),
        "mass_properties": lambda e, n: e.mass_properties(),
        "ray_cast": lambda e, n: e.ray_cast(origins[:n], directions[:n], cap=1 if n == 1 else None),
    }, pts


def blob(result):
    return tuple(a.tobytes() for a in (result if isinstance(result, tuple) else (result,)))


def first_on_a_fresh_engine(batch, call, n):
    e = Engine(0)
    try:
        e.upload(batch)
        return blob(call(e, n))
    finally:
        e.close()


def against_the_oracles(name, result, batch, pts):
    if name == "closest_points":
        for b, (v, f) in enumerate(batch):
            got, want = result[b], CO.closest(v, f, pts)
            for k in ("face", "region", "side", "status"):
                assert np.array_equal(got[k], want[k]), (b, k)
            worst = max(float(np.abs(got["dist"] - want["dist"]).max()), float(np.abs(got["point"] - want["point"]).max()))
            print("humerus", b, "Q", len(pts), "closest points: max |gpu - oracle|", worst)
            assert worst <= TOL, worst
    if name == "mass_properties":
        for b, (v, f) in enumerate(batch):
            assert result[b].tobytes() == MO.mass(v, f)[0].tobytes(), (b, result[b])


def test_one_mesh_small_large_small(engine):
    batch = [f32(CO.TETRA)]
    fn, pts = calls(1)
    engine.upload(batch)
    for name, call in fn.items():
        want = {n: first_on_a_fresh_engine(batch, call, n) for n in (1, 257)}
        for n in (1, 257, 1):
            got = call(engine, n)
            assert blob(got) == want[n], (name, n)
            against_the_oracles(name, got, batch, pts[:n])
    hits, counts = fn["ray_cast"](engine, 257)
    assert hits.shape[2] == 16 and (counts == 2).all()                                 # (every ray enters and leaves the solid: the pool held 514 keys)


def test_two_meshes_after_one(engine):
    batch = [f32(CO.TETRA), prism_cut()]
    fn, pts = calls(2)
    engine.upload(batch[:1])
    for call in calls(1)[0].values():                                                  # (run alone, the test starts from the sizes of one mesh and one point)
        call(engine, 1)
    engine.upload(batch)
    for name, call in fn.items():
        got = call(engine, 257)
        assert blob(got) == first_on_a_fresh_engine(batch, call, 257), name
        against_the_oracles(name, got, batch, pts)
