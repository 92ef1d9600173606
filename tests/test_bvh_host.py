"""The face hierarchy of sh_mesh_bvh without a GPU: the scalar rules of shoulder_amd/csrc/sh_scalar.h (bvh_*) -- the source k_bvh.h
runs on the device -- compiled for the host (tests/hostcheck/bvh_check.cpp) against the NumPy statement of tests/bvh_oracle.py.

Bounds: none.  The index (order, loose list, offsets, boxes, corners) is compared as bytes; the records of the host walk over the index
are compared as bytes with tests/closest_oracle.py closest, which looks at every face and knows neither a cull nor a tree."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bvh_oracle as B
import closest_oracle as O
import stem_oracle as SO
from conftest import BONES, ROOT
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

L_, W_ = B.LEAF, B.WIDTH
T_TILT = SO.rigid((0.3, -0.2, 0.5), (1.0, -0.5, 0.75))      # the frame of the 130-gon prism of tests/test_gpu_closest.py


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return B.build_shim(tmp_path_factory.mktemp("bvh_shim"))


def f32(vf):
    return np.ascontiguousarray(vf[0], np.float32), np.ascontiguousarray(vf[1], np.int32)


def prism130(F=None):
    v, f = f32(SO.mesh_in_ct(T_TILT, *SO.prism(130, 5.0, -2.5, 2.5, 0.011)))
    return (v, f) if F is None else (v, np.ascontiguousarray(f[:F]))


def bone(name):
    return f32(load_stl(os.path.join(BONES, name + ".stl")))


def sheet():
    """a flat sheet in z = const: 12 x 9 cells of two triangles, ext_z = 0"""
    xs, ys = np.meshgrid(np.arange(13, dtype=np.float32) * 1.5, np.arange(10, dtype=np.float32) * 0.75, indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 3.25, np.float32)], axis=1)
    idx = np.arange(xs.size).reshape(xs.shape)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.c_[a, b, c], np.c_[a, c, d]]).astype(np.int32)


def one_cell():
    """300 small faces that all share one cell of the quantisation, and two far corners' faces that span the box: a long tie"""
    rng = np.random.default_rng(5)
    base = rng.uniform(0.0, 0.05, size=(300, 1, 3)) + np.array([[(0.0, 0.0, 0.0), (0.2, 0.0, 0.0), (0.0, 0.2, 0.0)]])      # (0.2 mm legs: still tight)
    big = np.array([[(0.0, 0.0, 0.0), (400.0, 0.0, 0.0), (0.0, 400.0, 400.0)], [(400.0, 400.0, 400.0), (399.0, 400.0, 400.0), (400.0, 399.0, 399.0)]])
    tri = np.concatenate([big[:1], base, big[1:]]).astype(np.float32)
    return tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.int32).reshape(-1, 3)


def loose_only():
    v = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 5, 5), (1, 1e-5, 0)], np.float32)
    return v, np.array([(0, 1, 2), (3, 3, 3), (0, 2, 1), (1, 1, 2), (0, 2, 4)], np.int32)


def twice(vf):
    return vf[0], np.concatenate([vf[1], vf[1]]).astype(np.int32)


MESHES = {
    "tetrahedron": lambda: f32(O.TETRA),
    "prism_L": lambda: prism130(L_), "prism_L+1": lambda: prism130(L_ + 1), "prism_LW": lambda: prism130(L_ * W_), "prism_LW+1": lambda: prism130(L_ * W_ + 1),
    "prism_LWW-1": lambda: prism130(L_ * W_ * W_ - 1), "prism_LWW+1": lambda: prism130(L_ * W_ * W_ + 1),
    "sheet": sheet, "prism_twice": lambda: twice(prism130(200)), "one_cell": one_cell, "loose_only": loose_only,
    "humerus_left": lambda: bone("humerus_left"), "humerus_right": lambda: bone("humerus_right"),
}


def test_the_constants_and_the_record():
    """LEAF and WIDTH are powers of two in 4..16; the levels of the largest mesh an upload admits fit the word of a stack entry and the
    row of "bvh.off"; sh_bvh_info as a C compiler lays it out is the dtype of the binding"""
    assert L_ in (4, 8, 16) and W_ in (4, 8, 16)
    assert B.MAX_LEVELS <= 16 and -(-B.MAX_FACES // L_) < 1 << 28 and B.OFF_LEVEL + B.MAX_LEVELS + 1 <= B.OFF_WORDS
    names = list(_lib.BVH_INFO_DTYPE.names)
    lines = ['printf("%zu\\n", sizeof(sh_bvh_info));'] + ['printf("%%zu\\n", offsetof(sh_bvh_info, %s));' % n for n in names]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "shoulder_hip.h"\nint main(void) { sh_bvh_info r; (void)r;\n' + "\n".join(lines) + "\nreturn 0; }\n"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(tmp, "p"), os.path.join(tmp, "p.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(tmp, "p")], text=True).split()]
    assert got[0] == _lib.BVH_INFO_DTYPE.itemsize == _lib.BVH_INFO_BYTES == 48
    assert got[1:] == [_lib.BVH_INFO_DTYPE.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 20, 24, 36]
    assert (_lib.ACCEL_OFF, _lib.ACCEL_BVH) == (0, 1)


def test_twin_constants_are_the_oracles(shim):
    c = np.zeros(6, np.int32)
    shim.bc_consts(c.ctypes.data)
    assert list(c) == [L_, W_, B.MAX_LEVELS, B.STACK, B.OFF_WORDS, B.OFF_LEVEL] and shim.bc_max_faces() == B.MAX_FACES
    assert B.STACK == B.MAX_LEVELS * (W_ - 1) + 1


def test_sanitized_twin_runs_clean(tmp_path):
    """the twin as a stand-alone program under -fsanitize=address,undefined: every point through the tree against every face without it"""
    exe = B.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "bvh_check: ok" in r.stdout, r.stdout + r.stderr


def test_the_scalar_rules_on_numbers_worked_by_hand(shim):
    """the loose predicate at its threshold, the cells at the ends of the box and of a flat one, the interleave, the pruning rule"""
    def loose(tri):
        t = np.ascontiguousarray(tri, np.float32)
        return shim.bc_loose(t.ctypes.data)
    # a right triangle with legs 1 and h: g = h^2 / (1 + h^2)^1.5
    assert loose([(0, 0, 0), (1, 0, 0), (0, 1, 0)]) == 0 and loose([(0, 0, 0), (1, 0, 0), (0, 0.125, 0)]) == 0 and loose([(0, 0, 0), (1, 0, 0), (0, 0.0625, 0)]) == 1
    assert loose([(0, 0, 0), (1, 0, 0), (2, 0, 0)]) == 1 and loose([(3, 3, 3)] * 3) == 1
    assert shim.bc_quant(0.0, 0.0, 0.0, 8.0) == 0 and shim.bc_quant(8.0, 8.0, 0.0, 8.0) == 1023 and shim.bc_quant(4.0, 4.0, 0.0, 8.0) == 512
    assert shim.bc_quant(1.0, 3.0, 0.0, 8.0) == 256 and shim.bc_quant(5.0, 5.0, 5.0, 5.0) == 0
    assert shim.bc_code(1, 0, 0) == 1 and shim.bc_code(0, 1, 0) == 2 and shim.bc_code(0, 0, 1) == 4 and shim.bc_code(1023, 1023, 1023) == (1 << 30) - 1
    assert shim.bc_code(0b1000000000, 0, 0b11) == (1 << 27) | 0b100100
    rng = np.random.default_rng(2)
    q = rng.integers(0, 1024, size=(200, 3))
    want = B.spread(q[:, 0]) | (B.spread(q[:, 1]) << np.uint32(1)) | (B.spread(q[:, 2]) << np.uint32(2))
    assert [shim.bc_code(int(a), int(b), int(c)) for a, b, c in q] == [int(x) for x in want]
    for a, b, c in q[:20]:
        bits = sum(((int(a) >> i) & 1) << (3 * i) | ((int(b) >> i) & 1) << (3 * i + 1) | ((int(c) >> i) & 1) << (3 * i + 2) for i in range(10))
        assert shim.bc_code(int(a), int(b), int(c)) == bits
    box = np.array([0, 0, 0, 1, 1, 1], np.float32)

    def skip(p, best_r):
        p = np.array(p, np.float64)
        return shim.bc_box_skip(p.ctypes.data, box.ctypes.data, best_r)
    assert skip((3.0, 0.5, 0.5), 1.0) == 1 and skip((3.0, 0.5, 0.5), 2.0) == 0            # 2 mm away: a tie is not skipped
    assert skip((3.0, 0.5, 0.5), 2.0 * (1.0 - 2.0 ** -22)) == 0 and skip((3.0, 0.5, 0.5), 1.999) == 1      # inside the margin; outside it
    assert skip((3.0, 0.5, 0.5), np.inf) == 0 and skip((0.5, 0.5, 0.5), 0.0) == 0          # no best yet; a point in the box
    assert skip((9999.0, 0.5, 0.5), 1.0) == 1 and skip((10001.0, 0.5, 0.5), 1.0) == 0      # the far corner within ten metres, and beyond
    assert skip((1e200, 0.0, 0.0), 1.0) == 0


@pytest.mark.parametrize("name", list(MESHES))
def test_index_bytes_twin_against_oracle(shim, name):
    """order, loose list, offsets, boxes and corners of the twin are the oracle's bytes; the tree has the shape its size says"""
    v, f = MESHES[name]()
    base = 37 if name.startswith("prism") else 0
    want, got = B.build(v, f, base), B.host_build(shim, v, f, base)
    assert B.same_index(got, want) is None, B.same_index(got, want)
    assert got["info"].tobytes() == want["info"].tobytes()
    t, nl, leaves, levels, nodes = (int(x) for x in want["off"][:5])
    print(name, "F", len(f), "tight", t, "loose", nl, "leaves", leaves, "levels", levels, "nodes", nodes)
    assert t + nl == len(f) and leaves == -(-t // L_) and levels == B.levels_of(t) and nodes == B.nodes_of(t) and want["off"][5] == base
    assert np.array_equal(np.sort(np.concatenate([want["order"], want["loose"]])), np.arange(len(f))) and (np.diff(want["loose"]) > 0).all()
    key = want["code"].astype(np.uint64) << np.uint64(32) | want["order"].astype(np.uint64)
    assert (np.diff(key.astype(np.int64)) > 0).all()                                    # ascending by (code, id), strictly
    expect = {"tetrahedron": (4, 0, 1), "prism_L": (L_, 0, 1), "prism_L+1": (L_ + 1, 0, 2), "prism_LW": (L_ * W_, 0, 2), "prism_LW+1": (L_ * W_ + 1, 0, 3),
              "prism_LWW-1": (L_ * W_ * W_ - 1, 0, 3), "prism_LWW+1": (L_ * W_ * W_ + 1, 0, 4), "loose_only": (0, 5, 0), "humerus_left": (32431, 9, None),
              "humerus_right": (None, 0, None)}
    if name in expect:
        et, el, ek = expect[name]
        assert (et is None or t == et) and nl == el and (ek is None or levels == ek)
    if name == "sheet":
        assert want["info"]["lo"][2] == want["info"]["hi"][2] and not (want["code"] & np.uint32(0x24924924)).any()      # ext_z = 0: no z bit
    if name == "prism_twice":
        code_of = np.zeros(400, np.uint32)
        code_of[want["order"]] = want["code"]
        assert (code_of[:200] == code_of[200:]).all() and (np.unique(want["code"], return_counts=True)[1] % 2 == 0).all()      # every code twice: the id breaks the tie
    if name == "one_cell":
        assert np.unique(want["code"], return_counts=True)[1].max() >= 300
    if t:                                                                               # every box holds what it covers
        lv = want["off"][B.OFF_LEVEL:]
        tri = want["tri"].reshape(t, 3, 3)
        for j in range(leaves):
            c = tri[j * L_:(j + 1) * L_].reshape(-1, 3)
            assert np.array_equal(want["box"][j, :3], c.min(axis=0)) and np.array_equal(want["box"][j, 3:], c.max(axis=0))
        assert np.array_equal(want["box"][nodes - 1, :3], want["info"]["lo"]) and np.array_equal(want["box"][nodes - 1, 3:], want["info"]["hi"])
        assert lv[levels] == nodes and lv[levels] - lv[levels - 1] == 1


def test_the_fixtures_loose_counts():
    counts = {n: int(B.loose_faces(*bone(n)).sum()) for n in ("humerus_left", "humerus_left_trab", "humerus_right", "proximal_left_cut")}
    assert counts == dict(humerus_left=9, humerus_left_trab=3, humerus_right=0, proximal_left_cut=61), counts


@pytest.mark.parametrize("name", ["humerus_left", "proximal_left_cut"])
def test_walk_bytes_twin_against_the_oracle_without_a_tree(shim, name):
    """512 points -- 64 on vertices, 64 on edge midpoints, 64 inside, up to 50 mm outside, 8 at 2e4 mm, one at 1e200 -- through the twin's
    index and walk: the records are the bytes of closest_oracle.closest, which tests every face"""
    v, f = bone(name)
    pts = B.point_classes(v, f, seed=11)
    assert pts.shape == (512, 3)
    index = B.host_build(shim, v, f)
    got, counts = B.host_walk(shim, v, f, index, pts)
    want = O.closest(v, f, pts)
    bad = np.nonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(pts))])[0]
    assert len(bad) == 0, (bad[:8], got[bad[:4]], want[bad[:4]])
    assert got.tobytes() == want.tobytes()
    assert want["status"][-1] == B.GEOMETRY and want["face"][-1] == -1 and not want["status"][:-1].any()
    assert sum(O.ties(v, f, p) >= 3 for p in pts[:64]) >= 60                            # on a vertex three or more faces tie
    t, nl = int(index["off"][0]), int(index["off"][1])
    near, far = counts[:503], counts[503:511]
    assert (far[:, 1] == t).all() and (counts[:, 2] == nl).all() and (counts[511, 1] == t)      # beyond the guard nothing is pruned
    assert counts[:, 3].max() <= B.STACK
    print(name, "tight", t, "loose", nl, "per point: nodes", near[:, 0].mean(), "faces", near[:, 1].mean(), "max faces", near[:, 1].max(), "deepest stack",
          counts[:, 3].max(), "of", B.STACK)
    assert near[:, 1].mean() < 0.05 * t                                                 # the tree prunes: a regression to a full walk shows here


def test_walk_on_the_small_meshes(shim):
    """the meshes of the index test, 43 points each: vertices, edges, inside, outside, far, one at 1e200"""
    for name in ("tetrahedron", "prism_LW+1", "prism_LWW+1", "sheet", "prism_twice", "one_cell", "loose_only"):
        v, f = MESHES[name]()
        pts = B.point_classes(v, f, n_each=10, far=2, seed=3)
        got, counts = B.host_walk(shim, v, f, B.host_build(shim, v, f), pts)
        want = O.closest(v, f, pts)
        assert got.tobytes() == want.tobytes(), name


def test_the_plan_against_the_oracle(shim):
    """levels, offsets, capacities and refusals of the kernel-free plan (sh_query.h bvh_plan), F at the upload's maximum included"""
    for t in [0, 1, 3, L_ - 1, L_, L_ + 1, L_ * W_, L_ * W_ + 1, L_ * W_ * W_ - 1, L_ * W_ * W_, L_ * W_ * W_ + 1, 32440, 2076160, B.MAX_FACES]:
        row = np.zeros(B.OFF_WORDS, np.int32)
        shim.bc_off_row(t, 5, 11, row.ctypes.data)
        assert np.array_equal(row, B.off_row(t, 5, 11)), t
        assert shim.bc_levels_of(t) == B.levels_of(t) == int(row[3]) and shim.bc_nodes_of(t) == B.nodes_of(t) == int(row[4])
        lv = row[B.OFF_LEVEL:B.OFF_LEVEL + int(row[3]) + 1]
        sizes = np.diff(lv)
        assert (len(sizes) == 0 and t == 0) or (sizes[0] == -(-t // L_) and sizes[-1] == 1 and all(sizes[k + 1] == -(-sizes[k] // W_) for k in range(len(sizes) - 1)))
    assert B.levels_of(B.MAX_FACES) == B.MAX_LEVELS and (B.MAX_LEVELS - 1) * (W_ - 1) + 1 <= B.STACK

    def plan(counts):
        foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        out, base, blocks = np.zeros(7, np.int64), np.zeros(len(counts) + 1, np.int32), np.zeros(B.MAX_LEVELS, np.int32)
        rc = shim.bc_plan(len(counts), foff.ctypes.data, out.ctypes.data, base.ctypes.data, blocks.ctypes.data)
        return rc, out, base, blocks
    counts = [4, L_ * W_ + 1, 32440]
    rc, out, base, blocks = plan(counts)
    assert rc == 0 and list(base) == B.bases(counts)
    assert out[0] == -(-32440 // 256) and out[1] == B.levels_of(32440) and out[2] == -(-(-(-32440 // L_)) // 256) and out[3] == base[-1]
    assert out[4] == 24 * base[-1] and out[5] == 36 * sum(counts) and out[6] == 8 * sum(counts)
    n = -(-32440 // L_)
    for k in range(int(out[1])):
        assert blocks[k] == max(1, -(-n // 256)), k
        n = -(-n // W_)
    rc, out, base, _ = plan([B.MAX_FACES])
    assert rc == 0 and out[1] == B.MAX_LEVELS and base[1] == B.nodes_of(B.MAX_FACES) < 1 << 31
    assert plan([B.MAX_FACES, B.MAX_FACES])[0] == 0
    assert plan([B.MAX_FACES] * 4)[0] == B.NOMEM and plan([B.MAX_FACES + 1])[0] == B.ARG
    # the checks of the two entry points in their order
    assert shim.bc_precheck(0, 1, 0) == B.ARG and shim.bc_precheck(1, 0, 0) == B.STATE and shim.bc_precheck(1, 3, 1) == B.STATE and shim.bc_precheck(1, 3, 0) == 0
    assert shim.bc_precheck(0, 0, 1) == B.ARG
    assert [shim.bc_precheck_accel(1, m) for m in (0, 1, 2, -1)] == [0, 0, B.ARG, B.ARG] and shim.bc_precheck_accel(0, 1) == B.ARG
