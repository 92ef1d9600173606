"""The rays through the face hierarchy without a GPU: sh_scalar.h bvh_ray_descend and bvh_ray_box_skip -- the source k_raytree.h runs on
the device -- compiled for the host (tests/hostcheck/raytree_check.cpp) against the walk over all faces (ray_check.cpp's statement) and
against the NumPy statements of tests/raytree_oracle.py and tests/ray_oracle.py.

Bounds.  Tree against all faces, and nearest against row 0: bytes, no ray left out.  Against NumPy: counts, faces and sides equal, t and
points within 1e-6 mm, the project's bound (as tests/test_gpu_rays.py holds the device to NumPy); the skip rule: the same verdicts."""
import subprocess

import numpy as np
import pytest

import bvh_oracle as B
import ray_oracle as O
import raytree_oracle as RT
import stem_oracle as SO
from shoulder_amd import _lib
from test_bvh_host import L_, T_TILT, W_, bone, f32, loose_only, prism130, sheet

MM = 1e-6
CAP = 8
N_RANDOM = 4096


def tube24():
    return f32(SO.mesh_in_ct(T_TILT, *SO.tube(24, 4.0, 7.0, -5.0, 5.0, 0.05)))


MESHES = {
    "tetrahedron": lambda: f32(O.TETRA),
    "prism_L": lambda: prism130(L_), "prism_L+1": lambda: prism130(L_ + 1), "prism_LW": lambda: prism130(L_ * W_), "prism_LW+1": lambda: prism130(L_ * W_ + 1),
    "prism_520": prism130, "tube": tube24, "sheet": sheet, "loose_only": loose_only,
    "humerus_left": lambda: bone("humerus_left"), "proximal_left_cut": lambda: bone("proximal_left_cut"),
}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RT.build_shim(tmp_path_factory.mktemp("raytree_shim"))


@pytest.fixture(scope="module")
def cases(shim):
    """per mesh, once: the mesh, the twin's index, the rays, the walk over all faces and the walk through the tree"""
    done = {}

    def get(name):
        if name not in done:
            v, f = MESHES[name]()
            index = B.host_build(shim, v, f)
            o, d, names = RT.rays_for(v, f, index, N_RANDOM + RT.N_ADVERSARIAL, seed=len(name))
            assert len(o) == N_RANDOM + RT.N_ADVERSARIAL and names.count("random") == N_RANDOM
            brute = RT.host_brute(shim, v, f, o, d, CAP)
            tree = RT.host_cast(shim, v, f, index, o, d, CAP)
            done[name] = dict(v=v, f=f, index=index, o=o, d=d, names=names, brute=brute, tree=tree)
        return done[name]
    return get


def test_sanitized_twin_runs_clean(tmp_path):
    """the twin as a stand-alone program under -fsanitize=address,undefined: every ray through the tree against every face without it"""
    exe = RT.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "raytree_check: ok" in r.stdout, r.stdout + r.stderr


def twin_skip(shim, o, d, bx, tbest=np.inf):
    o, d, bx = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64), np.ascontiguousarray(bx, np.float32)
    tn = np.zeros(1)
    return bool(shim.rt_box_skip(o.ctypes.data, d.ctypes.data, bx.ctypes.data, float(tbest), tn.ctypes.data)), float(tn[0])


def test_the_skip_rule_on_numbers_worked_by_hand(shim):
    """the unit box from outside: pad = 2^-8 |d| D E^2 + 2^-40 m1 with E^2 = 3"""
    box = (0, 0, 0, 1, 1, 1)

    def skip(o, d, tbest=np.inf):
        got = twin_skip(shim, o, d, box, tbest)
        assert got == RT.box_skip(o, d, box, tbest), (o, d, got)
        return got[0]
    assert not skip((-3, 0.5, 0.5), (1, 0, 0)) and skip((-3, 0.5, 0.5), (-1, 0, 0))              # towards it; away from it
    assert skip((-3, 0.5, 2.0), (1, 0, 0)) and skip((-3, 0.5, 0.5), (0, 1, 0))                   # beside it, with zero components
    # o = (-3, .5, z), d = +x: D = |(4, .5, max(|z|, |z - 1|))|, pad = 2^-8 D 3; the slab in z is [-pad, 1 + pad]
    pad = 2.0 ** -8 * np.sqrt(16 + 0.25 + 1.06 ** 2) * 3.0
    assert 0.04 < pad < 0.06 and not skip((-3, 0.5, 1.04), (1, 0, 0)) and skip((-3, 0.5, 1.06), (1, 0, 0))
    assert not skip((-3, 1.0, 0.5), (1, 0, 0)) and not skip((-3, 0.0, 1.0), (1, 0, 0))           # in a face plane of the box, along an edge of it
    assert not skip((0.5, 0.5, 0.5), (0, 0, 1)) and not skip((0.5, 0.5, 0.5), (1e-300, 0, 0))    # from inside
    assert skip((-3, 0.5, 0.5), (1, 1, 0)) and not skip((-3, 0.5, 0.5), (1, 0.1, 0))             # a slanted miss and a slanted hit
    assert not skip((-3, 0.5, 2.0), (1e6, 0, 0)) and skip((-3, 0.5, 2.0), (1e-6, 0, 0))          # a long d grows the pad beyond the gap; a short one does not
    assert not skip((-3, 0.5, 2.0), (2.0 ** 21, 0, 0)) and not skip((2.0 ** 21, 0.5, 2.0), (1, 0, 0))      # beyond the guards nothing is skipped
    assert not skip((-3, 0.5, 0.5), (1, 0, 0), tbest=3.5) and skip((-3, 0.5, 0.5), (1, 0, 0), tbest=2.5)     # enters at t = 3 - pad: behind a best of 2.5
    assert not skip((-3, 0.5, 0.5), (1, 0, 0), tbest=2.92)                                       # within pad / |d| of the entry: not skipped
    assert not skip((-3, 0.5, 0.5), (np.nan, 0, 0)) and not skip((np.nan, 0.5, 0.5), (1, 0, 0)) and not skip((-3, 0.5, 0.5), (1, 0, 0), tbest=np.nan)
    flat = (0, 0, 2, 4, 4, 2)                                                                    # a box flat in z, and a ray in its plane
    assert twin_skip(shim, (-1, 1, 2), (1, 0, 0), flat)[0] is False and twin_skip(shim, (-1, 1, 4.0), (1, 0, 0), flat)[0] is True
    assert twin_skip(shim, (1, 1, 0), (0, 0, 1), flat)[0] is False and twin_skip(shim, (1, 1, 3), (0, 0, 1), flat)[0] is True


def test_the_skip_rule_twin_against_numpy(shim):
    """4 000 (ray, box) pairs about the nodes of a bone's index, with and without a best t: the same verdict and the same entry parameter"""
    v, f = bone("humerus_left")
    index = B.host_build(shim, v, f)
    o, d, _ = RT.rays_for(v, f, index, 1000, seed=4)
    rng = np.random.default_rng(9)
    box = index["box"][rng.integers(0, len(index["box"]), (len(o), 4))]
    n_skip = 0
    for r in range(len(o)):
        for k in range(4):
            tb = np.inf if k < 2 else float(rng.uniform(0.0, 200.0))
            got, want = twin_skip(shim, o[r], d[r], box[r, k], tb), RT.box_skip(o[r], d[r], box[r, k], tb)
            assert got == want, (r, k, got, want)
            n_skip += got[0]
    print("skipped", n_skip, "of", 4 * len(o))
    assert 0.5 * 4 * len(o) < n_skip < 4 * len(o)


@pytest.mark.parametrize("name", list(MESHES))
def test_tree_is_the_walk_over_all_faces_as_bytes(cases, name):
    """counts, and every hit's t, point, face and side after the (t, face) sort, for 4 096 random rays and the adversarial set"""
    c = cases(name)
    (bh, bc), (th, tc, tot) = c["brute"], c["tree"]
    bad = np.nonzero((bc != tc) | [bh[r].tobytes() != th[r].tobytes() for r in range(len(bc))])[0]
    assert len(bad) == 0, [(int(r), c["names"][r], int(bc[r]), int(tc[r])) for r in bad[:8]]
    assert bc.tobytes() == tc.tobytes() and bh.tobytes() == th.tobytes()
    t, nl, R = int(c["index"]["off"][0]), int(c["index"]["off"][1]), len(bc)
    print(name, "F", len(c["f"]), "tight", t, "loose", nl, "rays", R, "with a hit", int((bc > 0).sum()), "most hits", int(bc.max()),
          "| per ray: nodes", tot[0] / R, "tree faces", tot[1] / R, "deepest stack", int(tot[3]), "of", B.STACK)
    assert tot[3] <= B.STACK and (bc > 0).sum() >= (50 if t else 1)             # (the slivers of the loose-only mesh are hard to hit)
    if name in ("humerus_left", "proximal_left_cut"):
        assert tot[1] / R < 0.2 * t                                                     # the tree prunes: a regression to a full walk shows here


@pytest.mark.parametrize("name", list(MESHES))
def test_nearest_is_row_0_as_bytes(shim, cases, name):
    c = cases(name)
    near, tot = RT.host_near(shim, c["v"], c["f"], c["index"], c["o"], c["d"])
    row0 = np.ascontiguousarray(c["brute"][0][:, 0])
    bad = np.nonzero([near[r].tobytes() != row0[r].tobytes() for r in range(len(near))])[0]
    assert len(bad) == 0, [(int(r), c["names"][r], near[r], row0[r]) for r in bad[:4]]
    miss = c["brute"][1] == 0
    assert miss.any() and np.all(near["face"][miss] == -1) and not near["t"][miss].any() and not near["point"][miss].any() and not near["side"][miss].any()
    _, _, all_tot = c["tree"]
    print(name, "nearest, per ray: nodes", tot[0] / len(near), "tree faces", tot[1] / len(near), "| all hits, per ray: nodes", all_tot[0] / len(near))
    assert tot[0] <= all_tot[0] and tot[1] <= all_tot[1]                                        # pruning by t only ever visits less


@pytest.mark.parametrize("name", list(MESHES))
def test_numpy_oracle_against_the_twin(shim, cases, name):
    """ray_oracle.cast, and raytree_oracle.nearest on top of it, against the twin through the tree: every ray of the small meshes; of the
    bones the adversarial set and 256 random rays (NumPy visits every face of every ray)"""
    c = cases(name)
    n = len(c["o"]) if len(c["f"]) <= 1000 else RT.N_ADVERSARIAL + 256
    o, d = c["o"][:n], c["d"][:n]
    want, wn = O.cast(c["v"], c["f"], o, d, CAP)
    got, gn = c["tree"][0][:n], c["tree"][1][:n]
    assert np.array_equal(gn, wn), [(int(r), c["names"][r]) for r in np.nonzero(gn != wn)[0][:8]]
    assert np.array_equal(got["face"], want["face"]) and np.array_equal(got["side"], want["side"])
    scale = np.linalg.norm(d, axis=1)[:, None]                                                  # t counts in units of |d|: a length is t |d|
    assert (np.abs(got["t"] - want["t"]) * scale).max() <= MM and np.abs(got["point"] - want["point"]).max() <= MM
    near = RT.host_near(shim, c["v"], c["f"], c["index"], o, d)[0]
    wnear = RT.nearest(c["v"], c["f"], o, d)
    assert np.array_equal(near["face"], wnear["face"]) and np.array_equal(near["side"], wnear["side"])
    assert (np.abs(near["t"] - wnear["t"]) * scale[:, 0]).max() <= MM and np.abs(near["point"] - wnear["point"]).max() <= MM


def test_thickness_oracle_on_the_tube():
    """the NumPy thickness on the tube's outer wall from the middle of every outer side face: the wall between the two 24-gons, between
    r_out cos(pi/24) - r_in = 2.94 and r_out - r_in cos(pi/24) = 3.04 mm"""
    v, f = tube24()
    v64 = O.widen(v)
    outer = np.arange(48)
    A, Bc, C = v64[f[outer, 0]], v64[f[outer, 1]], v64[f[outer, 2]]
    n = np.cross(Bc - A, C - A)
    th, pt, face = RT.thickness(v, f, (A + Bc + C) / 3.0, n)
    assert np.all(face >= 48) and np.all(th > 7.0 * np.cos(np.pi / 24) - 4.0 - 1e-5) and np.all(th < 7.0 - 4.0 * np.cos(np.pi / 24) + 1e-5)
    th2, _, face2 = RT.thickness(v, f, (A + Bc + C) / 3.0, -n)                                    # outward: nothing there
    assert np.all(np.isinf(th2)) and np.all(face2 == -1)


def test_the_plan(shim):
    """chunks of 64 rays and no "ray.blockhit" in tree mode; "ray.near" for the nearest, alone with the rays in tree mode; the brute plan
    unchanged"""
    B_, maxF, cap = 3, 32440, 4
    tmax = -(-maxF // 256)
    for R in (1, 64, 65, _lib.RAY_MAX):
        n = B_ * R
        off = RT.host_plan(shim, B_, R, False, cap, maxF)
        assert off == dict(tmax=tmax, chunks=-(-R // RT.RAY_CHUNK), n=n, rays=R * 48, counts=n * 4, offs=(n + 1) * 8, cursor=n * 4, hits=n * cap * 40,
                           blockhit=tmax * B_ * -(-R // RT.RAY_CHUNK) * 4, near=0, status=0), R
        on = RT.host_plan(shim, B_, R, True, cap, maxF, tree=True)
        assert on == dict(off, chunks=-(-R // RT.TREE_CHUNK), rays=n * 48, blockhit=0), R
        near_off = RT.host_plan(shim, B_, R, False, 1, maxF, near=True)
        assert near_off == dict(off, hits=n * 40, near=n * 40), R
        near_on = RT.host_plan(shim, B_, R, False, 1, maxF, tree=True, near=True)
        assert near_on == dict(tmax=tmax, chunks=-(-R // RT.TREE_CHUNK), n=n, rays=R * 48, counts=0, offs=0, cursor=0, hits=0, blockhit=0, near=n * 40, status=0), R
    assert RT.host_plan(shim, 2, 4, True, 16, 100, with_status=True)["status"] == 8            # the anatomic-neck rays: as before


def test_the_precheck_of_the_nearest(shim):
    """the codes of sh_ray_cast in its order: no context, R, the state, the rays"""
    rays = np.zeros(3, dtype=_lib.RAY_DTYPE)
    rays["dir"] = (0.0, 0.0, 1.0)

    def code(r, R, per=0, ctx=1, B_=1, pending=0):
        return shim.rt_precheck_nearest(r.ctypes.data if r is not None else None, R, per, ctx, B_, pending)
    assert code(rays, 3) == 0 and code(rays, 3, ctx=0) == RT.ARG and code(None, 3) == RT.ARG and code(rays, 0) == RT.ARG
    assert code(rays, _lib.RAY_MAX + 1) == RT.ARG and code(rays, 3, B_=0) == RT.STATE and code(rays, 3, pending=1) == RT.STATE
    bad = rays.copy()
    bad["origin"][1, 2] = np.nan
    zero = rays.copy()
    zero["dir"][2] = 0.0
    assert code(bad, 3) == RT.ARG and code(zero, 3) == RT.ARG and code(zero, 2) == 0
    assert code(bad, 3, B_=0) == RT.STATE                                                       # the state ranks before the rays, as in sh_ray_cast
