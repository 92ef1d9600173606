"""Surface samples of the resident batch (include/shoulder_hip.h sh_sample_surface), the parts that need no GPU (the record layouts:
test_abi_exports.py): the known answers of the word generator, the host twin of the kernels (the device source,
host-compiled with -ffp-contract=off through tests/hostcheck/sample_check.cpp) against the NumPy statement of tests/sample_oracle.py,
the argument checks, the buffer plan, the round rule of the thinning, and the quality of what the definition draws.

Bounds.  Twin against the oracle: bytes (integer words; the same + - x sqrt in the same order).  Quality, as conditions on the oracle
at N = 4 096, seed 7: the chi-square of the draws over 32 bins of equally many consecutive faces against the bins' area shares below
61.1, the 99.9 % point of 31 degrees of freedom; the sample mean within 3 sqrt(trace of the sample covariance / N) of the area-weighted
centroid (each coordinate of the mean has the variance of that coordinate / N, so the distance has standard deviation at most that
root); with thinning no two kept points closer than the radius and every removed point within it of a kept one -- exact, the
comparison is the definition's own d2 < r r."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sample_oracle as O
from conftest import BONES
from mass_oracle import int_box
from ray_oracle import widen
from shoulder_amd import _lib
from shoulder_amd.stl import load_stl

NAMES = ["humerus_left", "humerus_right", "humerus_left_trab", "humerus_left_flipped"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return O.build_shim(tmp_path_factory.mktemp("sample_check"))


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for n in NAMES:
        v, f = load_stl(os.path.join(BONES, n + ".stl"))
        out[n] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    return out


@pytest.fixture(scope="module")
def drawn(meshes):
    """the oracle's 4 096 samples of every fixture with seed 7, drawn once"""
    return {n: O.sample(v, f, 4096, 7) for n, (v, f) in meshes.items()}


def test_known_answers_of_the_word_generator(shim):
    """SplitMix64 seeded with 1234567 gives these five outputs (the published sequence): state k is seed + k gamma, so w(seed, n) is
    output n"""
    assert [int(x) for x in O.words(O.KNOWN_SEED, np.arange(5))] == O.KNOWN_WORDS
    w = np.zeros(5, dtype=np.uint64)
    shim.sc_words(O.KNOWN_SEED, 0, 5, w.ctypes.data)
    assert [int(x) for x in w] == O.KNOWN_WORDS
    # the counter wraps mod 2^64, in the seed and in the product
    big = 0xFFFFFFFFFFFFFFF0
    shim.sc_words(big, 2 ** 62, 5, w.ctypes.data)
    assert w.tobytes() == O.words(big, np.arange(5, dtype=np.uint64) + np.uint64(2 ** 62)).tobytes()
    # unit: the top 53 bits, in [0, 1)
    assert shim.sc_unit(0) == 0.0 and shim.sc_unit(2 ** 64 - 1) == 1.0 - 2.0 ** -53 == float(O.unit(np.uint64(2 ** 64 - 1)))
    assert shim.sc_unit(1 << 11) == 2.0 ** -53 and shim.sc_unit((1 << 11) - 1) == 0.0
    u = O.unit(O.words(5, np.arange(1000)))
    assert u.min() >= 0.0 and u.max() < 1.0 and all(shim.sc_unit(int(x)) == float(y) for x, y in zip(O.words(5, np.arange(50)), u[:50]))


def same(shim, tag, v, f, N, seed, radius=0.0, max_rounds=32):
    got, want = O.host_sample(shim, v, f, N, seed, radius, max_rounds), O.sample(v, f, N, seed, radius, max_rounds)
    assert got[2].tobytes() == want[2].tobytes(), (tag, "cdf")
    assert got[0].tobytes() == want[0].tobytes(), (tag, "records")
    assert got[1].tobytes() == want[1].tobytes(), (tag, got[1], want[1])
    return got


def test_host_twin_gives_the_oracle_bytes(shim, meshes):
    v, f = meshes["humerus_left"]
    bv, bf = int_box()
    rec, info, cdf = same(shim, "box", bv, bf, 1000, 7)
    assert info["area"] == 2200.0 and info["kept"] == 1000 and info["status"] == 0 and cdf[-1] == 4400.0
    on = (rec["point"] == bv.min(axis=0)) | (rec["point"] == bv.max(axis=0))
    assert on.any(axis=1).all() and rec["face"].min() >= 0 and rec["face"].max() <= 11 and len(set(rec["face"])) == 12
    assert (rec["u"] >= 0).all() and (rec["v"] >= 0).all() and (rec["u"] + rec["v"] <= 1.0).all()
    same(shim, "humerus_left", v, f, 4096, 7)
    for n in (255, 256, 257, 513):
        rec, info, cdf = same(shim, f"{n} faces", v, f[:n], 1000, n)
        assert rec["face"].max() < n and info["status"] == 0
    rec, info, _ = same(shim, "one face", v, f[:1], 300, 3)
    assert not rec["face"].any() and info["kept"] == 300
    same(shim, "thinned", v, f[:513], 600, 11, radius=1.0)
    same(shim, "thinned, out of rounds", v, f[:513], 600, 11, radius=1.0, max_rounds=1)
    # faces of zero area in front, in the middle, on both sides of a block boundary and at the end: cdf repeats, none is drawn
    where = (0, 1, 100, 255, 256, 300, 519)
    zv, zf = O.zero_area_mesh(v, f[:513], where)
    assert len(zf) == 520
    rec, info, cdf = same(shim, "zero-area faces", zv, zf, 4096, 5)
    assert cdf[0] == 0.0 and cdf[1] == 0.0 and all(cdf[k] == cdf[k - 1] for k in where[2:]) and info["status"] == 0
    assert not np.isin(rec["face"], where).any() and len(set(rec["face"])) > 400
    # only faces of zero area, and no faces: the status, zero records
    for tag, ff in (("only zero-area faces", np.array([[0, 1, 1], [2, 2, 3], [4, 5, 4], [6, 6, 6]], np.int32)), ("no faces", f[:0])):
        for radius in (0.0, 2.0):
            rec, info, cdf = same(shim, tag, v, ff, 300, 1, radius=radius)
            assert info["status"] == O.GEOMETRY and info["area"] == 0.0 and info["kept"] == 0 and not np.frombuffer(rec.tobytes(), np.uint8).any()


def test_cdf_is_non_decreasing(shim, meshes):
    for name, (v, f) in meshes.items():
        cdf = O.host_sample(shim, v, f, 1, 0)[2]
        assert cdf.tobytes() == O.cdf_of(O.area2(v, f)).tobytes(), name
        assert (np.diff(cdf) >= 0.0).all() and cdf[0] >= 0.0, name
        tri = widen(v)[f]
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
        assert abs(cdf[-1] / 2.0 - area) <= 1e-9 * area, name      # (another order of summation: F eps relative, as in test_mass_host.py)


def test_arguments_are_checked_in_order(shim):
    text = ctypes.create_string_buffer(256)

    def pre(ctx=1, seeds=1, opt=1, N=10, radius=0.0, max_rounds=32, reserved=0, B=1, pending=0):
        code = shim.sc_precheck(ctx, seeds, opt, N, radius, max_rounds, reserved, B, pending, text, 256)
        return code, text.value.decode()
    assert pre() == (0, "")
    # the context and the pointers rank before N, N before the options, the options before the state
    for kw in (dict(ctx=0), dict(seeds=0), dict(opt=0)):
        code, msg = pre(N=0, radius=-1.0, B=0, **kw)
        assert code == O.ARG and "must be given" in msg
    for N in (0, -3, O.SAMPLE_MAX + 1):
        assert pre(N=N, radius=-1.0, B=0) == (O.ARG, "bad argument (N in 1..1048576)")
    assert pre(N=O.SAMPLE_MAX)[0] == 0
    for kw in (dict(radius=-1e-300), dict(radius=float("nan")), dict(radius=float("inf")), dict(max_rounds=0), dict(max_rounds=33), dict(reserved=1)):
        code, msg = pre(B=0, **kw)
        assert code == O.ARG and msg.startswith("bad options"), kw
    code, msg = pre(N=O.THIN_MAX + 1, radius=0.5, B=0)
    assert code == O.ARG and "with a radius" in msg
    assert pre(N=O.THIN_MAX, radius=0.5)[0] == 0 and pre(N=O.THIN_MAX + 1)[0] == 0 and pre(max_rounds=1)[0] == 0
    assert pre(B=0) == (O.STATE, "no meshes uploaded") and pre(pending=1)[0] == O.STATE and "in flight" in pre(pending=1)[1]
    L = _lib.load()
    opt, seeds = _lib.SampleOptions(0.0, 32, 0), np.zeros(1, np.uint64)
    assert L.sh_sample_surface(None, 10, seeds.ctypes.data, ctypes.byref(opt), None, None) == O.ARG      # (no context)
    assert "sh_sample_surface" in _lib.EXPORTS


def test_buffer_plan(shim):
    def plan(B, N, thin, maxF, sumF):
        out = np.zeros(9, dtype=np.uintp)
        shim.sc_plan(B, N, thin, maxF, sumF, out.ctypes.data)
        return [int(x) for x in out]
    # blocks, chunks, thin, int32 of "samp.state" per humerus, then the bytes of cdf, base, out, info, state
    assert plan(3, 1000, 1, 513, 1200) == [3, 4, 1, 64 + 2000, 1200 * 8, 3 * 3 * 8, 3 * 1000 * 48, 3 * 24, 3 * 2064 * 4]
    assert plan(3, 1000, 0, 513, 1200) == [3, 4, 0, 64, 1200 * 8, 3 * 3 * 8, 3 * 1000 * 48, 3 * 24, 3 * 64 * 4]
    assert plan(1, 1, 0, 4, 4)[:4] == [1, 1, 0, 64] and plan(1, 256, 0, 256, 256)[:2] == [1, 1] and plan(1, 257, 0, 257, 257)[:2] == [2, 2]
    big = plan(64, O.SAMPLE_MAX, 0, 2080000, 64 * 2080000)
    assert big[6] == 64 * O.SAMPLE_MAX * 48 and big[0] == 8125
    assert plan(64, O.THIN_MAX, 1, 32440, 64 * 32440)[8] == 64 * (64 + 2 * 65536) * 4


def test_round_rule_on_a_line(shim):
    """40 points 0.9 r apart in index order: each has its predecessor as its only lower neighbour, so the greedy set is every second
    point and a round decides exactly one more point"""
    pts = np.zeros((40, 3))
    pts[:, 0] = 0.9 * np.arange(40)
    want = (np.arange(40) % 2 == 0).astype(np.int32)
    for thin in (O.thin, lambda p, r, m: O.host_thin(shim, p, r, m)):
        keep, kept, rounds, status = thin(pts, 1.0, 64)
        assert np.array_equal(keep, want) and (kept, rounds, status) == (20, 40, 0)
        keep, kept, rounds, status = thin(pts, 1.0, 40)
        assert np.array_equal(keep, want) and (kept, rounds, status) == (20, 40, 0)
        keep, kept, rounds, status = thin(pts, 1.0, 8)
        assert (kept, rounds, status) == (4, 8, O.CAPACITY)
        assert np.array_equal(keep[:8], want[:8]) and (keep[8:] == -1).all()
    # far apart: all kept in one round; all within the radius: the first alone, in two
    assert O.host_thin(shim, pts * 10.0, 1.0)[1:] == (40, 1, 0) and O.host_thin(shim, pts, 1e9)[1:] == (1, 2, 0)
    assert O.thin(pts * 10.0, 1.0)[1:] == (40, 1, 0) and O.thin(pts, 1e9)[1:] == (1, 2, 0)
    # a distance of exactly the radius is no neighbour (d2 < r r)
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    assert O.host_thin(shim, two, 5.0)[1] == 2 and O.host_thin(shim, two, np.nextafter(5.0, 6.0))[1] == 1


def test_thinning_is_idempotent(shim, drawn):
    rec = drawn["humerus_left"][0]
    keep = O.host_thin(shim, rec["point"][:2048], 3.0)[0]
    kept = rec["point"][:2048][keep == 1]
    again, n, rounds, status = O.host_thin(shim, kept, 3.0)
    assert (again == 1).all() and n == len(kept) and rounds == 1 and status == 0


@pytest.mark.parametrize("name", NAMES)
def test_quality_of_the_draws(meshes, drawn, name):
    v, f = meshes[name]
    rec, info, cdf = drawn[name]
    N, nf = len(rec), len(f)
    a2 = O.area2(v, f)
    bins = np.arange(nf) * 32 // nf
    expect = N * np.bincount(bins, weights=a2, minlength=32) / a2.sum()
    seen = np.bincount(bins[rec["face"]], minlength=32)
    chi2 = float(((seen - expect) ** 2 / expect).sum())
    tri = widen(v)[f]
    centroid = (a2[:, None] * tri.mean(axis=1)).sum(axis=0) / a2.sum()
    p = rec["point"]
    unit = np.sqrt(np.trace(np.cov(p.T)) / N)
    off = float(np.linalg.norm(p.mean(axis=0) - centroid))
    print(f"{name}: chi2 {chi2:.1f} (bound 61.1), |mean - centroid| {off:.3f} mm = {off / unit:.2f} units of sqrt(trace cov / N) (bound 3)")
    assert info["status"] == 0 and info["kept"] == N
    assert chi2 < 61.1
    assert off <= 3.0 * unit
    # every point lies on its face: the weights are barycentric
    A, B, C = tri[rec["face"], 0], tri[rec["face"], 1], tri[rec["face"], 2]
    w = 1.0 - rec["u"] - rec["v"]
    assert (w >= -1e-15).all() and np.abs(w[:, None] * A + rec["u"][:, None] * B + rec["v"][:, None] * C - p).max() <= 1e-10


def min_d2(a, b, skip_self=False):
    """for every point of a the smallest d2 = (dx dx + dy dy) + dz dz to a point of b (skip_self: a is b, the point itself left out)"""
    out = np.empty(len(a))
    for i0 in range(0, len(a), 256):
        d = a[i0:i0 + 256, None, :] - b[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        if skip_self:
            d2[np.arange(len(d2)), i0 + np.arange(len(d2))] = np.inf
        out[i0:i0 + 256] = d2.min(axis=1)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_quality_of_the_thinning(drawn, name):
    p = drawn[name][0]["point"]
    for radius in (2.0, 4.0):
        keep, kept, rounds, status = O.thin(p, radius)
        print(f"{name}: radius {radius}: kept {kept} of {len(p)} in {rounds} rounds")
        assert status == 0 and rounds <= O.MAX_ROUNDS and kept == (keep == 1).sum() and set(keep) <= {0, 1}
        k, r = p[keep == 1], p[keep == 0]
        assert min_d2(k, k, skip_self=True).min() >= radius * radius                 # no two kept points closer than the radius
        assert (min_d2(r, k) < radius * radius).all()                                 # every removed point has a kept one within it


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/sample_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = O.build_shim(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sample_check: ok" in r.stdout and not r.stderr, (r.stdout, r.stderr)
