"""The host rules of the OBB stage (shoulder_amd/csrc/sh_obb_plan.h: what hulls need of the record and of a pinned slot, the two
growth rules, where a window's hulls come from, the early upload, and every number of the stage's launches), without a GPU.  The
expected values are what run_obb, grow_hull_records, hull_host_phase, hull_upload and the two preparation starters computed inline
before the header existed, written out here in plain Python with the lines they stood on at that commit (b1292d1), and a few
conditions stated independently of them."""
import ctypes
import itertools
import os
import subprocess

import pytest

import host_twin
from conftest import ROOT

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
START = (16384, 32768, 49152)              # SH_HV, SH_HF, SH_HE
GROWN = (20480, 40960, 61440)
HD_SLOTS, TILE, BND_DIRS = 3072, 16, 128
SMALL, LARGE, WORKSPACE = range(3)
REDO, DEVICE, PREPARED, FOREGROUND = range(4)
PLAN_KEYS = ("tier", "TT", "nemax", "area2_grid", "bnd_tiles", "bounds_grid", "ntiles", "mode0", "nt_pass0", "grid0", "mode1", "nt_pass1", "grid1",
             "nwg", "silcap", "ws_fmask", "ws_lists", "ws_sxy", "ws_area")
NFMAX = (1, 16, 17, 2732, 8192, 8193, 32768, 32769)
SIL = (0, 512, 513, 2048, 2049)
BS = (1, 7, 8, 9, 64)
i3 = ctypes.c_int * 3


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("obb_plan_check") / "libobb_plan_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "hostcheck", "obb_plan_check.cpp")])
    L = ctypes.CDLL(str(so))
    P = ctypes.c_void_p
    for name, args in dict(oc_hull_need=[P, ctypes.c_int, P], oc_hull_fits=[P, P], oc_record_grown=[P, P, P], oc_pitch_grown=[P, P], oc_start_caps=[P],
                           oc_hull_source=[ctypes.c_int] * 5 + [P], oc_early_upload_ok=[ctypes.c_int, ctypes.c_int, P, P],
                           oc_obb_plan=[ctypes.c_int, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]).items():
        getattr(L, name).argtypes = args
    return L


def test_the_header_compiles_alone(tmp_path):
    """sh_obb_plan.h by itself, plain g++, warnings are errors, no HIP include on the path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "sh_obb_plan.h"\nint main() { sh::HullNeed n = {1, 1, 1}; sh::HullCap c = {SH_HV, SH_HF, SH_HE};\n'
                   '  return !sh::hull_fits(n, c) || sh::obb_plan(1, 1, c, 0, false, true).tier != sh::OBB_TIER_SMALL || sh::hull_source(0, false, -1) != sh::HULL_FOREGROUND; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(tmp_path / "alone"), str(src)])
    subprocess.check_call([str(tmp_path / "alone")])


def test_the_constants_the_expected_values_are_written_with(shim):
    out = (ctypes.c_int * 5)()
    shim.oc_start_caps(out)
    assert tuple(out) == START + (HD_SLOTS, TILE)


# ---- the launch plan -------------------------------------------------------------------------------------------------------------------
def parent_plan(B, nfmax, hc, sil_need, nf_over, prune):
    """run_obb at the parent commit, shoulder_hip.hip:1075-1115, statement by statement (C's integer division on non-negative values)"""
    hv, hf, he = hc
    nemax = 3 * nfmax // 2 + 3
    area2_grid = (min(nemax, he) + 255) // 256
    bnd_tiles = (nfmax + BND_DIRS - 1) // BND_DIRS
    bounds_grid = bnd_tiles * ((B + 7) // 8) * 8
    huge = nfmax > 32768 or sil_need > 2048 or bool(nf_over)
    big = (not huge) and (nfmax > 8192 or sil_need > 512)
    TT = 8 if (big or huge) else TILE
    ntiles = (nfmax + TT - 1) // TT
    nwg = silcap = 0
    ws = [0, 0, 0, 0]
    if huge:
        nwg = 256
        silcap = max(hv + 64, sil_need + sil_need // 8)
        ws = [nwg * hf, nwg * 8 * silcap * 4, nwg * silcap * 16, nwg * silcap * 8]
    passes = []
    for p in (0, 1):
        mode = p if (prune or p == 0) else 2
        nt_pass = TILE // TT if p == 0 else ntiles
        grid = nt_pass * ((B + 7) // 8) * 8
        if huge:
            grid = min(grid, nwg)
        passes += [mode, nt_pass, grid]
    tier = WORKSPACE if huge else LARGE if big else SMALL
    return dict(zip(PLAN_KEYS, [tier, TT, nemax, area2_grid, bnd_tiles, bounds_grid, ntiles] + passes + [nwg, silcap] + ws))


def plan(L, B, nfmax, hc, sil_need, nf_over, prune):
    out = (ctypes.c_longlong * 19)()
    L.oc_obb_plan(B, nfmax, i3(*hc), sil_need, nf_over, prune, out)
    return dict(zip(PLAN_KEYS, [int(x) for x in out]))


PRODUCT = list(itertools.product(NFMAX, SIL, (0, 1), BS, (0, 1), (START, GROWN)))


def test_obb_plan_equals_the_parents_expressions(shim):
    assert len(PRODUCT) == 1600
    for nfmax, sil, over, B, prune, hc in PRODUCT:
        assert plan(shim, B, nfmax, hc, sil, over, prune) == parent_plan(B, nfmax, hc, sil, over, prune), (nfmax, sil, over, B, prune, hc)


def test_obb_plan_sanity(shim):
    """stated without the parent: the survivors' pass reaches every face, the seed pass is one tile of SH_OBB_TILE directions, the tiled
    grids come in rows of 8 humeri (the XCD-aware order of the kernels) unless the workspace tier's walk clamps them, and a workspace
    list holds a cycle through every hull vertex"""
    for nfmax, sil, over, B, prune, hc in PRODUCT:
        p = plan(shim, B, nfmax, hc, sil, over, prune)
        what = (nfmax, sil, over, B, prune, hc)
        assert p["nt_pass1"] * p["TT"] >= nfmax, what
        assert p["nt_pass0"] * p["TT"] == TILE, what
        assert p["bnd_tiles"] * BND_DIRS >= nfmax and p["area2_grid"] * 256 >= min(p["nemax"], hc[2]), what
        assert p["bounds_grid"] % 8 == 0 and p["bounds_grid"] // 8 == p["bnd_tiles"] * ((B + 7) // 8), what
        for k in ("0", "1"):
            full = p["nt_pass" + k] * ((B + 7) // 8) * 8
            if p["tier"] == WORKSPACE and full > 256:
                assert p["grid" + k] == 256, what
            else:
                assert p["grid" + k] == full and full % 8 == 0 and full >= B * p["nt_pass" + k], what
        assert (p["mode0"], p["mode1"]) == ((0, 1) if prune else (0, 2)), what
        assert (p["tier"] == WORKSPACE) == (nfmax > 32768 or sil > 2048 or bool(over)), what
        assert (p["tier"] == SMALL) == (nfmax <= 8192 and sil <= 512 and not over), what
        if p["tier"] == WORKSPACE:
            assert p["nwg"] == 256 and p["silcap"] >= hc[0] + 64 and p["silcap"] >= sil, what
            assert (p["ws_fmask"], p["ws_lists"], p["ws_sxy"], p["ws_area"]) == (256 * hc[1], 256 * 8 * p["silcap"] * 4, 256 * p["silcap"] * 16, 256 * p["silcap"] * 8), what
        else:
            assert (p["nwg"], p["silcap"], p["ws_fmask"], p["ws_lists"], p["ws_sxy"], p["ws_area"]) == (0,) * 6, what


# ---- hull counts -------------------------------------------------------------------------------------------------------------------------
def need(L, counts, B):
    out = i3()
    L.oc_hull_need((ctypes.c_int * len(counts))(*counts), B, out)
    return tuple(out)


def parent_need(counts, B):
    """the loop of hull_fits (shoulder_hip.hip:1006-1007), of hull_upload (hull.hip:289-290) and, for the faces, of run_obb (:1042, :1059)"""
    nv = nf = ne = 1
    for b in range(B):
        nv, nf, ne = max(nv, counts[b]), max(nf, counts[B + b]), max(ne, counts[2 * B + b])
    return nv, nf, ne


def test_hull_need(shim):
    for B in (1, 3):
        assert need(shim, [0] * (3 * B), B) == (1, 1, 1)
        for a, b in itertools.product(range(3), range(B)):      # the maximum in the first, middle, last humerus of each array
            counts = [5 + i for i in range(3 * B)]
            counts[a * B + b] = 9000 + a
            want = [max(counts[k * B:(k + 1) * B]) for k in range(3)]
            assert want[a] == 9000 + a
            assert need(shim, counts, B) == tuple(want) == parent_need(counts, B), (B, a, b)


def test_hull_fits(shim):
    fits = lambda n, c: shim.oc_hull_fits(i3(*n), i3(*c))
    assert fits(START, START) == 1 and fits((1, 1, 1), START) == 1
    for k in range(3):
        over = list(START)
        over[k] += 1
        assert fits(over, START) == 0 and fits(over, GROWN) == 1
        under = [1, 1, 1]
        under[k] = START[k]
        assert fits(under, START) == 1


# ---- the two growth rules ------------------------------------------------------------------------------------------------------------------
def parent_record_grown(now, n):
    """grow_hull_records, shoulder_hip.hip:1016-1020"""
    up = lambda x: (x + x // 8 + 1023) // 1024 * 1024
    return tuple(up(x) if x > cap else cap for cap, x in zip(now, n))


def parent_pitch_grown(demands):
    """hull_host_phase, hull.hip:269-272: `demands` the (v, f, e) of the humeri that did not fit"""
    dv, df, de = START
    for d in demands:
        dv, df, de = max(dv, d[0]), max(df, d[1]), max(de, d[2])
    up = lambda x: (x + 1023) // 1024 * 1024
    return up(dv), up(df), up(de)


def record_grown(L, now, n):
    out = i3()
    L.oc_record_grown(i3(*now), i3(*n), out)
    return tuple(out)


def pitch_grown(L, d):
    out = i3()
    L.oc_pitch_grown(i3(*d), out)
    return tuple(out)


def test_hull_record_grown(shim):
    """16 385 vertices: the rule, (x + x / 8 + 1023) / 1024 * 1024, gives (16 385 + 2 048 + 1 023) / 1024 * 1024 = 19 * 1024 = 19 456, and
    so did grow_hull_records before the header.  (The issue that asked for this test names 18 432 "by the formula": that is 18 433
    rounded DOWN to a multiple of 1024, which would not even hold the headroom; the formula rounds up.  The formula is what is pinned.)"""
    assert record_grown(shim, START, START) == START                                   # a need equal to the capacity: nothing
    assert (16385 + 16385 // 8 + 1023) // 1024 * 1024 == 19456
    assert record_grown(shim, START, (16385, 1, 1)) == (19456, START[1], START[2])
    assert record_grown(shim, GROWN, START) == GROWN                                   # never shrinks
    values = (1, 16384, 16385, 20480, 32768, 32769, 49152, 49153, 100000)
    for now in (START, GROWN):
        for n in itertools.product(values, repeat=3):
            g = record_grown(shim, now, n)
            assert g == parent_record_grown(now, n), (now, n)
            for k in range(3):
                assert (g[k] == now[k]) if n[k] <= now[k] else (g[k] >= n[k] and g[k] % 1024 == 0), (now, n, k)


def test_hull_pitch_grown(shim):
    assert pitch_grown(shim, (1, 1, 1)) == START and pitch_grown(shim, (4097, 8193, 12289)) == START      # below the start capacity: the start capacity
    assert pitch_grown(shim, (1, 40000, 1)) == (START[0], 40960, START[2])
    values = (1, 4097, 16384, 16385, 32768, 40000, 49152, 49153, 100000)
    for d in itertools.product(values, repeat=3):
        assert pitch_grown(shim, d) == parent_pitch_grown([d]), d
        assert pitch_grown(shim, d) == parent_pitch_grown([(d[0], 1, 1), (1, d[1], 1), (1, 1, d[2])]), d      # the maxima of several humeri
    # the rules differ: the record leaves headroom where it grows, the slot takes what is asked
    assert record_grown(shim, START, (1, 40000, 1))[1] == 45056 and pitch_grown(shim, (1, 40000, 1))[1] == 40960


# ---- where a window's hulls come from ------------------------------------------------------------------------------------------------------
def parent_source(redo_nf, device_now, prepared_slot, uploaded, skip_nfmax, slot_nf):
    """the `if` chain of run_obb, shoulder_hip.hip:1044-1068 -> (source, the foreground uploads, nfmax)"""
    if redo_nf > 0:
        return REDO, False, redo_nf
    if device_now:
        return DEVICE, False, max(HD_SLOTS, skip_nfmax)      # (run_device_hull, hull.hip:317)
    src = FOREGROUND if prepared_slot < 0 else PREPARED
    return src, not (prepared_slot >= 0 and uploaded), max(1, slot_nf)


def test_hull_source(shim):
    out = (ctypes.c_int * 5)()
    for redo, dev, prep, skip, slot_nf in itertools.product((0, 2732), (0, 1), (-1, 0, 1), (0, 2732, 9000), (1, 2732)):
        shim.oc_hull_source(redo, dev, prep, skip, slot_nf, out)
        src, from_host, pending, pending_uploaded, nfmax = out
        for uploaded, got in ((False, pending), (True, pending_uploaded)):
            assert (src, bool(got), nfmax) == parent_source(redo, dev, prep, uploaded, skip, slot_nf), (redo, dev, prep, uploaded, skip, slot_nf)
        assert bool(from_host) == (src in (PREPARED, FOREGROUND))
    shim.oc_hull_source(5, 1, 1, 0, 1, out)      # redo wins, then the device, then the prepared slot
    assert out[0] == REDO
    shim.oc_hull_source(0, 1, 1, 0, 1, out)
    assert out[0] == DEVICE
    shim.oc_hull_source(0, 0, 1, 0, 1, out)
    assert out[0] == PREPARED and (out[2], out[3]) == (1, 0)      # the upload is still to do unless the thread did it
    shim.oc_hull_source(0, 0, -1, 0, 1, out)
    assert out[0] == FOREGROUND and (out[2], out[3]) == (1, 1)


# ---- the early upload ----------------------------------------------------------------------------------------------------------------------
def test_early_upload_ok(shim):
    ok = lambda ev, B, hc, z: shim.oc_early_upload_ok(ev, B, i3(*hc), (ctypes.c_ulonglong * 6)(*z))
    for B, hc in itertools.product((1, 7, 64), (START, GROWN)):
        exact = [B * hc[0] * 24, B * hc[1] * 24, B * hc[2] * 16, B * 4, B * 4, B * 4]      # (start_prepare_staged, shoulder_hip.hip:1533-1534)
        assert ok(1, B, hc, exact) == 1 and ok(0, B, hc, exact) == 0
        assert ok(1, B, hc, [2 * x for x in exact]) == 1
        for k in range(6):
            short = list(exact)
            short[k] -= 1
            assert ok(1, B, hc, short) == 0, (B, hc, k)
        assert ok(1, B, hc, [0] * 6) == 0      # (buffers that do not exist yet)


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/obb_plan_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = host_twin.build_shim("obb_plan", tmp_path, sanitize=True, std="c++17")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "obb_plan_check OK (1600 plans)" in r.stdout, r.stdout + r.stderr
