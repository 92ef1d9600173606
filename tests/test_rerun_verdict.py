"""The capacity verdict of a run (shoulder_amd/csrc/sh_demand.h demand_verdict: what sh_collect and redo_given_up ask once the
demand words are on the host), without a GPU.  The expected values are the rules sh_collect has applied so far, written out
here: word 6 first, then words 8 / 9 (only for a run with SH_STAGE_OBB on the resident batch), then the pools and the end
sections; growth to need + need // 4, never below the old capacity; the silhouette demand clamped to 2^30; an end section
above 2^26 points and a silhouette demand that did not rise are errors."""
import ctypes
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
NONE, TIER, OBB_TIER, POOLS, FORCE_HOST = range(5)
SEG_NEED, RING_NEED, WORK_NEED, TIER_MISSED, END_NEED, SIL_NEED, NF_OVER = 3, 4, 5, 6, 7, 8, 9
NCTR = 16
CAPS = dict(seg=1 << 18, ring=1 << 18, work=32 << 20, end=8192, sil=0, nf=0)      # a fresh context's
ERR_END = "an end section has more than 2^26 crossing points"
ERR_SIL = "k_obb_candidates: silhouette demand did not shrink on the workspace tier"
KEYS = ("seg", "ring", "work", "end", "sil", "nf")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("demand_check") / "libdemand_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "hostcheck", "demand_check.cpp")])
    L = ctypes.CDLL(str(so))
    L.dc_verdict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p)]
    return L


def verdict(L, words, caps, obb=True, same=True):
    w = (ctypes.c_ulonglong * NCTR)(*[words.get(i, 0) for i in range(NCTR)])
    ci = (ctypes.c_ulonglong * 6)(*[caps[k] for k in KEYS])
    co = (ctypes.c_ulonglong * 6)()
    err = ctypes.c_char_p()
    r = L.dc_verdict(w, ci, int(obb), int(same), co, ctypes.byref(err))
    return r, dict(zip(KEYS, [int(x) for x in co])), (err.value.decode() if err.value else None)


def parent_rules(words, caps, obb, same):
    """sh_collect's decision at the parent commit, as plain Python: (reason, capacities after, error text or None)"""
    w = [words.get(i, 0) for i in range(NCTR)]
    new = dict(caps)
    if w[TIER_MISSED] != 0:
        return TIER, new, None
    if (w[SIL_NEED] != 0 or w[NF_OVER] != 0) and obb and same:
        if w[SIL_NEED] <= caps["sil"] and not (w[NF_OVER] != 0 and not caps["nf"]):
            return OBB_TIER, new, ERR_SIL
        new["sil"] = max(caps["sil"], min(w[SIL_NEED], 1 << 30))
        if w[NF_OVER] != 0:
            new["nf"] = 1
        return OBB_TIER, new, None
    if w[SEG_NEED] > caps["seg"] or w[RING_NEED] > caps["ring"] or w[WORK_NEED] > caps["work"] or w[END_NEED] > caps["end"]:
        for k, i in (("seg", SEG_NEED), ("ring", RING_NEED), ("work", WORK_NEED)):
            new[k] = max(caps[k], w[i] + w[i] // 4)
        if w[END_NEED] > caps["end"]:
            if w[END_NEED] > (1 << 26):
                return POOLS, new, ERR_END
            new["end"] = w[END_NEED] + w[END_NEED] // 4
        return POOLS, new, None
    return NONE, new, None


def test_the_words_keep_their_places(tmp_path):
    """a g++-compiled probe of the header (no HIP): the names of the demand words have the values the kernels were built with"""
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include "sh_demand.h"\nusing namespace sh;\n'
                   'int main() { printf("%d %d %d %d %d %d %d %d %d %d %d\\n", SH_CTR_SEG_USED, SH_CTR_RING_USED, SH_CTR_WORK_USED, SH_CTR_SEG_NEED, '
                   'SH_CTR_RING_NEED, SH_CTR_WORK_NEED, SH_CTR_TIER_MISSED, SH_CTR_END_NEED, SH_CTR_SIL_NEED, SH_CTR_NF_OVER, SH_NCTR);\n'
                   '  printf("%zu %zu %zu\\n", StatusBlock::words_off(3), StatusBlock::bytes(3), StatusBlock::bytes(64)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(x) for x in out[0].split()] == list(range(10)) + [16]
    # [err: B ints | pad to 8 | 16 x u64 | give-up: B ints]
    assert [int(x) for x in out[1].split()] == [16, 16 + 128 + 12, 256 + 128 + 256]


# (words, capacity overrides, obb, same) -> (reason, capacities that change, error): literal expectations
TABLE = [
    # nothing asked / all at capacity: valid
    ({}, {}, True, True, NONE, {}, None),
    ({SEG_NEED: 1 << 18, RING_NEED: 1 << 18, WORK_NEED: 32 << 20, END_NEED: 8192}, {}, True, True, NONE, {}, None),
    # every reason alone
    ({TIER_MISSED: 1}, {}, True, True, TIER, {}, None),
    ({SIL_NEED: 600}, {}, True, True, OBB_TIER, {"sil": 600}, None),
    ({NF_OVER: 1}, {}, True, True, OBB_TIER, {"nf": 1}, None),
    ({SEG_NEED: (1 << 18) + 1}, {}, True, True, POOLS, {"seg": (1 << 18) + 1 + (1 << 16)}, None),
    ({RING_NEED: (1 << 18) + 1}, {}, True, True, POOLS, {"ring": (1 << 18) + 1 + (1 << 16)}, None),
    ({WORK_NEED: (32 << 20) + 1}, {}, True, True, POOLS, {"work": (32 << 20) + 1 + (8 << 20)}, None),
    ({END_NEED: 8193}, {}, True, True, POOLS, {"end": 8193 + 2048}, None),
    # need // 4 truncates: 1 000 003 -> + 250 000; the pools that did not overflow keep their capacity (max with the old one)
    ({SEG_NEED: 1000003, RING_NEED: 7}, {}, True, True, POOLS, {"seg": 1250003}, None),
    ({END_NEED: 10007}, {}, True, True, POOLS, {"end": 12508}, None),
    # the 2^26 limit of an end section: at it a rerun, above it the error (the pools are grown by then)
    ({END_NEED: 1 << 26}, {}, True, True, POOLS, {"end": (1 << 26) + (1 << 24)}, None),
    ({END_NEED: (1 << 26) + 1, SEG_NEED: 400000}, {}, True, True, POOLS, {"seg": 500000}, ERR_END),
    # (the limit is on a demand above the capacity: end sections grown to 1.25 x 2^26 hold 2^26 + 1 points)
    ({END_NEED: (1 << 26) + 1, SEG_NEED: 400000}, {"end": (1 << 26) + (1 << 24)}, True, True, POOLS, {"seg": 500000}, None),
    # silhouette demand: clamp to 2^30; not above what the tier was chosen for -> error, unless word 9 is new
    ({SIL_NEED: (1 << 30) + 5}, {}, True, True, OBB_TIER, {"sil": 1 << 30}, None),
    ({SIL_NEED: 600}, {"sil": 600}, True, True, OBB_TIER, {}, ERR_SIL),
    ({SIL_NEED: 601}, {"sil": 600}, True, True, OBB_TIER, {"sil": 601}, None),
    ({SIL_NEED: 600, NF_OVER: 1}, {"sil": 600}, True, True, OBB_TIER, {"nf": 1}, None),
    ({SIL_NEED: 600, NF_OVER: 1}, {"sil": 600, "nf": 1}, True, True, OBB_TIER, {}, ERR_SIL),
    ({NF_OVER: 1}, {"sil": 0, "nf": 1}, True, True, OBB_TIER, {}, ERR_SIL),
    # words 8 / 9 of a run without SH_STAGE_OBB, or of an older batch: ignored
    ({SIL_NEED: 600, NF_OVER: 1}, {}, False, True, NONE, {}, None),
    ({SIL_NEED: 600, NF_OVER: 1}, {}, True, False, NONE, {}, None),
    ({SIL_NEED: 600, SEG_NEED: 400000}, {}, True, False, POOLS, {"seg": 500000}, None),
    # two reasons at once: the earlier check wins and takes nothing of the later one
    ({TIER_MISSED: 1, SIL_NEED: 600}, {}, True, True, TIER, {}, None),
    ({TIER_MISSED: 1, SEG_NEED: 400000}, {}, True, True, TIER, {}, None),
    ({TIER_MISSED: 1, END_NEED: (1 << 26) + 1}, {}, True, True, TIER, {}, None),
    ({SIL_NEED: 600, SEG_NEED: 400000}, {}, True, True, OBB_TIER, {"sil": 600}, None),
    ({NF_OVER: 1, END_NEED: 9000}, {}, True, True, OBB_TIER, {"nf": 1}, None),
    ({SEG_NEED: 400000, END_NEED: 9000}, {}, True, True, POOLS, {"seg": 500000, "end": 11250}, None),
]


@pytest.mark.parametrize("case", range(len(TABLE)))
def test_verdict_table(shim, case):
    words, over, obb, same, reason, change, error = TABLE[case]
    caps = dict(CAPS, **over)
    want = (reason, dict(caps, **change), error)
    assert parent_rules(words, caps, obb, same) == want      # (the table and the written-out rules agree)
    assert verdict(shim, words, caps, obb, same) == want


def test_verdict_grid(shim):
    """every combination of {below, at, one above, far above} per demand word x the run's two facts x two sets of capacities"""
    n = 0
    for over in ({}, {"sil": 700, "nf": 1, "seg": 1 << 20, "end": 20000}):
        caps = dict(CAPS, **over)
        vals = {SEG_NEED: (0, caps["seg"], caps["seg"] + 1, 3 * caps["seg"] + 3), RING_NEED: (0, caps["ring"] + 1), WORK_NEED: (0, caps["work"] + 2),
                TIER_MISSED: (0, 1), END_NEED: (0, caps["end"], caps["end"] + 1, 1 << 26, (1 << 26) + 1),
                SIL_NEED: (0, caps["sil"], caps["sil"] + 1, (1 << 30) + 9), NF_OVER: (0, 1)}
        for combo in itertools.product(*vals.values()):
            words = dict(zip(vals.keys(), combo))
            for obb, same in itertools.product((False, True), repeat=2):
                assert verdict(shim, words, caps, obb, same) == parent_rules(words, caps, obb, same), (words, caps, obb, same)
                n += 1
    assert n > 5000
