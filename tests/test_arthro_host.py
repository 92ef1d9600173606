"""The host decisions of the arthroplasty chain (shoulder_amd/csrc/sh_arthro.h: what sh_resect_*, sh_resect_ring, sh_canal_profile,
sh_resect_stems and sh_resect_plan check and which refusal comes first; how a sweep is split into passes and how large every
resect.* / canal.* / stem.* / plan.* buffer is; ArthroState, what is valid against what), without a GPU.  Every expected value is the
rule the entry points applied before the header existed, written out here (`Parent`: the thirteen context fields and the five
prologues; `parent_*_sizes`: the arithmetic of resect_ensure and the three ENS_SHARED blocks) -- none is the header's own output.
A text is the one BEHIND the entry point's name ("sh_resect_planes: " is the caller's)."""
import copy
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hostcheck", "arthro_check.cpp")
OK, ERR_ARG, ERR_STATE = 0, -1, -3
ANP, CSYS, ALL = 1 << 6, 1 << 9, 0x7FF
NONE = (1 << 64) - 1
RECORDS, FIT, SEAT = 0, 1, 2
CENTROID, SPHERE = 0, 1
MAXSEG = 1024
# sizeof of the records of include/shoulder_hip.h
S_RESECTION, S_HEAD_FIT, S_SEAT, S_HEAD, S_OFFSET, S_LEVEL, S_STEM, S_STEM_FIT, S_PLAN, S_PLAN_REF = 136, 128, 232, 16, 56, 104, 24, 128, 112, 96

E_RESECT_ARG = "bad argument (P in 1..4096)"
E_CATALOGUE = "bad catalogue (K in 1..64, 0 < thickness < 2 radius) or centre mode"
E_NO_MESHES = "no meshes uploaded"
E_IN_FLIGHT = "runs are in flight (sh_collect them first)"
E_NEEDS_RUN = "needs a run of the resident batch with SH_STAGE_ANP and SH_STAGE_CSYS"
E_OFFSET = "non-finite offset"
E_PLANE = "zero normal or non-finite plane"
E_RING_ARG = "bad argument"
E_NO_RESECTION = "no resection of the resident batch"
E_INDEX = "index out of range"
E_GRID = "bad grid (finite z0, dz > 0, L in 1..1024, A in 3..256)"
E_FRAME = "frame %d is not a rigid CT -> frame matrix"
E_FRAMES_NULL = "frames == NULL " + E_NEEDS_RUN
E_STEMS_ARG = "bad argument (K in 1..64)"
E_STEM = "length, r_prox and r_tip of a stem must be finite and > 0"
E_NO_PROFILE = "no canal profile of the resident batch"
E_PLAN_ARG = "bad argument (N in 1..64)"
E_RULE = "bad rule (no NaN, weights finite and >= 0, margin >= 0)"
E_NOT_SEATED = "no seated resection of the resident batch (sh_resect_planes_seat / sh_resect_offsets_seat)"
E_STALE_STEMS = "no stems fitted against the last resection and the current canal profile (sh_resect_stems)"
E_REF_NULL = "ref_planes == NULL " + E_NEEDS_RUN
E_REF_PLANE = "reference plane %d has a zero normal or is not finite"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("arthro_check") / "libarthro_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(so), SRC])
    L = ctypes.CDLL(str(so))
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.ac_new.restype = vp
    L.ac_clone.restype = vp
    L.ac_clone.argtypes = [vp]
    L.ac_free.argtypes = [vp]
    L.ac_event.argtypes = [vp, i, i, i, i]
    L.ac_query.argtypes = [vp, vp]
    L.ac_names.argtypes = [vp]
    L.ac_pre_resect.argtypes = [i, vp, vp, i, i, i, vp, i, i, i, i, i, i, i, vp, vp, i]
    L.ac_pre_ring.argtypes = [i, i, i, i, i, i, i, i, i, vp, vp, i]
    L.ac_pre_profile.argtypes = [vp, vp, i, i, i, i, vp, vp, i]
    L.ac_pre_stems.argtypes = [vp, i, i, i, i, i, i, vp, vp, i]
    L.ac_pre_plan.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, i]
    L.ac_resect_plan.argtypes = [i, i, ll, i, i, i, vp, vp, vp]
    L.ac_ring_tiles.argtypes = [ll]
    L.ac_canal_plan.argtypes = [i, i, i, ll, vp, vp, vp]
    L.ac_stem_bytes.argtypes = [i, i, i, vp, vp]
    L.ac_plan_plan.argtypes = [i, i, i, i, i, ll, vp, vp, vp]
    names = (ctypes.c_char_p * 64)()
    L.names = [names[k].decode() for k in range(L.ac_names(names))]
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, np.float64).reshape(-1)


def test_header_builds_with_gxx_alone(tmp_path):
    """compile-only: sh_arthro.h needs no HIP header and no hipcc"""
    src = tmp_path / "probe.cpp"
    src.write_text('#include "sh_arthro.h"\nint main() { sh::ArthroState s; sh::ArthroBytes z = sh::resect_plan(1, 1, 4, sh::RS_SEAT, 1, false).bytes;\n'
                   '  return (int)z.seat_out + s.P() + (int)sh::plan_plan(1, 1, 1, 1, 1, 4).cuts; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)])


def test_shim_runs_as_a_program(tmp_path):
    """the stand-alone main() of the shim (one case of each group; the form a sanitizer build takes) builds and passes"""
    exe = tmp_path / "arthro_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DARTHRO_CHECK_MAIN", "-o", str(exe), SRC])
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip() == "arthro_check: ok"


# ---- the parent's rules, written out ----------------------------------------------------------------------------------------------------
def plane_bad(planes, n):
    """index of the first of n planes that is not six finite doubles with a non-zero normal, or -1"""
    p = np.asarray(planes, np.float64).reshape(-1, 6)[:n]
    with np.errstate(all="ignore"):
        good = np.isfinite(p).all(axis=1) & ((p[:, 3] * p[:, 3] + p[:, 4] * p[:, 4]) + p[:, 5] * p[:, 5] > 0.0)
    bad = np.flatnonzero(~good)
    return int(bad[0]) if len(bad) else -1


def heads_ok(heads, K, mode, seat_out):
    if heads is None or not seat_out or K < 1 or K > 64 or mode not in (CENTROID, SPHERE):
        return False
    for R, h in np.asarray(heads, np.float64).reshape(-1, 2)[:K].tolist():
        if not np.isfinite(R) or not np.isfinite(h) or not h > 0.0 or not h < 2.0 * R:
            return False
    return True


def grid_ok(g):
    if g is None:
        return False
    z0, dz, Lv, A = g
    return bool(np.isfinite(z0) and np.isfinite(dz) and dz > 0.0 and 1 <= Lv <= 1024 and 3 <= A <= 256)


def frame_ok(T):
    T = [float(x) for x in T]
    if not all(np.isfinite(x) for x in T):
        return False
    if T[12] != 0.0 or T[13] != 0.0 or T[14] != 0.0 or T[15] != 1.0:
        return False
    for i in range(3):
        for j in range(i, 3):
            d = (T[4 * i] * T[4 * j] + T[4 * i + 1] * T[4 * j + 1]) + T[4 * i + 2] * T[4 * j + 2]
            if not abs(d - (1.0 if i == j else 0.0)) <= 1e-9:
                return False
    return T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]) > 0.0


def rule_ok(r):
    r = [float(x) for x in r]      # max_overhang, min_coverage, min_clearance, max_eccentricity, fill_target, margin, six weights
    if any(np.isnan(x) for x in r):
        return False
    if any(not np.isfinite(w) or w < 0.0 for w in r[6:12]):
        return False
    return r[5] >= 0.0


class Parent:
    """A context as the parent commit holds it: the thirteen fields of the chain, the facts its prologues read, and the five prologues
    in the parent's order.  A call returns (code, text); text None: no context to hold one."""

    def __init__(self):
        self.ctx, self.B, self.n_pending, self.landmarks, self.batch_gen = True, 0, 0, False, 0
        self.rec_mask, self.rec_gen, self.resect_gen, self.resect_P = 0, NONE, NONE, 0
        self.canal_gen, self.canal_grid = NONE, (0, 0)
        self.resect_seq, self.canal_seq = 0, 0
        self.seat_resect_seq, self.stem_resect_seq, self.stem_canal_seq, self.seat_K, self.stem_K = NONE, NONE, NONE, 0, 0

    # what happens between the calls
    def upload(self, B=1):
        self.batch_gen += 1
        self.B, self.landmarks = B, True      # (alloc_batch allocates "landmarks")

    def run(self, mask):
        self.rec_mask, self.rec_gen = mask, self.batch_gen

    # the expressions the prologues compare by hand
    def has_records(self):
        return self.rec_gen == self.batch_gen and (self.rec_mask & (ANP | CSYS)) == (ANP | CSYS) and self.landmarks

    def resected(self):
        return self.resect_gen == self.batch_gen and self.resect_P >= 1

    def seated(self):
        return self.resected() and self.seat_resect_seq == self.resect_seq

    def profiled(self):
        return self.canal_gen == self.batch_gen

    def stems_current(self):
        return self.profiled() and self.stem_resect_seq == self.resect_seq and self.stem_canal_seq == self.canal_seq

    def queries(self):
        return [int(self.has_records()), int(self.resected()), int(self.seated()), int(self.profiled()), int(self.stems_current()), self.resect_P, self.seat_K,
                self.stem_K, self.canal_grid[0], self.canal_grid[1]]

    def _refuse(self, code, text):
        return code, (text if self.ctx else None)

    # resect_run
    def resect(self, level, planes=None, offs=None, P=1, out=True, fit_out=True, heads=None, K=0, mode=CENTROID, seat_out=True, fail=False):
        if not self.ctx or (offs is None and planes is None) or not out or (level >= FIT and not fit_out) or P < 1 or P > 4096:
            return self._refuse(ERR_ARG, E_RESECT_ARG)
        if level == SEAT and not heads_ok(heads, K, mode, seat_out):
            return ERR_ARG, E_CATALOGUE
        if self.B < 1:
            return ERR_STATE, E_NO_MESHES
        if self.n_pending != 0:
            return ERR_STATE, E_IN_FLIGHT
        if offs is not None:
            if not self.has_records():
                return ERR_STATE, E_NEEDS_RUN
            if not np.isfinite(np.asarray(offs, np.float64).reshape(-1)[:7 * P]).all():
                return ERR_ARG, E_OFFSET
        elif plane_bad(planes, self.B * P) >= 0:
            return ERR_ARG, E_PLANE
        self.resect_gen = NONE
        self.resect_seq += 1
        if fail:
            return OK, ""
        self.resect_P, self.resect_gen = P, self.batch_gen
        if level == SEAT:
            self.seat_resect_seq, self.seat_K = self.resect_seq, K
        return OK, ""

    def ring(self, b, p, out=True, cap=8, n_out=True):
        if not self.ctx or not n_out or cap < 0 or (cap > 0 and not out):
            return self._refuse(ERR_ARG, E_RING_ARG)
        if self.n_pending != 0:
            return ERR_STATE, E_IN_FLIGHT
        if self.resect_gen != self.batch_gen or self.resect_P < 1:
            return ERR_STATE, E_NO_RESECTION
        if b < 0 or b >= self.B or p < 0 or p >= self.resect_P:
            return ERR_ARG, E_INDEX
        return OK, ""

    def profile(self, grid, frames=None, fail=False):
        if not self.ctx or not grid_ok(grid):
            return self._refuse(ERR_ARG, E_GRID)
        if self.B < 1:
            return ERR_STATE, E_NO_MESHES
        if self.n_pending != 0:
            return ERR_STATE, E_IN_FLIGHT
        if frames is not None:
            for b in range(self.B):
                if not frame_ok(np.asarray(frames, np.float64).reshape(-1)[16 * b:16 * b + 16]):
                    return ERR_ARG, E_FRAME % b
        elif not self.has_records():
            return ERR_STATE, E_FRAMES_NULL
        self.canal_gen = NONE
        self.canal_seq += 1
        if fail:
            return OK, ""
        self.canal_grid, self.canal_gen = (grid[2], grid[3]), self.batch_gen
        return OK, ""

    def stems(self, stems, K, out=True, fail=False):
        if not self.ctx or stems is None or not out or K < 1 or K > 64:
            return self._refuse(ERR_ARG, E_STEMS_ARG)
        for x in np.asarray(stems, np.float64).reshape(-1)[:3 * K].tolist():
            if not np.isfinite(x) or not x > 0.0:
                return ERR_ARG, E_STEM
        if self.n_pending != 0:
            return ERR_STATE, E_IN_FLIGHT
        if self.B < 1 or self.resect_gen != self.batch_gen or self.resect_P < 1:
            return ERR_STATE, E_NO_RESECTION
        if self.canal_gen != self.batch_gen:
            return ERR_STATE, E_NO_PROFILE
        self.stem_resect_seq = NONE
        if fail:
            return OK, ""
        self.stem_resect_seq, self.stem_canal_seq, self.stem_K = self.resect_seq, self.canal_seq, K
        return OK, ""

    def plan(self, rule, ref_planes=None, N=8, out=True):
        if rule is None or not out or N < 1 or N > 64:
            return self._refuse(ERR_ARG, E_PLAN_ARG)
        if not rule_ok(rule):
            return self._refuse(ERR_ARG, E_RULE)
        if not self.ctx:
            return ERR_ARG, None
        if self.n_pending != 0:
            return ERR_STATE, E_IN_FLIGHT
        if self.B < 1 or self.resect_gen != self.batch_gen or self.resect_P < 1 or self.seat_resect_seq != self.resect_seq:
            return ERR_STATE, E_NOT_SEATED
        if self.canal_gen != self.batch_gen or self.stem_resect_seq != self.resect_seq or self.stem_canal_seq != self.canal_seq:
            return ERR_STATE, E_STALE_STEMS
        if ref_planes is None and not self.has_records():
            return ERR_STATE, E_REF_NULL
        if ref_planes is not None:
            b = plane_bad(ref_planes, self.B)
            if b >= 0:
                return ERR_ARG, E_REF_PLANE % b
        return OK, ""


class Both:
    """The parent's context beside the header's (a Sim of the shim: an ArthroState and a batch generation).  Every call goes to both;
    the header's verdict must be the parent's, and an accepted call's events are applied to both."""

    def __init__(self, L, sim=None, m=None):
        self.L, self.sim, self.m = L, sim if sim is not None else L.ac_new(), m if m is not None else Parent()

    def clone(self):
        return Both(self.L, self.L.ac_clone(self.sim), copy.copy(self.m))

    def close(self):
        self.L.ac_free(self.sim)

    def facts(self):
        m = self.m
        return (int(m.ctx), m.B, m.n_pending, int(m.landmarks), self.sim if m.ctx else None)

    def _verdict(self, want, rc, text):
        got = (rc, text.value.decode())
        assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (got, want)
        return want

    def queries(self):
        q = np.zeros(10, np.int32)
        self.L.ac_query(self.sim, _p(q))
        q[0] = q[0] and self.m.landmarks      # (the "landmarks" fact is the caller's)
        assert q.tolist() == self.m.queries()
        return q.tolist()

    def upload(self, B=1):
        self.m.upload(B)
        self.L.ac_event(self.sim, 0, 0, 0, 0)

    def run(self, mask):
        self.m.run(mask)
        self.L.ac_event(self.sim, 1, mask, 0, 0)

    def resect(self, level, planes=None, offs=None, P=1, out=True, fit_out=True, heads=None, K=0, mode=CENTROID, seat_out=True, fail=False):
        pl, of, hd, text = _f64(planes), _f64(offs), _f64(heads), ctypes.create_string_buffer(256)
        rc = self.L.ac_pre_resect(level, _p(pl), _p(of), P, int(out), int(fit_out), _p(hd), K, mode, int(seat_out), *self.facts(), text, 256)
        want = self._verdict(self.m.resect(level, planes, offs, P, out, fit_out, heads, K, mode, seat_out, fail), rc, text)
        if want[0] == OK:
            self.L.ac_event(self.sim, 3 if fail else 2, level, P, K)
        return want

    def ring(self, b, p, out=True, cap=8, n_out=True):
        text = ctypes.create_string_buffer(256)
        rc = self.L.ac_pre_ring(b, p, int(out), cap, int(n_out), *self.facts(), text, 256)
        return self._verdict(self.m.ring(b, p, out, cap, n_out), rc, text)

    def profile(self, grid, frames=None, fail=False):
        fr, text = _f64(frames), ctypes.create_string_buffer(256)
        g = None if grid is None else np.array([(grid[0], grid[1], grid[2], grid[3])], dtype=[("z0", "f8"), ("dz", "f8"), ("L", "i4"), ("A", "i4")])
        rc = self.L.ac_pre_profile(_p(g), _p(fr), *self.facts(), text, 256)
        want = self._verdict(self.m.profile(grid, frames, fail), rc, text)
        if want[0] == OK:
            self.L.ac_event(self.sim, 7 if fail else 4, grid[2], grid[3], 0)
        return want

    def stems(self, stems, K, out=True, fail=False):
        st, text = _f64(stems), ctypes.create_string_buffer(256)
        rc = self.L.ac_pre_stems(_p(st), K, int(out), *self.facts(), text, 256)
        want = self._verdict(self.m.stems(stems, K, out, fail), rc, text)
        if want[0] == OK:
            self.L.ac_event(self.sim, 6 if fail else 5, K, 0, 0)
        return want

    def plan(self, rule, ref_planes=None, N=8, out=True):
        ru, rp, text = _f64(rule), _f64(ref_planes), ctypes.create_string_buffer(256)
        rc = self.L.ac_pre_plan(_p(ru), _p(rp), N, int(out), *self.facts(), text, 256)
        return self._verdict(self.m.plan(rule, ref_planes, N, out), rc, text)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _good_planes(B, P):
    p = np.zeros((B, P, 6))
    p[..., :3] = np.arange(B * P * 3).reshape(B, P, 3)
    p[..., 5] = 1.0
    return p


def good_planes(B, P):
    return _good_planes(B, P).copy()


HEADS2 = [(6.0, 3.0), (5.0, 2.0)]
GRID = (1.9, 0.069, 64, 64)
STEMS3 = [(2.8, 2.0, 1.0), (3.0, 2.9, 2.5), (2.0, 3.5, 1.0)]
RULE = [np.inf, -np.inf, -np.inf, np.inf, 0.5, 0.0, 10.0, 1.0, 0.0, 0.25, 2.0, 3.0]
EYE = np.eye(4).reshape(-1)


def frames_of(*Ts):
    return np.concatenate([np.asarray(T, np.float64).reshape(-1) for T in Ts])


def changed(a, index, value):
    a = np.array(a, np.float64)
    a.reshape(-1)[index] = value
    return a


@pytest.fixture
def ctx(shim):
    made = []

    def make(B=2, run=None, chain=False, pending=0):
        """a context with B meshes uploaded (0: none), optionally a run with `run` stages and a complete seated chain"""
        c = Both(shim)
        made.append(c)
        if B:
            c.upload(B)
        if run is not None:
            c.run(run)
        if chain:
            assert c.profile(GRID, frames_of(*[EYE] * B))[0] == OK and c.resect(SEAT, good_planes(B, 3), P=3, heads=HEADS2, K=2)[0] == OK
            assert c.stems(STEMS3, 3)[0] == OK
        c.m.n_pending = pending
        return c
    yield make
    for c in made:
        c.close()


# ---- acceptance: the code and the exact text of every check -----------------------------------------------------------------------------
@pytest.mark.parametrize("P,want", [(0, (ERR_ARG, E_RESECT_ARG)), (1, (OK, "")), (4096, (OK, "")), (4097, (ERR_ARG, E_RESECT_ARG))])
def test_planes_per_humerus(ctx, P, want):
    assert ctx(B=1).resect(RECORDS, good_planes(1, max(P, 1)), P=P) == want


@pytest.mark.parametrize("b,p,comp,value", [(1, 2, None, 0.0), (1, 0, 1, np.nan), (0, 1, 4, np.inf), (1, 2, 0, -np.inf)])
def test_a_bad_plane_that_is_not_the_first(ctx, b, p, comp, value):
    """comp None: a zero normal; otherwise component comp of plane (b, p) is not finite"""
    def spoil(planes, b, p):
        planes = planes.copy()
        if comp is None:
            planes[b, p, 3:] = 0.0
        else:
            planes[b, p, comp] = value
        return planes
    planes = spoil(good_planes(2, 3), b, p)
    assert plane_bad(planes, 6) == b * 3 + p > 0
    for level in (RECORDS, FIT, SEAT):
        assert ctx().resect(level, planes, P=3, heads=HEADS2, K=2) == (ERR_ARG, E_PLANE)
    c = ctx(chain=True)
    assert c.plan(RULE, spoil(good_planes(2, 1), 1, 0)) == (ERR_ARG, E_REF_PLANE % 1)      # the same defect in the second reference plane
    assert c.plan(RULE, good_planes(2, 1)) == (OK, "")


def test_offsets(ctx):
    offs = np.zeros((3, 7))
    assert ctx(run=ALL).resect(FIT, offs=offs, P=3) == (OK, "")
    assert ctx(run=ALL & ~ANP).resect(FIT, offs=offs, P=3) == (ERR_STATE, E_NEEDS_RUN)
    assert ctx(run=ALL & ~CSYS).resect(RECORDS, offs=offs, P=3) == (ERR_STATE, E_NEEDS_RUN)
    assert ctx().resect(RECORDS, offs=offs, P=3) == (ERR_STATE, E_NEEDS_RUN)
    for value in (np.nan, np.inf, -np.inf):
        assert ctx(run=ALL).resect(RECORDS, offs=changed(offs, 20, value), P=3) == (ERR_ARG, E_OFFSET)
    c = ctx(run=ALL)
    c.upload(2)                                                                            # the run was of the batch before
    assert c.resect(RECORDS, offs=offs, P=3) == (ERR_STATE, E_NEEDS_RUN)


@pytest.mark.parametrize("K,ok", [(0, False), (1, True), (64, True), (65, False)])
def test_heads_in_a_catalogue(ctx, K, ok):
    heads = [(6.0 + k, 3.0) for k in range(max(K, 1))]
    assert ctx().resect(SEAT, good_planes(2, 1), heads=heads, K=K) == ((OK, "") if ok else (ERR_ARG, E_CATALOGUE))


def test_head_thickness_and_centre_mode(ctx):
    R = 6.0
    for h, ok in ((0.0, False), (2.0 * R, False), (np.nextafter(2.0 * R, 0.0), True), (-1.0, False), (np.nan, False), (np.inf, False)):
        assert ctx().resect(SEAT, good_planes(2, 1), heads=[(5.0, 2.0), (R, h)], K=2) == ((OK, "") if ok else (ERR_ARG, E_CATALOGUE)), h
    assert ctx().resect(SEAT, good_planes(2, 1), heads=[(np.inf, 2.0)], K=1) == (ERR_ARG, E_CATALOGUE)
    for mode, ok in ((CENTROID, True), (SPHERE, True), (2, False), (-1, False)):
        assert ctx().resect(SEAT, good_planes(2, 1), heads=HEADS2, K=2, mode=mode) == ((OK, "") if ok else (ERR_ARG, E_CATALOGUE)), mode
    assert ctx().resect(SEAT, good_planes(2, 1), heads=None, K=2) == (ERR_ARG, E_CATALOGUE)
    assert ctx().resect(SEAT, good_planes(2, 1), heads=HEADS2, K=2, seat_out=False) == (ERR_ARG, E_CATALOGUE)
    assert ctx().resect(FIT, good_planes(2, 1), fit_out=False) == (ERR_ARG, E_RESECT_ARG)
    assert ctx().resect(RECORDS, good_planes(2, 1), fit_out=False) == (OK, "")
    assert ctx().resect(RECORDS, good_planes(2, 1), out=False) == (ERR_ARG, E_RESECT_ARG)
    assert ctx().resect(RECORDS) == (ERR_ARG, E_RESECT_ARG)                                # neither planes nor offsets


@pytest.mark.parametrize("grid,ok", [((1.0, 0.0, 8, 8), False), ((1.0, -0.5, 8, 8), False), ((np.nan, 0.5, 8, 8), False), ((1.0, np.inf, 8, 8), False),
                                     ((1.0, 0.5, 0, 8), False), ((1.0, 0.5, 1, 8), True), ((1.0, 0.5, 1024, 8), True), ((1.0, 0.5, 1025, 8), False),
                                     ((1.0, 0.5, 8, 2), False), ((1.0, 0.5, 8, 3), True), ((1.0, 0.5, 8, 256), True), ((1.0, 0.5, 8, 257), False), (None, False)])
def test_canal_grid(ctx, grid, ok):
    assert ctx().profile(grid, frames_of(EYE, EYE)) == ((OK, "") if ok else (ERR_ARG, E_GRID))


def test_frames(ctx):
    mirror = changed(EYE, 10, -1.0)                                                        # determinant -1
    assert ctx().profile(GRID, frames_of(EYE, mirror)) == (ERR_ARG, E_FRAME % 1)
    assert ctx().profile(GRID, frames_of(mirror, mirror)) == (ERR_ARG, E_FRAME % 0)
    assert ctx().profile(GRID, frames_of(EYE, changed(EYE, 0, 1.0 + 1e-9))) == (ERR_ARG, E_FRAME % 1)       # |row 0|^2 is off by 2e-9
    assert ctx().profile(GRID, frames_of(EYE, changed(EYE, 0, 1.0 + 2.5e-10))) == (OK, "")                    # ... by 5e-10
    assert ctx().profile(GRID, frames_of(EYE, changed(EYE, 1, 2e-9))) == (ERR_ARG, E_FRAME % 1)             # rows 0 and 1 off orthogonal by 2e-9
    assert ctx().profile(GRID, frames_of(EYE, changed(EYE, 1, 5e-10))) == (OK, "")
    for index, value in ((12, 1e-300), (15, np.nextafter(1.0, 2.0)), (14, -0.0 + 1.0), (3, np.nan), (7, np.inf)):      # a bad last row, a non-finite shift
        assert ctx().profile(GRID, frames_of(EYE, changed(EYE, index, value))) == (ERR_ARG, E_FRAME % 1), index
    assert ctx().profile(GRID, frames_of(EYE, changed(EYE, 3, 1e6))) == (OK, "")           # any finite shift
    assert ctx(run=ALL).profile(GRID) == (OK, "")
    assert ctx(run=ALL & ~CSYS).profile(GRID) == (ERR_STATE, E_FRAMES_NULL)
    assert ctx().profile(GRID) == (ERR_STATE, E_FRAMES_NULL)


def test_stem_catalogue(ctx):
    def ready():
        c = ctx()
        assert c.profile(GRID, frames_of(EYE, EYE))[0] == OK and c.resect(RECORDS, good_planes(2, 2), P=2)[0] == OK
        return c
    for K, ok in ((0, False), (1, True), (64, True), (65, False)):
        assert ready().stems([STEMS3[0]] * max(K, 1), K) == ((OK, "") if ok else (ERR_ARG, E_STEMS_ARG))
    for index in range(3, 6):
        for value in (0.0, -1.0, np.nan, np.inf):
            assert ready().stems(changed(STEMS3, index, value), 3) == (ERR_ARG, E_STEM), (index, value)
    assert ready().stems(None, 3) == (ERR_ARG, E_STEMS_ARG)
    assert ready().stems(STEMS3, 3, out=False) == (ERR_ARG, E_STEMS_ARG)
    c = ctx()
    assert c.stems(STEMS3, 3) == (ERR_STATE, E_NO_RESECTION)
    assert c.resect(FIT, good_planes(2, 2), P=2) == (OK, "") and c.stems(STEMS3, 3) == (ERR_STATE, E_NO_PROFILE)
    assert ctx(B=0).stems(STEMS3, 3) == (ERR_STATE, E_NO_RESECTION)


def test_plan_rule_and_size(ctx):
    c = ctx(chain=True)
    ref = good_planes(2, 1)
    for N, ok in ((0, False), (1, True), (64, True), (65, False)):
        assert c.plan(RULE, ref, N) == ((OK, "") if ok else (ERR_ARG, E_PLAN_ARG))
    for index, value, ok in ((0, np.nan, False), (4, np.nan, False), (0, -np.inf, True), (3, 0.0, True), (4, -2.0, True), (5, -1.0, False), (5, np.inf, True),
                             (6, -1.0, False), (8, -0.5, False), (9, np.inf, False), (11, np.nan, False), (11, 0.0, True)):
        assert c.plan(changed(RULE, index, value), ref) == ((OK, "") if ok else (ERR_ARG, E_RULE)), (index, value)
    assert c.plan(None, ref) == (ERR_ARG, E_PLAN_ARG) and c.plan(RULE, ref, out=False) == (ERR_ARG, E_PLAN_ARG)
    assert c.plan(RULE) == (ERR_STATE, E_REF_NULL)
    c.run(ALL)
    assert c.plan(RULE) == (OK, "")


def test_ring(ctx):
    c = ctx()
    assert c.ring(0, 0) == (ERR_STATE, E_NO_RESECTION)
    assert c.resect(RECORDS, good_planes(2, 3), P=3) == (OK, "")
    for b, p, ok in ((0, 0, True), (1, 2, True), (2, 0, False), (0, 3, False), (-1, 0, False), (0, -1, False)):
        assert c.ring(b, p) == ((OK, "") if ok else (ERR_ARG, E_INDEX))
    assert c.ring(0, 0, out=False, cap=0) == (OK, "") and c.ring(0, 0, out=False, cap=1) == (ERR_ARG, E_RING_ARG)
    assert c.ring(0, 0, cap=-1) == (ERR_ARG, E_RING_ARG) and c.ring(0, 0, n_out=False) == (ERR_ARG, E_RING_ARG)
    c.upload(2)
    assert c.ring(0, 0) == (ERR_STATE, E_NO_RESECTION)


# ---- which of two refusals comes first ----------------------------------------------------------------------------------------------------
def test_a_bad_argument_beats_runs_in_flight(ctx):
    def flying(**kw):
        return ctx(pending=1, **kw)
    assert flying().resect(RECORDS, good_planes(2, 1), P=0) == (ERR_ARG, E_RESECT_ARG)
    assert flying().resect(SEAT, good_planes(2, 1), heads=HEADS2, K=65) == (ERR_ARG, E_CATALOGUE)
    assert flying().ring(0, 0, cap=-1) == (ERR_ARG, E_RING_ARG)
    assert flying().profile((1.0, 0.0, 8, 8), frames_of(EYE, EYE)) == (ERR_ARG, E_GRID)
    assert flying(chain=True).stems(changed(STEMS3, 4, -1.0), 3) == (ERR_ARG, E_STEM)
    assert flying(chain=True).stems(STEMS3, 65) == (ERR_ARG, E_STEMS_ARG)
    assert flying(chain=True).plan(RULE, good_planes(2, 1), N=0) == (ERR_ARG, E_PLAN_ARG)
    assert flying(chain=True).plan(changed(RULE, 6, -1.0), good_planes(2, 1)) == (ERR_ARG, E_RULE)
    # ... but what a prologue checks BEHIND the state loses to it: the planes, the offsets, the frames, the indices, the reference planes
    bad = changed(good_planes(2, 1), 5, 0.0)
    assert flying().resect(RECORDS, bad) == (ERR_STATE, E_IN_FLIGHT)
    assert flying(run=ALL).resect(RECORDS, offs=np.full((1, 7), np.nan)) == (ERR_STATE, E_IN_FLIGHT)
    assert flying().profile(GRID, frames_of(EYE, changed(EYE, 10, -1.0))) == (ERR_STATE, E_IN_FLIGHT)
    assert flying(chain=True).ring(7, 0) == (ERR_STATE, E_IN_FLIGHT)
    assert flying(chain=True).plan(RULE, bad) == (ERR_STATE, E_IN_FLIGHT)
    assert flying(chain=True).stems(STEMS3, 3) == (ERR_STATE, E_IN_FLIGHT)


def test_no_meshes_beats_runs_in_flight(ctx):
    assert ctx(B=0, pending=1).resect(RECORDS, good_planes(1, 1)) == (ERR_STATE, E_NO_MESHES)
    assert ctx(B=0, pending=1).profile(GRID, EYE) == (ERR_STATE, E_NO_MESHES)
    assert ctx(B=0, pending=1).stems(STEMS3, 3) == (ERR_STATE, E_IN_FLIGHT)                # (these three look at the flight first)
    assert ctx(B=0, pending=1).plan(RULE, good_planes(1, 1)) == (ERR_STATE, E_IN_FLIGHT)
    assert ctx(B=0, pending=1).ring(0, 0) == (ERR_STATE, E_IN_FLIGHT)
    assert ctx(B=0).plan(RULE, good_planes(1, 1)) == (ERR_STATE, E_NOT_SEATED)
    assert ctx(B=0).ring(0, 0) == (ERR_STATE, E_NO_RESECTION)


def test_a_bad_catalogue_beats_no_resection(ctx):
    assert ctx().stems(changed(STEMS3, 0, np.nan), 3) == (ERR_ARG, E_STEM)
    assert ctx().stems(STEMS3, 0) == (ERR_ARG, E_STEMS_ARG)
    assert ctx(B=0).resect(SEAT, good_planes(1, 1), heads=[(6.0, 12.0)], K=1) == (ERR_ARG, E_CATALOGUE)      # (and no meshes)


def test_plan_order(ctx, shim):
    ref = good_planes(2, 1)
    c = ctx(chain=True)
    c.m.ctx = False                                                                        # a null context
    assert c.plan(changed(RULE, 5, -1.0), ref) == (ERR_ARG, None)                          # (nowhere to put the text: the code alone)
    text = ctypes.create_string_buffer(256)
    ru, rp = _f64(changed(RULE, 5, -1.0)), _f64(ref)
    assert shim.ac_pre_plan(_p(ru), _p(rp), 8, 1, 0, 0, 0, 0, None, text, 256) == ERR_ARG and text.value.decode() == E_RULE      # the rule is what is refused
    ru = _f64(RULE)
    assert shim.ac_pre_plan(_p(ru), _p(rp), 8, 1, 0, 0, 0, 0, None, text, 256) == ERR_ARG and text.value.decode() == ""          # then the context
    assert c.plan(RULE, ref, N=0) == (ERR_ARG, None) and c.plan(RULE, ref) == (ERR_ARG, None)
    for fn in (lambda: c.resect(RECORDS, good_planes(2, 1)), lambda: c.ring(0, 0), lambda: c.profile(GRID, frames_of(EYE, EYE)), lambda: c.stems(STEMS3, 3)):
        assert fn() == (ERR_ARG, None)
    c.m.ctx = True
    # not seated together with stale stems: fitted, then stems -- "seated" wins
    c = ctx()
    assert c.profile(GRID, frames_of(EYE, EYE))[0] == OK and c.resect(SEAT, good_planes(2, 2), P=2, heads=HEADS2, K=2)[0] == OK and c.stems(STEMS3, 3)[0] == OK
    assert c.plan(RULE, ref) == (OK, "")
    assert c.resect(FIT, good_planes(2, 2), P=2) == (OK, "")                               # voids the seats AND the stems
    assert c.plan(RULE, ref) == (ERR_STATE, E_NOT_SEATED)
    # stale stems together with ref_planes == NULL and no run: the stems win
    assert c.resect(SEAT, good_planes(2, 2), P=2, heads=HEADS2, K=2) == (OK, "")
    assert c.plan(RULE) == (ERR_STATE, E_STALE_STEMS) and c.plan(RULE, ref) == (ERR_STATE, E_STALE_STEMS)
    assert c.stems(STEMS3, 3) == (OK, "") and c.plan(RULE) == (ERR_STATE, E_REF_NULL)
    assert c.plan(RULE, changed(ref, 3 + 6, np.nan)) == (ERR_ARG, E_REF_PLANE % 1)


# ---- the pass plan and the bytes of every buffer --------------------------------------------------------------------------------------------
def parent_resect_sizes(B, P, maxF, level, K, offs):
    """resect_ensure of the parent commit -> planes per pass, tmax, {name: (bytes, elem)}"""
    tmax = max(1, (maxF + 256 - 1) // 256)
    pc = min(8192 // B, (128 << 20) // (32 * B * tmax))
    pc = max(1, min(pc, P))
    z = {"resect.planes": (B * P * 48, 8), "resect.status": (B * P * 4, 4), "resect.slab": (B * pc * tmax * 32, 8), "resect.segcnt": (B * pc * 4, 4),
         "resect.segs": (B * pc * MAXSEG * 4, 4), "resect.out": (B * P * S_RESECTION, 8), "resect.one": (S_RESECTION, 8), "resect.ring": ((MAXSEG + 1) * 24, 8)}
    if level >= FIT:
        pcf = min(4096 // B, (128 << 20) // (8 * 16 * B * tmax))
        pc = max(1, min(pcf, pc))
        z.update({"resect.fit_slab": (B * pc * tmax * 16 * 8, 8), "resect.fit_moments": (B * P * 16 * 8, 8), "resect.fit_ring": (B * P * 8 * 8, 8),
                  "resect.fit_out": (B * P * S_HEAD_FIT, 8)})
    if level == SEAT:
        z.update({"resect.seat_ring": (B * pc * 2 * MAXSEG * 8, 8), "resect.seat_heads": (K * S_HEAD, 8), "resect.seat_out": (B * P * K * S_SEAT, 8)})
    if offs:
        z["resect.offs"] = (P * 56, 8)
    return pc, tmax, z


def sizes_of(L, n, bytes_, elems):
    assert n == len(L.names) == 35
    return {name: (int(b), int(e)) for name, b, e in zip(L.names, bytes_, elems) if b}


def test_resect_pass_plan(shim):
    bytes_, elems, pt = np.zeros(64, np.uint64), np.zeros(64, np.int32), np.zeros(2, np.int32)
    seen = set()
    for B, P, maxF, level, K in itertools.product((1, 2, 3, 63, 64, 65, 1000, 4096, 5000), (1, 2, 64, 65, 1365, 1366, 4096), (4, 255, 256, 257, 32440, 2000000),
                                                  (RECORDS, FIT, SEAT), (1, 64)):
        for offs in (0, 1):
            n = shim.ac_resect_plan(B, P, maxF, level, K, offs, _p(pt), _p(bytes_), _p(elems))
            pc, tmax, want = parent_resect_sizes(B, P, maxF, level, K, offs)
            assert (int(pt[0]), int(pt[1])) == (pc, tmax), (B, P, maxF, level)
            assert sizes_of(shim, n, bytes_, elems) == want, (B, P, maxF, level, K, offs)
            seen.add((level, pc))
    assert parent_resect_sizes(64, 65, 520, SEAT, 4, 0)[:2] == (64, 3) and parent_resect_sizes(64, 129, 520, RECORDS, 0, 0)[0] == 128      # (tests/test_gpu_arthro_launches.py)
    assert parent_resect_sizes(3, 4096, 2000000, RECORDS, 0, 0)[0] == 178 and parent_resect_sizes(3, 4096, 2000000, FIT, 0, 0)[0] == 44      # the slabs' 128 MB decide
    assert {pc for lv, pc in seen if lv == RECORDS} >= {1, 2, 8, 64, 126, 128, 1365, 1366, 4096}
    for nf in (0, 1, 4, 255, 256, 257, 512, 513, 2000000):
        assert shim.ac_ring_tiles(nf) == max(1, (nf + 255) // 256)


def test_canal_stem_and_plan_buffers(shim):
    bytes_, elems, two = np.zeros(64, np.uint64), np.zeros(64, np.int32), np.zeros(2, np.uint64)
    for B, Lv, A, maxF in ((1, 1, 3, 4), (3, 64, 64, 520), (64, 161, 64, 32440), (5000, 1024, 256, 2000000), (2, 7, 255, 257)):
        n = shim.ac_canal_plan(B, Lv, A, maxF, _p(two), _p(bytes_), _p(elems))
        rays = B * Lv * A
        assert two.tolist() == [max(1, (maxF + 255) // 256), rays]
        assert sizes_of(shim, n, bytes_, elems) == {"canal.near": (rays * 8, 8), "canal.far": (rays * 8, 8), "canal.levels": (B * Lv * S_LEVEL, 8),
                                                    "canal.frames": (B * 128, 8), "canal.status": (B * 4, 4), "canal.dirs": (A * 16, 8)}
    for B, P, K in ((1, 1, 1), (3, 4, 8), (64, 27, 16), (5000, 4096, 64)):
        n = shim.ac_stem_bytes(B, P, K, _p(bytes_), _p(elems))
        assert sizes_of(shim, n, bytes_, elems) == {"stem.catalogue": (K * S_STEM, 8), "stem.out": (B * P * K * S_STEM_FIT, 8)}
    for B, P, Kh, Ks, N, maxV in ((1, 1, 1, 1, 1, 4), (3, 4, 4, 8, 8, 262), (3, 4, 4, 8, 64, 256), (64, 27, 16, 16, 8, 16222), (5000, 4096, 64, 64, 64, 1000001)):
        n = shim.ac_plan_plan(B, P, Kh, Ks, N, maxV, _p(two), _p(bytes_), _p(elems))
        tmax, cuts = max(1, (maxV + 255) // 256), B * P
        assert two.tolist() == [tmax, cuts]
        assert sizes_of(shim, n, bytes_, elems) == {
            "plan.ref_planes": (B * 48, 8), "plan.compat": (64 * 8, 8), "plan.ref_slab": (B * tmax * 2 * 16, 8), "plan.ref": (B * S_PLAN_REF, 8),
            "plan.cut_terms": (cuts * 16, 8), "plan.head_terms": (cuts * Kh * 16, 8), "plan.stem_terms": (cuts * Ks * 16, 8), "plan.cut_vals": (cuts * 8, 8),
            "plan.head_vals": (cuts * Kh * 64, 8), "plan.stem_vals": (cuts * Ks * 8, 8), "plan.out": (B * N * S_PLAN, 8)}


# ---- the state ------------------------------------------------------------------------------------------------------------------------------
def step(c, event, depth):
    """one event on both contexts (with numbers that differ from step to step); a refused call changes nothing on either side"""
    B = max(c.m.B, 1)
    P, K = 2 + depth, 3 + depth
    if event == "upload":
        c.upload(1 + depth % 2)
    elif event in ("run", "run_without"):
        if c.m.B:      # (a run needs a batch)
            c.run(ALL if event == "run" else ALL & ~ANP)
    elif event in ("records", "fit", "seat", "resect_fails"):
        level = {"records": RECORDS, "fit": FIT, "seat": SEAT, "resect_fails": SEAT}[event]
        c.resect(level, _good_planes(B, P), P=P, heads=[(6.0, 3.0)] * K, K=K, fail=event == "resect_fails")
    elif event == "profile":
        c.profile((1.5, 0.25, 10 + depth, 20 + depth), frames_of(*[EYE] * B))
    else:
        c.stems([STEMS3[0]] * K, K, fail=event == "stems_fail")
    return c.queries()


EVENTS = ("upload", "run", "run_without", "records", "fit", "seat", "resect_fails", "profile", "stems", "stems_fail")


def test_every_sequence_of_five_events(shim):
    """after each step of each of the 111 110 sequences the five queries, P, K_h, K_s (and the grid) are the parent's fields'"""
    reached = set()

    def walk(c, depth):
        for ev in EVENTS:
            d = c.clone()
            reached.add(tuple(step(d, ev, depth)[:5]))
            if depth < 4:
                walk(d, depth + 1)
            d.close()
    root = Both(shim)
    assert root.queries() == [0] * 10
    walk(root, 0)
    root.close()
    assert (1, 1, 1, 1, 1) in reached and (0, 1, 0, 1, 0) in reached and (0, 0, 0, 1, 0) in reached and (1, 1, 1, 0, 0) in reached
    assert not any(q[2] and not q[1] for q in reached) and not any(q[4] and not q[3] for q in reached)


def test_the_sequence_of_the_plan_test_on_the_gpu(ctx):
    """tests/test_gpu_plan.py::test_state_and_arguments, call by call"""
    c, ref, planes, frames = ctx(B=3), good_planes(3, 1), good_planes(3, 4), frames_of(EYE, EYE, EYE)
    heads, stems = [(6.0, 3.0), (5.0, 2.0), (8.0, 1.5), (6.0, 3.0)], [STEMS3[0]] * 8
    assert c.profile(GRID, frames) == (OK, "") and c.resect(FIT, planes, P=4) == (OK, "") and c.stems(stems, 8) == (OK, "")      # fitted, not seated
    assert c.plan(RULE, ref) == (ERR_STATE, E_NOT_SEATED)
    assert c.profile(GRID, frames) == (OK, "") and c.resect(SEAT, planes, P=4, heads=heads, K=4) == (OK, "") and c.stems(stems, 8) == (OK, "")
    assert c.plan(RULE, ref) == (OK, "")
    assert c.plan(RULE, ref, N=0) == (ERR_ARG, E_PLAN_ARG) and c.plan(RULE, ref, N=65) == (ERR_ARG, E_PLAN_ARG)
    for index, value in ((11, -1.0), (5, -1.0), (0, np.nan)):
        assert c.plan(changed(RULE, index, value), ref) == (ERR_ARG, E_RULE)
    bad = ref.copy()
    bad[1, 0, 3:] = 0.0
    assert c.plan(RULE, bad) == (ERR_ARG, E_REF_PLANE % 1)
    assert c.plan(RULE) == (ERR_STATE, E_REF_NULL)                                         # no run of this batch
    assert c.resect(SEAT, planes, P=4, heads=heads, K=4) == (OK, "")                       # a new resection, the old stems
    assert c.plan(RULE, ref) == (ERR_STATE, E_STALE_STEMS)
    assert c.stems(stems, 8) == (OK, "") and c.plan(RULE, ref) == (OK, "")
    assert c.profile(GRID, frames) == (OK, "")                                             # a new profile, the old stems
    assert c.plan(RULE, ref) == (ERR_STATE, E_STALE_STEMS)
    assert c.stems(stems, 8) == (OK, "") and c.plan(RULE, ref) == (OK, "")                 # (sh_resect_stems keeps its own preconditions)
    assert c.queries() == [0, 1, 1, 1, 1, 4, 4, 8, 64, 64]
    c.upload(3)
    assert c.plan(RULE, ref) == (ERR_STATE, E_NOT_SEATED)
    assert c.queries() == [0, 0, 0, 0, 0, 4, 4, 8, 64, 64]


def test_the_sequence_of_the_stem_test_on_the_gpu(ctx):
    """tests/test_gpu_stem.py::test_stems_on_the_fixture_and_state, call by call"""
    c, offs, stems = ctx(B=1), np.zeros((4, 7)), [STEMS3[0]] * 5
    assert c.profile((0.0, 1.0, 4, 64)) == (ERR_STATE, E_FRAMES_NULL)                      # frames=None without a run
    assert c.stems(stems, 5) == (ERR_STATE, E_NO_RESECTION)                                # stems before a profile and a resection
    c.run(ALL)
    assert c.resect(SEAT, offs=offs, P=4, heads=HEADS2, K=2) == (OK, "")
    assert c.stems(stems, 5) == (ERR_STATE, E_NO_PROFILE)                                  # a resection, no profile yet
    assert c.profile((60.0, 2.0, 90, 64)) == (OK, "") and c.stems(stems, 5) == (OK, "")
    assert c.queries() == [1, 1, 1, 1, 1, 4, 2, 5, 90, 64]
    assert c.resect(SEAT, offs=offs, P=4, heads=HEADS2, K=2) == (OK, "")
    assert c.queries() == [1, 1, 1, 1, 0, 4, 2, 5, 90, 64]
    c.upload(1)                                                                            # a new upload voids both
    assert c.stems(stems, 5) == (ERR_STATE, E_NO_RESECTION)
    assert c.resect(RECORDS, good_planes(1, 1)) == (OK, "")
    assert c.stems(stems, 5) == (ERR_STATE, E_NO_PROFILE)                                  # the profile went with the old batch
    assert c.queries() == [0, 1, 0, 0, 0, 1, 2, 5, 90, 64]


def test_a_call_that_fails_half_way_leaves_what_the_parent_leaves(ctx):
    c, ref = ctx(chain=True), good_planes(2, 1)
    assert c.plan(RULE, ref) == (OK, "")
    assert c.stems(STEMS3, 3, fail=True) == (OK, "")                                       # no stems for sh_resect_plan ...
    assert c.plan(RULE, ref) == (ERR_STATE, E_STALE_STEMS) and c.queries()[:5] == [0, 1, 1, 1, 0]
    assert c.stems(STEMS3, 3) == (OK, "") and c.plan(RULE, ref) == (OK, "")
    assert c.profile(GRID, frames_of(EYE, EYE), fail=True) == (OK, "")                     # no profile, and the stems were the old one's
    assert c.stems(STEMS3, 3) == (ERR_STATE, E_NO_PROFILE) and c.plan(RULE, ref) == (ERR_STATE, E_STALE_STEMS)
    assert c.profile(GRID, frames_of(EYE, EYE)) == (OK, "") and c.plan(RULE, ref) == (ERR_STATE, E_STALE_STEMS)
    assert c.stems(STEMS3, 3) == (OK, "") and c.plan(RULE, ref) == (OK, "")
    assert c.resect(SEAT, good_planes(2, 3), P=3, heads=HEADS2, K=2, fail=True) == (OK, "")      # no resection: no ring, no stems, no plan
    assert c.ring(0, 0) == (ERR_STATE, E_NO_RESECTION) and c.stems(STEMS3, 3) == (ERR_STATE, E_NO_RESECTION) and c.plan(RULE, ref) == (ERR_STATE, E_NOT_SEATED)
    assert c.resect(RECORDS, good_planes(2, 3), P=3) == (OK, "") and c.plan(RULE, ref) == (ERR_STATE, E_NOT_SEATED)
