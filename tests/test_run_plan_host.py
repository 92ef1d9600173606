"""The host rules of a run (shoulder_amd/csrc/sh_run.h: what sh_submit refuses and plans, what is known about the resident batch,
the key of the prepared-hull record), without a GPU.  The expected values are the rules sh_submit, sh_collect, redo_given_up, run_obb
and the preparation starters applied before the header existed, written out here in plain Python: the refusals in their order, the
four facts of a submit derived from the context's fields, and every assignment to the loose fields the header's BatchState replaced."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
OBB, FULL, NECK, CANAL, PROXIMAL, GROOVE, ANP, DISTAL, TE, CSYS, APPLY = (1 << i for i in range(11))
ALL = 0x7FF
HUMERUS, PROX = 0, 1
OK, ARG, STATE = 0, -1, -3
NONE = (1 << 64) - 1
NO_RERUN, TIER, OBB_TIER, POOLS, FORCE_HOST = range(5)
SEG_NEED, RING_NEED = 3, 4
WINDOW = 1 << 30
T_NO_MESH = "sh_run: no meshes uploaded"
T_TWO = "sh_submit: two runs are in flight already (sh_collect first)"
T_DISTAL = "sh_run: a proximal humerus has no distal / trans-epicondylar stage (bone.py:24-64)"
T_APPLY = "sh_run: SH_STAGE_APPLY needs SH_STAGE_CSYS in the same run"
T_CSYS = "sh_run: SH_STAGE_CSYS of a proximal humerus needs SH_STAGE_ANP in the same run (canal / articular frame)"
T_FRAME = 'sh_run: no OBB transform (run SH_STAGE_OBB or sh_store("obb_transform"))'
u64, i64 = ctypes.c_ulonglong, ctypes.c_longlong


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("run_check") / "librun_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "hostcheck", "run_check.cpp")])
    L = ctypes.CDLL(str(so))
    L.rc_batch_new.restype = ctypes.c_void_p
    L.rc_refusal_text.restype = ctypes.c_char_p
    for name, args in dict(rc_batch_free=[ctypes.c_void_p], rc_batch_resident=[ctypes.c_void_p], rc_params_set=[ctypes.c_void_p],
                           rc_buffer_touched=[ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int], rc_obb_begins=[ctypes.c_void_p, u64],
                           rc_frame_computed=[ctypes.c_void_p], rc_run_enqueued=[ctypes.c_void_p, ctypes.c_uint],
                           rc_run_collected=[ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, u64, u64],
                           rc_rerun=[ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int],
                           rc_hull_above_record=[ctypes.c_void_p], rc_redo_used_faces=[ctypes.c_void_p, ctypes.c_int],
                           rc_skip_list_cleared=[ctypes.c_void_p], rc_batch_queries=[ctypes.c_void_p, u64, ctypes.c_void_p],
                           rc_vouches=[ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int], rc_refusal_text=[ctypes.c_int],
                           rc_key_event=[ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64, ctypes.c_int], rc_key_fresh=[ctypes.c_void_p],
                           rc_key_usable=[ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64, ctypes.c_int],
                           rc_precheck=[ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p)],
                           rc_plan=[ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]).items():
        getattr(L, name).argtypes = args
    return L


def test_the_header_compiles_alone(tmp_path):
    """sh_run.h by itself, plain g++, warnings are errors, no HIP include on the path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "sh_run.h"\nint main() { sh::BatchState s; sh::PreparedKey k; return s.has_frame() || k.active; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(tmp_path / "alone"), str(src)])
    subprocess.check_call([str(tmp_path / "alone")])


# ---- the state of the resident batch: the parent's loose fields and every place that assigned them ------------------------------------
class ParentFields:
    """sh_ctx at the parent commit: ovf_none_gen, obb_gen, obb_sil_need, obb_nf_over, hull_force_host, obb_injected, skip_nfmax and
    the four capacities; one method per place that assigned them, with the statements of that place."""

    def __init__(self):
        self.ovf_none_gen = self.obb_gen = NONE
        self.obb_sil_need, self.obb_nf_over, self.hull_force_host, self.obb_injected, self.skip_nfmax = 0, False, False, False, 0
        self.seg, self.ring, self.work, self.end = 1 << 18, 1 << 18, 32 << 20, 8192

    def alloc_batch(self):
        self.obb_injected = False

    def set_params(self):
        self.ovf_none_gen = NONE

    def buffer_device(self, name):
        self.ovf_none_gen = NONE

    def store(self, name):      # (sh_store: the vouch in front of the copy, the frame behind it)
        self.ovf_none_gen = NONE
        if name == "obb_transform":
            self.obb_injected = True

    def run_obb_begin(self, batch_gen):
        if self.obb_gen != batch_gen:
            self.obb_gen, self.obb_sil_need, self.obb_nf_over, self.hull_force_host = batch_gen, 0, False, False

    def run_obb_end(self):
        self.obb_injected = True

    def submit_enqueued(self, mask):
        if mask & OBB:
            self.obb_injected = True

    def collect(self, w, mask, bone_kind, tk_gen, batch_gen):
        slice_stages = FULL | DISTAL | NECK | PROXIMAL
        if (w[RING_NEED] == 0 and w[SEG_NEED] == 0 and (mask & OBB)
                and (mask & slice_stages) == ((slice_stages & ~DISTAL) if bone_kind == PROX else slice_stages) and tk_gen == batch_gen):
            self.ovf_none_gen = batch_gen

    def rerun(self, why, caps, error, redo, others_in_flight):
        """sh_collect behind `v.rerun != SH_RERUN_NONE`.  -> "obb.endpts" grows (1 / 0), -1: refused, another run is in flight"""
        if why == TIER or redo:
            self.ovf_none_gen = NONE
        if others_in_flight:
            return -1
        self.seg, self.ring, self.work, self.obb_sil_need, self.obb_nf_over = caps[0], caps[1], caps[2], caps[4], bool(caps[5])
        if error:
            return 0
        if caps[3] != self.end:
            self.end = caps[3]
            return 1
        return 0

    def redo_above_record(self):
        self.hull_force_host = True

    def redo_faces(self, fn):
        self.skip_nfmax = max(self.skip_nfmax, fn)

    def device_hull_scratch_new_batch(self):
        self.skip_nfmax = 0

    def device_hull_now(self, hull_mode, batch_gen):
        return hull_mode == 1 and not (self.hull_force_host and self.obb_gen == batch_gen)

    def queries(self, gen):
        return [int(self.ovf_none_gen != gen), int(self.device_hull_now(0, gen)), int(self.device_hull_now(1, gen)), int(self.obb_injected), self.skip_nfmax,
                self.seg, self.ring, self.work, self.end, self.obb_sil_need, int(self.obb_nf_over)]


class Both:
    """one event to the header's BatchState and to the parent's fields; check() compares every query and capacity for the generations in play"""

    def __init__(self, L):
        self.L, self.h, self.p = L, ctypes.c_void_p(L.rc_batch_new()), ParentFields()

    def close(self):
        self.L.rc_batch_free(self.h)

    def queries(self, gen):
        out = (u64 * 11)()
        self.L.rc_batch_queries(self.h, gen, out)
        return [int(x) for x in out]

    def check(self, gens, what=""):
        for g in gens:
            assert self.queries(g) == self.p.queries(g), (what, g)

    def resident(self):
        self.L.rc_batch_resident(self.h); self.p.alloc_batch()

    def params(self):
        self.L.rc_params_set(self.h); self.p.set_params()

    def buffer_device(self, name):
        self.L.rc_buffer_touched(self.h, name.encode(), 0); self.p.buffer_device(name)

    def store(self, name):
        self.L.rc_buffer_touched(self.h, name.encode(), 0); self.L.rc_buffer_touched(self.h, name.encode(), 1); self.p.store(name)

    def obb_begins(self, gen):
        self.L.rc_obb_begins(self.h, gen); self.p.run_obb_begin(gen)

    def frame_computed(self):
        self.L.rc_frame_computed(self.h); self.p.run_obb_end()

    def enqueued(self, mask):
        self.L.rc_run_enqueued(self.h, mask); self.p.submit_enqueued(mask)

    def collected(self, words, mask, bone, run_gen, batch_gen):
        w = (u64 * 16)(*[words.get(i, 0) for i in range(16)])
        self.L.rc_run_collected(self.h, w, mask, bone, run_gen, batch_gen); self.p.collect(list(w), mask, bone, run_gen, batch_gen)

    def rerun(self, why, caps, error=False, redo=False, others=False):
        got = self.L.rc_rerun(self.h, why, (u64 * 6)(*caps), int(error), int(redo), int(others))
        assert got == self.p.rerun(why, caps, error, redo, others)
        return got

    def above_record(self):
        self.L.rc_hull_above_record(self.h); self.p.redo_above_record()

    def redo_faces(self, n):
        self.L.rc_redo_used_faces(self.h, n); self.p.redo_faces(n)

    def skip_cleared(self):
        self.L.rc_skip_list_cleared(self.h); self.p.device_hull_scratch_new_batch()

    def caps(self):
        return self.queries(0)[5:]


@pytest.fixture()
def both(shim):
    b = Both(shim)
    yield b
    b.close()


TIER_ON, DEV0, DEV1, FRAME, SKIP_NF = range(5)
SLICES = FULL | DISTAL | NECK | PROXIMAL


def test_a_fresh_context(both):
    assert both.queries(0) == [1, 0, 1, 0, 0, 1 << 18, 1 << 18, 32 << 20, 8192, 0, 0]
    both.check((0, 1, NONE), "fresh")


def test_vouch_needs_everything(shim, both):
    """OBB, all slice stages (proximal: all but distal), the same generation, zero ring and segment demand"""
    g = 5
    cases = [(ALL, HUMERUS, g, {}, True), (OBB | SLICES, HUMERUS, g, {}, True), (ALL & ~OBB, HUMERUS, g, {}, False)]
    cases += [(ALL & ~s, HUMERUS, g, {}, False) for s in (FULL, DISTAL, NECK, PROXIMAL)]
    cases += [(ALL & ~(DISTAL | TE), PROX, g, {}, True), (ALL, PROX, g, {}, False)]
    cases += [(ALL & ~(DISTAL | TE) & ~s, PROX, g, {}, False) for s in (FULL, NECK, PROXIMAL)]
    cases += [(ALL & ~(DISTAL | TE), HUMERUS, g, {}, False), (ALL, HUMERUS, g - 1, {}, False), (ALL, HUMERUS, g, {RING_NEED: 1}, False),
              (ALL, HUMERUS, g, {SEG_NEED: 1}, False), (ALL, HUMERUS, g, {5: 9, 0: 3, 1: 2, 7: 400}, True)]
    for mask, bone, run_gen, words, vouches in cases:
        both.params()      # (void again)
        assert both.queries(g)[TIER_ON] == 1
        both.collected(words, mask, bone, run_gen, g)
        both.check((g, g - 1, g + 1), (mask, bone, run_gen, words))
        assert both.queries(g)[TIER_ON] == (0 if vouches else 1), (mask, bone, run_gen, words)
        w = (u64 * 16)(*[words.get(i, 0) for i in range(16)])
        assert shim.rc_vouches(w, mask, bone, int(run_gen == g)) == int(vouches)
    assert both.queries(g + 1)[TIER_ON] == 1      # the vouch is for its generation only


def test_what_voids_the_vouch(both):
    g = 3
    caps = both.caps()
    voids = [both.params, lambda: both.buffer_device("landmarks"), lambda: both.buffer_device("params"), lambda: both.store("obb_transform"),
             lambda: both.store("z_bounds"), lambda: both.rerun(TIER, caps), lambda: both.rerun(TIER, caps, others=True),
             lambda: both.rerun(POOLS, caps, redo=True), lambda: both.rerun(OBB_TIER, caps, redo=True, others=True), lambda: both.rerun(FORCE_HOST, caps, redo=True)]
    keeps = [lambda: both.rerun(POOLS, caps), lambda: both.rerun(OBB_TIER, caps), lambda: both.rerun(FORCE_HOST, caps, others=True), both.resident,
             lambda: both.obb_begins(g), lambda: both.obb_begins(g + 1), lambda: both.enqueued(ALL), both.above_record, lambda: both.redo_faces(9), both.frame_computed]
    for k, ev in enumerate(voids + keeps):
        both.collected({}, ALL, HUMERUS, g, g)
        assert both.queries(g)[TIER_ON] == 0
        ev()
        both.check((g, g + 1), k)
        assert both.queries(g)[TIER_ON] == (1 if k < len(voids) else 0), k


def test_frame(both):
    assert both.queries(0)[FRAME] == 0
    for ev, want in ((lambda: both.enqueued(ALL & ~OBB), 0), (lambda: both.store("obb_transformx"), 0), (lambda: both.buffer_device("obb_transform"), 0),
                     (lambda: both.store("obb_transform"), 1), (both.resident, 0), (lambda: both.enqueued(OBB), 1), (both.resident, 0), (both.frame_computed, 1),
                     (both.params, 1), (lambda: both.obb_begins(4), 1), (both.resident, 0)):
        ev()
        both.check((0,))
        assert both.queries(0)[FRAME] == want


def test_a_new_batch_keeps_the_tier_choice_until_its_first_obb_stage(both):
    """... and device_hull agrees with the parent's device_hull_now there; hulls from the host hold only for their generation"""
    g = 8
    both.obb_begins(g)
    assert both.rerun(OBB_TIER, both.caps()[:4] + [700, 1]) == 0
    both.above_record()
    assert both.queries(g)[DEV0:DEV1 + 1] == [0, 0] and both.caps()[4:] == [700, 1]
    both.obb_begins(g)      # (every later OBB stage of the batch: nothing)
    both.check((g, g + 1), "same batch")
    assert both.queries(g)[DEV1] == 0 and both.caps()[4:] == [700, 1]
    both.resident()         # the batch with generation g + 1 becomes resident: sh_stage_* asks device_hull_now before its first run
    both.check((g, g + 1), "new batch, no OBB stage yet")
    assert both.queries(g + 1)[DEV1] == 1 and both.queries(g)[DEV1] == 0      # (force-host holds only for its generation)
    assert both.caps()[4:] == [700, 1]      # the old tier choice stands ...
    both.obb_begins(g + 1)
    both.check((g, g + 1), "first OBB stage")
    assert both.caps()[4:] == [0, 0] and both.queries(g + 1)[DEV1] == 1 and both.queries(g)[DEV1] == 1      # ... until here
    assert both.queries(g + 1)[DEV0] == 0      # host mode is host mode


def test_rerun_takes_the_capacities(both):
    c0 = both.caps()
    grown = [c0[0] * 2, c0[1] + 5, c0[2] * 3, 10000, 600, 1]
    assert both.rerun(POOLS, grown, others=True) == -1 and both.caps() == c0       # another run in flight: refused, nothing taken
    assert both.rerun(POOLS, grown, error=True) == 0 and both.caps() == grown[:3] + [c0[3]] + grown[4:]      # an error keeps the end sections
    assert both.rerun(POOLS, grown) == 1 and both.caps() == grown
    assert both.rerun(POOLS, grown) == 0 and both.caps() == grown
    both.check((0,))


def test_redone_faces(both):
    for ev, want in ((lambda: both.redo_faces(50), 50), (lambda: both.redo_faces(20), 50), (lambda: both.redo_faces(70), 70), (lambda: both.obb_begins(3), 70),
                     (both.resident, 70), (both.skip_cleared, 0), (lambda: both.redo_faces(5), 5)):
        ev()
        both.check((3,))
        assert both.queries(3)[SKIP_NF] == want


def test_random_event_sequences(shim):
    """3000 events, fixed seed: after every one all queries and capacities agree with the parent's fields, for every generation in play"""
    rng = random.Random(20240607)
    names = ["obb_transform", "verts", "landmarks", "params", "z_bounds", "err"]
    masks = [ALL, ALL & ~OBB, OBB | SLICES, ALL & ~(DISTAL | TE), OBB, FULL | NECK, ALL & ~PROXIMAL, 0]
    b = Both(shim)
    try:
        gen = 1
        for step in range(3000):
            k = rng.randrange(14)
            if k == 0:
                gen += 1; b.resident()
            elif k == 1:
                b.params()
            elif k == 2:
                b.buffer_device(rng.choice(names))
            elif k == 3:
                name = rng.choice(names)
                if name == "verts":
                    gen += 1      # (a store to "verts" takes a new generation without alloc_batch)
                b.store(name)
            elif k == 4:
                b.obb_begins(rng.choice((gen, gen, gen - 1)))
            elif k == 5:
                b.frame_computed()
            elif k == 6:
                b.enqueued(rng.choice(masks))
            elif k in (7, 8):
                words = {SEG_NEED: rng.choice((0, 0, 0, 5)), RING_NEED: rng.choice((0, 0, 0, 1)), 5: rng.randrange(3), 6: rng.randrange(2)}
                b.collected(words, rng.choice(masks), rng.choice((HUMERUS, PROX)), rng.choice((gen, gen, gen - 1)), gen)
            elif k == 9:
                c = b.caps()
                caps = [c[0] + rng.choice((0, 1000)), c[1] + rng.choice((0, 77)), c[2] * rng.choice((1, 2)) % (1 << 63), c[3] + rng.choice((0, 0, 2048)), rng.choice((c[4], 600, 2100)), rng.choice((c[5], 1))]
                b.rerun(rng.choice((TIER, OBB_TIER, POOLS, FORCE_HOST)), caps, error=rng.random() < 0.15, redo=rng.random() < 0.3, others=rng.random() < 0.3)
            elif k == 10:
                b.above_record()
            elif k == 11:
                b.redo_faces(rng.randrange(1, 40000))
            elif k == 12:
                b.skip_cleared()
            else:
                gen += 1; b.resident(); b.obb_begins(gen)
            b.check((gen, gen - 1, gen + 1, NONE), (step, k))
    finally:
        b.close()


def test_refusal_texts_of_a_rerun(shim):
    tail = " while another run is in flight: collect it, then run the batch again "
    assert shim.rc_refusal_text(TIER).decode() == "a section needs the overflow tier" + tail + "(the tier is on by then)"
    assert shim.rc_refusal_text(OBB_TIER).decode() == "the OBB stage needs a larger tier" + tail + "(the tier is chosen by then)"
    assert shim.rc_refusal_text(FORCE_HOST).decode() == "a hull is above the device hull's record" + tail + "(its hulls come from the host by then)"
    assert shim.rc_refusal_text(POOLS).decode() == "slice overflow pools too small" + tail + "(the pools are grown by then)"


# ---- the key of the prepared-hull record ---------------------------------------------------------------------------------------------------
def parent_key_event(key, event, slot, B, batch_gen, hulls):
    """the statements of start_prepare | start_prepare_staged | join_prepared | `prep.gen = ~0ull` | discard_staged on
    (active, staged, slot, B, gen)"""
    active, staged, kslot, kB, gen = key
    if event == 0:
        return [1, 0, slot, B, batch_gen]
    if event == 1:
        return [1, 1, slot, B, (batch_gen + 1) if hulls else NONE]
    if event == 2:
        return [0, staged, kslot, kB, gen]
    if event == 3:
        return [active, staged, kslot, kB, NONE]
    return [active, 0, kslot, kB, NONE]


def parent_usable(key, obb, whole, prc, batch_gen, B):
    """the condition of sh_submit behind its join (the caller has checked `active`)"""
    return int(bool(obb and whole and prc == OK and key[4] == batch_gen and key[3] == B))


def test_prepared_key_events_and_usable(shim):
    fresh = (u64 * 5)()
    shim.rc_key_fresh(fresh)
    assert list(fresh) == [0, 0, 0, 0, 0]
    rng = random.Random(7)
    key = [0, 0, 0, 0, 0]
    for step in range(2000):
        event, slot, B, gen, hulls = rng.randrange(5), rng.randrange(2), rng.choice((1, 2, 64)), rng.randrange(1, 6), rng.randrange(2)
        k = (u64 * 5)(*key)
        shim.rc_key_event(k, event, slot, B, gen, hulls)
        key = parent_key_event(key, event, slot, B, gen, hulls)
        assert [int(x) for x in k] == key, (step, event)
        for obb, whole, prc, bg, Bq in itertools.product((0, 1), (0, 1), (OK, -5, -2), (gen, gen + 1), (1, 2, 64)):
            assert shim.rc_key_usable(k, obb, whole, prc, bg, Bq) == parent_usable(key, obb, whole, prc, bg, Bq), (step, key)
    # literal: every condition alone
    good = (u64 * 5)(1, 0, 1, 64, 9)
    assert shim.rc_key_usable(good, 1, 1, OK, 9, 64) == 1
    for args in ((0, 1, OK, 9, 64), (1, 0, OK, 9, 64), (1, 1, -5, 9, 64), (1, 1, OK, 10, 64), (1, 1, OK, 9, 63)):
        assert shim.rc_key_usable(good, *args) == 0, args
    shim.rc_key_event(good, 3, 0, 0, 0, 0)
    assert shim.rc_key_usable(good, 1, 1, OK, 9, 64) == 0 and shim.rc_key_usable(good, 1, 1, OK, NONE, 64) == 1      # (no batch has generation ~0)


# ---- sh_submit: the refusals ---------------------------------------------------------------------------------------------------------------
def parent_precheck(mask, B, n_pending, bone, frame):
    """sh_submit's refusals at the parent commit in the order they stood (what lay between them left out)"""
    if B < 1:
        return STATE, T_NO_MESH
    if n_pending >= 2:
        return STATE, T_TWO
    if bone == PROX and mask & (DISTAL | TE):
        return ARG, T_DISTAL
    if (mask & APPLY) and not (mask & CSYS):
        return ARG, T_APPLY
    if bone == PROX and (mask & CSYS) and not (mask & ANP):
        return ARG, T_CSYS
    if not (mask & OBB) and not frame:
        return STATE, T_FRAME
    return OK, ""


def facts(B=1, n_pending=0, bone=HUMERUS, hull_mode=0, window=0, overlap=0, staged_active=0, batch_gen=7, hslot=0, prep_rc=OK):
    return (i64 * 10)(B, n_pending, bone, hull_mode, window, overlap, staged_active, batch_gen, hslot, prep_rc)


def precheck(L, batch, mask, **kw):
    text = ctypes.c_char_p()
    code = L.rc_precheck(mask, facts(**kw), batch, (u64 * 5)(), ctypes.byref(text))
    return code, text.value.decode()


@pytest.fixture()
def frames(shim):
    """a BatchState without a frame and one with"""
    hs = [ctypes.c_void_p(shim.rc_batch_new()) for _ in range(2)]
    shim.rc_buffer_touched(hs[1], b"obb_transform", 1)
    yield hs
    for h in hs:
        shim.rc_batch_free(h)


# (mask, B, n_pending, bone, frame) -> (code, text): every refusal alone, then pairs that apply at once (the earlier one wins)
PRECHECK_TABLE = [
    ((ALL, 1, 0, HUMERUS, 0), (OK, "")),
    ((ALL & ~OBB, 1, 1, HUMERUS, 1), (OK, "")),
    ((ALL & ~(DISTAL | TE), 1, 1, PROX, 0), (OK, "")),
    ((ALL, 0, 0, HUMERUS, 0), (STATE, T_NO_MESH)),
    ((ALL, 1, 2, HUMERUS, 0), (STATE, T_TWO)),
    ((ALL & ~TE, 1, 0, PROX, 0), (ARG, T_DISTAL)),
    ((ALL & ~DISTAL, 1, 0, PROX, 0), (ARG, T_DISTAL)),
    ((ALL & ~CSYS, 1, 0, HUMERUS, 0), (ARG, T_APPLY)),
    ((ALL & ~(DISTAL | TE | ANP | APPLY), 1, 0, PROX, 0), (ARG, T_CSYS)),
    ((FULL, 1, 0, HUMERUS, 0), (STATE, T_FRAME)),
    ((FULL, 1, 0, PROX, 0), (STATE, T_FRAME)),
    # pairs
    ((ALL, 0, 2, HUMERUS, 0), (STATE, T_NO_MESH)),
    ((FULL | DISTAL, 0, 0, PROX, 0), (STATE, T_NO_MESH)),
    ((ALL, 1, 2, PROX, 0), (STATE, T_TWO)),
    ((FULL | APPLY, 1, 2, HUMERUS, 0), (STATE, T_TWO)),
    ((ALL & ~CSYS, 1, 0, PROX, 0), (ARG, T_DISTAL)),
    ((FULL | TE | CSYS, 1, 0, PROX, 0), (ARG, T_DISTAL)),
    ((FULL | DISTAL, 1, 0, PROX, 0), (ARG, T_DISTAL)),
    ((FULL | APPLY, 1, 0, HUMERUS, 0), (ARG, T_APPLY)),
    ((FULL | APPLY, 1, 0, PROX, 0), (ARG, T_APPLY)),
    ((FULL | CSYS | APPLY, 1, 0, PROX, 0), (ARG, T_CSYS)),
    ((FULL | CSYS, 1, 0, PROX, 0), (ARG, T_CSYS)),
]


@pytest.mark.parametrize("case", range(len(PRECHECK_TABLE)))
def test_precheck_table(shim, frames, case):
    (mask, B, n_pending, bone, frame), want = PRECHECK_TABLE[case]
    assert parent_precheck(mask, B, n_pending, bone, frame) == want
    assert precheck(shim, frames[frame], mask, B=B, n_pending=n_pending, bone=bone) == want


def test_precheck_grid(shim, frames):
    """all 2^6 masks of the stage bits a rule reads (beside two fixed backgrounds of the others) x bone kind x B x runs in flight x frame"""
    bits = (OBB, ANP, DISTAL, TE, CSYS, APPLY)
    n = 0
    for pick in itertools.product((0, 1), repeat=len(bits)):
        for background in (0, FULL | NECK | CANAL | PROXIMAL | GROOVE):
            mask = background | sum(b for b, on in zip(bits, pick) if on)
            for bone, B, n_pending, frame in itertools.product((HUMERUS, PROX), (0, 1), (0, 1, 2), (0, 1)):
                assert precheck(shim, frames[frame], mask, B=B, n_pending=n_pending, bone=bone) == parent_precheck(mask, B, n_pending, bone, frame), (mask, bone, B, n_pending, frame)
                n += 1
    assert n == 64 * 2 * 24


# ---- sh_submit: the plan -------------------------------------------------------------------------------------------------------------------
PLAN_KEYS = ("dev_hull", "win", "prepared_slot", "next_hslot", "void_staged_hulls", "fetch_points", "start_overlap")


def parent_plan(mask, B, window, hull_mode, force_host, obb_gen, batch_gen, overlap, staged_active, hslot, key, prc):
    """what sh_submit derived inline at the parent commit; key = c->prep's (active, staged, slot, B, gen), prc = join_prepared's answer"""
    active, staged, slot, pB, pgen = key
    obb = bool(mask & OBB)
    wsize = WINDOW
    if window > 0:
        wsize = window
    dev_hull = obb and (hull_mode == 1 and not (force_host and obb_gen == batch_gen))
    win = wsize if (obb and B > wsize and not dev_hull) else B
    prepared = -1
    if active:
        if obb and win == B and prc == OK and pgen == batch_gen and pB == B:
            prepared = slot
            hslot = prepared ^ 1
    void_staged = bool(obb and staged and pgen != batch_gen)
    if dev_hull:
        prepared = -1
    fetch = obb and prepared < 0 and not dev_hull
    start = bool(overlap and obb and win == B and not dev_hull and not staged_active)
    return dict(zip(PLAN_KEYS, (int(dev_hull), win, prepared, hslot, int(void_staged), int(fetch), int(start))))


def plan(L, batch, mask, key, **kw):
    out = (i64 * 7)()
    L.rc_plan(mask, facts(**kw), batch, (u64 * 5)(*key), out)
    return dict(zip(PLAN_KEYS, [int(x) for x in out]))


@pytest.fixture()
def forced(shim):
    """BatchStates by (force_host, obb_gen): none, hulls from the host for generation 7 (the resident one below), for generation 6 (stale)"""
    hs = {}
    for name, gen in (("none", None), ("match", 7), ("stale", 6)):
        h = hs[name] = ctypes.c_void_p(shim.rc_batch_new())
        if gen is not None:
            shim.rc_obb_begins(h, gen); shim.rc_hull_above_record(h)
    yield hs
    for h in hs.values():
        shim.rc_batch_free(h)


FORCED = {"none": (False, NONE), "match": (True, 7), "stale": (True, 6)}
G = 7


def prep_states(B, slot):
    """name -> (key, rc of the join)"""
    return {"none": ([0, 0, 0, 0, 0], OK), "resident, current": ([1, 0, slot, B, G], OK), "resident, stale generation": ([1, 0, slot, B, G - 1], OK),
            "B differs": ([1, 0, slot, B + 1, G], OK), "rc failed": ([1, 0, slot, B, G], -5), "staged for gen + 1": ([1, 1, slot, 4, G + 1], OK),
            "staged and voided": ([1, 1, slot, 4, NONE], OK), "staged, committed since": ([1, 1, slot, B, G], OK), "staged, joined by an upload": ([0, 1, slot, 4, G + 1], OK),
            "resident, joined": ([0, 0, slot, B, G], OK)}


def test_plan_grid(shim, forced):
    n = 0
    for B, window, hull_mode, force, overlap, staged_active, mask, slot, hslot in itertools.product(
            (1, 2, 3, 5), (0, 1, 2, 4), (0, 1), ("none", "match", "stale"), (0, 1), (0, 1), (ALL, ALL & ~OBB), (0, 1), (0, 1)):
        for name, (key, prc) in prep_states(B, slot).items():
            got = plan(shim, forced[force], mask, key, B=B, window=window, hull_mode=hull_mode, overlap=overlap, staged_active=staged_active, batch_gen=G, hslot=hslot, prep_rc=prc)
            want = parent_plan(mask, B, window, hull_mode, *FORCED[force], G, overlap, staged_active, hslot, key, prc)
            assert got == want, (B, window, hull_mode, force, overlap, staged_active, mask, slot, hslot, name)
            n += 1
    assert n > 30000


def test_plan_literals(shim, forced):
    cur = [1, 0, 1, 5, G]
    base = dict(B=5, batch_gen=G, hslot=0, overlap=1)
    # host hulls, everything lines up: the prepared slot is taken, the next foreground hull goes to the other one, the next preparation starts
    assert plan(shim, forced["none"], ALL, cur, hull_mode=0, **base) == dict(dev_hull=0, win=5, prepared_slot=1, next_hslot=0, void_staged_hulls=0, fetch_points=0, start_overlap=1)
    # the device hull never takes a prepared slot (nor fetches points, nor starts a preparation)
    for force in ("none", "stale"):
        p = plan(shim, forced[force], ALL, cur, hull_mode=1, **base)
        assert (p["dev_hull"], p["prepared_slot"], p["fetch_points"], p["start_overlap"]) == (1, -1, 0, 0), force
    # ... but a batch with a hull above the record is on the host hull in device mode
    p = plan(shim, forced["match"], ALL, cur, hull_mode=1, **base)
    assert (p["dev_hull"], p["prepared_slot"], p["start_overlap"]) == (0, 1, 1)
    # windows only with host hulls and B > win; a windowed run takes no prepared hulls and starts no preparation
    assert plan(shim, forced["none"], ALL, cur, hull_mode=0, window=2, **base) == dict(dev_hull=0, win=2, prepared_slot=-1, next_hslot=0, void_staged_hulls=0, fetch_points=1, start_overlap=0)
    assert plan(shim, forced["none"], ALL, cur, hull_mode=1, window=2, **base)["win"] == 5
    assert plan(shim, forced["none"], ALL, cur, hull_mode=0, window=5, **base)["win"] == 5
    assert plan(shim, forced["none"], ALL & ~OBB, cur, hull_mode=0, window=2, **base)["win"] == 5
    # overlap does not start while a batch is staged, nor without SH_STAGE_OBB, nor when it is off
    assert plan(shim, forced["none"], ALL, cur, hull_mode=0, staged_active=1, **base)["start_overlap"] == 0
    assert plan(shim, forced["none"], ALL & ~OBB, cur, hull_mode=0, **base)["start_overlap"] == 0
    assert plan(shim, forced["none"], ALL, cur, hull_mode=0, **dict(base, overlap=0))["start_overlap"] == 0
    # a resident run with OBB voids the hulls waiting for a staged batch (one without leaves them)
    waiting = [1, 1, 1, 4, G + 1]
    p = plan(shim, forced["none"], ALL, waiting, hull_mode=0, staged_active=1, **base)
    assert (p["void_staged_hulls"], p["prepared_slot"], p["fetch_points"], p["next_hslot"]) == (1, -1, 1, 0)
    assert plan(shim, forced["none"], ALL & ~OBB, waiting, hull_mode=0, staged_active=1, **base)["void_staged_hulls"] == 0
    # ... and behind the commit they are the resident batch's: taken
    p = plan(shim, forced["none"], ALL, [1, 1, 1, 5, G], hull_mode=0, **base)
    assert (p["void_staged_hulls"], p["prepared_slot"], p["next_hslot"]) == (0, 1, 0)
