"""The host rules of the parameters (shoulder_amd/csrc/sh_params.h: the layout of the device parameter block, the forest check, the
checks of sh_set_params, ParamState; sh_unet_plan.h: the layer table of sh_load_unet), without a GPU.  The expected values are what
upload_params, sh_param_block, stage_groove, sh_load_rfc, sh_param_block_commit, sh_set_params, sh_load_unet and the writers of the
loose parameter fields of sh_ctx did before the header existed, written out here in plain Python."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import host_twin
from conftest import ROOT
from shoulder_amd import _lib
from shoulder_amd.engine import unet_pack_order

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
RFC = os.path.join(ROOT, "shoulder_amd", "models", "rfc_bg3.npz")
OK, ARG = 0, -1
MAXBASE = 256
SHIPPED = (7759521, 32282, 40)      # floats of the base-32 depth-4 network, nodes and trees of models/rfc_bg3.npz
T_FEAT, T_CHILD, T_ROOT = "feature id out of range", "bad child index", "bad root"
T_FOREST = "the node tables do not describe a forest (a node is reachable twice)"
T_UNET = "sh_load_unet: bad argument (base must be a multiple of 32, at most 256; depth 1..6)"
u64, i64 = ctypes.c_ulonglong, ctypes.c_longlong
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = host_twin.build_shim("params", tmp_path_factory.mktemp("params_check"), std="c++17")
    vp, txt, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int
    L.pc_state_new.restype = vp
    for name, args in dict(pc_layout=[u64, u64, u64, vp], pc_forest_view=[u64, u64, u64, u64, vp], pc_mirror=[u64, u64, u64, vp], pc_features=[],
                           pc_forest_check=[i32p, i32p, i32p, i, i32p, i, txt], pc_default_params=[vp], pc_run_params=[vp, txt],
                           pc_layer_table=[i, i, ctypes.c_char_p, i, ctypes.POINTER(i64), txt], pc_layer_names=[i, ctypes.c_char_p, i],
                           pc_state_free=[vp], pc_state_event=[vp, i, i64, i64, i64], pc_state_queries=[vp, vp], pc_same_shape=[vp, vp]).items():
        getattr(L, name).argtypes = args
    return L


@pytest.mark.parametrize("header,body", [("sh_params.h", "sh::ParamState s; sh::ParamMirror m; m.resize(s.shape()); return s.has_unet() || sh::ParamLayout(s.shape()).total;"),
                                         ("sh_unet_plan.h", "sh::UnetLayers l; size_t n; return sh::unet_layer_table(32, 4, &l, &n).code;")])
def test_the_header_compiles_alone(tmp_path, header, body):
    """each header by itself, plain g++, warnings are errors, no HIP include on the path"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { %s }\n' % (header, body))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(tmp_path / "alone"), str(src)])
    subprocess.check_call([str(tmp_path / "alone")])


def test_the_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/hostcheck/params_check.cpp as a stand-alone program with -fsanitize=address,undefined (nothing loaded into python)"""
    exe = host_twin.build_shim("params", tmp_path, sanitize=True, std="c++17")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "params_check OK" in r.stdout, r.stdout + r.stderr


# ---- layout ------------------------------------------------------------------------------------------------------------------------------
def parent_offsets(F, N, T):
    """upload_params' seven puts (`o += n` behind each), and sh_param_block's size formula"""
    offs, o = [], 0
    for n in (F * 4, N * 4, N * 4, N * 4, N * 4, N * 4, T * 4):
        offs.append(o)
        o += n
    assert o == F * 4 + N * 20 + T * 4
    return offs, F * 4 + N * 20 + T * 4


SHAPES = [SHIPPED, (0, 32282, 40), (SHIPPED[0], 0, 0), (0, 0, 0), (100961, 801, 1), (1, 1, 1), (0, 801, 1), (100961, 1634, 2)]


@pytest.mark.parametrize("F,N,T", SHAPES)
def test_layout(shim, F, N, T):
    out = (u64 * 8)()
    shim.pc_layout(F, N, T, out)
    offs, total = parent_offsets(F, N, T)
    assert list(out) == offs + [total]
    # stage_groove's hand-computed pointers: pp = block + unet_floats * 4, then pp + N * 4 k
    view = (u64 * 6)()
    block = 0x7F0000001000
    shim.pc_forest_view(F, N, T, block, view)
    assert list(view) == [block + 4 * F + 4 * N * k for k in range(6)]
    # a mirror resized to the shape hands out every section at its offset with its bytes (upload and commit walk this)
    m = (u64 * 21)()
    shim.pc_mirror(F, N, T, m)
    assert [tuple(m[3 * k:3 * k + 3]) for k in range(7)] == [(n, o, 4 * n) for n, o in zip((F, N, N, N, N, N, T), offs)]


# ---- the forest check ------------------------------------------------------------------------------------------------------------------------
def parent_load_rfc(feat, ti, fi, n, roots):
    """sh_load_rfc's loops at the parent commit (texts behind "sh_load_rfc: ")"""
    for i in range(n):
        if feat[i] < 0 or feat[i] >= 9:
            return ARG, T_FEAT
        if (ti[i] < 0) != (fi[i] < 0) or ti[i] >= n or fi[i] >= n:
            return ARG, T_CHILD
    for r in roots:
        if r < 0 or r >= n:
            return ARG, T_ROOT
    seen = [False] * n
    for r in roots:
        stack = [r]
        while stack:
            i = stack.pop()
            if seen[i]:
                return ARG, T_FOREST
            seen[i] = True
            if ti[i] >= 0:
                stack += [ti[i], fi[i]]
    return OK, ""


def parent_commit(feat, ti, fi, n, roots):
    """sh_param_block_commit's loops at the parent commit: the roots are checked tree by tree, between the walks"""
    for i in range(n):
        if feat[i] < 0 or feat[i] >= 9:
            return ARG
        if (ti[i] < 0) != (fi[i] < 0) or ti[i] >= n or fi[i] >= n:
            return ARG
    seen = [False] * n
    for r in roots:
        if r < 0 or r >= n:
            return ARG
        stack = [r]
        while stack:
            i = stack.pop()
            if seen[i]:
                return ARG
            seen[i] = True
            if ti[i] >= 0:
                stack += [ti[i], fi[i]]
    return OK


def forest_check(L, z):
    c = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    text = ctypes.c_char_p()
    code = L.pc_forest_check(c(z["feat"]), c(z["true_idx"]), c(z["false_idx"]), len(z["feat"]), c(z["roots"]), len(z["roots"]), ctypes.byref(text))
    return code, text.value.decode()


@pytest.fixture(scope="module")
def forest():
    return {k: v for k, v in np.load(RFC).items() if k in ("feat", "true_idx", "false_idx", "roots")}


def first_trees(z, k):
    """the first k trees alone (their nodes point only at each other)"""
    n = int(z["roots"][k])
    return dict(feat=z["feat"][:n].copy(), true_idx=z["true_idx"][:n].copy(), false_idx=z["false_idx"][:n].copy(), roots=z["roots"][:k].copy())


def edited(z, **edits):
    out = {k: v.copy() for k, v in z.items()}
    for key, (at, value) in edits.items():
        out[key][at] = value
    return out


def test_the_shipped_forest_and_its_first_trees_pass(shim, forest):
    assert shim.pc_features() == 9 and forest["feat"].max() == 8
    assert forest_check(shim, forest) == (OK, "")
    one, two = first_trees(forest, 1), first_trees(forest, 2)
    assert len(one["feat"]) == 801 and list(one["roots"]) == [0] and len(two["feat"]) == 1634 and list(two["roots"]) == [0, 801]
    assert forest_check(shim, one) == (OK, "") and forest_check(shim, two) == (OK, "")


def test_every_fault_alone_and_the_earlier_of_two(shim, forest):
    z = first_trees(forest, 2)
    n = len(z["feat"])
    branch = np.nonzero(z["true_idx"] >= 0)[0]
    leaf = np.nonzero(z["true_idx"] < 0)[0]
    second = branch[branch > 801]
    faults = {
        "feature id -1": (dict(feat=(17, -1)), T_FEAT),
        "feature id at the count": (dict(feat=(n - 1, shim.pc_features())), T_FEAT),
        "a leaf with one child": (dict(true_idx=(leaf[3], 5)), T_CHILD),
        "a child index >= n": (dict(false_idx=(branch[7], n)), T_CHILD),
        "a negative root": (dict(roots=(1, -1)), T_ROOT),
        "a root >= n": (dict(roots=(0, n)), T_ROOT),
        "a cycle": (dict(true_idx=(branch[5], 0)), T_FOREST),
        "a shared subtree": (dict(true_idx=(second[4], branch[2])), T_FOREST),
    }
    for name, (edits, text) in faults.items():
        bad = edited(z, **edits)
        assert forest_check(shim, bad) == (ARG, text), name
        assert parent_load_rfc(bad["feat"], bad["true_idx"], bad["false_idx"], n, bad["roots"]) == (ARG, text), name
        assert parent_commit(bad["feat"], bad["true_idx"], bad["false_idx"], n, bad["roots"]) == ARG, name
    assert "forest" in T_FOREST      # (tests/test_gpu_errors.py matches the word)
    # two faults: all nodes in index order, then all roots, then reachability (sh_load_rfc's order)
    assert leaf[0] < 900
    assert forest_check(shim, edited(z, feat=(900, 9), true_idx=(leaf[0], 3)))[1] == T_CHILD
    assert forest_check(shim, edited(z, feat=(900, 9), roots=(0, -4)))[1] == T_FEAT
    assert forest_check(shim, edited(z, false_idx=(branch[-1], n + 7), roots=(1, n)))[1] == T_CHILD
    assert forest_check(shim, edited(z, true_idx=(branch[5], 0), roots=(1, n)))[1] == T_ROOT        # (the commit used to name the cycle of tree 0 here)
    assert forest_check(shim, edited(z, true_idx=(branch[5], 0), feat=(1600, -3)))[1] == T_FEAT


def test_random_corruptions_agree_with_the_parent_loops(shim, forest):
    """300 seeded corruptions (one to three edits) of the 801-node forest: the code is both parent loops', the text sh_load_rfc's"""
    z = first_trees(forest, 1)
    n = 801
    rng = random.Random(801)
    seen = set()
    for step in range(300):
        bad = {k: v.copy() for k, v in z.items()}
        index = lambda: rng.choice((rng.randrange(n), rng.randrange(n), -1, n, -3, n + 2))      # in range, or just outside it
        if step % 4 == 0:
            bad["roots"] = np.array([0, index()], np.int32)      # a second root: in range it shares a subtree
        for _ in range(rng.randrange(1, 4)):
            key = rng.choice(("feat", "true_idx", "false_idx", "true_idx", "false_idx", "roots"))
            at = rng.randrange(len(bad[key]))
            bad[key][at] = rng.randrange(-2, 11) if key == "feat" else index()
        got = forest_check(shim, bad)
        assert got == parent_load_rfc(bad["feat"], bad["true_idx"], bad["false_idx"], n, bad["roots"]), step
        assert got[0] == parent_commit(bad["feat"], bad["true_idx"], bad["false_idx"], n, bad["roots"]), step
        seen.add(got[1])
    assert seen == {"", T_FEAT, T_CHILD, T_ROOT, T_FOREST}


# ---- the run parameters ----------------------------------------------------------------------------------------------------------------------
T_CUT = "cut-off fractions must lie in [0, 1]"
T_GROOVE = "groove_cutoff must select 330 proximal rows"
T_CANAL = "canal_cutoff selects fewer than 2 slices"
T_WINDOW = "groove_deg_window must lie in [0, 180] degrees"
T_DTYPE = "unet_dtype must be SH_UNET_F32, SH_UNET_F32X, SH_UNET_BF16 or SH_UNET_F16"
T_BONE = "bone_kind must be SH_BONE_HUMERUS or SH_BONE_PROXIMAL"
DEFAULTS = dict(canal=(0.35, 0.75), groove=(0.2, 0.75), window=7.0, dtype=0, bone=0)


def parent_set_params(canal, groove, window, dtype, bone):
    """sh_set_params' checks at the parent commit, in their order"""
    cutoff_range = lambda n, c0, c1: (int((1.0 - c1) * n), int((1.0 - c0) * n))      # (sh_common.h; the fractions are in [0, 1] by then)
    for x in (groove[0], groove[1], canal[0], canal[1]):
        if not (0.0 <= x <= 1.0):
            return ARG, T_CUT
    a, b = cutoff_range(600, *groove)
    if b - a != 330:
        return ARG, T_GROOVE
    a, b = cutoff_range(200, *canal)
    if b - a < 2 or a < 0 or b > 200:
        return ARG, T_CANAL
    if not (0.0 <= window <= 180.0):
        return ARG, T_WINDOW
    if dtype not in (0, 1, 2, 3):
        return ARG, T_DTYPE
    if bone not in (0, 1):
        return ARG, T_BONE
    return OK, ""


def run_params(L, canal, groove, window, dtype, bone):
    p = _lib.Params()
    p.canal_cutoff[:] = canal
    p.groove_cutoff[:] = groove
    p.groove_deg_window, p.unet_dtype, p.bone_kind = window, dtype, bone
    text = ctypes.c_char_p()
    return L.pc_run_params(ctypes.byref(p), ctypes.byref(text)), text.value.decode()


def test_the_defaults_are_sh_default_params_and_are_accepted(shim):
    p = _lib.Params()
    shim.pc_default_params(ctypes.byref(p))
    got = dict(canal=tuple(p.canal_cutoff), groove=tuple(p.groove_cutoff), window=p.groove_deg_window, dtype=p.unet_dtype, bone=p.bone_kind)
    assert got == DEFAULTS      # (sh_default_params at the parent commit, field by field)
    assert run_params(shim, **DEFAULTS) == (OK, "") == parent_set_params(**DEFAULTS)


def test_every_refusal_of_set_params_in_its_order(shim):
    nan = float("nan")
    alone = [(dict(groove=(-0.1, 0.75)), T_CUT), (dict(groove=(0.2, 1.01)), T_CUT), (dict(canal=(nan, 0.75)), T_CUT), (dict(canal=(0.35, 2.0)), T_CUT),
             (dict(groove=(0.3, 0.75)), T_GROOVE), (dict(groove=(0.75, 0.2)), T_GROOVE), (dict(canal=(0.75, 0.75)), T_CANAL), (dict(canal=(0.8, 0.3)), T_CANAL),
             (dict(window=-1.0), T_WINDOW), (dict(window=180.5), T_WINDOW), (dict(window=nan), T_WINDOW), (dict(dtype=4), T_DTYPE), (dict(dtype=-1), T_DTYPE),
             (dict(bone=2), T_BONE), (dict(bone=-1), T_BONE)]
    for kw, text in alone:
        args = dict(DEFAULTS, **kw)
        assert parent_set_params(**args) == (ARG, text), kw
        assert run_params(shim, **args) == (ARG, text), kw
    # accepted edges
    for kw in (dict(window=0.0), dict(window=180.0), dict(dtype=3), dict(bone=1), dict(canal=(0.0, 1.0)), dict(groove=(0.45, 1.0))):
        args = dict(DEFAULTS, **kw)
        assert run_params(shim, **args) == (OK, "") == parent_set_params(**args), kw
    # every pair of faults: the earlier check names it
    bad = [dict(canal=(0.35, 2.0)), dict(groove=(0.3, 0.75)), dict(canal=(0.75, 0.75)), dict(window=200.0), dict(dtype=9), dict(bone=7)]
    order = [T_CUT, T_GROOVE, T_CANAL, T_WINDOW, T_DTYPE, T_BONE]
    for (i, a), (j, b) in itertools.combinations(enumerate(bad), 2):
        if "canal" in a and "canal" in b:
            continue
        args = dict(DEFAULTS, **a, **b)
        assert run_params(shim, **args) == (ARG, order[i]) == parent_set_params(**args), (a, b)


def test_set_params_grid(shim):
    n = 0
    for c0, c1, g0, g1, window, dtype, bone in itertools.product((0.0, 0.35, 0.75, 1.2), (0.36, 0.75, 1.0), (0.2, 0.25, -0.5), (0.75, 0.8), (7.0, 181.0), (0, 3, 4), (0, 1, 2)):
        args = dict(canal=(c0, c1), groove=(g0, g1), window=window, dtype=dtype, bone=bone)
        assert run_params(shim, **args) == parent_set_params(**args), args
        n += 1
    assert n == 4 * 3 * 3 * 2 * 2 * 3 * 3


# ---- the layer table of sh_load_unet ---------------------------------------------------------------------------------------------------------
def parent_layer_table(base, depth):
    """sh_load_unet's construction at the parent commit -> {name: (taps, cin, cout, w_off, b_off)}, floats"""
    layers, o = {}, 0

    def add(name, taps, cin, cout):
        nonlocal o
        w_off = o
        o += taps * cin * cout
        layers[name] = (taps, cin, cout, w_off, o)
        o += cout

    ch = [base << i for i in range(depth + 1)]
    cin = 1
    for i in range(depth):
        add(f"enc{i}a", 9, cin, ch[i])
        add(f"enc{i}b", 9, ch[i], ch[i])
        cin = ch[i]
    add("bota", 9, ch[depth - 1], ch[depth])
    add("botb", 9, ch[depth], ch[depth])
    for i in reversed(range(depth)):
        add(f"up{i}", 4, ch[i + 1], ch[i])
        add(f"dec{i}a", 9, 2 * ch[i], ch[i])
        add(f"dec{i}b", 9, ch[i], ch[i])
    add("head", 1, ch[0], 1)
    return layers, o


def layer_table(L, base, depth):
    out, n, text = ctypes.create_string_buffer(1 << 14), i64(), ctypes.c_char_p()
    rc = L.pc_layer_table(base, depth, out, len(out), ctypes.byref(n), ctypes.byref(text))
    rows = [ln.split(" ") for ln in out.value.decode().splitlines()]
    return rc, text.value.decode(), {r[0]: tuple(int(x) for x in r[1:]) for r in rows}, n.value


@pytest.mark.parametrize("base,depth", [(32, 1), (32, 4), (96, 2), (256, 1), (64, 6)])
def test_layer_table(shim, base, depth):
    rc, text, table, floats = layer_table(shim, base, depth)
    want, want_floats = parent_layer_table(base, depth)
    assert (rc, text) == (OK, "") and table == want and floats == want_floats
    if (base, depth) == (32, 4):
        assert floats == SHIPPED[0]
    # the names in block order: what the Python side concatenates the caller's arrays by
    out = ctypes.create_string_buffer(1 << 12)
    assert shim.pc_layer_names(depth, out, len(out)) == 0
    names = out.value.decode().split()
    assert [n + s for n in names for s in ("_w", "_b")] == unet_pack_order(depth)
    assert names == sorted(want, key=lambda k: want[k][3]) and names == list(want)      # ... which is the order of the offsets


@pytest.mark.parametrize("base,depth", [(16, 4), (48, 4), (MAXBASE + 32, 1), (32, 0), (32, 7), (0, 1), (-32, 1)])
def test_layer_table_refuses_bad_shapes(shim, base, depth):
    assert layer_table(shim, base, depth) == (ARG, T_UNET, {}, 0)


# ---- the state: the parent's loose fields and every place that assigned them -------------------------------------------------------------------
UNET_LOADED, RFC_LOADED, BLOCK_EXPOSED, BLOCK_LOST, PACKED16, PACKED_X3, PACKTAB_UPLOADED, FOREST_PACKED = range(8)
FRESH = [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1]      # neither loaded, no shape, every packed copy stale


class ParentFields:
    """sh_ctx at the parent commit: have_rfc, have_unet, rfc_nodes, rfc_trees, unet_base, unet_depth, unet_floats, the sizes of the
    mirrors h_unet / h_feat / h_roots, packed_rfc, and sh_ctx::Unet's packtab_ready, packed_x3, packed_kind; one method per place that
    assigned them, with the statements of that place."""

    def __init__(self):
        self.have_rfc = self.have_unet = self.packed_rfc = self.packtab_ready = self.packed_x3 = False
        self.rfc_nodes = self.rfc_trees = self.unet_base = self.unet_depth = self.unet_floats = 0
        self.h_unet = self.h_feat = self.h_roots = 0
        self.packed_kind = -1

    def params_changed(self):
        self.packed_kind, self.packed_x3, self.packed_rfc = -1, False, False

    def buffer_device(self, name):
        if name == "params":
            self.params_changed()

    def store(self, name):
        if name == "params":
            self.params_changed()

    def upload_params(self):
        self.params_changed()

    def load_rfc(self, nodes, trees):
        self.h_feat, self.h_roots = nodes, trees
        self.rfc_nodes, self.rfc_trees, self.have_rfc, self.packed_rfc = nodes, trees, True, False
        self.upload_params()

    def load_unet(self, base, depth, floats):
        self.packtab_ready = False
        self.h_unet = floats
        self.unet_floats, self.unet_base, self.unet_depth, self.have_unet = floats, base, depth, True
        self.upload_params()

    def param_block_commit(self):
        self.params_changed()

    def param_block(self):
        self.params_changed()
        return self.unet_floats * 4 + self.h_feat * 20 + self.h_roots * 4

    def pack_weights(self, kind):
        if (self.packed_x3 if kind < 0 else self.packed_kind == kind):
            return
        if not self.packtab_ready:
            self.packtab_ready = True
        if kind < 0:
            self.packed_x3 = True
        else:
            self.packed_kind = kind

    def stage_groove(self):
        if not self.packed_rfc:
            self.packed_rfc = True

    def bcast_differs(self, root):
        """sh_bcast_weights' comparison of a context with the root"""
        return (self.param_block() != root.param_block() or self.unet_base != root.unet_base or self.unet_depth != root.unet_depth
                or self.rfc_nodes != root.rfc_nodes or self.rfc_trees != root.rfc_trees)

    def queries(self):
        return [int(self.have_unet), int(self.have_rfc), self.unet_base, self.unet_depth, self.h_unet, self.h_feat, self.h_roots,
                int(self.packed_kind != 0), int(self.packed_kind != 1), int(not self.packed_x3), int(not self.packtab_ready), int(not self.packed_rfc)]


class Both:
    """one call of the library to the parent's fields and, as the events the library now fires there, to the header's ParamState"""

    def __init__(self, L):
        self.L, self.h, self.p = L, ctypes.c_void_p(L.pc_state_new()), ParentFields()

    def close(self):
        self.L.pc_state_free(self.h)

    def ev(self, event, a=0, b=0, c=0):
        self.L.pc_state_event(self.h, event, a, b, c)

    def queries(self):
        out = (i64 * 12)()
        self.L.pc_state_queries(self.h, out)
        return [int(x) for x in out]

    def check(self, what=""):
        assert self.queries() == self.p.queries(), what

    def upload(self, ok):
        self.ev(BLOCK_EXPOSED)
        if not ok:
            # THE INTENDED CHANGE: a failed upload has freed the block, so neither half stays loaded and every packed copy is stale (the
            # parent left the forest loaded behind a failed sh_load_unet, and both halves behind a failed sh_load_rfc)
            self.ev(BLOCK_LOST)
            assert self.queries() == FRESH
            self.p = ParentFields()

    def load_rfc(self, nodes, trees, ok=True):
        self.p.load_rfc(nodes, trees); self.ev(RFC_LOADED, nodes, trees); self.upload(ok)

    def load_unet(self, base, depth, floats, ok=True):
        self.p.load_unet(base, depth, floats); self.ev(UNET_LOADED, base, depth, floats); self.upload(ok)

    def exposed(self, how, name="params"):
        getattr(self.p, how)(*((name,) if how in ("buffer_device", "store") else ()))
        if name == "params":
            self.ev(BLOCK_EXPOSED)

    def pack_weights(self, kind):
        self.p.pack_weights(kind)
        q = self.queries()
        if not (q[9] if kind < 0 else q[7 + kind]):
            return
        if q[10]:
            self.ev(PACKTAB_UPLOADED)
        self.ev(PACKED_X3) if kind < 0 else self.ev(PACKED16, kind)

    def stage_groove(self):
        self.p.stage_groove()
        if self.queries()[11]:
            self.ev(FOREST_PACKED)


@pytest.fixture()
def both(shim):
    b = Both(shim)
    yield b
    b.close()


NEED16_BF16, NEED16_F16, NEED_X3, NEED_PACKTAB, NEED_FOREST = 7, 8, 9, 10, 11


def test_a_fresh_context(both):
    assert both.queries() == FRESH
    both.check()


def test_packed_copies_follow_the_block(both):
    both.load_rfc(32282, 40); both.load_unet(32, 4, SHIPPED[0]); both.check()
    assert both.queries() == [1, 1, 32, 4, *SHIPPED, 1, 1, 1, 1, 1]
    for how in ("param_block", "param_block_commit", "buffer_device", "store", "load_rfc", "load_unet"):
        both.pack_weights(0); both.pack_weights(-1); both.stage_groove(); both.check(how)
        assert both.queries()[NEED16_BF16:] == [0, 1, 0, 0, 0]
        both.pack_weights(1); both.check(how)
        assert both.queries()[NEED16_BF16:] == [1, 0, 0, 0, 0]      # one 16-bit copy: the other kind is stale again
        if how == "load_rfc":
            both.load_rfc(801, 1)
        elif how == "load_unet":
            both.load_unet(32, 1, 100961)
        else:
            both.exposed(how)
        both.check(how)
        assert both.queries()[NEED16_BF16:] == [1, 1, 1, int(how == "load_unet"), 1], how      # the layer table goes up once per loaded network
    both.pack_weights(1)
    for name in ("landmarks", "rfc.nodes", "params_bf16"):      # another buffer's pointer or bytes: nothing is stale
        both.exposed("buffer_device", name); both.exposed("store", name); both.check(name)
        assert both.queries()[NEED16_F16] == 0


def test_a_failed_upload_leaves_nothing_loaded(both):
    both.load_rfc(32282, 40); both.load_unet(32, 4, SHIPPED[0]); both.pack_weights(0); both.stage_groove()
    both.load_unet(64, 2, 5, ok=False)      # (asserts FRESH: the parent kept have_rfc over the freed block)
    both.check()
    both.load_unet(32, 1, 100961); both.load_rfc(801, 1, ok=False)
    assert both.queries() == FRESH
    both.load_rfc(801, 1); both.check()
    assert both.queries()[:7] == [0, 1, 0, 0, 0, 801, 1]


def test_same_shape_is_the_five_way_comparison(shim):
    shapes = [(32, 4, SHIPPED[0], 32282, 40), (32, 1, 100961, 32282, 40), (32, 4, SHIPPED[0], 801, 1), (32, 4, SHIPPED[0], 32282, 39), (64, 4, SHIPPED[0], 32282, 40),
              (32, 4, SHIPPED[0] - 5, 32283, 40), (32, 4, SHIPPED[0], 0, 0), (0, 0, 0, 801, 1)]
    made = []
    for base, depth, floats, nodes, trees in shapes:
        b = Both(shim)
        if nodes:
            b.load_rfc(nodes, trees)
        if floats:
            b.load_unet(base, depth, floats)
        b.pack_weights(len(made) % 2)      # (what is packed is no part of the shape)
        made.append(b)
    try:
        for a, r in itertools.product(made, made):
            assert shim.pc_same_shape(a.h, r.h) == int(not a.p.bcast_differs(r.p))
            assert shim.pc_same_shape(a.h, r.h) == int(a is r)
    finally:
        for b in made:
            b.close()


def test_random_event_sequences(shim):
    """4000 calls, fixed seed: after every one all queries agree with the parent's fields -- but behind a failed upload, where the
    state is fresh (Both.upload)"""
    rng = random.Random(20241020)
    names = ["params", "params", "landmarks", "obb_transform", "rfc.nodes"]
    nets = [(32, 1, 100961), (32, 4, SHIPPED[0]), (96, 2, 1234567)]
    forests = [(32282, 40), (801, 1), (1634, 2)]
    b = Both(shim)
    try:
        lost = 0
        for step in range(4000):
            k = rng.randrange(12)
            ok = rng.random() > 0.04
            lost += not ok and k < 2
            if k == 0:
                b.load_rfc(*rng.choice(forests), ok=ok)
            elif k == 1:
                b.load_unet(*rng.choice(nets), ok=ok)
            elif k == 2:
                b.exposed("buffer_device", rng.choice(names))
            elif k == 3:
                b.exposed("store", rng.choice(names))
            elif k == 4:
                b.exposed("param_block")
            elif k == 5:
                b.exposed("param_block_commit")
            elif k in (6, 7, 8):
                b.pack_weights(rng.choice((-1, 0, 1)))
            else:
                b.stage_groove()
            b.check((step, k))
        assert lost > 5
    finally:
        b.close()
