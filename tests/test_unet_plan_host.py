"""The host decisions of the UNet runner (shoulder_amd/csrc/sh_unet_plan.h: the steps of a forward pass, the ticket table of a
persistent launch, the layer table of the weight-packing kernels), without a GPU.  The expected values are the rules the runner
applied so far -- its two walks (f32 / f32x and 16-bit) and its two kernel ladders -- written out here as they stood, not read
from the plan; bench.sym_key, the third statement of the kernel rule, is held against the same steps."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402
from shoulder_amd import unet_spec  # noqa: E402

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "hostcheck", "unet_plan_check.cpp")
ERR_ARG = -1
F32, BF16, F16, F32X = 0, 1, 2, 3
DTYPES = {"f32": F32, "bf16": BF16, "f16": F16, "f32x": F32X}
FIRST, HEAD, POOL = 1, 2, 4
NONE, IMAGE, A, B, LOGITS, SKIP = -1, 0, 1, 2, 3, 4
E_SIZE = "unet: input size must be a multiple of 16 << depth"
FIELDS = ("timer", "text", "grid", "block", "C0", "C1", "H", "W", "cout", "relu", "fuse", "src0", "src1", "dst", "pool", "layers", "tickets", "targs")
DEFAULT_SIZES = [(256, 256), (256, 512), (512, 512)]
OTHER_NETS = [(96, 2, 64, 64), (160, 1, 32, 64), (64, 3, 128, 256), (256, 1, 32, 32)]      # test_other_widths_and_depths
NIMGS = (1, 5, 64, 200)
GRIDS = (256, 224)      # every CU of the device | with the CU reserve of a context that takes UNet turns


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("unet_plan_check") / "libunet_plan_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(so), SHIM])
    L = ctypes.CDLL(str(so))
    vp, txt, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int
    L.up_plan.argtypes = [i] * 9 + [ctypes.c_char_p, i, txt]
    L.up_tickets.argtypes = [i, i, i, vp, i]
    L.up_pack.argtypes = [i, i, vp, vp, i, vp, vp, txt]
    L.up_floats.restype = L.up_w_off.restype = ctypes.c_longlong
    L.up_w_off.argtypes = [i, i, ctypes.c_char_p]
    return L


def test_header_builds_with_gxx_alone(tmp_path):
    """compile-only: sh_unet_plan.h needs no HIP header and no hipcc"""
    src = tmp_path / "probe.cpp"
    src.write_text('#include "sh_unet_plan.h"\nint main() { sh::UnetStep s; std::vector<sh::UnetStep> v; sh::UnetLayers l;\n'
                   '  return sh::unet_plan(l, 32, 4, SH_UNET_BF16, false, 250, 512, 1, 256, false, &v).code == SH_ERR_ARG ? s.kind : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)])


# ---- the plan, as the shim prints it -----------------------------------------------------------------------------------------
def plan(L, base, depth, dtype, reference, H, W, nimg, pgrid, raw):
    out, t = ctypes.create_string_buffer(1 << 16), ctypes.c_char_p()
    rc = L.up_plan(base, depth, dtype, int(reference), H, W, nimg, pgrid, int(raw), out, len(out), ctypes.byref(t))
    if rc != 0:
        return rc, t.value.decode() if t.value else None, None
    steps = []
    for ln in out.value.decode().splitlines():
        f = ln.split(" ")
        n = [int(x) for x in f[2:23] + f[25:28]]
        steps.append(dict(timer=f[0], text=f[1], ek=n[1], targs=tuple(n[2:6]), grid=tuple(n[6:9]), block=n[9], C0=n[10], C1=n[11], H=n[12], W=n[13], cout=n[14],
                          relu=n[15], fuse=n[16], src0=n[17], src1=n[18], dst=n[19], pool=n[20], layers=(f[23], f[24]), tickets=tuple(n[21:24])))
    return 0, None, steps


# ---- the parent's rules --------------------------------------------------------------------------------------------------------
def layer_table(base, depth):
    """name -> (cin, cout, taps), as sh_load_unet builds it"""
    ch = [base << i for i in range(depth + 1)]
    t = {}
    for i in range(depth):
        t["enc%da" % i] = (ch[i - 1] if i else 1, ch[i], 9)
        t["enc%db" % i] = t["dec%db" % i] = (ch[i], ch[i], 9)
        t["up%d" % i] = (ch[i + 1], ch[i], 4)
        t["dec%da" % i] = (2 * ch[i], ch[i], 9)
    t["bota"], t["botb"], t["head"] = (ch[depth - 1], ch[depth], 9), (ch[depth], ch[depth], 9), (ch[0], 1, 1)
    return t


def step(timer, text, targs, grid, block, C0, C1, H, W, cout, relu=0, fuse=0, src0=NONE, src1=NONE, dst=NONE, pool=NONE, layer2="-", tickets=(0, 0, 0)):
    grid = tuple(grid) + (1,) * (3 - len(grid))
    return dict(timer=timer, text=text, targs=tuple(targs) + (0,) * (4 - len(targs)), grid=grid, block=block, C0=C0, C1=C1, H=H, W=W, cout=cout, relu=relu, fuse=fuse,
                src0=src0, src1=src1, dst=dst, pool=pool if fuse & POOL else NONE, layers=("-" if timer == "unet.pool" else timer[5:], layer2), tickets=tickets)


def flat(n, cap=8192):
    return (min((n + 255) // 256, cap),)


def parent_conv_layer(q, name, dtype, src0, src1, C0, C1, dst, H, W, relu, fuse=0, pooled=NONE):
    """conv_layer of unet.hip at the parent commit: the f32 and split-f16 kernels"""
    cin, cout, taps = q["layers"][name]
    nimg, tiles = q["nimg"], (H // 16) * (W // 16)
    assert H % 16 == 0 and W % 16 == 0
    kw = dict(C0=C0, C1=C1, H=H, W=W, cout=cout, fuse=fuse, src0=src0, src1=src1, dst=dst, pool=pooled)
    if dtype == F32X and C0 % 32 == 0 and C1 % 32 == 0 and cout % 32 == 0:
        x3 = lambda t, grid, relu_, l2="-": step("unet." + name, "k_conv_mfma_x3<%d,%d,%d>" % (t[0], t[1], t[2] & ~FIRST), t, grid, 256, relu=relu_, layer2=l2, **kw)
        if taps == 9 and fuse == (FIRST | POOL) and cout == 32 and C0 == 32 and C1 == 0:
            return x3((9, 2, FIRST | POOL, 0), (tiles, 1, nimg), relu, "enc0a")
        if taps == 9 and fuse == HEAD and cout == 32:
            return x3((9, 2, HEAD, 1), (tiles, 1, nimg), relu, "head")
        if taps == 9 and fuse == POOL and cout % 64 == 0:
            return x3((9, 4, POOL, 1), (tiles, cout // 64, nimg), relu)
        if taps == 9 and fuse == POOL:
            return x3((9, 2, POOL, 0), (tiles, cout // 32, nimg), relu)
        assert fuse == 0, "unet: unsupported fusion"
        if taps == 9 and cout % 64 == 0:
            return x3((9, 4, 0, 1), (tiles, cout // 64, nimg), relu)
        if taps == 9:
            return x3((9, 2, 0, 0), (tiles, cout // 32, nimg), relu)
        if C1 == 0 and W % 32 == 0 and H % 16 == 0 and C0 in (64, 128, 256, 512):
            nch, mt, rows = {64: (2, 4, 16), 128: (4, 4, 16), 256: (8, 2, 8), 512: (16, 1, 4)}[C0]
            return step("unet." + name, "k_upconv_x3r<%d,%d>" % (nch, mt), (nch, mt), ((W // 32) * (H // rows), nimg), 512, relu=relu, **kw)
        if cout % 64 == 0:
            return x3((1, 4, 0, 1), (tiles, cout // 64, nimg * 4), 0)
        return x3((1, 2, 0, 1), (tiles, cout // 32, nimg * 4), 0)
    t = (9 if taps == 9 else 1, 4 if cout % 64 == 0 else 2)
    return step("unet." + name, "k_conv_mfma_f32<%d,%d>" % t, t, (tiles, cout // (64 if cout % 64 == 0 else 32), nimg if taps == 9 else nimg * 4), 256,
                relu=relu if taps == 9 else 0, **kw)


def parent_forward(q, dtype):
    """unet_forward of unet.hip at the parent commit"""
    D, base, nimg, H, W, Ls = q["depth"], q["base"], q["nimg"], q["H"], q["W"], q["layers"]
    out = []
    a, b = A, B
    h, w = H, W
    x3 = dtype == F32X and base % 32 == 0
    x3_first = x3 and base == 32
    if not x3_first:
        out.append(step("unet.enc0a", "k_conv_first", (), flat(nimg * h * w), 256, 1, 0, h, w, Ls["enc0a"][1], relu=1, src0=IMAGE, dst=a))
    out.append(parent_conv_layer(q, "enc0b", dtype, a, NONE, base, 0, SKIP, h, w, 1, (FIRST | POOL) if x3_first else POOL if x3 else 0, b))
    if x3:
        a, b = b, a
    ch = base
    for i in range(1, D + 1):
        if not x3:
            out.append(step("unet.pool", "k_maxpool2", (), flat(nimg * (h // 2) * (w // 2) * (ch // 4)), 256, ch, 0, h, w, ch, src0=SKIP + i - 1, dst=a))
        h, w = h // 2, w // 2
        na, nb = ("enc%da" % i, "enc%db" % i) if i < D else ("bota", "botb")
        out.append(parent_conv_layer(q, na, dtype, a, NONE, ch, 0, b, h, w, 1))
        ch *= 2
        out.append(parent_conv_layer(q, nb, dtype, b, NONE, ch, 0, SKIP + i if i < D else a, h, w, 1, POOL if (x3 and i < D) else 0, a))
    x, y = a, b
    for i in range(D - 1, -1, -1):
        out.append(parent_conv_layer(q, "up%d" % i, dtype, x, NONE, ch, 0, y, h, w, 0))
        h, w, ch = h * 2, w * 2, ch // 2
        out.append(parent_conv_layer(q, "dec%da" % i, dtype, SKIP + i, y, ch, ch, x, h, w, 1))
        out.append(parent_conv_layer(q, "dec%db" % i, dtype, x, NONE, ch, 0, y, h, w, 1))
        x, y = y, x
    cin = Ls["head"][0]
    maxc, cap = (32, 16384) if cin <= 32 else (64, 8192)
    out.append(step("unet.head", "k_head<%d>" % maxc, (maxc,), flat(nimg * H * W, cap), 256, cin, 0, H, W, 1, src0=x, dst=LOGITS))
    return out


def parent_conv_layer16(q, name, et, src0, src1, C0, C1, dst, H, W, relu, fuse=0, pooled=NONE):
    """conv_layer16 of unet.hip at the parent commit"""
    cin, cout, taps = q["layers"][name]
    nimg, pgrid, ref, tiles = q["nimg"], q["pgrid"], q["reference"], (H // 16) * (W // 16)
    assert H % 16 == 0 and W % 16 == 0
    kw = dict(C0=C0, C1=C1, H=H, W=W, cout=cout, fuse=fuse, src0=src0, src1=src1, dst=dst, pool=pooled)
    generic = lambda t, grid, relu_: step("unet." + name, "k_conv_mfma16<%s,%d,%d,%d>" % ((et,) + t), t, grid, 256, relu=relu_, **kw)
    ldr = (not ref and taps == 9 and cout % 64 == 0 and cout <= 512 and W % 32 == 0 and H % 16 == 0 and C0 % 32 == 0 and C1 % 32 == 0
           and (fuse == 0 or (fuse == POOL and relu)))
    if ldr:
        total = nimg * (W // 32) * (H // 16) * (cout // 64)
        g = min(total, pgrid)
        wres = int(cout == 64 and ((C0 + C1) // 32) * 64 <= 128)
        return step("unet." + name, "k_conv3_ldr16<%s,%d,%d>" % (et, fuse, wres), (fuse, wres), (g,), 512, relu=relu, tickets=(total, g, cout // 64), **kw)
    if taps == 9 and cout % 64 == 0:
        assert fuse in (0, POOL), "unet: unsupported fusion"
        return generic((9, 4, fuse), (tiles, cout // 64, nimg), relu)
    if taps == 9:
        assert fuse == 0, "unet: unsupported fusion"
        return generic((9, 2, 0), (tiles, cout // 32, nimg), relu)
    if not ref and cout % 32 == 0 and C1 == 0 and C0 % 32 == 0:
        if W % 32 == 0 and H % 16 == 0 and C0 in (128, 256, 512) and cout <= 512:
            mt = 4 if C0 == 128 else 2
            nitems = (W // 32) * (H // (4 * mt)) * nimg
            grid = nitems if C0 == 512 else min(nitems, pgrid)
            t = {128: (4, 4, 4, 1), 256: (8, 2, 4, 1), 512: (16, 2, 2, 0)}[C0]
            return step("unet." + name, "k_upconv16g<%s,%d,%d,%d,%s>" % ((et,) + t[:3] + ("true" if t[3] else "false",)), t, (grid,), 512, relu=relu,
                        tickets=(nitems, grid, 1) if C0 != 512 else (0, 0, 0), **kw)
        return step("unet." + name, "k_upconv16<%s>" % et, (), (tiles, cout // 32, nimg * 2), 256, relu=relu, **kw)
    if cout % 64 == 0:
        return generic((1, 4, 0), (tiles, cout // 64, nimg * 4), 0)
    return generic((1, 2, 0), (tiles, cout // 32, nimg * 4), 0)


def parent_level0_fused(q):
    """unet16_level0_fused of unet.hip at the parent commit"""
    D, H, W = q["depth"], q["H"], q["W"]
    return not q["reference"] and q["base"] == 32 and D >= 1 and W % 32 == 0 and H % 16 == 0 and (H >> D) % 16 == 0 and (W >> D) % 16 == 0


def parent_forward16(q, et):
    """unet_forward16 of unet.hip at the parent commit.  What the three ping-pong launches state of their layers (C0 / C1 / fuse) is
    the layers' own: dec0a reads skip0 and the up-convolved input like the layer-by-layer dec0a."""
    D, base, nimg, H, W, Ls, pgrid = q["depth"], q["base"], q["nimg"], q["H"], q["W"], q["layers"], q["pgrid"]
    out = []
    fused = parent_level0_fused(q)
    h, w = H, W
    pp = lambda total: dict(grid=(min(total, pgrid),), block=0, tickets=(total, min(total, pgrid), 1))
    if fused:
        out.append(step("unet.enc0b", "k_enc0_pp<%s,%s>" % (et, "true" if q["raw"] else "false"), (int(q["raw"]),), C0=1, C1=0, H=h, W=w, cout=base, relu=1, fuse=FIRST | POOL,
                        src0=IMAGE, dst=SKIP, pool=A, layer2="enc0a", **pp(nimg * (w // 32) * (h // 16))))
    else:
        out.append(step("unet.enc0a", "k_conv_first16<%s>" % et, (), flat(nimg * h * w), 256, 1, 0, h, w, Ls["enc0a"][1], relu=1, src0=IMAGE, dst=A))
        out.append(parent_conv_layer16(q, "enc0b", et, A, NONE, base, 0, SKIP, h, w, 1))
    ch = base
    for i in range(1, D + 1):
        if not fused:
            out.append(step("unet.pool", "k_maxpool2_16<%s>" % et, (), flat(nimg * (h // 2) * (w // 2) * (ch // 8)), 256, ch, 0, h, w, ch, src0=SKIP + i - 1, dst=A))
        h, w = h // 2, w // 2
        na, nb = ("enc%da" % i, "enc%db" % i) if i < D else ("bota", "botb")
        out.append(parent_conv_layer16(q, na, et, A, NONE, ch, 0, B, h, w, 1))
        ch *= 2
        out.append(parent_conv_layer16(q, nb, et, B, NONE, ch, 0, SKIP + i if i < D else A, h, w, 1, POOL if (fused and i < D) else 0, A))      # fz.pooled = A
    x, y = A, B
    for i in range(D - 1, -1, -1):
        if fused and i == 0:
            h, w, ch = h * 2, w * 2, ch // 2
            out.append(step("unet.dec0a", "k_dec0a_up_pp<%s>" % et, (), C0=ch, C1=ch, H=h, W=w, cout=ch, relu=1, src0=SKIP, src1=x, dst=y, layer2="up0",
                            **pp(nimg * (w // 32) * (h // 8))))
            out.append(step("unet.dec0b", "k_dec0b_head_pp<%s>" % et, (), C0=ch, C1=0, H=h, W=w, cout=ch, relu=1, fuse=HEAD, src0=y, dst=LOGITS, layer2="head",
                            **pp(nimg * (w // 32) * (h // 16))))
            return out
        out.append(parent_conv_layer16(q, "up%d" % i, et, x, NONE, ch, 0, y, h, w, 0))
        h, w, ch = h * 2, w * 2, ch // 2
        out.append(parent_conv_layer16(q, "dec%da" % i, et, SKIP + i, y, ch, ch, x, h, w, 1))
        out.append(parent_conv_layer16(q, "dec%db" % i, et, x, NONE, ch, 0, y, h, w, 1))
        x, y = y, x
    out.append(step("unet.head", "k_head16<%s>" % et, (), flat(nimg * H * W), 256, Ls["head"][0], 0, H, W, 1, src0=x, dst=LOGITS))
    return out


def parent_plan(base, depth, dtype, reference, H, W, nimg, pgrid, raw):
    """unet_dispatch at the parent commit"""
    if (H >> depth) % 16 or (W >> depth) % 16:
        return ERR_ARG, E_SIZE, None
    q = dict(base=base, depth=depth, reference=reference, H=H, W=W, nimg=nimg, pgrid=pgrid, raw=raw, layers=layer_table(base, depth))
    if dtype in (BF16, F16):
        return 0, None, parent_forward16(q, "bf16" if dtype == BF16 else "f16")
    return 0, None, parent_forward(q, dtype)


def check(L, *case):
    want, got = parent_plan(*case), plan(L, *case)
    assert got[:2] == want[:2], case
    assert [s["timer"] for s in got[2]] == [s["timer"] for s in want[2]], case
    for g, w in zip(got[2], want[2]):
        for k in FIELDS:
            assert g[k] == w[k], (case, w["timer"], k, g[k], w[k])
        assert g["ek"] == {F32: -1, F32X: -1, BF16: 0, F16: 1}[case[2]]
    return want[2]


def all_cases():
    for name in sorted(DTYPES):
        for reference in (False, True):
            for nimg in NIMGS:
                for pgrid in GRIDS:
                    for raw in ((False, True) if name in ("bf16", "f16") else (False,)):
                        for H, W in DEFAULT_SIZES:
                            yield (unet_spec.BASE, unet_spec.DEPTH, DTYPES[name], reference, H, W, nimg, pgrid, raw)
                        for base, depth, H, W in OTHER_NETS:
                            yield (base, depth, DTYPES[name], reference, H, W, nimg, pgrid, raw)


def test_default_network_is_32_by_4():
    assert (unet_spec.BASE, unet_spec.DEPTH) == (32, 4)


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("reference", [False, True])
def test_plan_is_the_parents(shim, name, reference):
    n = 0
    for case in all_cases():
        if case[2] == DTYPES[name] and case[3] == reference:
            check(shim, *case)
            n += 1
    assert n == len(NIMGS) * len(GRIDS) * (len(DEFAULT_SIZES) + len(OTHER_NETS)) * (2 if name in ("bf16", "f16") else 1)


def test_the_steps_of_the_production_network(shim):
    """the counts the launch test on the GPU expects, and the two buffer swaps: enc0b's pool goes to B on the f32x path (the level loop
    then reads B as its A), to A on the 16-bit path"""
    d = (unet_spec.BASE, unet_spec.DEPTH)
    names = lambda *c: [s["timer"] for s in check(shim, *c)]
    prod = names(*d, BF16, False, 256, 256, 1, 256, False)
    assert len(prod) == 20 and not {"unet.enc0a", "unet.pool", "unet.up0", "unet.head"} & set(prod) and len(set(prod)) == 20
    for c in ((*d, BF16, True), (*d, F16, True), (*d, F32, False)):
        n = names(*c, 256, 256, 1, 256, False)
        assert len(n) == 27 and n.count("unet.pool") == 4 and len(set(n)) == 24
    x = names(*d, F32X, False, 256, 256, 1, 256, False)
    assert len(x) == 22 and "unet.enc0a" not in x and "unet.pool" not in x
    px = plan(shim, *d, F32X, False, 256, 256, 1, 256, False)[2]
    assert (px[0]["timer"], px[0]["pool"], px[0]["targs"]) == ("unet.enc0b", B, (9, 2, 5, 0)) and (px[1]["src0"], px[1]["dst"]) == (B, A)
    assert (px[2]["timer"], px[2]["src0"], px[2]["pool"]) == ("unet.enc1b", A, B)
    p16 = plan(shim, *d, BF16, False, 256, 256, 1, 256, True)[2]
    assert (p16[0]["timer"], p16[0]["pool"], p16[0]["text"]) == ("unet.enc0b", A, "k_enc0_pp<bf16,true>") and (p16[1]["src0"], p16[1]["dst"]) == (A, B)
    assert (p16[2]["timer"], p16[2]["src0"], p16[2]["pool"]) == ("unet.enc1b", B, A)


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("reference", [False, True])
def test_kernel_texts_against_bench_sym_key(shim, name, reference):
    """bench.sym_key states the kernel of a layer of the default network from (name, dtype, cout) alone: it carries no map size and
    is written for maps that tile by 32 x 16 down to the bottom level.  That holds at 256 x 512 and 512 x 512; at 256 x 256 the bottom
    level is 16 x 16, where the runner always took the generic kernels for bota, botb and up3 -- every other layer is held there too.
    sym_key answers with the layer's own name for the three element-wise kernels (first conv, pool, head)."""
    base, depth = unet_spec.BASE, unet_spec.DEPTH
    couts = {"unet." + k: v[1] for k, v in layer_table(base, depth).items()}
    odd = ("unet.up3",) if name == "f32x" else ("unet.bota", "unet.botb", "unet.up3") if name in ("bf16", "f16") and not reference else ()
    n = 0
    for H, W in DEFAULT_SIZES:
        for raw in (False, True):
            for nimg, pgrid in ((1, 256), (64, 224)):
                rc, _, steps = plan(shim, base, depth, DTYPES[name], reference, H, W, nimg, pgrid, raw)
                assert rc == 0
                for s in steps:
                    key = bench.sym_key(s["timer"], name, couts.get(s["timer"], 0), fused_net=not reference, raw_image=raw)
                    if s["timer"] in ("unet.enc0a", "unet.pool", "unet.head"):
                        assert key == s["timer"] and s["text"].split("<")[0] in ("k_conv_first", "k_maxpool2", "k_head", "k_conv_first16", "k_maxpool2_16", "k_head16")
                    elif (H, W) == (256, 256) and s["timer"] in odd:
                        assert s["W"] == 16 and s["text"] != key      # (no 32-wide tile: the generic kernel, which sym_key does not know of)
                    else:
                        assert s["text"] == key, (H, W, s["timer"], s["text"], key)
                        n += 1
    assert n > 200


def test_level0_fused_is_the_parents(shim):
    for base, depth, H, W in [(32, 4, 512, 512), (32, 4, 256, 256), (32, 1, 16, 32), (32, 1, 32, 32), (32, 1, 32, 48), (64, 3, 128, 256), (32, 4, 250, 512), (32, 2, 64, 64)]:
        for reference in (False, True):
            q = dict(base=base, depth=depth, reference=reference, H=H, W=W)
            for dtype in DTYPES.values():
                assert bool(shim.up_level0_fused(dtype, int(reference), base, depth, H, W)) == (dtype in (BF16, F16) and parent_level0_fused(q))


@pytest.mark.parametrize("H,W", [(250, 512), (512, 250), (256, 384), (128, 512)])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_input_size_error_comes_first(shim, name, H, W):
    for reference in (False, True):
        case = (unet_spec.BASE, unet_spec.DEPTH, DTYPES[name], reference, H, W, 3, 256, False)
        assert plan(shim, *case) == (ERR_ARG, E_SIZE, None) == parent_plan(*case)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_a_map_below_one_tile_is_refused(shim, name):
    """8 >> 4 is 0, which the size check lets through: the first conv layer's own check refuses the map"""
    assert plan(shim, unet_spec.BASE, unet_spec.DEPTH, DTYPES[name], False, 8, 8, 1, 256, False) == (ERR_ARG, "unet: feature map is not a multiple of 16", None)


# ---- ticket tables -------------------------------------------------------------------------------------------------------------
def parent_ticket_table(total, nwg, ngrp):
    """the loop of unet_tickets at the parent commit"""
    tab, pos = [], 0
    while pos < total:
        sz = max(1, int(math.ceil((total - pos) / (3.0 * float(nwg)))))
        if sz >= ngrp:
            sz = sz // ngrp * ngrp
        tab.append(pos)
        pos += min(sz, total - pos)
    tab.append(total)
    return tab


def test_ticket_tables(shim):
    triples = set()
    for case in all_cases():
        for s in parent_plan(*case)[2]:
            if s["tickets"][0]:
                triples.add(s["tickets"])
    assert len(triples) > 40 and any(t[2] == 8 for t in triples) and any(t[1] == 224 for t in triples) and any(t[0] == t[1] < 224 for t in triples)
    # total < nwg; total no multiple of ngrp (the last ticket is a partial set); ngrp > sz (single items, sets are split)
    edges = [(5, 256, 1), (1030, 224, 4), (64, 256, 8)]
    out = np.zeros(1 << 18, np.int32)
    for total, nwg, ngrp in sorted(triples) + edges:
        n = shim.up_tickets(total, nwg, ngrp, ctypes.c_void_p(out.ctypes.data), len(out))
        want = parent_ticket_table(total, nwg, ngrp)
        assert out[:n].tolist() == want, (total, nwg, ngrp)
        assert want[0] == 0 and want[-1] == total and all(a < b for a, b in zip(want, want[1:]))
    assert parent_ticket_table(5, 256, 1) == [0, 1, 2, 3, 4, 5]
    assert any((b - a) % 4 for a, b in zip(parent_ticket_table(1030, 224, 4), parent_ticket_table(1030, 224, 4)[1:]))
    assert parent_ticket_table(64, 256, 8) == list(range(65))


# ---- weight packing ------------------------------------------------------------------------------------------------------------
def pack(L, base, depth, w):
    rows, n, total, t = np.zeros((64, 6), np.int64), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_char_p()
    rc = L.up_pack(base, depth, ctypes.c_void_p(w.ctypes.data) if w is not None else None, ctypes.c_void_p(rows.ctypes.data), 64, ctypes.byref(n), ctypes.byref(total),
                   ctypes.byref(t))
    return rc, (t.value.decode() if t.value else None), rows[:n.value].tolist(), total.value


def parent_pack_table(L, base, depth):
    """the loop over c->ulayers (a std::map: by name) of both runners at the parent commit"""
    rows, total = [], 0
    for name, (cin, cout, taps) in sorted(layer_table(base, depth).items()):
        if cin < 32 or cout < 32:
            continue
        rows.append([total, L.up_w_off(base, depth, name.encode()), taps, cin, cout, 0])
        total += taps * cin * cout
    return rows, total


@pytest.mark.parametrize("base,depth", [(32, 4)] + [n[:2] for n in OTHER_NETS])
def test_pack_table(shim, base, depth):
    rows, total = parent_pack_table(shim, base, depth)
    assert len(rows) == 5 * depth + 1 and [r[0] for r in rows] == sorted(r[0] for r in rows)
    assert pack(shim, base, depth, None) == (0, None, rows, total)
    w = np.full(shim.up_floats(base, depth), 1023.0, np.float32)      # just inside the range
    assert pack(shim, base, depth, w) == (0, None, rows, total)


def test_f32x_weight_range_names_the_layer_and_the_bound(shim):
    base, depth = 32, 4
    bound = 65504.0 / 64.0
    w = np.full(shim.up_floats(base, depth), 0.25, np.float32)
    w[shim.up_w_off(base, depth, b"enc2a") + 11] = -2000.0
    w[shim.up_w_off(base, depth, b"dec1a") + 5] = np.float32(bound)      # the bound itself is outside; "dec1a" sorts before "enc2a"
    w[shim.up_w_off(base, depth, b"enc0a")] = 5000.0      # no MFMA layer: not split
    rc, text, _, _ = pack(shim, base, depth, w)
    assert rc == ERR_ARG
    assert text == "SH_UNET_F32X: layer dec1a has a weight of magnitude %g; the split-f16 operands hold |w| < %g (use SH_UNET_F32 for this network)" % (bound, bound)
    assert "1023.5" in text
    w[shim.up_w_off(base, depth, b"dec1a") + 5] = np.float32(1023.4375)      # the largest f32 below it that the text would round to the bound
    rc, text, _, _ = pack(shim, base, depth, w)
    assert rc == ERR_ARG and text.startswith("SH_UNET_F32X: layer enc2a has a weight of magnitude 2000;")


# ---- the same calls in a program of their own ----------------------------------------------------------------------------------
def test_standalone_program(tmp_path):
    exe = tmp_path / "unet_plan_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DUNET_PLAN_MAIN", "-o", str(exe), SHIM])
    out = subprocess.check_output([str(exe)]).decode()
    assert out.startswith("unet_plan_check: ") and out.rstrip().endswith("OK")
