"""The exact-integer UNet oracle (tests/unet_exact.py) on the CPU, before any kernel runs: its own conditions C1 (every value an integer
the element types hold), C2 (the networks stay alive) and C3 (the weights reach every output channel, every (tap, 32-channel slice) and,
over a small network's seeds, every row), its runtime, and which kernels of the runner's plan (sh_unet_plan.h) the case table reaches.
A mismatch on the GPU (test_gpu_unet_exact.py) can then only be a kernel's."""
import pytest

import unet_exact as ux
from test_unet_plan_host import BF16, DTYPES, F16, F32X, plan, shim  # noqa: F401  (shim: the fixture that builds tests/hostcheck/unet_plan_check.cpp)
from shoulder_amd import unet_spec

CASES = ux.CASES
IDS = ["base%d_depth%d" % c[:2] for c in CASES]
FIRST, HEAD, POOL = 1, 2, 4
# forward_exact over the whole table: 49 s on 8 cores (25 s of it the default network's 30 images of 256 x 256 in all; the depth-5 network
# 4 s).  The bound leaves a loaded or slower machine five times that; past it the table has outgrown a suite that runs on every change.
ORACLE_SECONDS_MAX = 240.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c1_c2_c3(case):
    base, depth, seeds, shapes, _ = case
    small = ux.max_rows(base, depth) <= ux.ROWS_ALL_COVERED
    held = []
    for seed in seeds:
        w = ux.weights_of(seed, base, depth)
        ux.check_weights(w, base, depth)      # C1 (parameters), C3 (per network and seed)
        for shape in shapes:
            logits, skips, stats = ux.oracle(base, depth, seed, shape)      # C1 (every layer, the logits) and C2 inside
            assert len(stats) == 5 * depth + 3 and logits.shape == shape and len(skips) == depth
            ux.check_live(stats)
        if small:
            held.append({k: v for k, v in w.items() if k.endswith("_w")})
    if small:
        assert len(seeds) == 18 and ux.rows_missing(held, base, depth) == {}      # C3 (every row, the seeds together)
    ux.forget_weights()


def test_the_table_is_the_issues():
    assert [(c[0], c[1], len(c[2])) for c in CASES] == [(32, 4, 2), (32, 2, 18), (32, 1, 18), (64, 2, 18), (96, 1, 18), (32, 5, 1)]
    assert [ux.max_rows(*c[:2]) <= ux.ROWS_ALL_COVERED for c in CASES] == [False, True, True, True, True, False]
    assert all(c[4] == ux.ALL_CONFIGS for c in CASES[:5]) and set(CASES[5][4]) == {"bf16", "f16", "f32x", "f32"}
    for base, depth, _, shapes, _ in CASES:
        assert all(H % (16 << depth) == 0 and W % (16 << depth) == 0 for _, H, W in shapes)


def test_oracle_runtime():
    for base, depth, seeds, shapes, _ in CASES:
        for seed in seeds:
            for shape in shapes:
                ux.oracle(base, depth, seed, shape)
    ux.forget_weights()
    print("forward_exact over the whole table: %.1f s" % ux.ORACLE_SECONDS[0])
    assert ux.ORACLE_SECONDS[0] < ORACLE_SECONDS_MAX


# ---- which kernels the cases reach -----------------------------------------------------------------------------------------------
def kernels(L, base, depth, config, n, H, W):
    """(text, template arguments) of every step of the pass, on both persistent grids; `raw` aside (unet_infer never passes it)"""
    name, _, ref = config.partition("_")
    out = set()
    for pgrid in (224, 256):
        rc, text, steps = plan(L, base, depth, DTYPES[name], bool(ref), H, W, n, pgrid, False)
        assert rc == 0, (text, base, depth, H, W)
        out |= {(s["text"], s["targs"]) for s in steps}
    return out


def reached(L):
    got = set()
    for base, depth, _, shapes, configs in CASES:
        for n, H, W in shapes:
            for config in configs:
                got |= kernels(L, base, depth, config, n, H, W)
    return got


def test_cases_reach_every_kernel_the_product_runs(shim):
    """The default network at 64 x 512 x 512 and 1 x 512 x 512, all four element types, reference on and off, both grids: every kernel of
    those passes also runs in some case of the table (the 32-wide bottom level of 512 x 512 -- bota / botb on the LDS-DMA kernel, up3 on
    k_upconv16g<16,...> and k_upconv_x3r<16,1> -- through the depth-5 network, whose level 4 is that map)."""
    got = {t for t, _ in reached(shim)}
    product = set()
    for n in (64, 1):
        for name in DTYPES:
            for ref in ("", "_reference"):
                product |= {t for t, _ in kernels(shim, unet_spec.BASE, unet_spec.DEPTH, name + ref, n, 512, 512)}
    assert len(product) > 40 and product <= got, sorted(product - got)


def test_cases_reach_the_kernels_named(shim):
    """The variants no pass of the default network takes, by name.  Two cannot be reached and are left out:
      k_conv_mfma_x3<9,2,UF_HEAD>  no plan fuses the head into dec0b on the f32x path (sh_unet_plan.h: it stays on k_head, whose sequential
                                   chain is the exact path's); the library only keeps the instantiation.  Held below: no accepted network
                                   plans it.
      k_conv_mfma16<.,9,4,UF_POOL> the pool fused into the generic 16-bit kernel needs more than 512 output channels above the bottleneck
                                   of a base-32 network: depth 6, whose smallest image is 1024 x 1024.  Held below: every plan that
                                   names a kernel the cases do not reach has depth 6."""
    got = reached(shim)
    texts = {t for t, _ in got}
    want = {"k_head<32>", "k_head<64>"} | {"k_upconv_x3r<%d,%d>" % (c0 // 32, 4 if c0 <= 128 else 2 if c0 == 256 else 1) for c0 in (64, 128, 256, 512)}
    for e in ("bf16", "f16"):
        want |= {"k_conv_first16<%s>" % e, "k_maxpool2_16<%s>" % e, "k_head16<%s>" % e, "k_conv_mfma16<%s,9,2,0>" % e, "k_conv_mfma16<%s,9,4,0>" % e, "k_upconv16<%s>" % e}
        want |= {"k_upconv16g<%s,%d,%d,%d,%s>" % (e, c0 // 32, 4 if c0 == 128 else 2, 2 if c0 == 512 else 4, "false" if c0 == 512 else "true") for c0 in (128, 256, 512)}
        want |= {"k_conv3_ldr16<%s,%d,%d>" % (e, fuse, wres) for fuse in (0, POOL) for wres in (0, 1)}
    assert want <= texts, sorted(want - texts)
    x3 = {a for t, a in got if t.startswith("k_conv_mfma_x3<9,")}      # (the text hides the FIRST bit: the template arguments)
    assert {a[1] for a in x3} == {2, 4} and {a[2] for a in x3} == {0, POOL, FIRST | POOL}
    assert {nt for nt in (2, 4) for a in x3 if a[1] == nt and a[2] == 0} == {2, 4} and (9, 2, POOL, 0) in x3 and (9, 4, POOL, 1) in x3
    # every kernel any accepted network plans, on maps of one and two tiles a side at the bottom level (the sizes every branch turns on)
    by_depth = {}
    for base in range(32, 257, 32):
        for depth in range(1, 7):
            for config in ux.ALL_CONFIGS:
                for H in (16 << depth, 32 << depth):
                    for W in (16 << depth, 32 << depth, 64 << depth):
                        for k in kernels(shim, base, depth, config, 1, H, W):
                            by_depth.setdefault(k, set()).add(depth)
    assert not any(t.startswith("k_conv_mfma_x3") and a[2] & HEAD for t, a in by_depth)
    left = set(by_depth) - got
    assert {t for t, _ in left} == {"k_conv_mfma16<bf16,9,4,4>", "k_conv_mfma16<f16,9,4,4>"} and all(by_depth[k] == {6} for k in left)


def test_the_depth5_case_takes_the_branches_no_other_network_does(shim):
    base, depth, _, shapes, configs = CASES[-1]
    (n, H, W), = shapes
    assert (base, depth) == (32, 5)
    for name, e in (("bf16", BF16), ("f16", F16)):
        assert name in configs
        s = {x["timer"]: x for x in plan(shim, base, depth, e, False, H, W, n, 256, False)[2]}
        assert s["unet.bota"]["text"] == "k_conv_mfma16<%s,9,4,0>" % name and s["unet.bota"]["cout"] == 1024      # generic kernel inside the production network
        assert s["unet.up4"]["text"] == "k_upconv16<%s>" % name and s["unet.up4"]["C0"] == 1024                  # staged up-convolution
        assert s["unet.dec4a"]["text"] == "k_conv3_ldr16<%s,0,0>" % name and s["unet.dec4a"]["C0"] + s["unet.dec4a"]["C1"] == 1024
        assert s["unet.up3"]["text"] == "k_upconv16g<%s,16,2,2,false>" % name
    s = {x["timer"]: x for x in plan(shim, base, depth, F32X, False, H, W, n, 256, False)[2]}
    assert s["unet.up3"]["text"] == "k_upconv_x3r<16,1>" and s["unet.up4"]["text"] == "k_conv_mfma_x3<1,4,0>"
