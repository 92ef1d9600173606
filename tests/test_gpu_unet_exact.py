"""Every UNet kernel variant against exact answers.  On the integer networks of tests/unet_exact.py every activation, weight, bias and
partial sum is an integer that bf16, f16, the split-f16 operands and f32 accumulation hold exactly (test_unet_exact_host.py proves that on
the CPU), so all six configurations -- f32, f32x, bf16, f16, and the 16-bit reference network (SHOULDER_UNET_REFERENCE=1) -- must return
the bytes of one float64 evaluation: the logits, and every skip tensor the runner keeps (enc<i>b's output), so that a failure names the
level.  That includes the two deliberate differences of the fused level-0 kernels (first-conv weights rounded to the element type with a
hi + lo image, head summed from unrounded activations): both are exact on such data.  No tolerance anywhere.

The cases (unet_exact.CASES): the default network on 1 and 5 images of 256 x 256 (ragged work tickets over 256 workgroups), 256 x 768 and
768 x 256 (24 tiles across, 48 down: the persistent kernels' item -> (image, tile, group) arithmetic off the powers of two); base 32 at
depth 2 and 1 (the fused level 0 beside a short decoder, one tile); base 64 depth 2 (unfused 16-bit production kernels beside the LDS-DMA
and register-resident up-conv kernels); base 96 depth 1 (cout % 64 != 0, staged up-conv, NT = 2); base 32 depth 5 on 512 x 512 (1 024
channels: generic kernel inside the production network, staged up4, 1 024-channel LDS-DMA input, the 512-channel up-convs).

Time.  CPU: forward_exact over the whole table 40 - 49 s on 8 cores (20 s on the GPU machine's 16), spent once per session in the `case`
fixture (per case 10.3 / 4.4 / 0.9 / 2.0 / 0.7 / 1.8 s there), not in the test functions.  GPU: every test function (one case in one
configuration: all its seeds and shapes, with the network loaded per seed) takes 0.02 - 0.54 s on an MI355X; the slowest are the f32
configurations (0.40 s for the default network's four shapes and two seeds, 0.07 s for the depth-5 network), the 18-seed cases take
0.02 - 0.29 s."""
import contextlib

import numpy as np
import pytest

import unet_exact as ux
from shoulder_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = {"f32": _lib.UNET_F32, "f32x": _lib.UNET_F32X, "bf16": _lib.UNET_BF16, "f16": _lib.UNET_F16}
PARAMS = [(i, config) for i, c in enumerate(ux.CASES) for config in c[4]]
IDS = ["base%d_depth%d-%s" % (ux.CASES[i][0], ux.CASES[i][1], config) for i, config in PARAMS]


@pytest.fixture(scope="module")
def case(request):
    """the case's oracle, once for its configurations (C1 and C2 asserted as it is computed)"""
    c = ux.CASES[request.param]
    base, depth, seeds, shapes, _ = c
    for seed in seeds:
        for shape in shapes:
            ux.oracle(base, depth, seed, shape)
    yield c
    ux.forget_weights()      # (the depth-5 network: 31 M parameters)


@pytest.fixture(scope="module")
def engines():
    """config -> engine: one of this module's own for the production arms, one created under SHOULDER_UNET_REFERENCE=1 for the reference arms"""
    from conftest import engine_with_env
    from shoulder_amd.engine import Engine
    with contextlib.ExitStack() as stack:
        made = {}

        def get(config):
            ref = config.endswith("_reference")
            if ref not in made:
                if ref:
                    made[ref] = stack.enter_context(engine_with_env(SHOULDER_UNET_REFERENCE=1))
                else:
                    made[ref] = Engine(0)
                    stack.callback(made[ref].close)
            return made[ref]
        yield get


def decode(config, u):
    if config.startswith("bf16"):
        return (u.astype(np.uint32) << 16).view(np.float32)
    return u.view(np.float16).astype(np.float32)


def mismatch(config, case, seed, shape, what, got, want):
    """None when equal; else the configuration, the case, the first differing (image, y, x) and the differing pixels per row and column of
    32 x 16 tiles (a halo fault draws lines along tile edges, a dropped ticket range whole tiles or cout groups of them)"""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return "%s %s seed %d %s %s: shape %s, expected %s" % (config, case[:2], seed, shape, what, got.shape, want.shape)
    bad = got != want
    if bad.ndim == 4:
        chans = np.flatnonzero(bad.any(axis=(0, 1, 2)))
        bad = bad.any(axis=3)
    else:
        chans = None
    img, y, x = np.nonzero(bad)
    rows, cols = np.bincount(y // 16, minlength=(bad.shape[1] + 15) // 16), np.bincount(x // 32, minlength=(bad.shape[2] + 31) // 32)
    i0 = (int(img[0]), int(y[0]), int(x[0]))
    return ("%s base %d depth %d seed %d shape %s %s: %d of %d pixels differ, first at (image, y, x) = %s (got %s, expected %s)%s; per tile row (16 px) %s; "
            "per tile column (32 px) %s; per image %s" % (config, case[0], case[1], seed, shape, what, len(img), bad.size, i0, got[i0].ravel()[:8], want[i0].ravel()[:8],
                                                          "" if chans is None else "; channels %s" % chans[:16].tolist(), rows.tolist(), cols.tolist(),
                                                          np.bincount(img, minlength=bad.shape[0]).tolist()))


@pytest.mark.parametrize("case,config", PARAMS, indirect=["case"], ids=IDS)
def test_kernels_return_the_oracles_bytes(engines, case, config):
    base, depth, seeds, shapes, configs = case
    assert config in configs
    e = engines(config)
    name = config.partition("_")[0]
    b16 = name in ("bf16", "f16")
    e.set_params(unet_dtype=DTYPES[name])
    try:
        for seed in seeds:
            e.load_unet(ux.weights_of(seed, base, depth), base, depth)
            for shape in shapes:
                want, skips, _ = ux.oracle(base, depth, seed, shape)
                got = e.unet_infer(ux.make_exact_image(seed, *shape))
                n, H, W = shape
                for lvl in range(depth):      # top level first: the first level named is where the fault entered
                    h, w, C = H >> lvl, W >> lvl, base << lvl
                    if b16:      # channel-blocked: [n][C / 32][h][w][32] (k_unet16_base.h); with 32 channels that is [n][h][w][C]
                        t = decode(config, e.fetch("unet16.skip%d" % lvl, np.uint16, (n, C // 32, h, w, 32))).transpose(0, 2, 3, 1, 4).reshape(n, h, w, C)
                    else:
                        t = e.fetch("unet.skip%d" % lvl, np.float32, (n, h, w, C))
                    m = mismatch(config, case, seed, shape, "skip%d (enc%db)" % (lvl, lvl), t, skips[lvl].astype(np.float32))
                    assert m is None, m
                assert got.dtype == np.float32
                m = mismatch(config, case, seed, shape, "logits", got, want)
                assert m is None, m
    finally:
        e.set_params(unet_dtype=_lib.UNET_F32)
