"""Networks and images on which every element type of the UNet computes exactly (helper of test_unet_exact_host.py and
test_gpu_unet_exact.py; no test functions, no library code under test).

Every intermediate value of the forward pass is an integer in [0, 255]: representable in bf16 (8 significant bits), f16 and f32.
Every weight is 0, +-1 or +-2 and every bias an integer of magnitude <= 255: representable in every type, the 64 w of the split-f16
operands included.  Every partial sum of every layer is an integer far below 2^24 in any summation order, so f32 accumulation and
every rounding to the element type are exact, and all kernel variants must return the bytes of one float64 evaluation.

Layers (rows of a layer: r = tap * cin + c, the order of its weight array [taps][cin][cout]):
  3x3 conv + ReLU   per output channel one of  copy (+1 at one row) | complement (-1 there, bias 255) | difference (+1 at one row, -1
                    at another, bias in [-32, 0]) | threshold (+1, bias in [-128, -1]); with one input channel the first two only.
                    Each maps integers in [0, 255] to integers in [0, 255].
  2x2 up-conv       per output channel one sign for its four taps (+1 with bias 0 | -1 with bias 255), each tap its own input channel.
  head              +1 +2 +1 +1 -1 -2 -1 -1 over and over on ALL channels (turned by the seed), bias 3: |logit| <= 2 * 96 * 255 + 3 < 2^16.  On
                    eight channels only, one dropped weight of bota, up1 or dec0b changed no logit at all: the logits are all the
                    decoder shows of itself, so the head has to look at every channel of it.
An output channel's first non-zero row is dealt by stride, not drawn (C3 below): row (j * rows // cout + seed) % rows.

The conditions the tests assert -- they belong to this oracle, not to the library:
  C1 exactness   check_exact (inside forward_exact) and check_weights
  C2 liveness    check_live on the LayerStats forward_exact returns
  C3 coverage    check_weights (every output channel, every (tap, 32-channel slice)); rows_missing (all rows, over the seeds of a case)
"""
import time

import numpy as np

from oracle.unet import _conv3, _pool, _up

HEAD_TAPS = (1, 2, 1, 1, -1, -2, -1, -1)
ROWS_ALL_COVERED = 2304      # C3: networks whose largest layer has at most this many rows get every row covered by their seeds together


def channels(base, depth):
    return [base << i for i in range(depth + 1)]


def layer_shapes(base, depth):
    """name -> (taps, cin, cout) in the order of the forward pass"""
    ch = channels(base, depth)
    t = {}
    for i in range(depth):
        t["enc%da" % i] = (9, ch[i - 1] if i else 1, ch[i])
        t["enc%db" % i] = (9, ch[i], ch[i])
    t["bota"], t["botb"] = (9, ch[depth - 1], ch[depth]), (9, ch[depth], ch[depth])
    for i in reversed(range(depth)):
        t["up%d" % i] = (4, ch[i + 1], ch[i])
        t["dec%da" % i] = (9, 2 * ch[i], ch[i])
        t["dec%db" % i] = (9, ch[i], ch[i])
    t["head"] = (1, ch[0], 1)
    return t


def first_row(j, rows, cout, seed):
    """C3: the row of output channel j's first non-zero weight"""
    return ((j * rows // cout if rows >= cout else j) + seed) % rows


def make_exact_weights(seed, base, depth):
    """The weight dict of oracle/unet.py (float32) of the seeded exact network."""
    rng = np.random.default_rng([seed, base, depth])
    w = {}
    for name, (taps, cin, cout) in layer_shapes(base, depth).items():
        rows = taps * cin
        if name == "head":
            w["head_w"], w["head_b"] = np.roll(np.tile(np.array(HEAD_TAPS, np.float32), cin // 8), seed), np.float32(3.0)
            continue
        W = np.zeros((rows, cout), np.float32)
        b = np.zeros(cout, np.float32)
        j = np.arange(cout)
        if taps == 4:
            neg = rng.integers(0, 2, cout).astype(bool)
            c0 = (j * cin // cout if cin >= cout else j) + seed
            for t in range(4):      # tap t reads a channel of its own: the strided one moved on by t quarters of the channels and t
                W[t * cin + (c0 + t * (cin // 4 + 1)) % cin, j] = np.where(neg, -1.0, 1.0)
            b[neg] = 255.0
        else:
            r1 = np.array([first_row(k, rows, cout, seed) for k in j])
            pat = rng.integers(0, 2 if cin == 1 else 4, cout)
            r2 = (r1 + rng.integers(1, rows, cout)) % rows      # another row
            W[r1, j] = np.where(pat == 1, -1.0, 1.0)
            d = pat == 2
            W[r2[d], j[d]] = -1.0
            b[pat == 1] = 255.0
            b[d] = -rng.integers(0, 33, int(d.sum()))
            b[pat == 3] = -rng.integers(1, 129, int((pat == 3).sum()))
        w[name + "_w"], w[name + "_b"] = W.reshape(2 if taps == 4 else 3, 2 if taps == 4 else 3, cin, cout), b
    return w


def make_exact_image(seed, n, H, W):
    """n images of integers 0..255 as float32"""
    return np.random.default_rng([seed, n, H, W]).integers(0, 256, (n, H, W)).astype(np.float32)


def check_weights(weights, base, depth):
    """C1 for the parameters, and the two parts of C3 that hold for every network and seed."""
    for name, (taps, cin, cout) in layer_shapes(base, depth).items():
        W, b = np.asarray(weights[name + "_w"], np.float64).reshape(taps * cin, cout), np.asarray(weights[name + "_b"], np.float64).reshape(-1)
        assert np.isin(W, (0.0, 1.0, -1.0, 2.0, -2.0)).all(), name
        assert (b == np.rint(b)).all() and np.abs(b).max() <= 255, name
        assert (W != 0).any(axis=0).all(), "%s: an output channel without a weight" % name
        if cin >= 32:
            assert (W != 0).reshape(taps, cin // 32, 32, cout).any(axis=(2, 3)).all(), "%s: a (tap, 32-channel slice) without a weight" % name


def rows_missing(weight_list, base, depth):
    """C3 over the seeds of a case: layer -> rows (tap * cin + c) no seed puts a weight on; empty when all are covered"""
    out = {}
    for name, (taps, cin, cout) in layer_shapes(base, depth).items():
        hit = np.zeros(taps * cin, bool)
        for w in weight_list:
            hit |= (np.asarray(w[name + "_w"]).reshape(taps * cin, cout) != 0).any(axis=1)
        if not hit.all():
            out[name] = np.flatnonzero(~hit).tolist()
    return out


def max_rows(base, depth):
    return max(t * cin for t, cin, _ in layer_shapes(base, depth).values())


class LayerStats(dict):
    """layer -> (fraction of non-zero elements, distinct values); "logits" -> (fraction > 0, fraction < 0)"""


def check_exact(name, x):
    """C1 for one layer's output (float64) -> the same values as uint8"""
    assert (x == np.rint(x)).all() and x.min() >= 0 and x.max() <= 255, "%s leaves the integers of [0, 255]" % name
    return x.astype(np.uint8)


def check_live(stats):
    """C2"""
    for name, (a, b) in stats.items():
        if name == "logits":
            assert a >= 0.05 and b >= 0.05, ("logits", a, b)
        else:
            assert a >= 0.25 and b >= 64, (name, a, b)


def forward_exact(weights, image):
    """image (n, H, W) -> (logits float64 (n, H, W), layers: name -> uint8 (n, h, w, C) of every layer's output, LayerStats).
    One float64 evaluation with oracle/unet.py's layer functions; C1 is asserted on every layer as it is computed (which is what
    lets the outputs be kept as bytes)."""
    dt = np.float64
    image = np.asarray(image, np.float32)
    assert image.ndim == 3
    d = 0
    while "enc%da_w" % d in weights:
        d += 1
    logits, layers = [], {}

    def keep(name, x):
        layers.setdefault(name, []).append(check_exact(name, x))
        return x

    for img in image:
        x = img.astype(dt)[:, :, None]
        skips = []
        for i in range(d):
            x = keep("enc%da" % i, _conv3(x, weights["enc%da_w" % i], weights["enc%da_b" % i], True, dt))
            x = keep("enc%db" % i, _conv3(x, weights["enc%db_w" % i], weights["enc%db_b" % i], True, dt))
            skips.append(x)
            x = _pool(x)
        x = keep("bota", _conv3(x, weights["bota_w"], weights["bota_b"], True, dt))
        x = keep("botb", _conv3(x, weights["botb_w"], weights["botb_b"], True, dt))
        for i in reversed(range(d)):
            x = keep("up%d" % i, _up(x, weights["up%d_w" % i], weights["up%d_b" % i], dt))
            x = np.concatenate([skips[i], x], axis=2)
            x = keep("dec%da" % i, _conv3(x, weights["dec%da_w" % i], weights["dec%da_b" % i], True, dt))
            x = keep("dec%db" % i, _conv3(x, weights["dec%db_w" % i], weights["dec%db_b" % i], True, dt))
        lg = x @ weights["head_w"].astype(dt) + dt(weights["head_b"])
        assert (lg == np.rint(lg)).all() and np.abs(lg).max() < 2 ** 16, "logits"
        logits.append(lg)
    logits = np.stack(logits)
    layers = {k: np.stack(v) for k, v in layers.items()}
    stats = LayerStats((k, (float(np.count_nonzero(v)) / v.size, int(np.count_nonzero(np.bincount(v.ravel(), minlength=256))))) for k, v in layers.items())
    stats["logits"] = (float((logits > 0).mean()), float((logits < 0).mean()))
    return logits, layers, stats


# ---- the cases: one table for the host test and the GPU test --------------------------------------------------------------------
ALL_CONFIGS = ("f32", "f32x", "bf16", "f16", "bf16_reference", "f16_reference")
# 18 seeds per small network: 18 is the stride of the widest layer's first rows (dec<i>a: 9 * 2C rows over C output channels), so seeds
# that cover the residues 0..17 put a weight on every row.  A seed that failed C2 (logits of one sign) is replaced by seed + 36 k, which
# keeps its residue for every stride a layer here has (2, 4, 8, 9, 12, 18).
def seeds18(*other):
    s = {k % 36: k for k in other}
    assert all(k >= 36 and k % 36 < 18 for k in other) and len(s) == len(other)
    return tuple(s.get(k, k) for k in range(18))


# (base, depth, seeds, shapes (n, H, W), configurations)
CASES = (
    (32, 4, (0, 1), ((1, 256, 256), (5, 256, 256), (1, 256, 768), (2, 768, 256)), ALL_CONFIGS),
    (32, 2, seeds18(42, 79), ((2, 64, 64), (3, 64, 192), (1, 192, 64), (1, 128, 128)), ALL_CONFIGS),      # (128: a 32-wide bottom level, up1 on k_upconv16g)
    (32, 1, seeds18(), ((1, 32, 32), (4, 32, 96), (2, 96, 32)), ALL_CONFIGS),
    (64, 2, seeds18(41, 46, 52), ((2, 64, 128),), ALL_CONFIGS),
    (96, 1, seeds18(41, 48), ((2, 32, 64),), ALL_CONFIGS),
    (32, 5, (0,), ((1, 512, 512),), ("bf16", "f16", "f32x", "f32")),
)

_ORACLE = {}
_WEIGHTS = {}      # the network built last (the deepest one: 31 M parameters, 125 MB)
ORACLE_SECONDS = [0.0]      # wall time spent in forward_exact by oracle()


def weights_of(seed, base, depth):
    key = (seed, base, depth)
    if key not in _WEIGHTS:
        _WEIGHTS.clear()
        _WEIGHTS[key] = make_exact_weights(seed, base, depth)
    return _WEIGHTS[key]


def forget_weights():
    _WEIGHTS.clear()


def oracle(base, depth, seed, shape):
    """(logits float32, [enc<i>b as uint8 (n, h, w, C)], LayerStats) of one (network, seed, shape): computed once per process, C1 and C2
    asserted, shared by every test and configuration that needs it, never written to."""
    key = (base, depth, seed, tuple(shape))
    if key not in _ORACLE:
        w, img = weights_of(seed, base, depth), make_exact_image(seed, *shape)
        t0 = time.perf_counter()
        logits, layers, stats = forward_exact(w, img)
        ORACLE_SECONDS[0] += time.perf_counter() - t0
        check_live(stats)
        out = logits.astype(np.float32), [layers["enc%db" % i] for i in range(depth)], stats
        out[0].setflags(write=False)
        for s in out[1]:
            s.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]
