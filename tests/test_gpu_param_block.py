"""The parameter block on the device (shoulder_amd/csrc/sh_params.h states its layout: unet floats | feat | thr | true_idx | false_idx |
leaf_weight | roots): its bytes after every order of loading, the host mirrors behind a commit, a refused block, and the packed forest
of the groove stage following the block.  Every test builds its own engines and closes them."""
import contextlib
import os

import numpy as np
import pytest

from conftest import BONES, ROOT

pytestmark = pytest.mark.gpu

RFC = os.path.join(ROOT, "shoulder_amd", "models", "rfc_bg3.npz")
FOREST_KEYS = ("feat", "thr", "true_idx", "false_idx", "leaf_weight", "roots")
FOREST_TYPES = (np.int32, np.float32, np.int32, np.int32, np.float32, np.int32)


@pytest.fixture(scope="module")
def forest():
    return dict(np.load(RFC))


@pytest.fixture(scope="module")
def one_tree(forest):
    """the first tree of the shipped forest alone: 801 nodes that point only at each other, roots [0]"""
    n = int(forest["roots"][1])
    z = {k: forest[k][:n].copy() for k in FOREST_KEYS[:5]}
    z["roots"] = forest["roots"][:1].copy()
    assert n == 801 and z["true_idx"].max() < n and z["false_idx"].max() < n
    return z


@pytest.fixture(scope="module")
def small_net():
    from shoulder_amd import unet_spec
    return unet_spec.make_teacher_weights(base=32, depth=1)      # the smallest network sh_load_unet takes


def packed(weights, depth=1):
    from shoulder_amd.engine import unet_pack_order
    return np.concatenate([np.asarray(weights[k], dtype=np.float32).ravel() for k in unet_pack_order(depth)])


def forest_bytes(z):
    return np.concatenate([np.ascontiguousarray(z[k], dtype=t).view(np.uint8) for k, t in zip(FOREST_KEYS, FOREST_TYPES)])


def block_bytes(weights, z):
    return np.concatenate([packed(weights).view(np.uint8), forest_bytes(z)])


def save(tmp_path, name, z):
    p = str(tmp_path / name)
    np.savez(p, **z)
    return p


@contextlib.contextmanager
def new_engine():
    from shoulder_amd.engine import Engine
    e = Engine(0)
    try:
        yield e
    finally:
        e.close()


def block(e):
    n = e.param_block()[1]
    return e.fetch("params", np.uint8, (n,))


def test_bytes_of_the_block(tmp_path, forest, one_tree, small_net):
    want = block_bytes(small_net, forest)
    with new_engine() as e, new_engine() as f:
        e.load_rfc()
        e.load_unet(small_net, 32, 1)
        assert e.param_block()[1] == len(want)
        np.testing.assert_array_equal(block(e), want)
        f.load_unet(small_net, 32, 1)      # the other order
        f.load_rfc()
        assert f.param_block()[1] == len(want)
        np.testing.assert_array_equal(block(f), want)
        # a smaller forest afterwards: the block is laid out again, the network part as it was
        e.load_rfc(save(tmp_path, "one_tree.npz", one_tree))
        relaid = block_bytes(small_net, one_tree)
        assert len(relaid) == 4 * len(packed(small_net)) + 20 * 801 + 4
        assert e.param_block()[1] == len(relaid)
        np.testing.assert_array_equal(block(e), relaid)


def test_mirrors_follow_a_commit(tmp_path, forest, one_tree, small_net):
    F = len(packed(small_net))
    N = len(forest["feat"])
    leaf = int(np.nonzero(forest["true_idx"] < 0)[0][3])
    lw_at = 4 * F + 16 * N + 4 * leaf
    one = save(tmp_path, "one_tree.npz", one_tree)

    def prepared(e):
        e.load_rfc()
        e.load_unet(small_net, 32, 1)
        b = block(e)
        b[4 * 7:4 * 8] = np.array([0.375], np.float32).view(np.uint8)
        b[lw_at:lw_at + 4] = np.array([0.8125], np.float32).view(np.uint8)
        e.store("params", b)
        e.param_block_commit()
        return b

    with new_engine() as e, new_engine() as f:
        b = prepared(e)
        assert not np.array_equal(b, block_bytes(small_net, forest))
        e.load_rfc(one)      # re-uploads the network from its mirror
        got = block(e)
        np.testing.assert_array_equal(got[:4 * F], b[:4 * F])
        assert got[4 * 7:4 * 8].view(np.float32)[0] == np.float32(0.375)
        np.testing.assert_array_equal(got[4 * F:], forest_bytes(one_tree))
        b = prepared(f)
        f.load_unet(small_net, 32, 1)      # re-uploads the forest from its mirrors
        got = block(f)
        np.testing.assert_array_equal(got[:4 * F], packed(small_net).view(np.uint8))
        np.testing.assert_array_equal(got[4 * F:], b[4 * F:])
        assert got[lw_at:lw_at + 4].view(np.float32)[0] == np.float32(0.8125)


def test_a_bad_block_is_refused_and_nothing_moves(forest, small_net):
    from shoulder_amd.engine import ShoulderHipError
    F = len(packed(small_net))
    N = len(forest["feat"])
    with new_engine() as e:
        e.load_rfc()
        e.load_unet(small_net, 32, 1)
        good = block(e)
        branch = np.nonzero(forest["true_idx"] >= 0)[0]
        bad = dict(forest)
        bad["true_idx"] = forest["true_idx"].copy()
        bad["true_idx"][branch[5]] = forest["roots"][0]      # a branch points back at its root: a cycle
        e.store("params", block_bytes(small_net, bad))
        assert not np.array_equal(block(e)[4 * F + 8 * N:4 * F + 12 * N], good[4 * F + 8 * N:4 * F + 12 * N])
        with pytest.raises(ShoulderHipError) as err:
            e.param_block_commit()
        assert err.value.code == -1 and "forest" in str(err.value)
        e.load_unet(small_net, 32, 1)      # the mirrors did not move: the original forest comes back
        np.testing.assert_array_equal(block(e)[4 * F:], forest_bytes(forest))
        np.testing.assert_array_equal(block(e), good)


def test_the_packed_forest_follows_the_block(tmp_path, forest):
    """The groove stage packs the forest's nodes once per parameter block ("rfc.nodes"): a second sh_load_rfc, and a block written over
    it and committed, must both be seen by the next run (no stale packed copy).  No network: stages OBB .. GROOVE."""
    from shoulder_amd import _lib
    stages = _lib.STAGE_OBB | _lib.STAGE_FULL | _lib.STAGE_NECK | _lib.STAGE_CANAL | _lib.STAGE_PROXIMAL | _lib.STAGE_GROOVE
    stl = os.path.join(BONES, "humerus_left.stl")
    half = dict(forest)
    half["leaf_weight"] = forest["leaf_weight"] * np.float32(0.5)
    half_npz = save(tmp_path, "half.npz", half)

    def proba(e):
        e.run(stages, strict=False)      # (with halved leaf weights no peak may pass the groove's 0.4: that humerus' status, not an error here)
        return e.fetch("groove.proba", np.float32, (330 * 7,))

    with new_engine() as e, new_engine() as f:
        e.load_rfc()
        e.upload_stl([stl])
        first = block(e)
        a = proba(e)
        assert np.isfinite(a).all() and a.max() > 0
        e.load_rfc(half_npz)
        b = proba(e)
        assert not np.array_equal(a, b)
        f.load_rfc(half_npz)
        f.upload_stl([stl])
        np.testing.assert_array_equal(proba(f), b)
        # the first block written over the halved one (what a broadcast does), then committed
        e.store("params", first)
        e.param_block_commit()
        np.testing.assert_array_equal(proba(e), a)
