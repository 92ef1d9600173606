"""Open contours in bridge mode (include/shoulder_hip.h sh_set_open_contours): meshes with isolated single-triangle holes give
the intact meshes' records bit for bit, the drop rule and the failures, the open-edge count, strict=False and the facade."""
import os

import numpy as np
import pytest

from conftest import BONES, engine_with_env
from shoulder_amd import _lib
from shoulder_amd.engine import ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu

FIXTURES = ["humerus_left", "humerus_right", "humerus_left_flipped", "humerus_left_trab"]
GAP = 4.0      # mm: holes are triangles whose longest edge is below it, pairwise farther apart than 4 * GAP


def _mesh(name):
    v, f = load_stl(os.path.join(BONES, name + ".stl"))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


def _np_open_edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return int(np.count_nonzero(cnt != 2))


def _holes(v, f, avoid, n_holes=12):
    """Single-triangle holes at evenly spaced heights (shaft, proximal region, distal end), deterministic by face centroid:
    the face nearest to each height whose longest edge is < GAP, > 4 GAP from every hole taken and from every point in `avoid`,
    and sharing no vertex with another hole."""
    c = v[f].astype(np.float64).mean(axis=1)
    L = np.linalg.norm(v[f] - v[np.roll(f, -1, axis=1)], axis=2).max(axis=1)
    z0, z1 = c[:, 2].min(), c[:, 2].max()
    taken, used_v = [], set()
    for q in np.linspace(0.03, 0.97, n_holes):
        order = np.argsort(np.abs(c[:, 2] - (z0 + q * (z1 - z0))), kind="stable")
        for i in order[:4000]:
            if L[i] >= GAP or used_v & set(f[i].tolist()):
                continue
            if taken and np.min(np.linalg.norm(c[taken] - c[i], axis=1)) <= 4 * GAP:
                continue
            if len(avoid) and np.min(np.linalg.norm(avoid - c[i], axis=1)) <= 4 * GAP:
                continue
            taken.append(int(i)); used_v |= set(f[i].tolist())
            break
    return np.array(taken)


def _rings(e, B):
    out = {}
    for s in ("distal", "prox", "neckc"):
        rn = e.fetch(s + ".ring_n", np.int32)
        N = rn.size // B
        rg = e.fetch(s + ".ring", np.float64).reshape(B * N, -1)
        out[s] = [(int(rn[p]), rg[p, : 2 * (int(rn[p]) + 1)].copy()) for p in range(B * N)]
    return out


@pytest.fixture(scope="module")
def holed_batch():
    meshes = [_mesh(n) for n in FIXTURES]
    with engine_with_env() as e:
        e.upload(meshes)
        intact = e.run(_lib.STAGE_ALL)
    out = []
    for b, (v, f) in enumerate(meshes):
        anp = np.array(intact[b]["anp_points"][: int(intact[b]["n_anp"])], dtype=np.float64)
        h = _holes(v, f, anp)
        out.append((v, np.delete(f, h, axis=0), h))
    return meshes, out


@pytest.mark.parametrize("dtype", [_lib.UNET_F32, _lib.UNET_BF16])
def test_single_triangle_holes_give_the_intact_records(holed_batch, dtype):
    meshes, holed = holed_batch
    with engine_with_env() as e:
        e.set_params(unet_dtype=dtype)
        e.upload(meshes)
        intact = e.run(_lib.STAGE_ALL)
        rings0 = _rings(e, len(meshes))
        cnt0 = {s: e.fetch(s + ".seg_count", np.int32) for s in ("distal", "prox")}
        e.set_open_contours("bridge", GAP)
        e.upload([(v, f) for v, f, _ in holed])
        assert all(8 <= len(h) <= 20 for _, _, h in holed), [len(h) for _, _, h in holed]
        got = e.run(_lib.STAGE_ALL)
        bridged, dropped = e.open_contour_stats()
        assert np.all(bridged > 0) and np.all(dropped == 0), (bridged, dropped)
        for name in intact.dtype.names:
            assert intact[name].tobytes() == got[name].tobytes(), name
        rings1 = _rings(e, len(meshes))
        for s, c0 in cnt0.items():      # holes do lie on planes of the ring-keeping sets: those planes lost a crossing each
            assert np.count_nonzero(e.fetch(s + ".seg_count", np.int32) < c0) > 0, s
        for s in rings0:
            assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(rings0[s], rings1[s])), s
        # the same batch in the default mode fails as before
        e.set_open_contours("error")
        with pytest.raises(ShoulderHipError) as ex:
            e.run(_lib.STAGE_ALL)
        assert ex.value.code == -5


def test_max_gap_zero_drops_the_open_chains(holed_batch):
    """The drop rule (max_gap = 0): a plane whose only loop a hole opens has no loop left -- SH_ERR_GEOMETRY on that record,
    with the dropped chains counted."""
    _, holed = holed_batch
    with engine_with_env() as e:
        e.set_open_contours("bridge", 0.0)
        e.upload([(v, f) for v, f, _ in holed])
        recs = e.run(_lib.STAGE_ALL, strict=False)
        assert np.all(recs["status"] == -5)
        bridged, dropped = e.open_contour_stats()
        assert np.all(bridged == 0) and np.all(dropped > 0)


def test_open_edge_count(holed_batch):
    meshes, holed = holed_batch
    with engine_with_env() as e:
        e.upload(meshes)
        assert e.open_edges().tolist() == [0] * len(meshes)
        e.upload([(v, f) for v, f, _ in holed])
        assert e.open_edges().tolist() == [_np_open_edges(f) for _, f, _ in holed] == [3 * len(h) for _, _, h in holed]
        # a synthetic batch of 64: the fixtures with 0..63 faces dropped from the front
        batch = [(meshes[i % 4][0], meshes[i % 4][1][i:]) for i in range(64)]
        e.upload(batch)
        assert e.open_edges().tolist() == [_np_open_edges(f) for _, f in batch]


def test_wide_band_stays_an_error_and_strict_false_keeps_the_good_records(oracle_bones):
    """The wide band of test_gpu_errors.py is far wider than a small max_gap: SH_ERR_GEOMETRY on its own record.  strict=False
    hands back the other 63 records, byte-equal to the all-good run's."""
    h = oracle_bones("humerus_left")
    zc = h.verts[:, 2][h.faces].mean(axis=1)
    keep = ~((zc > np.percentile(zc, 45)) & (zc < np.percentile(zc, 47)) & (h.verts[:, 0][h.faces].mean(axis=1) > np.median(h.verts[:, 0])))
    good = [(h.verts, h.faces)] * 64
    with engine_with_env() as e:
        e.upload(good)
        ref = e.run(_lib.STAGE_ALL)
        e.set_open_contours("bridge", 1.0)
        assert e.get_open_contours() == ("bridge", 1.0)
        e.upload([(h.verts, h.faces[keep])] + good[1:])
        with pytest.raises(ShoulderHipError) as ex:
            e.run(_lib.STAGE_ALL)
        assert ex.value.code == -5 and "mesh 0" in str(ex.value)
        recs = e.run(_lib.STAGE_ALL, strict=False)
        assert recs["status"][0] == -5 and np.all(recs["status"][1:] == 0)
        assert recs[1:].tobytes() == ref[1:].tobytes()
        e.submit(_lib.STAGE_ALL, fetch="view")
        recs2 = e.collect(strict=False)
        assert recs2[1:].tobytes() == ref[1:].tobytes()


def _write_stl(path, v, f):
    tri = v[f].astype(np.float32)
    rec = np.zeros(len(f), dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
    rec["v"] = tri
    with open(path, "wb") as fh:
        fh.write(b"\0" * 80 + np.uint32(len(f)).tobytes() + rec.tobytes())


def test_facade_warns_and_measures_a_holed_stl(holed_batch, tmp_path):
    from shoulder_amd.bone import Humerus
    meshes, holed = holed_batch
    v, f0 = meshes[0]
    # the holes whose vertices all appear in an earlier face: the STL reader numbers vertices by first appearance, so the holed
    # file keeps the fixture's numbering (and with it every edge key)
    first = np.full(len(v), len(f0))
    np.minimum.at(first, f0.ravel(), np.repeat(np.arange(len(f0)), 3))
    h = np.array([i for i in holed[0][2] if first[f0[i]].max() < i])
    assert len(h) > 0
    f = np.delete(f0, h, axis=0)
    p = tmp_path / "holed_left.stl"
    _write_stl(p, v, f)
    assert np.array_equal(load_stl(p)[1], f)
    with engine_with_env() as e:
        intact = Humerus(os.path.join(BONES, "humerus_left.stl"), engine=e)
        with pytest.warns(UserWarning, match="is not watertight"):
            bone = Humerus(p, engine=e, open_contours="bridge", max_gap=GAP)
        assert bone.canal.axis().tobytes() == intact.canal.axis().tobytes()
        assert bone.anatomic_neck.axis_normal().tobytes() == intact.anatomic_neck.axis_normal().tobytes()
        assert bone.bicipital_groove.axis().tobytes() == intact.bicipital_groove.axis().tobytes()
        assert bone.trans_epiconylar.axis().tobytes() == intact.trans_epiconylar.axis().tobytes()
        assert bone.neckshaft() == intact.neckshaft() and bone.retroversion() == intact.retroversion()
        assert e.get_open_contours()[0] == "error"      # (the intact bone ran last, with its own setting)
