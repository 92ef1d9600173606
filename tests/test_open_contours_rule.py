"""CPU-only: the open-contour bridging rule (include/shoulder_hip.h sh_set_open_contours) restated in NumPy on
hand-made segment sets, and the argument checks of the Python API that need no device."""
import numpy as np
import pytest

from shoulder_amd import _lib


def bridge_loops(skey, ekey, ps, pe, max_gap):
    """The rule, step by step.  skey / ekey: start / end edge key of every segment ((lo, hi) tuples, compared as lo << 32 | hi),
    ps / pe: their crossing points (n x 2).  Returns (loops, bridged, dropped): every loop as (start key, vertices in walk order
    from the minimum start key), in ascending start-key order; chains closed by bridges; chains dropped."""
    n = len(skey)
    by_start = {k: i for i, k in enumerate(skey)}
    nxt = [by_start.get(ekey[i], -1) for i in range(n)]
    has_pred = set(j for j in nxt if j >= 0)
    tails = [i for i in range(n) if nxt[i] < 0]
    heads = [i for i in range(n) if i not in has_pred]
    cands = []
    for t in tails:
        for h in heads:
            dx, dy = pe[t][0] - ps[h][0], pe[t][1] - ps[h][1]
            d = np.sqrt(dx * dx + dy * dy)
            if d <= max_gap:
                cands.append((d, ekey[t], skey[h], t, h))
    cands.sort()
    key, pt = list(skey), [tuple(p) for p in ps]
    used_t, used_h = set(), set()
    for d, _, _, t, h in cands:
        if t in used_t or h in used_h:
            continue
        used_t.add(t); used_h.add(h)
        v = len(key)
        key.append(ekey[t]); pt.append(tuple(pe[t])); nxt.append(h)
        nxt[t] = v
    m = len(key)
    state = [0] * m      # 0 unseen, 1 on the current walk, 2 done
    on_loop = [False] * m
    loops = []
    for s in range(m):
        if state[s]:
            continue
        path, i = [], s
        while i >= 0 and state[i] == 0:
            state[i] = 1; path.append(i); i = nxt[i]
        if i >= 0 and state[i] == 1:      # a cycle closes on this walk
            cyc = path[path.index(i):]
            if len(cyc) >= 3:
                r = min(range(len(cyc)), key=lambda q: key[cyc[q]])
                cyc = cyc[r:] + cyc[:r]
                for q in cyc:
                    on_loop[q] = True
                loops.append((key[cyc[0]], np.array([pt[q] for q in cyc])))
        for q in path:
            state[q] = 2
    loops.sort(key=lambda lp: lp[0])
    bridged = sum(1 for t in tails if nxt[t] >= n and on_loop[t])
    dropped = sum(1 for t in tails if not on_loop[t])
    return loops, bridged, dropped


def _ring(n_pts, r=10.0, phase=0.0):
    a = phase + np.linspace(0, 2 * np.pi, n_pts, endpoint=False)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def _segments(pts, keys):
    """A closed ring as segments: segment i runs from the crossing on edge keys[i] to the one on keys[i + 1]."""
    n = len(pts)
    return list(keys), [keys[(i + 1) % n] for i in range(n)], pts, np.roll(pts, -1, axis=0)


def _drop(sk, ek, ps, pe, idx):
    keep = [i for i in range(len(sk)) if i not in set(idx)]
    return [sk[i] for i in keep], [ek[i] for i in keep], ps[keep], pe[keep]


def test_single_gap_rebuilds_the_ring_exactly():
    pts = _ring(12)
    keys = [(10 + i, 500 + i) for i in range(12)]
    full, _, _ = bridge_loops(*_segments(pts, keys), max_gap=0.0)
    holed = _drop(*_segments(pts, keys), [5])
    loops, bridged, dropped = bridge_loops(*holed, max_gap=6.0)
    assert (bridged, dropped) == (1, 0) and len(loops) == 1
    assert loops[0][0] == full[0][0] and np.array_equal(loops[0][1], full[0][1])
    # the gap is one edge of the 12-gon (5.18): smaller max_gap, nothing bridged, the chain is dropped
    loops, bridged, dropped = bridge_loops(*holed, max_gap=5.0)
    assert loops == [] and (bridged, dropped) == (0, 1)


def test_two_crossed_gaps_pair_by_distance():
    """Two rings side by side, each with one gap, ends placed so that the nearest head of each tail is on the OTHER ring:
    the greedy rule bridges across, one loop through both chains."""
    a = [(-5.0, 0.0), (-5.0, 5.0), (-10.0, 5.0), (-10.0, -5.0), (-5.0, -5.0)]       # chain A: head at (-5, 0) ... tail ends at (-5, -1)
    b = [(5.0, -1.0), (5.0, -5.0), (10.0, -5.0), (10.0, 5.0), (5.0, 5.0)]
    ska = [(1, 100 + i) for i in range(5)]
    skb = [(2, 200 + i) for i in range(5)]
    sk = ska + skb
    ek = ska[1:] + [(9, 1)] + skb[1:] + [(9, 2)]           # tail ends: (9, 1) and (9, 2), keys no head has
    ps = np.array(a + b)
    pe = np.array(a[1:] + [(5.0 - 0.5, -1.0)] + b[1:] + [(-5.0 + 0.5, 0.0)])   # A's tail ends next to B's head, and back
    loops, bridged, dropped = bridge_loops(sk, ek, ps, pe, max_gap=1.0)
    assert (bridged, dropped) == (2, 0) and len(loops) == 1 and len(loops[0][1]) == 12
    assert loops[0][0] == (1, 100)


def test_tie_is_broken_by_the_tail_key_then_the_head_key():
    """Two tails at the same distance from one head: the smaller end key wins; the other chain is dropped."""
    sk = [(1, 10), (1, 11), (1, 12), (2, 20), (2, 21), (2, 22)]
    ek = [(1, 11), (1, 12), (7, 0), (2, 21), (2, 22), (7, 1)]      # chain A: 0-1-2, tail end (7, 0); chain B: 3-4-5, tail end (7, 1)
    ps = np.array([[0, 0], [1, 0], [1, 1], [5, 5], [6, 5], [6, 6]], float)
    pe = np.array([[1, 0], [1, 1], [0, 1], [6, 5], [6, 6], [0, -1]], float)      # both tails end 1 away from A's head (0, 0)
    loops, bridged, dropped = bridge_loops(sk, ek, ps, pe, max_gap=1.0)
    # (d, end key): tail of A (7, 0) < tail of B (7, 1) -> A closes on itself; B's head (5, 5) is too far from anything left
    assert (bridged, dropped) == (1, 1) and len(loops) == 1 and loops[0][0] == (1, 10) and len(loops[0][1]) == 4


def test_unpaired_chain_is_dropped_and_closed_loops_stay():
    pts = _ring(8)
    keys = [(30 + i, 900 + i) for i in range(8)]
    sk, ek, ps, pe = _segments(pts, keys)
    sk, ek = sk + [(3, 4), (3, 5)], ek + [(3, 5), (3, 6)]      # an open two-segment chain far from everything
    ps = np.vstack([ps, [[100.0, 100.0], [101.0, 100.0]]])
    pe = np.vstack([pe, [[101.0, 100.0], [102.0, 100.0]]])
    loops, bridged, dropped = bridge_loops(sk, ek, ps, pe, max_gap=1.5)      # (its gap: 2)
    assert (bridged, dropped) == (0, 1) and len(loops) == 1 and len(loops[0][1]) == 8
    # a gap that closes the chain on itself makes a cycle of 3 (two segments + the bridge): a loop of its own
    loops, bridged, dropped = bridge_loops(sk, ek, ps, pe, max_gap=2.5)
    assert (bridged, dropped) == (1, 0) and len(loops) == 2


def test_max_gap_zero_is_the_oracle_drop_rule():
    pts = _ring(10)
    keys = [(50 + i, 700 + i) for i in range(10)]
    holed = _drop(*_segments(pts, keys), [3])
    loops, bridged, dropped = bridge_loops(*holed, max_gap=0.0)
    assert loops == [] and (bridged, dropped) == (0, 1)


def test_python_api_checks_its_arguments_without_a_gpu():
    from shoulder_amd.engine import Engine
    e = Engine.__new__(Engine)      # (no context: the checks come first)
    for bad in [dict(mode="close"), dict(mode="bridge", max_gap=-1.0), dict(mode="bridge", max_gap=float("nan")),
                dict(mode="bridge", max_gap=float("inf"))]:
        with pytest.raises(ValueError):
            e.set_open_contours(**bad)
    from shoulder_amd.bone import ProximalHumerus
    with pytest.raises(ValueError):
        ProximalHumerus("nothing.stl", engine=object(), open_contours="close")
    with pytest.raises(ValueError):
        ProximalHumerus("nothing.stl", engine=object(), open_contours="bridge", max_gap=-2)


def test_c_abi_checks_its_arguments_without_a_gpu():
    L = _lib.load()
    assert L.sh_set_open_contours(None, 1, 1.0) == -1
    assert L.sh_get_open_contours(None, None, None) == -1
    assert L.sh_open_contour_stats(None, None, None) == -1
    assert L.sh_mesh_open_edges(None, None) == -1
    assert _lib.OPEN_ERROR == 0 and _lib.OPEN_BRIDGE == 1
