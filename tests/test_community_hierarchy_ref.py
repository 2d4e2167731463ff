"""CPU tests of the community hierarchy reference (tests/community_hierarchy_ref.py): the two worked examples of the
definition entry for entry, and on the golden graphs, random graphs and hand cases its walk-up labels and sizes against
truss_communities_ref.brute_force for every k from 3 to k_max + 1, with the invariants of the forest."""
import numpy as np
import pytest

import community_hierarchy_ref as CH
import truss_communities_ref as R


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


EXAMPLE_A = (10, np.concatenate([clique(range(5)), [[5, 0], [5, 1]], clique([4, 6, 7, 8]), [[8, 9]]]),
             [5, 5, 5, 5, 3, 5, 5, 5, 3, 5, 5, 5, 4, 4, 4, 4, 4, 4, 2],
             {"k": [3, 4, 5], "rep": [0, 12, 0], "parent": [-1, -1, 0], "size": [12, 6, 10], "shell": [2, 6, 10],
              "node": [2, 2, 2, 2, 0, 2, 2, 2, 0, 2, 2, 2, 1, 1, 1, 1, 1, 1, -1]},
             (3, 2, 5, 2, 18))
EXAMPLE_B = (11, np.concatenate([clique(range(5)), clique(range(5, 10)), [[10, 0], [10, 1], [10, 5], [10, 6]], [[0, 5]]]),
             None,
             {"k": [3, 5, 5], "rep": [0, 0, 13], "parent": [-1, 0, 0], "size": [25, 10, 10], "shell": [5, 10, 10]},
             (3, 1, 5, 2, 25))


def _truss(O, nv, uv):
    rowptr, col = O.simplify(nv, np.asarray(uv, np.int64).reshape(-1, 2))
    eu, ev = O.edge_list(rowptr, col)
    return np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(O.trussness(rowptr, col), np.int64)


def _check(nv, eu, ev, tr, name):
    """The forest of the reference, checked through the walk-up rule against the brute force for every k."""
    eu, ev, tr = (np.asarray(x, np.int64) for x in (eu, ev, tr))
    h = CH.community_hierarchy(nv, eu, ev, tr)
    CH.check_invariants(h)
    assert np.array_equal(h["node"] >= 0, tr >= 3), name
    mem = h["node"] >= 0
    assert np.array_equal(h["k"][h["node"][mem]], tr[mem]), name
    tmax = int(tr.max()) if len(tr) else 2
    assert CH.info(h)[2] == max(tmax, 2), name
    for k in range(2, tmax + 2):
        want = R.brute_force(nv, eu, ev, tr, k)
        label, size = CH.walk_up(h, tr, k)
        assert np.array_equal(label, want), (name, k)
        assert np.array_equal(size, R.sizes(want)), (name, k)
    return h


def test_worked_examples(O):
    for nv, uv, want_tr, want, want_info in (EXAMPLE_A, EXAMPLE_B):
        eu, ev, tr = _truss(O, nv, uv)
        assert len(eu) == len(uv)
        if want_tr is not None:
            assert tr.tolist() == want_tr
        h = _check(nv, eu, ev, tr, "example")
        for f in want:
            assert h[f].tolist() == want[f], f
        assert CH.info(h) == want_info
    # no edges; edges but no triangle
    e = np.zeros(0, np.int64)
    assert CH.info(CH.community_hierarchy(3, e, e, e)) == (0, 0, 2, 0, 0)
    h = CH.community_hierarchy(4, [0, 1, 2], [1, 2, 3], [2, 2, 2])
    assert CH.info(h) == (0, 0, 2, 0, 0) and h["node"].tolist() == [-1] * 3
    assert CH.walk_up(h, [2, 2, 2], 2)[0].tolist() == [0, 1, 2] and CH.walk_up(h, [2, 2, 2], 3)[0].tolist() == [-1] * 3


def test_golden_graphs(golden):
    n = 0
    for g in golden:
        if g["nv"] > 400 or len(g["eu"]) > 6000:
            continue
        n += 1
        _check(g["nv"], g["eu"], g["ev"], g["trussness"], g["name"])
        _check(g["nv"], g["sub_eu"], g["sub_ev"], g["sub_trussness"], g["name"] + " maxcore")
    assert n >= 3


@pytest.mark.parametrize("seed", range(30))
def test_random_graphs(K, O, seed):
    rng = np.random.default_rng(2000 + seed)
    nv = int(rng.integers(5, 160))
    if seed % 3 == 0:
        uv = K.gen_hug_edges(nv, int(2.45 * nv), [2.1, 2.2, 2.6][seed % 9 // 3], seed)
    elif seed % 3 == 1:
        uv = rng.integers(0, nv, (int(nv * rng.uniform(1.0, 6.0)), 2))
    else:                                           # overlapping cliques: many communities sharing vertices
        parts = []
        for _ in range(int(rng.integers(2, 12))):
            mem = rng.choice(nv, int(rng.integers(3, min(9, nv))), replace=False)
            parts.append(mem[np.stack(np.triu_indices(len(mem), 1), 1)])
        uv = np.concatenate(parts)
    _check(nv, *_truss(O, nv, uv), seed)


def test_hand_cases(O):
    # bow-tie: two roots at level 3
    h = _check(5, *_truss(O, 5, [[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]]), "bow-tie")
    assert (h["k"].tolist(), h["rep"].tolist(), h["parent"].tolist(), h["size"].tolist()) == ([3, 3], [0, 3], [-1, -1], [3, 3])
    # two K5 sharing one vertex: two roots at 5, nothing below; sharing one edge: one node of 19 edges at 5
    h = _check(9, *_truss(O, 9, np.concatenate([clique(range(5)), clique(range(4, 9))])), "vertex")
    assert (h["k"].tolist(), h["parent"].tolist(), h["size"].tolist()) == ([5, 5], [-1, -1], [10, 10])
    h = _check(8, *_truss(O, 8, np.concatenate([clique(range(5)), clique(range(3, 8))])), "edge")
    assert (h["k"].tolist(), h["size"].tolist(), h["shell"].tolist()) == ([5], [19], [19])
    # two K6 joined by a strip of triangles: one node at 3 with two children at 6
    strip = [[12, 4], [12, 5], [5, 6], [12, 6], [12, 7]]      # 4-5-12, 5-12-6, 12-6-7: each shares an edge with the next
    h = _check(13, *_truss(O, 13, np.concatenate([clique(range(6)), clique(range(6, 12)), strip])), "strip")
    assert (h["k"].tolist(), h["parent"].tolist(), h["size"].tolist(), h["shell"].tolist()) == ([3, 6, 6], [-1, 0, 0], [35, 15, 15], [5, 15, 15])
    # the chain K3, K4, K5, K6, consecutive cliques sharing an edge: one node per level
    parts, off = [], 0
    for n in range(3, 7):
        parts.append(clique(range(off, off + n)))
        off += n - 2
    h = _check(off + 2, *_truss(O, off + 2, np.concatenate(parts)), "chain")
    assert (h["k"].tolist(), h["parent"].tolist()) == ([3, 4, 5, 6], [-1, 0, 1, 2]) and CH.info(h)[3] == 4
    # a book: one node of 601 edges; triangle-free: nothing
    pages = np.arange(2, 302)
    uv = np.concatenate([[[0, 1]], np.stack([np.zeros(300, np.int64), pages], 1), np.stack([np.ones(300, np.int64), pages], 1)])
    h = _check(302, *_truss(O, 302, uv), "book")
    assert {f: h[f].tolist() for f in CH.FIELDS} == {"k": [3], "rep": [0], "parent": [-1], "size": [601], "shell": [601]}
    idx = np.arange(20).reshape(4, 5)
    uv = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    assert CH.info(_check(20, *_truss(O, 20, uv), "grid")) == (0, 0, 2, 0, 0)
