"""CPU tests of tests/betweenness_ref.py, the reference the GPU results are compared with bit for bit: it agrees with networkx
(twice its undirected unnormalised betweenness, and its shortest-path lengths exactly), it gives the closed forms of a tree, a
star, a path and a cycle exactly, the stored fixture can tell a fused multiply-add and a different row order from the
definition, and the ROUNDED flag and the overflow appear where they must."""
import json
import os

import numpy as np
import pytest

import betweenness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "betweenness_fixture.json")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def load_fixture():
    with open(FIXTURE) as f:
        d = json.load(f)
    return d["nv"], np.asarray(d["pairs"], dtype=np.int64), np.asarray([int(h, 16) for h in d["bc_hex"]], dtype=np.uint64)


@pytest.mark.parametrize("seed", range(12))
def test_agrees_with_networkx(seed):
    """The error bound of these sums is of order n 2^-53, about 1e-14; 1e-9 only has to separate rounding from a wrong formula."""
    import networkx as nx
    rng = np.random.default_rng(seed)
    nv = 60
    pairs = rng.integers(0, nv, size=(150, 2))
    rows = R.adjacency(nv, pairs)
    G = nx.Graph()
    G.add_nodes_from(range(nv))
    G.add_edges_from((u, v) for u in range(nv) for v in rows[u] if u < v)
    want = nx.betweenness_centrality(G, normalized=False)
    got = R.betweenness(rows)
    worst = 0.0
    for v in range(nv):
        err = abs(got["bc"][v] - 2.0 * want[v]) / max(1.0, 2.0 * want[v])
        worst = max(worst, err)
        assert err <= 1e-9, (v, got["bc"][v], want[v])
    print("largest relative difference from networkx: %.3g" % worst)
    for i, s in enumerate(got["source"].tolist()):
        d = nx.single_source_shortest_path_length(G, s)
        assert got["n_reached"][i] == len(d) and got["sum_dist"][i] == sum(d.values()) and got["ecc"][i] == max(d.values())
    assert got["flags"] == 0 and got["n_sources"] == nv and got["n_batches"] == 1 and got["depth_max"] == int(got["ecc"].max())
    # a sample of sources in an order of its own, with a repeat: the sum of those sources' dependencies
    src = [5, 3, 3, 59]
    part = R.betweenness(rows, src)
    for v in range(nv):
        terms = [R.one_source(rows, s)[2][v] for s in src if s != v]
        assert abs(part["bc"][v] - sum(terms)) <= 1e-9 * max(1.0, sum(terms))
    assert part["source"].tolist() == src and part["n_reached"][1] == part["n_reached"][2]


def test_ternary_tree_has_integer_values():
    """In a tree sigma is 1 everywhere, so every delta is an integer: bc[v] = 2 x the pairs of other vertices v separates."""
    nv = 40
    pairs = [((v - 1) // 3, v) for v in range(1, nv)]
    rows = R.adjacency(nv, pairs)
    got = R.betweenness(rows)["bc"]
    size = [1] * nv
    for v in range(nv - 1, 0, -1):
        size[(v - 1) // 3] += size[v]
    for v in range(nv):
        parts = [size[c] for c in range(3 * v + 1, min(3 * v + 4, nv))] + ([nv - size[v]] if v else [])
        pairs_through = ((nv - 1) ** 2 - sum(p * p for p in parts)) // 2
        assert got[v] == float(2 * pairs_through) and got[v] == int(got[v])


def test_star_path_cycle_closed_forms():
    n = 30
    star = R.betweenness(R.adjacency(n, [(0, v) for v in range(1, n)]))
    assert star["bc"].tolist() == [float((n - 1) * (n - 2))] + [0.0] * (n - 1)
    assert star["ecc"].tolist() == [1] + [2] * (n - 1) and star["sum_dist"].tolist() == [n - 1] + [1 + 2 * (n - 2)] * (n - 1)
    path = R.betweenness(R.adjacency(n, [(v, v + 1) for v in range(n - 1)]))
    assert path["bc"].tolist() == [float(2 * v * (n - 1 - v)) for v in range(n)]
    assert path["depth_max"] == n - 1 and path["n_level_steps"] == n + (n - 2)
    for n in (9, 10):                                                        # odd: one shortest path per pair; even: two to the opposite vertex
        cyc = R.betweenness(R.adjacency(n, [(v, (v + 1) % n) for v in range(n)]))
        want = (n - 1) * (n - 3) / 4.0 if n % 2 else (n - 2) ** 2 / 4.0
        assert cyc["bc"].tolist() == [want] * n
        assert cyc["ecc"].tolist() == [n // 2] * n and cyc["n_reached"].tolist() == [n] * n


def test_degenerate_inputs():
    assert R.betweenness([])["bc"].shape == (0,) and R.betweenness([])["n_level_steps"] == 0
    one = R.betweenness([[]])
    assert one["bc"].tolist() == [0.0] and one["n_reached"].tolist() == [1] and one["ecc"].tolist() == [0] and one["n_level_steps"] == 1
    none = R.betweenness(R.adjacency(5, [(0, 1)]), [])
    assert none["bc"].tolist() == [0.0] * 5 and none["n_sources"] == 0 and none["n_batches"] == 0 and none["n_level_steps"] == 0
    rows = R.adjacency(6, [(0, 1), (1, 2), (3, 4)])                         # two components and an isolated vertex
    got = R.betweenness(rows, [5, 0, 3])
    assert got["n_reached"].tolist() == [1, 3, 2] and got["sum_dist"].tolist() == [0, 3, 1] and got["ecc"].tolist() == [0, 2, 1]
    assert got["bc"].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert got["n_level_steps"] == (2 + 1) + (2 - 1)


def test_the_bitwise_fixture_has_teeth():
    """GPU bit-equality on this graph proves something about contraction and order only because both change its result."""
    nv, pairs, stored = load_fixture()
    rows = R.adjacency(nv, pairs)
    plain = R.betweenness(rows)["bc"]
    assert np.array_equal(bits(plain), stored)                                # the stored patterns are the definition's
    fused = R.betweenness(rows, fused=True)["bc"]
    back = R.betweenness(rows, descending=True)["bc"]
    n_fused, n_back = int((bits(fused) != bits(plain)).sum()), int((bits(back) != bits(plain)).sum())
    print("fixture: %d vertices; fusion changes %d entries, descending rows %d" % (nv, n_fused, n_back))
    assert n_fused >= 1 and n_back >= 1
    assert n_fused >= 5                                                      # (several: the fixture was searched for)
    assert np.allclose(fused, plain, rtol=1e-12) and np.allclose(back, plain, rtol=1e-12)


def test_rounded_flag_on_the_diamond_chain():
    for k, flag in ((52, 0), (53, R.ROUNDED)):
        nv, pairs = R.diamond_chain(k)
        assert nv == 3 * k + 1
        got = R.betweenness(R.adjacency(nv, pairs), [0, nv - 1, nv // 2])
        assert got["flags"] == flag, k
        assert got["ecc"].tolist()[:2] == [2 * k, 2 * k]
        assert R.one_source(R.adjacency(nv, pairs), 0)[1][nv - 1] == 2.0 ** k


def test_overflow_of_the_layered_graph():
    nv, pairs = R.layered(256)
    assert nv == 4097
    got = R.betweenness(R.adjacency(nv, pairs), [0])
    assert got["flags"] == R.ROUNDED and got["ecc"].tolist() == [256] and np.isfinite(got["bc"]).all()
    nv, pairs = R.layered(257)
    assert nv == 4113 and len(pairs) == 65552
    rows = R.adjacency(nv, pairs)
    with pytest.raises(R.Limit):
        R.betweenness(rows, [0])
    assert R.one_source(rows, 1)[0][nv - 1] == 256 and R.betweenness(rows, [1])["ecc"].tolist() == [256]   # (layer 1 is under the limit)


def test_sample_sources():
    assert R.sample_sources(10, 10) == list(range(10)) and R.sample_sources(10, 99, 5) == list(range(10))
    a, b = R.sample_sources(1000, 7, 1), R.sample_sources(1000, 7, 2)
    assert len(a) == 7 and a == sorted(set(a)) and a != b
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF                              # the reference value of the generator's first output
