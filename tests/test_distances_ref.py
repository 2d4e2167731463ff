"""CPU tests of tests/distances_ref.py, the reference the GPU results are compared with: it agrees with networkx (the shortest
path lengths exactly, harmonic centrality within rounding, the eccentricities per component), it gives the closed forms of a
path, a cycle, a star and a complete graph, its per-source integers are those of tests/betweenness_ref.py, and the stored
fixture can tell the defined order of the harmonic sum from two other orders."""
import numpy as np
import pytest

import betweenness_ref as B
import distances_ref as R

INFO = ("n_sources", "flags", "depth_max", "depth_min", "n_pairs", "sum_all", "n_batches", "n_level_steps")


def _graph(seed):
    """Sixty vertices, three groups that no edge joins and a few isolated vertices."""
    rng = np.random.default_rng(seed)
    pairs = np.concatenate([rng.integers(0, 30, size=(50, 2)), rng.integers(30, 48, size=(25, 2)), rng.integers(48, 56, size=(8, 2))])
    return 60, pairs


@pytest.mark.parametrize("seed", range(12))
def test_agrees_with_networkx(seed):
    """The harmonic sums have at most 60 terms: their rounding error is of order 60 x 2^-53, about 1e-14; 1e-9 only has to
    separate rounding from a wrong formula (the tolerance of test_betweenness_ref.py)."""
    import networkx as nx
    nv, pairs = _graph(seed)
    rows = R.adjacency(nv, pairs)
    G = nx.Graph()
    G.add_nodes_from(range(nv))
    G.add_edges_from((u, v) for u in range(nv) for v in rows[u] if u < v)
    assert nx.number_connected_components(G) > 3
    got = R.distances(rows)
    lengths = {s: nx.single_source_shortest_path_length(G, s) for s in range(nv)}
    per = got["sources"]
    for s in range(nv):
        d = lengths[s]
        assert per["n_reached"][s] == len(d) and per["sum_dist"][s] == sum(d.values()) and per["ecc"][s] == max(d.values())
    for name in ("n_reached", "sum_dist", "ecc"):                            # from every vertex the two views agree by symmetry
        assert np.array_equal(got[name], per[name]), name
    want = nx.harmonic_centrality(G)
    worst = 0.0
    for v in range(nv):
        err = abs(got["harmonic"][v] - want[v]) / max(1.0, want[v])
        worst = max(worst, err)
        assert err <= 1e-9, (v, got["harmonic"][v], want[v])
    print("largest relative difference from networkx.harmonic_centrality: %.3g" % worst)
    for comp in nx.connected_components(G):
        ecc = nx.eccentricity(G.subgraph(comp))
        for v in comp:
            assert got["ecc"][v] == ecc[v]
    counted = np.bincount([d for s in range(nv) for d in lengths[s].values()])
    assert np.array_equal(got["pairs"], counted)
    info = got["info"]
    assert info["flags"] == R.ALL and info["depth_max"] == len(counted) - 1 and info["depth_min"] == min(per["ecc"]) == 0
    assert info["n_pairs"] == counted.sum() and info["sum_all"] == sum(sum(lengths[s].values()) for s in range(nv))
    assert info["sum_all"] == 2 * sum(nx.wiener_index(G.subgraph(c)) for c in nx.connected_components(G))
    # a sample in an order of its own, with a repeat
    src = [5, 31, 31, 59, 0, 49]
    part = R.distances(rows, src)
    for v in range(nv):
        ds = [lengths[s][v] for s in src if v in lengths[s]]
        assert part["n_reached"][v] == len(ds) and part["sum_dist"][v] == sum(ds) and part["ecc"][v] == max(ds, default=-1)
        h = sum(1.0 / d for d in ds if d > 0)
        assert abs(part["harmonic"][v] - h) <= 1e-9 * max(1.0, h)
    assert part["info"]["flags"] == 0 and part["sources"]["source"].tolist() == src


def test_closed_forms():
    n = 30
    path = R.distances(R.adjacency(n, [(v, v + 1) for v in range(n - 1)]))
    assert path["ecc"].tolist() == [max(v, n - 1 - v) for v in range(n)]
    assert path["sum_dist"].tolist() == [v * (v + 1) // 2 + (n - 1 - v) * (n - v) // 2 for v in range(n)]
    assert path["pairs"].tolist() == [n] + [2 * (n - L) for L in range(1, n)]
    assert path["info"]["depth_max"] == n - 1 and path["info"]["depth_min"] == n // 2 and path["info"]["sum_all"] == (n - 1) * n * (n + 1) // 3
    assert path["info"]["n_batches"] == 1 and path["info"]["n_level_steps"] == n
    for n in (9, 10):
        cyc = R.distances(R.adjacency(n, [(v, (v + 1) % n) for v in range(n)]))
        assert cyc["ecc"].tolist() == [n // 2] * n and cyc["n_reached"].tolist() == [n] * n
        assert cyc["pairs"].tolist() == [n] + [2 * n] * ((n - 1) // 2) + ([n] if n % 2 == 0 else [])
        assert cyc["info"]["depth_min"] == n // 2
    n = 30
    star = R.distances(R.adjacency(n, [(0, v) for v in range(1, n)]))
    assert star["ecc"].tolist() == [1] + [2] * (n - 1) and star["sum_dist"].tolist() == [n - 1] + [1 + 2 * (n - 2)] * (n - 1)
    assert star["harmonic"].tolist() == [float(n - 1)] + [1.0 + (n - 2) / 2.0] * (n - 1)
    assert star["info"]["depth_min"] == 1 and star["info"]["depth_max"] == 2
    n = 12
    full = R.distances(R.adjacency(n, [(u, v) for u in range(n) for v in range(u)]))
    assert full["harmonic"].tolist() == [float(n - 1)] * n and full["pairs"].tolist() == [n, n * (n - 1)]
    assert full["ecc"].tolist() == [1] * n and full["info"]["sum_all"] == n * (n - 1)


def test_degenerate_inputs():
    none = R.distances([])
    assert none["pairs"].tolist() == [0] and none["harmonic"].shape == (0,)
    assert {k: none["info"][k] for k in INFO} == dict(zip(INFO, (0, R.ALL, 0, 0, 0, 0, 0, 0)))
    one = R.distances([[]])
    assert one["n_reached"].tolist() == [1] and one["sum_dist"].tolist() == [0] and one["ecc"].tolist() == [0]
    assert one["harmonic"].tolist() == [0.0] and one["pairs"].tolist() == [1] and one["info"]["n_level_steps"] == 1
    rows = R.adjacency(6, [(0, 1), (1, 2), (3, 4)])                         # two components and an isolated vertex
    got = R.distances(rows, [5, 0, 3, 0])
    assert got["n_reached"].tolist() == [2, 2, 2, 1, 1, 1] and got["sum_dist"].tolist() == [0, 2, 4, 0, 1, 0]
    assert got["ecc"].tolist() == [0, 1, 2, 0, 1, 0] and got["harmonic"].tolist() == [0.0, 2.0, 1.0, 0.0, 1.0, 0.0]
    assert got["sources"]["n_reached"].tolist() == [1, 3, 2, 3] and got["sources"]["ecc"].tolist() == [0, 2, 1, 2]
    assert got["pairs"].tolist() == [4, 3, 2] and got["info"]["depth_min"] == 0 and got["info"]["n_level_steps"] == 3
    alone = R.distances(rows, [5])
    assert alone["ecc"].tolist() == [-1] * 5 + [0] and alone["pairs"].tolist() == [1] and alone["info"]["depth_max"] == 0
    edgeless = R.distances([[] for _ in range(70)], words=1)
    assert edgeless["n_reached"].tolist() == [1] * 70 and edgeless["info"]["n_batches"] == 2 and edgeless["info"]["n_level_steps"] == 2
    empty = R.distances(rows, [])
    assert empty["ecc"].tolist() == [-1] * 6 and not empty["n_reached"].any() and not empty["harmonic"].any()
    assert empty["pairs"].tolist() == [0] and {k: empty["info"][k] for k in INFO} == dict(zip(INFO, (0, 0, 0, 0, 0, 0, 0, 0)))


@pytest.mark.parametrize("seed", range(3))
def test_per_source_integers_are_those_of_betweenness(seed):
    nv, pairs = _graph(seed)
    rows = R.adjacency(nv, pairs)
    assert rows == B.adjacency(nv, pairs)
    for sources in (None, [3, 58, 3, 40, 17], []):
        ours, theirs = R.distances(rows, sources), B.betweenness(rows, sources)
        for name in ("source", "n_reached", "sum_dist", "ecc"):
            assert ours["sources"][name].dtype == theirs[name].dtype and np.array_equal(ours["sources"][name], theirs[name]), name
        assert ours["info"]["depth_max"] == theirs["depth_max"] and ours["info"]["n_sources"] == theirs["n_sources"]


def test_batches_and_level_steps_follow_the_words():
    nv, pairs, sources, stored = R.load_fixture()
    rows = R.adjacency(nv, pairs)
    cache = {}
    base = R.distances(rows, sources, 1, cache=cache)
    assert base["info"]["n_batches"] == 5
    for words in (2, 4):
        other = R.distances(rows, sources, words, cache=cache)
        assert other["info"]["n_batches"] == -(-len(sources) // (64 * words))
        assert other["info"]["n_level_steps"] < base["info"]["n_level_steps"]
        assert np.array_equal(R.bits(other["harmonic"]), R.bits(base["harmonic"]))   # the value does not depend on the words


def test_the_order_fixture_has_teeth():
    """GPU bit-equality on this list proves something about the order of the sum only because other orders change it."""
    nv, pairs, sources, stored = R.load_fixture()
    made = R.make_fixture()
    assert nv == made[0] and np.array_equal(pairs, made[1]) and sources == made[2].tolist()   # the stored file is the seeded one
    assert len(sources) > 128
    rows = R.adjacency(nv, pairs)
    cache = {}
    plain = R.distances(rows, sources, cache=cache)["harmonic"]
    assert np.array_equal(R.bits(plain), stored)                              # the stored patterns are the definition's
    one_by_one = R.distances(rows, sources, order="per_source", cache=cache)["harmonic"]
    whole_batch = R.distances(rows, sources, order="batch256", cache=cache)["harmonic"]
    n_one, n_batch = int((R.bits(one_by_one) != R.bits(plain)).sum()), int((R.bits(whole_batch) != R.bits(plain)).sum())
    print("fixture: %d vertices, %d sources; adding 1/d per source changes %d entries, one sum per 256-source batch %d"
          % (nv, len(sources), n_one, n_batch))
    assert n_one >= 1 and n_batch >= 1
    assert np.allclose(one_by_one, plain, rtol=1e-12) and np.allclose(whole_batch, plain, rtol=1e-12)
