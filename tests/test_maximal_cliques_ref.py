"""CPU tests of tests/maximal_cliques_ref.py, the restatement the GPU tests compare komb_maximal_cliques_* with: against
networkx.find_cliques on random graphs of 2 .. 22 vertices at k_min in {2, 3, 4, 6} and both pivot rules, against the closed
forms of K_n, the cocktail-party graphs and the complete 5-partite graph 3,3,3,3,3, and on the identities between the outputs."""
import random

import numpy as np
import pytest

import maximal_cliques_ref as M
import nucleus_ref as R

K_MIN = (2, 3, 4, 6)


def _by_networkx(nv, edges):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(nv))
    g.add_edges_from(edges)
    cliques = sorted(tuple(sorted(c)) for c in nx.find_cliques(g) if len(c) >= 2)
    t_max = 0
    if edges:
        t_max = 2
        while nx.k_truss(g, t_max + 1).number_of_edges():
            t_max += 1
    return cliques, t_max


def _random_graph(seed):
    rng = random.Random(seed)
    nv = rng.randint(2, 22)
    p = rng.choice([0.15, 0.3, 0.5, 0.7, 0.85])
    return nv, [(u, v) for u in range(nv) for v in range(u + 1, nv) if rng.random() < p]


def _identities(got, nv):
    sizes = np.arange(got["k_min"], got["k_hi"] + 1)
    assert int(got["count"].sum()) == int((sizes * got["hist"]).sum())
    assert got["n_cliques"] == int(got["hist"].sum()) == len(got["cliques"])
    largest = [0] * nv
    for c in got["cliques"]:
        for v in c:
            largest[v] = max(largest[v], len(c))
    assert got["largest"].tolist() == largest
    assert got["omega"] == max([int(k) for k, h in zip(sizes, got["hist"]) if h], default=0)


@pytest.mark.parametrize("seed", range(24))
def test_random_graphs_against_networkx(seed):
    nv, edges = _random_graph(seed)
    cliques, t_max = _by_networkx(nv, edges)
    for k_min in K_MIN:
        want = [c for c in cliques if len(c) >= k_min]
        for pivot in ("max", "first"):
            got = M.solve_edges(nv, edges, k_min=k_min, pivot=pivot)
            assert (got["k_min"], got["k_hi"], got["t_max"], got["flags"]) == (k_min, max(k_min, t_max), t_max, 3)
            assert got["cliques"] == want
            assert got["hist"].tolist() == [sum(1 for c in want if len(c) == k) for k in range(k_min, max(k_min, t_max) + 1)]
            assert got["count"].tolist() == [sum(1 for c in want if v in c) for v in range(nv)]
            _identities(got, nv)


def test_degenerate_graphs_and_arguments():
    for nv, edges in ((0, []), (5, [])):
        got = M.solve_edges(nv, edges)
        assert (got["k_hi"], got["t_max"], got["omega"], got["flags"], got["n_cliques"]) == (2, 0, 0, 3, 0)
        assert got["hist"].tolist() == [0] and got["count"].tolist() == [0] * nv and got["cliques"] == []
    got = M.solve_edges(6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)])             # a path: every edge is maximal
    assert got["hist"].tolist() == [5] and got["count"].tolist() == [1, 3, 2, 2, 1, 1] and got["largest"].tolist() == [2] * 6
    got = M.solve_edges(4, [(0, 1), (1, 3), (0, 3)])                             # a triangle: its edges are not
    assert got["cliques"] == [(0, 1, 3)] and got["hist"].tolist() == [0, 1] and got["largest"].tolist() == [3, 3, 0, 3]
    got = M.solve_edges(4, [(0, 1), (1, 3), (0, 3)], k_min=5)                    # k_min above t_max: one entry, zero
    assert (got["k_hi"], got["hist"].tolist(), got["omega"], got["flags"]) == (5, [0], 0, 3)
    with pytest.raises(ValueError):
        M.solve_edges(4, [(0, 1)], k_min=1)
    assert M.solve_edges(12, M.cocktail_party(6)[1], list_cap=10)["flags"] == M.COMPLETE


@pytest.mark.parametrize("n", [2, 3, 5, 12, 70])
def test_complete_graphs(n):
    edges = R.clique(range(n))
    got = M.solve(n, [u for u, _ in edges], [v for _, v in edges], truss=[n] * len(edges))
    assert got["cliques"] == [tuple(range(n))] and got["hist"].tolist() == [0] * (n - 2) + [1]
    assert got["count"].tolist() == [1] * n and got["largest"].tolist() == [n] * n and got["omega"] == n == got["t_max"]
    _identities(got, n)


@pytest.mark.parametrize("m", [3, 6, 12])
def test_cocktail_party(m):
    nv, edges = M.cocktail_party(m)
    for k_min in (2, m, m + 1):
        got = M.solve_edges(nv, edges, k_min=k_min)
        n = 2 ** m if k_min <= m else 0
        assert got["t_max"] == 2 * m - 2 and got["n_cliques"] == n
        assert got["hist"].tolist() == [n if k == m else 0 for k in range(k_min, max(k_min, 2 * m - 2) + 1)]
        assert got["count"].tolist() == [n // 2] * nv and got["largest"].tolist() == [m if n else 0] * nv
        _identities(got, nv)


def test_complete_five_partite():
    nv, edges = M.complete_multipartite([3] * 5)
    got = M.solve_edges(nv, edges)
    assert got["n_cliques"] == 243 and got["omega"] == 5 and int(got["hist"][5 - 2]) == 243
    assert got["count"].tolist() == [81] * 15
    assert all(sorted(v // 3 for v in c) == [0, 1, 2, 3, 4] for c in got["cliques"])
    _identities(got, nv)
