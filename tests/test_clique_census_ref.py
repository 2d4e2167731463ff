"""CPU tests of tests/clique_census_ref.py, the restatement the GPU tests compare komb_clique_census_* with: against
networkx.enumerate_all_cliques (every clique, one by one) on random graphs of at most 20 vertices, against the closed forms of
K_n and the cocktail-party graphs, on K_70, where the counts pass 2^64, and on the identity between the two outputs."""
import random
from math import comb

import numpy as np
import pytest

import clique_census_ref as C
import nucleus_ref as R

SAT = 2 ** 64 - 1


def _by_networkx(nv, edges, k_local):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(nv))
    g.add_edges_from(edges)
    total = {}
    local = [0] * nv
    for c in nx.enumerate_all_cliques(g):
        total[len(c)] = total.get(len(c), 0) + 1
        if len(c) == k_local:
            for v in c:
                local[v] += 1
    t_max = 0
    if edges:
        t_max = 2
        while nx.k_truss(g, t_max + 1).number_of_edges():
            t_max += 1
    return total, local, t_max


def _random_graph(seed):
    rng = random.Random(seed)
    nv = rng.randint(5, 20)
    p = rng.choice([0.3, 0.5, 0.7, 0.85])
    return nv, [(u, v) for u in range(nv) for v in range(u + 1, nv) if rng.random() < p]


@pytest.mark.parametrize("seed", range(16))
def test_random_graphs_against_networkx(seed):
    nv, edges = _random_graph(seed)
    by_k = {k_local: _by_networkx(nv, edges, k_local) for k_local in (0, 2, 3, 4, 5)}
    t_max = by_k[0][2]
    for k_lo in (2, 4):
        for k_hi in (-1, k_lo + 2):
            used = max(k_lo, t_max if k_hi == -1 else min(k_hi, t_max))
            for k_local in (0, k_lo, k_lo + 1):
                if k_local > used:                       # (a window that t_max cut short)
                    with pytest.raises(ValueError):
                        C.census_edges(nv, edges, k_lo=k_lo, k_hi=k_hi, k_local=k_local)
                    continue
                got = C.census_edges(nv, edges, k_lo=k_lo, k_hi=k_hi, k_local=k_local)
                total, local, _ = by_k[k_local]
                assert (got["t_max"], got["k_lo"], got["k_hi"], got["flags"]) == (t_max, k_lo, used, C.COMPLETE)
                assert got["total"].tolist() == [total.get(k, 0) for k in range(k_lo, used + 1)]
                assert got["omega"] == max([k for k in range(k_lo, used + 1) if total.get(k, 0)], default=0)
                if k_local:
                    assert got["local"].tolist() == local
                    assert sum(local) == k_local * total.get(k_local, 0)
                else:
                    assert got["local"] is None


def test_degenerate_graphs_and_arguments():
    for nv, edges in ((0, []), (5, [])):
        got = C.census_edges(nv, edges, k_lo=2, k_hi=-1, k_local=2)
        assert (got["k_hi"], got["t_max"], got["omega"], got["flags"]) == (2, 0, 0, 1)
        assert got["total"].tolist() == [0] and got["local"].tolist() == [0] * nv
    got = C.census_edges(6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)], k_local=2)
    assert got["total"].tolist() == [5] and got["local"].tolist() == [1, 3, 2, 2, 1, 1] and got["omega"] == 2
    got = C.census_edges(4, [(0, 1), (1, 3), (0, 3)], k_lo=4, k_hi=9)         # a window above t_max: zeros
    assert (got["k_hi"], got["total"].tolist(), got["omega"]) == (4, [0], 0)
    for bad in (dict(k_lo=1), dict(k_lo=3, k_hi=2), dict(k_local=-1), dict(k_lo=2, k_hi=3, k_local=4), dict(k_lo=3, k_local=2)):
        with pytest.raises(ValueError):
            C.census_edges(4, [(0, 1), (1, 3), (0, 3)], **bad)


@pytest.mark.parametrize("n", [2, 3, 5, 12, 40])
def test_complete_graphs(n):
    got = C.census_edges(n, R.clique(range(n)), k_local=max(n // 2, 2))
    assert got["t_max"] == n == got["omega"] == got["k_hi"]
    assert got["total"].tolist() == [comb(n, k) for k in range(2, n + 1)]
    assert got["local"].tolist() == [comb(n - 1, max(n // 2, 2) - 1)] * n


@pytest.mark.parametrize("m", [3, 6, 10, 12])
def test_cocktail_party(m):
    nv, edges = C.cocktail_party(m)
    got = C.census_edges(nv, edges, k_local=m)
    assert got["t_max"] == 2 * m - 2 == got["k_hi"] and got["omega"] == m
    assert got["total"].tolist() == [comb(m, k) * 2 ** k for k in range(2, 2 * m - 1)]
    assert got["local"].tolist() == [2 ** (m - 1)] * nv
    low = C.census_edges(nv, edges, k_lo=3, k_hi=5, k_local=3)
    assert low["total"].tolist() == [comb(m, k) * 2 ** k for k in range(3, min(5, 2 * m - 2) + 1)]
    assert int(low["local"].sum()) == 3 * comb(m, 3) * 8


def test_k70_saturates_in_the_middle():
    n = 70
    edges = R.clique(range(n))
    eu, ev = [u for u, _ in edges], [v for _, v in edges]
    got = C.census(n, eu, ev, k_local=35, truss=[n] * len(edges))
    assert got["flags"] == C.COMPLETE | C.SATURATED and got["omega"] == n
    assert got["total"].tolist() == [min(comb(n, k), SAT) for k in range(2, n + 1)]
    assert [k for k in range(2, n + 1) if got["total"][k - 2] == SAT] == list(range(28, 43))
    assert got["exact"][0] == [comb(n, k) for k in range(2, n + 1)]
    assert got["local"].tolist() == [min(comb(n - 1, 34), SAT)] * n and comb(n - 1, 34) > SAT
    assert sum(got["exact"][1]) == 35 * got["exact"][0][35 - 2]                 # the identity, before saturation
    low = C.census(n, eu, ev, k_lo=60, k_local=66, truss=[n] * len(edges))
    assert low["flags"] == C.COMPLETE and low["local"].tolist() == [comb(n - 1, 65)] * n
