"""CPU tests of tests/max_clique_ref.py, the restatement the GPU tests compare komb_max_clique_* with: against
networkx.find_cliques (every maximal clique, which the restatement never lists) on the small graphs, against the table of the
suite's graphs, and on the cocktail-party graphs, whose numbers are known in closed form."""
import numpy as np
import pytest

import max_clique_ref as M
import nucleus_ref as R


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _canonical(uv):
    return R.canonical(np.asarray(uv).reshape(-1, 2).tolist())


def _by_networkx(nv, edges):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(nv))
    g.add_edges_from(edges)
    cliques = [tuple(sorted(c)) for c in nx.find_cliques(g) if len(c) >= 2]
    omega = max((len(c) for c in cliques), default=0)
    best = sorted(c for c in cliques if len(c) == omega)
    truss = 0
    if edges:
        k = 2
        while nx.k_truss(g, k + 1).number_of_edges():
            k += 1
        truss = k
    return omega, best, truss


def _check_against_networkx(nv, edges):
    got = M.solve_edges(nv, edges)
    omega, best, t_max = _by_networkx(nv, edges)
    assert got["flags"] == 7 and got["omega"] == got["upper"] == omega and got["t_max"] == t_max
    assert got["cliques"] == best and got["n_max_cliques"] == len(best)
    assert got["witness"] == (best[0] if best else ())
    count = np.zeros(nv, np.int32)
    for c in best:
        count[list(c)] += 1
    assert np.array_equal(got["count"], count)
    return got


def test_small_graphs_against_networkx(K, golden):
    _check_against_networkx(0, [])
    _check_against_networkx(5, [])
    _check_against_networkx(6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)])
    for g in golden:
        _check_against_networkx(len(g["rowptr"]) - 1, list(zip(g["eu"], g["ev"])))
        _check_against_networkx(len(g["rowptr"]) - 1, list(zip(g["sub_eu"], g["sub_ev"])))
    nv, edges = R.hand_graph()
    _check_against_networkx(nv, edges)
    _check_against_networkx(120, R.clique_union(120, 220, 2, 9, 1))
    _check_against_networkx(300, _canonical(K.gen_hug_edges(300, 735, 2.6, 6)))


TABLE = [("hand", None, 7, 1, 7, 7),
         ("cascade", None, 11, 1, 11, 15),
         ("hug", (300, 735, 2.6, 6), 9, 2, 10, 9),
         ("hug", (2000, 4900, 2.2, 11), 17, 8, 21, 17),
         ("hug", (3000, 7350, 2.2, 5), 18, 9, 27, 19),
         ("hug", (5000, 12250, 2.1, 7), 23, 14, 31, 26)]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s%s" % (r[0], r[1] or ""))
def test_table_of_the_suite_graphs(K, row):
    kind, args, omega, n_max, n_vertices, t_max = row
    if kind == "hand":
        nv, edges = R.hand_graph()
    elif kind == "cascade":
        nv, edges = 120, R.clique_union(120, 220, 2, 9, 1)
    else:
        nv, edges = args[0], _canonical(K.gen_hug_edges(*args))
    got = M.solve_edges(nv, edges)
    assert (got["flags"], got["omega"], got["upper"], got["n_max_cliques"], got["t_max"]) == (7, omega, omega, n_max, t_max)
    assert int(np.count_nonzero(got["count"])) == n_vertices and int(got["count"].sum()) == n_max * omega
    assert len(got["cliques"]) == n_max and got["witness"] == got["cliques"][0]
    if kind == "cascade":
        assert got["cliques"] == [(16, 24, 32, 51, 68, 71, 78, 96, 99, 105, 117)]
    adj = set(R.canonical(edges))
    for c in got["cliques"]:
        assert len(c) == omega and all((c[i], c[j]) in adj for i in range(omega) for j in range(i + 1, omega))


@pytest.mark.parametrize("m", [3, 6, 12])
def test_cocktail_party(m):
    nv, edges = M.cocktail_party(m)
    got = M.solve_edges(nv, edges)
    assert (got["flags"], got["omega"], got["upper"], got["t_max"], got["n_max_cliques"]) == (7, m, m, 2 * m - 2, 2 ** m)
    assert got["count"].tolist() == [2 ** (m - 1)] * nv
    assert got["cliques"][0] == tuple(range(0, 2 * m, 2)) and got["cliques"][-1] == tuple(range(1, 2 * m, 2))
    assert all(sorted(v // 2 for v in c) == list(range(m)) for c in got["cliques"])


def test_budget_and_list_cap():
    nv, edges = M.cocktail_party(12)
    full = M.solve_edges(nv, edges)
    capped = M.solve_edges(nv, edges, list_cap=1000)                          # the list is refused, the counts are not
    assert capped["flags"] == 3 and capped["cliques"] is None and capped["n_max_cliques"] == 4096
    assert np.array_equal(capped["count"], full["count"])
    cut = M.solve_edges(nv, edges, budget=full["nodes"] - 1)                  # out of nodes in the enumeration: omega stays proven
    assert cut["flags"] == 1 and cut["omega"] == cut["upper"] == 12 and cut["n_max_cliques"] == -1
    assert sorted(np.flatnonzero(cut["count"]).tolist()) == sorted(cut["witness"]) and int(cut["count"].sum()) == 12
    short = M.solve_edges(nv, edges, budget=3)                                # out of nodes in the search: a clique and a bound
    assert short["flags"] == 0 and 2 <= short["omega"] <= 12 <= short["upper"] == short["t_max"] == 22
    assert short["nodes"] <= 3 and len(set(short["witness"])) == short["omega"]
    adj = set(R.canonical(edges))
    assert all((u, v) in adj for i, u in enumerate(short["witness"]) for v in short["witness"][i + 1:])
    nothing = M.solve_edges(nv, edges, budget=0)
    assert nothing["flags"] == 0 and nothing["omega"] == 2 and nothing["witness"] == (0, 2)
