"""CPU tests of tests/clique_communities_ref.py, the restatement the GPU tests compare komb_clique_communities_* with: against
networkx.k_clique_communities on 240 random graphs of 4 .. 18 vertices at k in {2 .. 6}, against the literal definition (all
k-cliques, joined through shared (k - 1)-cliques) on graphs of at most 10 vertices, on the nesting between k and k + 1, on the
k = 3 identity with the triangle-connected edge classes, and on the hand values of the pivot rule's pair_tests."""
import itertools
import random

import numpy as np
import pytest

import clique_communities_ref as C
import maximal_cliques_ref as M
import truss_communities_ref as T

KS = (2, 3, 4, 5, 6)


def _random_graph(seed, lo=4, hi=18):
    rng = random.Random(seed)
    nv = rng.randint(lo, hi)
    p = rng.choice([0.15, 0.3, 0.5, 0.7, 0.85])
    return nv, [(u, v) for u in range(nv) for v in range(u + 1, nv) if rng.random() < p]


def _cliques(nv, edges):
    return M.solve_edges(nv, edges)["cliques"]


def _identities(res, nv, cliques):
    n = res["n_communities"]
    assert len(res["rep"]) == len(res["n_cliques"]) == n == len(res["offset"]) - 1 and int(res["offset"][-1]) == len(res["verts"])
    assert res["rep"].tolist() == sorted(set(res["label"][res["label"] >= 0].tolist()))
    assert int(res["n_cliques"].sum()) == res["n_member_cliques"] == int((res["label"] >= 0).sum())
    for c in range(n):
        vs = res["verts"][res["offset"][c]:res["offset"][c + 1]].tolist()
        assert vs == sorted(set(vs)) == list(res["communities"][c])
        assert int(res["label"][res["rep"][c]]) == int(res["rep"][c])
    assert int(res["n_comm"].sum()) == len(res["verts"])
    assert res["first"].tolist() == [min([c for c in range(n) if v in res["communities"][c]], default=-1) for v in range(nv)]
    assert ((res["label"] < 0) == np.asarray([len(c) < res["k"] for c in cliques], bool)).all()


@pytest.mark.parametrize("block", range(12))
def test_random_graphs_against_networkx(block):
    import networkx as nx
    from networkx.algorithms.community import k_clique_communities
    for seed in range(20 * block, 20 * block + 20):
        nv, edges = _random_graph(seed)
        g = nx.Graph()
        g.add_nodes_from(range(nv))
        g.add_edges_from(edges)
        cliques = _cliques(nv, edges)
        for k in KS:
            want = sorted(tuple(sorted(c)) for c in k_clique_communities(g, k))
            res = C.solve(nv, cliques, k)
            assert C.vertex_sets(res) == want, (seed, k)
            assert res["n_comm"].tolist() == [sum(1 for c in want if v in c) for v in range(nv)]
            _identities(res, nv, cliques)


def _literal(nv, edges, k):
    """The definition: every k-clique, two joined when they share k - 1 vertices, the unions of the classes."""
    adj = {(u, v) for u, v in edges} | {(v, u) for u, v in edges}
    kc = [c for c in itertools.combinations(range(nv), k) if all((a, b) in adj for a, b in itertools.combinations(c, 2))]
    parent = list(range(len(kc)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a in range(len(kc)):
        for b in range(a + 1, len(kc)):
            if len(set(kc[a]) & set(kc[b])) == k - 1:
                parent[find(a)] = find(b)
    out = {}
    for a, c in enumerate(kc):
        out.setdefault(find(a), set()).update(c)
    return sorted(tuple(sorted(s)) for s in out.values())


@pytest.mark.parametrize("seed", range(30))
def test_small_graphs_against_the_literal_definition(seed):
    nv, edges = _random_graph(1000 + seed, 4, 10)
    cliques = _cliques(nv, edges)
    for k in KS:
        assert C.vertex_sets(C.solve(nv, cliques, k)) == _literal(nv, edges, k), (seed, k)


@pytest.mark.parametrize("seed", range(30))
def test_nesting_between_k_and_k_plus_1(seed):
    nv, edges = _random_graph(2000 + seed)
    cliques = _cliques(nv, edges)
    prev = None
    for k in (6, 5, 4, 3, 2):
        res = C.solve(nv, cliques, k)
        if prev is not None:
            for inner in prev["communities"]:                                    # every community of k + 1 lies inside one of k
                assert any(set(inner) <= set(outer) for outer in res["communities"]), (seed, k)
            assert res["n_covered"] >= prev["n_covered"]
        prev = res
    comps = C.solve(nv, cliques, 2)                                              # k = 2: the components of the non-isolated vertices
    import networkx as nx
    g = nx.Graph(edges)
    assert C.vertex_sets(comps) == sorted(tuple(sorted(c)) for c in nx.connected_components(g))
    assert comps["n_overlap"] == 0


@pytest.mark.parametrize("seed", range(30))
def test_k3_is_the_triangle_connected_edge_classes(seed):
    nv, edges = _random_graph(3000 + seed)
    e = sorted(edges)
    eu, ev = [u for u, _ in e], [v for _, v in e]
    tr = M.trussness(nv, eu, ev) if e else []
    label = T.communities(nv, eu, ev, tr, 3)
    sets = {}
    for u, v, l in zip(eu, ev, np.asarray(label).tolist()):
        if l >= 0:
            sets.setdefault(l, set()).update((u, v))
    assert C.vertex_sets(C.solve(nv, _cliques(nv, edges), 3)) == sorted(tuple(sorted(s)) for s in sets.values())


@pytest.mark.parametrize("name,k,n_comm,tests", C.HAND_TABLE, ids=["%s, k %d" % r[:2] for r in C.HAND_TABLE])
def test_hand_graphs(name, k, n_comm, tests):
    nv, edges = C.HAND_GRAPHS[name]
    cliques = _cliques(nv, edges)
    res = C.solve(nv, cliques, k)
    assert res["n_communities"] == n_comm and C.pair_tests(cliques, k) == tests
    _identities(res, nv, cliques)
    if name == "two K_4 sharing one vertex" and k == 3:
        assert res["n_comm"].tolist() == [1, 1, 1, 2, 1, 1, 1] and res["n_overlap"] == 1 and res["first"].tolist() == [0, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("m,k,tests", [(6, 3, 4960), (6, 6, 1984), (12, 3, 46114816), (12, 12, 8384512)])
def test_cocktail_party_pair_tests(m, k, tests):
    nv, edges = M.cocktail_party(m)
    cliques = sorted(tuple(2 * i + ((x >> i) & 1) for i in range(m)) for x in range(2 ** m))
    if m == 6:
        assert cliques == _cliques(nv, edges)
        res = C.solve(nv, cliques, k)
        assert res["n_communities"] == 1 and res["communities"] == [tuple(range(nv))] and res["size"].tolist() == [64] * 64
    assert C.pair_tests(cliques, k) == tests


def test_book_windmill_and_arguments():
    nv, edges = C.book(200)
    cliques = _cliques(nv, edges)
    res = C.solve(nv, cliques, 3)
    assert res["n_communities"] == 1 and res["largest"] == 202 and C.pair_tests(cliques, 3) == 19900
    assert C.solve(nv, cliques, 2)["n_communities"] == 1
    nv, edges = C.windmill(200)
    cliques = _cliques(nv, edges)
    res = C.solve(nv, cliques, 3)
    assert res["n_communities"] == 200 and int(res["n_comm"][0]) == 200 and C.pair_tests(cliques, 3) == 0 and res["n_overlap"] == 1
    assert C.solve(nv, cliques, 2)["n_communities"] == 1
    res = C.solve(5, [], 3)                                                      # nothing to percolate
    assert res["n_communities"] == 0 and res["offset"].tolist() == [0] and res["first"].tolist() == [-1] * 5 and res["largest"] == 0
    with pytest.raises(ValueError):
        C.solve(4, [(0, 1)], 1)
