"""CPU tests of tests/nucleus_hierarchy_ref.py, the reference the GPU tests of komb_nucleus_hierarchy_run compare with:
entry for entry on the graphs worked out by hand, through the walk-up rule against a brute force that shares nothing with it
(4-cliques from vertex 4-subsets, theta from test_nucleus_ref's fixed point, the k-nuclei of every k by plain BFS), and
through the invariants of the forest."""
import itertools
from collections import deque

import numpy as np
import pytest

import nucleus_hierarchy_ref as R
import nucleus_ref as N
from test_nucleus_ref import brute_theta, random_graphs


def _nodes(h):
    return [tuple(int(h[f][i]) for f in R.FIELDS) for i in range(len(h["k"]))]


def test_k4_and_shared_triangle_and_shared_edge():
    h, dec = R.hierarchy_edges(4, N.clique(range(4)))
    assert _nodes(h) == [(1, 0, -1, 4, 4)] and h["node"].tolist() == [0] * 4
    h, dec = R.hierarchy_edges(7, N.clique([0, 1, 2, 3, 4]) + N.clique([0, 1, 2, 5, 6]))
    assert _nodes(h) == [(2, 0, -1, 19, 19)]
    h, dec = R.hierarchy_edges(*R.two_k5_sharing_an_edge())             # theta cannot tell these two apart: the forest does
    assert dec["theta"].tolist() == [2] * 20
    assert _nodes(h) == [(2, 0, -1, 10, 10), (2, 3, -1, 10, 10)]
    assert R.info(h, dec["theta"]) == (2, 2, 2, 1, 20)
    got = R.nuclei(h, dec, 2)
    assert [got[f].tolist() for f in R.NUCLEI_FIELDS] == [[0, 3], [10, 10], [10, 10], [5, 5]]


def test_clique_weight_decides():
    """The two graphs that come out wrong when a clique links at the level of its triangles' largest theta."""
    h, dec = R.hierarchy_edges(*R.k6_plus_vertex())
    assert _nodes(h) == [(1, 0, -1, 23, 3), (3, 0, 0, 20, 20)]
    h, dec = R.hierarchy_edges(*R.two_k6_joined_by_a_band())
    assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (48, 33)
    nodes = _nodes(h)
    assert len(nodes) == 3 and nodes[0][0] == 1 and nodes[0][2] == -1 and nodes[0][3:] == (48, 8)
    assert [(n[0], n[2], n[3], n[4]) for n in nodes[1:]] == [(3, 0, 20, 20)] * 2
    assert R.info(h, dec["theta"])[:2] == (3, 1)


def test_hand_graph():
    nv, edges = N.hand_graph()
    h, dec = R.hierarchy_edges(nv, edges)
    assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (50, 41)
    assert [(n[0], n[1], n[2], n[3]) for n in _nodes(h)] == [(1, 45, -1, 4), (2, 35, -1, 10), (4, 0, -1, 35)]
    assert h["node"][-1] == -1 and (h["node"][:-1] >= 0).all()
    assert R.info(h, dec["theta"]) == (3, 3, 4, 1, 49)


def test_chains_bands_and_many_roots():
    h, dec = R.hierarchy_edges(*R.clique_chain(9))
    assert h["size"].tolist() == [204, 201, 192, 173, 139, 84] and h["k"].tolist() == [1, 2, 3, 4, 5, 6]
    assert h["parent"].tolist() == [-1, 0, 1, 2, 3, 4] and R.info(h, dec["theta"])[3] == 6
    h, dec = R.hierarchy_edges(*R.band(2000))
    assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (5992, 1997)
    assert _nodes(h) == [(1, 0, -1, 5992, 5992)]                         # every triangle lies in a K_4 on four consecutive vertices
    h, dec = R.hierarchy_edges(*R.disjoint_k4(50))
    assert _nodes(h) == [(1, 4 * i, -1, 4, 4) for i in range(50)]
    h, dec = R.hierarchy_edges(40, N.clique(range(40)))
    assert dec["info"]["n_cliques4"] == 91390 and _nodes(h) == [(37, 0, -1, 9880, 9880)]
    nv, edges = R.triangle_in_n_cliques(65)
    h, dec = R.hierarchy_edges(nv, edges)
    assert dec["key0"][0] == 65 and _nodes(h) == [(1, 0, -1, 1 + 3 * 65, 1 + 3 * 65)]


def test_clique_union():
    edges = N.clique_union(600, 150, 4, 12, 11)
    h, dec = R.hierarchy_edges(600, edges)
    assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (14223, 25839)
    assert R.info(h, dec["theta"])[:2] == (161, 79) and R.info(h, dec["theta"])[3] == 4
    R.check_invariants(h, dec["theta"])


def test_no_members():
    for nv, edges in ((0, []), (5, []), (4, [(0, 1), (1, 2), (2, 3)]), (4, [(0, 1), (1, 3), (0, 3)])):
        h, dec = R.hierarchy_edges(nv, edges)
        nt = dec["info"]["n_triangles"]
        assert _nodes(h) == [] and h["node"].tolist() == [-1] * nt
        assert R.info(h, dec["theta"]) == (0, 0, 0 if nt else -1, 0, 0)
        for k in (-1, 0, 1, 2):
            label, size = R.walk_up(h, dec["theta"], k)
            assert label.tolist() == [-1] * nt and size.tolist() == [0] * nt
            assert all(len(v) == 0 for v in R.nuclei(h, dec, k).values())


# ---- the brute force

def brute_nuclei(nv, edges):
    """(triangles in (a, b, c) order, theta, {k: label[]}) from the definition alone: label = the smallest triangle index of
    the class under "in a common 4-clique whose four triangles all have theta >= k", -1 where theta < k."""
    theta = brute_theta(nv, edges)
    tris = sorted(theta)
    tid = {t: i for i, t in enumerate(tris)}
    es = {frozenset(e) for e in edges}
    cliques = []
    for quad in itertools.combinations(range(nv), 4):
        if all(frozenset(p) in es for p in itertools.combinations(quad, 2)):
            cliques.append([tid[t] for t in itertools.combinations(quad, 3)])
    th = [theta[t] for t in tris]
    labels = {}
    for k in range(1, max(th, default=0) + 2):
        nb = [[] for _ in tris]
        for q in cliques:
            if min(th[t] for t in q) >= k:
                for t in q:
                    nb[t] += q
        lab = [-1] * len(tris)
        for s in range(len(tris)):
            if th[s] < k or lab[s] >= 0:
                continue
            lab[s] = s
            todo = deque([s])
            while todo:
                for u in nb[todo.popleft()]:
                    if lab[u] < 0:
                        lab[u] = s
                        todo.append(u)
        labels[k] = lab
    return tris, th, labels


GRAPHS = random_graphs()


@pytest.mark.parametrize("i", range(len(GRAPHS)))
def test_walk_up_against_the_definition(i):
    nv, edges = GRAPHS[i]
    h, dec = R.hierarchy_edges(nv, edges)
    tris, th, labels = brute_nuclei(nv, edges)
    assert list(zip(dec["a"].tolist(), dec["b"].tolist(), dec["c"].tolist())) == tris and dec["theta"].tolist() == th
    R.check_invariants(h, dec["theta"])
    for k, lab in labels.items():
        label, size = R.walk_up(h, dec["theta"], k)
        assert label.tolist() == lab, k
        assert size.tolist() == [lab.count(x) if x >= 0 else 0 for x in lab], k
        got = R.nuclei(h, dec, k)
        assert got["rep"].tolist() == sorted(set(x for x in lab if x >= 0))
        for r, nt, ne, nvx in zip(*(got[f].tolist() for f in R.NUCLEI_FIELDS)):
            mine = [tris[t] for t in range(len(tris)) if lab[t] == r]
            assert nt == len(mine)
            assert nvx == len({v for t in mine for v in t})
            assert ne == len({p for t in mine for p in itertools.combinations(t, 2)})
    # every node is a class of its level that is no class of the next one
    for j in range(len(h["k"])):
        k, r = int(h["k"][j]), int(h["rep"][j])
        members = {t for t, x in enumerate(labels[k]) if x == r}
        assert members and len(members) == int(h["size"][j])
        assert members != {t for t, x in enumerate(labels[k + 1]) if x == labels[k + 1][r] and x >= 0}
    top = max(th, default=0)
    assert np.array_equal(R.walk_up(h, dec["theta"], -1)[0], R.walk_up(h, dec["theta"], max(top, 1))[0])
    assert np.array_equal(R.walk_up(h, dec["theta"], 0)[0], R.walk_up(h, dec["theta"], 1)[0])
