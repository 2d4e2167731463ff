"""CPU tests of tests/nucleus_ref.py, the restatement the GPU tests of komb_nucleus_run compare with: against a brute force
taken from the definition (for every k the greatest fixed point of "drop every triangle with fewer than k 4-cliques inside
the family", recomputed from adjacency sets each pass -- no incidence lists, no decrements), on the graphs worked out by hand,
and through the invariants of the outputs."""
import itertools
from collections import Counter

import numpy as np
import pytest

import nucleus_ref as R


def brute_theta(nv, edges):
    """{(a, b, c): theta} from the definition alone."""
    adj = [set() for _ in range(nv)]
    for u, v in edges:
        adj[u].add(v); adj[v].add(u)
    tris = [t for t in itertools.combinations(range(nv), 3) if t[1] in adj[t[0]] and t[2] in adj[t[0]] and t[2] in adj[t[1]]]
    theta = {t: 0 for t in tris}
    family, k = set(tris), 1
    while family:
        while True:                                       # the greatest fixed point for this k, inside the one for k - 1
            keep = set()
            for t in family:
                a, b, c = t
                inside = 0
                for d in adj[a] & adj[b] & adj[c]:
                    others = [tuple(sorted((a, b, d))), tuple(sorted((a, c, d))), tuple(sorted((b, c, d)))]
                    inside += all(o in family for o in others)
                if inside >= k:
                    keep.add(t)
            if keep == family:
                break
            family = keep
        for t in family:
            theta[t] = k
        k += 1
    return theta


def random_graphs():
    rng = np.random.default_rng(20)
    out = []
    for nv in range(4, 11):
        for p in (0.35, 0.6, 0.8, 0.95):
            for _ in range(3):
                pairs = [e for e in itertools.combinations(range(nv), 2) if rng.random() < p]
                out.append((nv, pairs))
    return out


GRAPHS = random_graphs()


def test_enough_random_graphs():
    assert len(GRAPHS) >= 60
    assert {nv for nv, _ in GRAPHS} == set(range(4, 11))


@pytest.mark.parametrize("i", range(len(GRAPHS)))
def test_restatement_against_the_definition(i):
    nv, edges = GRAPHS[i]
    got = R.decompose_edges(nv, edges)
    want = brute_theta(nv, edges)
    tris = list(zip(got["a"].tolist(), got["b"].tolist(), got["c"].tolist()))
    assert tris == sorted(want)                           # every triangle, in (a, b, c) order
    assert got["theta"].tolist() == [want[t] for t in tris]
    adj = [set() for _ in range(nv)]
    for u, v in edges:
        adj[u].add(v); adj[v].add(u)
    assert got["key0"].tolist() == [len(adj[a] & adj[b] & adj[c]) for a, b, c in tris]
    assert got["info"]["n_cliques4"] * 4 == int(got["key0"].sum())


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, nv, edges, n_tri, n_clq, counts = case
    got = R.decompose_edges(nv, edges)
    assert got["info"]["n_triangles"] == n_tri and got["info"]["n_cliques4"] == n_clq
    assert dict(Counter(got["theta"].tolist())) == counts
    assert got["levels"] == sorted(counts) and got["info"]["n_levels"] == len(counts)
    assert got["info"]["theta_max"] == max(counts)
    if nv <= 9:
        want = brute_theta(nv, edges)
        assert got["theta"].tolist() == [want[t] for t in sorted(want)]


def test_shared_triangle_and_hand_graph():
    got = R.decompose_edges(7, R.clique([0, 1, 2, 3, 4]) + R.clique([0, 1, 2, 5, 6]))
    assert (got["a"][0], got["b"][0], got["c"][0], got["key0"][0]) == (0, 1, 2, 4)
    nv, edges = R.hand_graph()
    got = R.decompose_edges(nv, edges)
    assert got["levels"] == [0, 1, 2, 4]                  # the lone triangle, the K_4, the K_5, the K_7
    assert got["vertex_theta"].tolist() == [4, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1, 0, 0]


def test_empty_inputs():
    for nv, edges in ((0, []), (5, []), (4, [(0, 1), (1, 2), (2, 3)])):
        got = R.decompose_edges(nv, edges)
        assert got["info"] == {"n_triangles": 0, "n_cliques4": 0, "theta_max": -1, "n_levels": 0}
        assert got["levels"] == [] and got["subrounds"] == []
        assert got["edge_theta"].tolist() == [-1] * len(edges) and got["vertex_theta"].tolist() == [-1] * nv
        assert all(got[k].dtype == np.int32 and len(got[k]) == 0 for k in ("a", "b", "c", "key0", "theta"))


@pytest.mark.parametrize("i", range(0, len(GRAPHS), 3))
def test_invariants_and_relabelling(i):
    nv, edges = GRAPHS[i]
    got = R.decompose_edges(nv, edges)
    th, key0 = got["theta"], got["key0"]
    assert np.all(th <= key0) and np.all(th >= 0)
    assert len(got["subrounds"]) == len(got["levels"]) and all(r >= 1 for r in got["subrounds"])
    assert got["levels"] == sorted(set(th.tolist()))
    can = R.canonical(edges)
    for j, (u, v) in enumerate(can):                      # the maxima, from the triangle list alone
        on = [int(t) for t, a, b, c in zip(th, got["a"], got["b"], got["c"]) if {u, v} <= {a, b, c}]
        assert got["edge_theta"][j] == (max(on) if on else -1)
    for v in range(nv):
        on = [int(t) for t, a, b, c in zip(th, got["a"], got["b"], got["c"]) if v in (a, b, c)]
        assert got["vertex_theta"][v] == (max(on) if on else -1)
    rng = np.random.default_rng(i)
    for _ in range(2):                                    # theta is a property of the graph, not of the labels
        perm = rng.permutation(nv)
        other = R.decompose_edges(nv, [(int(perm[u]), int(perm[v])) for u, v in edges])
        assert sorted(other["theta"].tolist()) == sorted(th.tolist())
        assert sorted(other["key0"].tolist()) == sorted(key0.tolist())
        assert other["vertex_theta"][perm].tolist() == got["vertex_theta"].tolist()
