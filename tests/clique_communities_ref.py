"""Restatement of the k-clique communities of include/komb_accel.h (clique percolation) in plain Python.  It tests ALL pairs of
member cliques with Python sets and joins the adjacent ones with a small union-find of its own: it does not use the pigeonhole
rule by which the library finds the pairs.  It is fed a sorted list of maximal cliques (maximal_cliques_ref.solve()["cliques"],
or the library's own maximal_cliques_list()); all clique indices are positions in that list.  pair_tests() restates the pivot
rule separately, for the one output that is defined by it.  tests/test_clique_communities_ref.py checks both against
networkx.k_clique_communities and the literal definition."""
import bisect

import numpy as np


def solve(nv, cliques, k):
    """cliques: ascending tuples in lexicographic order.  dict of every output of the contract: label, size (int32[len(cliques)]),
    rep, n_cliques (int32[n]), offset (int64[n + 1]), verts (int32), n_comm, first (int32[nv]), n_member_cliques,
    n_communities, largest, n_covered, n_overlap, and communities (the list of ascending vertex tuples, in community order).
    ValueError for a k the library answers KOMB_ERR_ARG."""
    if k < 2:
        raise ValueError("bad k")
    cliques = [tuple(int(v) for v in c) for c in cliques]
    assert cliques == sorted(set(cliques)) and all(list(c) == sorted(set(c)) for c in cliques), "a sorted list of ascending tuples expected"
    n = len(cliques)
    member = [i for i in range(n) if len(cliques[i]) >= k]
    sets = {i: set(cliques[i]) for i in member}
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, i in enumerate(member):
        for j in member[a + 1:]:
            if len(sets[i] & sets[j]) >= k - 1:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)             # the root of a class is its smallest index
    label = np.full(n, -1, np.int32)
    size = np.zeros(n, np.int32)
    for i in member:
        label[i] = find(i)
    reps = sorted(set(int(x) for x in label[member]))
    number = {r: c for c, r in enumerate(reps)}
    n_cl = np.zeros(len(reps), np.int32)
    comm = [set() for _ in reps]
    for i in member:
        c = number[int(label[i])]
        n_cl[c] += 1
        comm[c] |= sets[i]
    for i in member:
        size[i] = n_cl[number[int(label[i])]]
    communities = [tuple(sorted(s)) for s in comm]
    offset = np.zeros(len(reps) + 1, np.int64)
    for c, s in enumerate(communities):
        offset[c + 1] = offset[c] + len(s)
    verts = np.asarray([v for s in communities for v in s], np.int32)
    n_comm = np.zeros(nv, np.int32)
    first = np.full(nv, -1, np.int32)
    for c, s in enumerate(communities):
        for v in s:
            n_comm[v] += 1
            if first[v] < 0:
                first[v] = c
    return {"k": k, "label": label, "size": size, "rep": np.asarray(reps, np.int32), "n_cliques": n_cl, "offset": offset, "verts": verts,
            "n_comm": n_comm, "first": first, "n_member_cliques": len(member), "n_communities": len(reps),
            "largest": max((len(s) for s in communities), default=0), "n_covered": int((n_comm >= 1).sum()),
            "n_overlap": int((n_comm >= 2).sum()), "communities": communities}


def pair_tests(cliques, k):
    """The candidates the pivot rule looks at: load(v) = the member cliques through v; the pivots of a member clique of s vertices
    are its s - k + 2 vertices of smallest (load(v), v); the sum over member cliques i and their pivots v of the member cliques
    j > i through v."""
    member = [i for i, c in enumerate(cliques) if len(c) >= k]
    rows = {}
    for i in member:
        for v in cliques[i]:
            rows.setdefault(int(v), []).append(i)                 # ascending: member is
    total = 0
    for i in member:
        c = [int(v) for v in cliques[i]]
        pivots = sorted(c, key=lambda v: (len(rows[v]), v))[:len(c) - k + 2]
        for v in pivots:
            total += len(rows[v]) - bisect.bisect_right(rows[v], i)
    return total


def vertex_sets(res):
    """The communities as a sorted list of vertex tuples (what compares with another notion of community)."""
    return sorted(res["communities"])


# ---- the hand graphs of the tests, as (nv, edges)
def _clique(ids):
    ids = list(ids)
    return [(ids[a], ids[b]) for a in range(len(ids)) for b in range(a + 1, len(ids))]


def two_cliques(n, shared):
    """Two K_n that share `shared` vertices: the first on 0 .. n - 1, the second on n - shared .. 2 n - shared - 1."""
    return 2 * n - shared, sorted(set(_clique(range(n)) + _clique(range(n - shared, 2 * n - shared))))


def strip(n_triangles=5):
    """A strip of triangles: the path edges i -- i + 1 and i -- i + 2 on n_triangles + 2 vertices."""
    nv = n_triangles + 2
    return nv, [(i, i + 1) for i in range(nv - 1)] + [(i, i + 2) for i in range(nv - 2)]


def book(pages):
    """`pages` triangles on the one edge (0, 1)."""
    return pages + 2, [(0, 1)] + [(u, w) for w in range(2, pages + 2) for u in (0, 1)]


def windmill(blades):
    """`blades` triangles on the one hub 0."""
    return 2 * blades + 1, [e for b in range(blades) for e in ((0, 2 * b + 1), (0, 2 * b + 2), (2 * b + 1, 2 * b + 2))]


# (graph, k, communities, pair_tests): worked out once with a prototype of the pivot rule, candidates j > i only, the list in
# lexicographic order, pivot ties to the smaller vertex id
HAND_TABLE = (
    ("two K_4 sharing one vertex", 2, 1, 1), ("two K_4 sharing one vertex", 3, 2, 0), ("two K_4 sharing one vertex", 4, 2, 0),
    ("two K_4 sharing one vertex", 5, 0, 0),
    ("two K_4 sharing an edge", 2, 1, 2), ("two K_4 sharing an edge", 3, 1, 1), ("two K_4 sharing an edge", 4, 2, 0),
    ("two K_5 sharing a triangle", 2, 1, 3), ("two K_5 sharing a triangle", 3, 1, 2), ("two K_5 sharing a triangle", 4, 1, 1),
    ("two K_5 sharing a triangle", 5, 2, 0),
    ("strip of 5 triangles", 2, 1, 11), ("strip of 5 triangles", 3, 1, 4),
)
HAND_GRAPHS = {"two K_4 sharing one vertex": two_cliques(4, 1), "two K_4 sharing an edge": two_cliques(4, 2),
               "two K_5 sharing a triangle": two_cliques(5, 3), "strip of 5 triangles": strip(5)}
