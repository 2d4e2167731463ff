"""CPU tests of the two graphlet references (tests/graphlets_ref.py) against each other: the closed forms of census() and
the subset enumeration of brute() share nothing but the orbit numbering.  The sparse path of census() (above 3000 vertices) is
held against the dense one and against brute()."""
from itertools import combinations

import numpy as np
import pytest

from graphlets_ref import DENSE_MAX_NV, IDENTITIES, ORBITS, TYPES, brute, census, census_sparse, check_identities, ordered_items

# the six connected graphs of 4 vertices: edges and, per vertex, the one 4-vertex orbit it holds
FOUR = {
    "path4": ([(0, 1), (1, 2), (2, 3)], [4, 5, 5, 4]),
    "claw": ([(0, 1), (0, 2), (0, 3)], [7, 6, 6, 6]),
    "cycle4": ([(0, 1), (1, 2), (2, 3), (0, 3)], [8, 8, 8, 8]),
    "paw": ([(0, 1), (0, 2), (1, 2), (0, 3)], [11, 10, 10, 9]),
    "diamond": ([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)], [13, 13, 12, 12]),
    "clique4": ([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], [14, 14, 14, 14]),
}


def both(nv, edges):
    edges = sorted((min(u, v), max(u, v)) for u, v in edges)
    eu, ev = [e[0] for e in edges], [e[1] for e in edges]
    c, b = census(nv, eu, ev), brute(nv, edges)
    for key in ("orbit", "cycles4", "cliques4", "sup"):
        assert np.array_equal(c[key], b[key]), key
    assert c["total"] == b["total"]
    check_identities(c["orbit"])
    assert ordered_items(nv, eu, ev) >= 0
    return c


@pytest.mark.parametrize("name", sorted(FOUR))
def test_four_vertex_graphs_are_one_hot(name):
    edges, where = FOUR[name]
    c = both(4, edges)
    want = np.zeros((ORBITS - 4, 4), dtype=np.uint64)
    for v, o in enumerate(where):
        want[o - 4, v] = 1
    assert np.array_equal(c["orbit"][4:], want)
    assert c["total"][name] == 1
    assert sum(c["total"][t] for t in TYPES[3:]) == 1


def test_three_vertex_graphs():
    c = both(3, [(0, 1), (1, 2)])
    assert c["orbit"][:4].tolist() == [[1, 2, 1], [1, 0, 1], [0, 1, 0], [0, 0, 0]]
    c = both(3, [(0, 1), (1, 2), (0, 2)])
    assert c["orbit"][:4].tolist() == [[2, 2, 2], [0, 0, 0], [0, 0, 0], [1, 1, 1]]
    assert not c["orbit"][4:].any()


@pytest.mark.parametrize("seed", range(20))
def test_random_graphs(seed):
    rng = np.random.default_rng(1000 + seed)
    nv = int(rng.integers(5, 29))
    p = float(rng.choice([0.1, 0.2, 0.35, 0.5, 0.8, 1.0]))
    alive = rng.random(nv) < 0.85                                           # isolated vertices included
    edges = [(u, v) for u, v in combinations(range(nv), 2) if alive[u] and alive[v] and rng.random() < p]
    both(nv, edges)


def test_named_graphs():
    c = both(7, list(combinations(range(7), 2)))                           # K_7
    assert c["total"]["clique4"] == 35 and c["cliques4"].tolist() == [10] * 21 and c["cycles4"].tolist() == [2 * 10] * 21
    c = both(7, [(u, 3 + v) for u in range(3) for v in range(4)])           # K_{3,4}
    assert c["total"]["cycle4"] == 3 * 6 and c["total"]["triangle"] == 0 and c["cycles4"].tolist() == [2 * 3] * 12
    c = both(5, [(i, (i + 1) % 5) for i in range(5)])                       # C_5
    assert c["total"]["path4"] == 5 and c["total"]["cycle4"] == 0
    c = both(9, [(4, v) for v in range(9) if v != 4])                       # a star, the centre in the middle of the ids
    assert c["orbit"][7, 4] == 56 and c["orbit"][6, 0] == 21 and c["total"]["claw"] == 56
    assert ordered_items(9, [4] * 8, [v for v in range(9) if v != 4]) == 0


def test_identities_are_not_vacuous():
    """a wrong orbit table trips them"""
    c = census(4, [0, 0, 1, 0], [1, 2, 2, 3])
    bad = c["orbit"].copy()
    bad[9, 3] += np.uint64(1)
    with pytest.raises(AssertionError):
        check_identities(bad)
    assert len(IDENTITIES) == 6


# ---- the sparse path of census(): the graphs above 3000 vertices of tests/sequence_model.py

def _simple(nv, uv):
    """(eu, ev): the canonical edges of the raw pairs -- u < v, ascending, loops and repeats dropped"""
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    uv = np.unique(np.sort(uv[uv[:, 0] != uv[:, 1]], axis=1), axis=0)
    return uv[:, 0], uv[:, 1]


def _equal(x, y):
    for key in ("orbit", "cycles4", "cliques4", "sup"):
        assert x[key].dtype == y[key].dtype and np.array_equal(x[key], y[key]), key
    assert x["total"] == y["total"]


@pytest.fixture(scope="module")
def sequence_graphs(built):
    import komb_amd
    import sequence_model as SM
    return SM.raw_graphs(komb_amd.gen_hug_edges, SM.hand_graphs())


@pytest.mark.parametrize("name", ["A", "B", "D", "hand_sc", "hand_nuc"])
def test_sparse_path_equals_the_dense_one(sequence_graphs, name):
    nv, uv = sequence_graphs[name]
    eu, ev = _simple(nv, uv)
    assert nv <= DENSE_MAX_NV and len(eu) > 0
    dense, sparse = census(nv, eu, ev, dense=True), census_sparse(nv, eu, ev)
    _equal(dense, sparse)
    assert dense["cycles4"].any() and dense["sup"].any()


def test_sparse_path_on_the_strided_graph_equals_the_dense_one_on_its_vertices_with_edges(sequence_graphs):
    """524 549 vertices, far past the dense identity: the default is the sparse path; the dense one sees the four vertices that
    have edges, renumbered, and every other vertex has fifteen zeros."""
    nv, uv = sequence_graphs["strided"]
    eu, ev = _simple(nv, uv)
    assert nv > DENSE_MAX_NV
    got = census(nv, eu, ev)                                                # (the dense one would assert)
    ids = np.unique(np.concatenate([eu, ev]))
    small = census(len(ids), np.searchsorted(ids, eu), np.searchsorted(ids, ev), dense=True)
    for key in ("cycles4", "cliques4", "sup"):
        assert np.array_equal(got[key], small[key]), key
    assert np.array_equal(got["orbit"][:, ids], small["orbit"]) and got["total"] == small["total"] and got["total"]["clique4"] == 1
    rest = np.ones(nv, dtype=bool)
    rest[ids] = False
    assert not got["orbit"][:, rest].any()


@pytest.mark.parametrize("seed", range(20))
def test_sparse_path_equals_brute_on_small_permuted_graphs(seed):
    """The random graphs of test_random_graphs, their ids permuted."""
    rng = np.random.default_rng(1000 + seed)
    nv = int(rng.integers(5, 29))
    p = float(rng.choice([0.1, 0.2, 0.35, 0.5, 0.8, 1.0]))
    alive = rng.random(nv) < 0.85
    edges = [(u, v) for u, v in combinations(range(nv), 2) if alive[u] and alive[v] and rng.random() < p]
    ids = np.random.default_rng(2000 + seed).permutation(nv)
    edges = sorted((int(min(ids[u], ids[v])), int(max(ids[u], ids[v]))) for u, v in edges)
    s, b = census_sparse(nv, [e[0] for e in edges], [e[1] for e in edges]), brute(nv, edges)
    _equal(s, b)
    check_identities(s["orbit"])


def test_sparse_path_on_the_strip_of_triangles(sequence_graphs):
    """Graph C, 9000 vertices: the identities hold, and the counts are the strip's -- 2 n - 3 edges, n - 2 triangles, a diamond
    on every four consecutive vertices, no 4-cycle without a chord and no 4-clique."""
    nv, uv = sequence_graphs["C"]
    eu, ev = _simple(nv, uv)
    c = census(nv, eu, ev)
    check_identities(c["orbit"])
    assert c["total"]["edge"] == 2 * nv - 3 and c["total"]["triangle"] == nv - 2 and c["total"]["diamond"] == nv - 3
    assert c["total"]["cycle4"] == 0 and c["total"]["clique4"] == 0 and not c["cliques4"].any()
    assert int(c["cycles4"].sum()) == 4 * c["total"]["diamond"]
