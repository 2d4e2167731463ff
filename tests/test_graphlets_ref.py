"""CPU tests of the two graphlet references (tests/graphlets_ref.py) against each other: the closed forms of census() and
the subset enumeration of brute() share nothing but the orbit numbering."""
from itertools import combinations

import numpy as np
import pytest

from graphlets_ref import IDENTITIES, ORBITS, TYPES, brute, census, check_identities, ordered_items

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
