"""CPU tests that pin the native references of the distance analysis, the betweenness centrality and the graphlet census
(oracle/komb_oracle.c: orc_bfs_sources, orc_betweenness, orc_graphlets, orc_orbits_by_definition, through the wrappers of
oracle/oracle.py) to the Python restatements under tests/ and to the stored fixtures: every array exactly, harmonic[] and bc[]
as raw 64-bit patterns, every info field.  tests/test_gpu_midsize_traversals.py then holds the library against these
references at sizes the Python ones cannot reach.

The Python restatements are themselves tied to networkx, to closed forms and to each other by tests/test_distances_ref.py,
tests/test_betweenness_ref.py and tests/test_graphlets_ref.py; the two stored fixtures tell a fused multiply-add, a different
row order and a different order of the harmonic sum from the definition, so bit equality here says the C code keeps all
three."""
from itertools import combinations

import numpy as np
import pytest

import betweenness_ref as B
import distances_ref as D
import graphlets_ref as G
from oracle import oracle as O
from test_betweenness_ref import load_fixture as load_bc_fixture
from test_graphlets_ref import FOUR

INFO_D = ("n_sources", "flags", "depth_max", "depth_min", "n_pairs", "sum_all", "n_batches", "n_level_steps")
INFO_B = ("flags", "depth_max", "n_sources", "n_batches", "n_level_steps")
LISTS = (1, 63, 64, 65, 257)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same_distances(got, want):
    for name in ("n_reached", "sum_dist", "ecc"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert got["harmonic"].dtype == np.float64 and np.array_equal(bits(got["harmonic"]), bits(want["harmonic"]))
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert got["sources"][name].dtype == want["sources"][name].dtype, name
        assert np.array_equal(got["sources"][name], want["sources"][name]), name
    assert got["pairs"].dtype == np.int64 and np.array_equal(got["pairs"], want["pairs"])
    assert got["info"] == want["info"] and tuple(sorted(got["info"])) == tuple(sorted(INFO_D))


def same_betweenness(got, want):
    assert got["bc"].dtype == np.float64 and np.array_equal(bits(got["bc"]), bits(want["bc"]))
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert {k: got[k] for k in INFO_B} == {k: want[k] for k in INFO_B}


def same_graphlets(got, want):
    for key in ("orbit", "cycles4", "cliques4", "sup"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert got["total"] == want["total"]


@pytest.fixture(scope="module")
def hug(built):
    """The generated graph of tests/test_gpu_distances.py and tests/test_gpu_betweenness.py: 3000 vertices, a hub of more than a
    thousand neighbours, isolated vertices; `master` is that file's list of 513 entries drawn from 150 vertices -- repeats
    everywhere, no order, the hub first and isolated vertices among the first entries."""
    import komb_amd
    nv = 3000
    rowptr, col = O.simplify(nv, komb_amd.gen_hug_edges(3000, 7350, 2.2, 5))
    rows = D.rows_of_csr(rowptr.tolist(), col.tolist())
    deg = np.diff(rowptr)
    assert deg.max() > 1000
    rng = np.random.default_rng(11)
    hub = int(deg.argmax())
    isolated = np.flatnonzero(deg == 0).tolist()
    assert len(isolated) >= 2
    pool = rng.permutation(nv)[:150]
    master = rng.choice(pool, size=513).tolist()
    master[0], master[5], master[40], master[41], master[70] = hub, isolated[0], isolated[1], isolated[0], hub
    return {"nv": nv, "rowptr": rowptr, "col": col, "rows": rows, "master": master, "hub": hub, "isolated": isolated}


# ---- orc_bfs_sources

@pytest.mark.parametrize("words", [1, 2, 4])
def test_bfs_sources_reproduce_the_stored_fixture(built, words):
    nv, pairs, sources, stored = D.load_fixture()
    rowptr, col = O.simplify(nv, pairs)
    rows = D.adjacency(nv, pairs)
    assert rows == D.rows_of_csr(rowptr.tolist(), col.tolist())
    got = O.distances(rowptr, col, sources, words)
    same_distances(got, D.distances(rows, sources, words))
    assert np.array_equal(bits(got["harmonic"]), stored)
    assert got["info"]["n_batches"] == -(-300 // (64 * words))


def test_bfs_sources_on_the_golden_graphs(golden):
    for g in golden:
        rowptr, col = np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32)
        rows = D.rows_of_csr(g["rowptr"], g["col"])
        cache = {}
        if g["nv"] <= 300:
            same_distances(O.distances(rowptr, col), D.distances(rows, cache=cache))
        some = list(range(g["nv"] - 1, -1, -3))
        for words in (1, 4):
            same_distances(O.distances(rowptr, col, some, words), D.distances(rows, some, words, cache=cache))


@pytest.mark.parametrize("n", LISTS)
def test_bfs_sources_on_the_generated_graph(hug, n):
    """Lists of 1, 63, 64, 65 and 257 entries: below, at and past one block of 64, and past four of them, with repeats and
    isolated vertices."""
    src = hug["master"][:n]
    if n >= 63:
        assert len(set(src)) < n and set(hug["isolated"][:2]) <= set(src)
    cache = hug.setdefault("dist_cache", {})
    for words in (1, 4):
        same_distances(O.distances(hug["rowptr"], hug["col"], src, words), D.distances(hug["rows"], src, words, cache=cache))


def test_bfs_sources_degenerate_inputs(built):
    rowptr, col = O.simplify(6, np.asarray([(0, 1), (1, 2), (3, 4)]))
    rows = D.rows_of_csr(rowptr.tolist(), col.tolist())
    for src in ([5, 0, 3, 0], [5], [], None):
        same_distances(O.distances(rowptr, col, src), D.distances(rows, src))
    rowptr, col = O.simplify(70, np.zeros((0, 2)))
    same_distances(O.distances(rowptr, col, None, 1), D.distances([[] for _ in range(70)], words=1))
    with pytest.raises(ValueError):
        O.distances(rowptr, col, [70])


# ---- orc_betweenness

def test_betweenness_reproduces_the_stored_fixture(built):
    nv, pairs, stored = load_bc_fixture()
    rowptr, col = O.simplify(nv, pairs)
    rows = B.adjacency(nv, pairs)
    assert rows == B.rows_of_csr(rowptr.tolist(), col.tolist())
    got = O.betweenness(rowptr, col)
    same_betweenness(got, B.betweenness(rows))
    assert np.array_equal(bits(got["bc"]), stored)
    fused = B.betweenness(rows, fused=True)["bc"]                             # (what a contracted multiply-add would have given)
    assert (bits(fused) != bits(got["bc"])).sum() >= 5
    same_betweenness(O.betweenness(rowptr, col, [48, 0, 17, 17, 3]), B.betweenness(rows, [48, 0, 17, 17, 3]))


def test_betweenness_on_the_generated_graph(hug):
    """One source (the hub), a partial second batch, repeats, isolated sources beside the hub."""
    rng = np.random.default_rng(11)
    hub, isolated = hug["hub"], hug["isolated"]
    cache = {}
    for src in ([hub], rng.permutation(hug["nv"])[:65].tolist(), [7, 7, hub, 2999, 7, hub] * 12, isolated[:3] + [hub] + isolated[:1]):
        same_betweenness(O.betweenness(hug["rowptr"], hug["col"], src), B.betweenness(hug["rows"], src, cache=cache))


def test_betweenness_on_the_golden_graphs(golden):
    for g in golden:
        rowptr, col = np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32)
        rows = B.rows_of_csr(g["rowptr"], g["col"])
        some = list(range(g["nv"] - 1, -1, -3))
        same_betweenness(O.betweenness(rowptr, col, some), B.betweenness(rows, some))


@pytest.mark.parametrize("k", [52, 53, 60])
def test_betweenness_rounded_flag_on_the_diamond_chain(built, k):
    nv, pairs = B.diamond_chain(k)
    rowptr, col = O.simplify(nv, pairs)
    src = [0, nv - 1, nv // 2]
    got = O.betweenness(rowptr, col, src)
    same_betweenness(got, B.betweenness(B.adjacency(nv, pairs), src))
    assert got["flags"] == (B.ROUNDED if k >= 53 else 0)


def test_betweenness_limit_on_the_layered_graph(built):
    nv, pairs = B.layered(257)
    rowptr, col = O.simplify(nv, pairs)
    rows = B.adjacency(nv, pairs)
    with pytest.raises(B.Limit):
        B.betweenness(rows, [0])
    for src in ([0], [3, 0, 4]):
        with pytest.raises(O.Limit):
            O.betweenness(rowptr, col, src)
    same_betweenness(O.betweenness(rowptr, col, [1]), B.betweenness(rows, [1]))          # (from layer 1 the counts stay finite)
    nv, pairs = B.layered(256)
    rowptr, col = O.simplify(nv, pairs)
    got = O.betweenness(rowptr, col, [0])
    same_betweenness(got, B.betweenness(B.adjacency(nv, pairs), [0]))
    assert got["flags"] == B.ROUNDED and np.isfinite(got["bc"]).all()


def test_betweenness_degenerate_inputs(built):
    rowptr, col = O.simplify(6, np.asarray([(0, 1), (1, 2), (3, 4)]))
    rows = B.rows_of_csr(rowptr.tolist(), col.tolist())
    for src in ([5, 0, 3], [], None):
        same_betweenness(O.betweenness(rowptr, col, src), B.betweenness(rows, src))
    with pytest.raises(ValueError):
        O.betweenness(rowptr, col, [-1])


def test_per_source_integers_of_the_two_references_agree(hug):
    src = hug["master"][:257]
    d, b = O.distances(hug["rowptr"], hug["col"], src), O.betweenness(hug["rowptr"], hug["col"], src)
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert np.array_equal(d["sources"][name], b[name]), name


# ---- orc_graphlets and orc_orbits_by_definition

def small_graphs():
    """(nv, edges) of the small graphs of tests/test_graphlets_ref.py: the connected 3- and 4-vertex graphs, its twenty random
    graphs (isolated vertices included) and its named ones."""
    out = [(4, FOUR[name][0]) for name in sorted(FOUR)] + [(3, [(0, 1), (1, 2)]), (3, [(0, 1), (1, 2), (0, 2)])]
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        nv = int(rng.integers(5, 29))
        p = float(rng.choice([0.1, 0.2, 0.35, 0.5, 0.8, 1.0]))
        alive = rng.random(nv) < 0.85
        out.append((nv, [(u, v) for u, v in combinations(range(nv), 2) if alive[u] and alive[v] and rng.random() < p]))
    out += [(7, list(combinations(range(7), 2))), (7, [(u, 3 + v) for u in range(3) for v in range(4)]),
            (5, [(i, (i + 1) % 5) for i in range(5)]), (9, [(4, v) for v in range(9) if v != 4]), (4, [])]
    return out


def test_graphlets_equal_brute_on_the_small_graphs(built):
    seen = np.zeros(G.ORBITS, dtype=bool)
    for nv, edges in small_graphs():
        rowptr, col = O.simplify(nv, np.asarray(edges, dtype=np.int64).reshape(-1, 2))
        eu, ev = O.edge_list(rowptr, col)
        want = G.brute(nv, list(zip(eu.tolist(), ev.tolist())))
        got = O.graphlets(rowptr, col)
        same_graphlets(got, want)
        for v in range(nv):                                                   # and the definitional walk, vertex by vertex
            vec, ball = O.orbits_by_definition(rowptr, col, v)
            assert vec.dtype == np.uint64 and np.array_equal(vec, want["orbit"][:, v]), (nv, v)
            assert 1 <= ball <= nv
        seen |= want["orbit"].any(axis=1)
    assert seen.all()                                                         # every orbit occurred


def _clique(n):
    return np.asarray(list(combinations(range(n), 2)), dtype=np.int64)


def _hub_graph():
    """K_60 and a hub joined to all of it and to 1940 leaves (tests/test_gpu_graphlets.py)"""
    return 2001, np.concatenate([_clique(60), [[60, v] for v in range(60)], [[60, 61 + v] for v in range(1940)]])


@pytest.fixture(scope="module")
def hug_census(hug):
    eu, ev = O.edge_list(hug["rowptr"], hug["col"])
    return G.census(hug["nv"], eu, ev), O.graphlets(hug["rowptr"], hug["col"])


def test_graphlets_equal_census_on_the_generated_graph(hug_census):
    want, got = hug_census
    same_graphlets(got, want)
    G.check_identities(got["orbit"])
    assert want["cycles4"].any() and want["cliques4"].any() and want["orbit"][4:].any(axis=1).all()


@pytest.mark.parametrize("which", ["k90", "hub"])
def test_graphlets_equal_census_on_k90_and_the_hub_graph(built, which):
    nv, uv = (90, _clique(90)) if which == "k90" else _hub_graph()
    rowptr, col = O.simplify(nv, uv)
    eu, ev = O.edge_list(rowptr, col)
    same_graphlets(O.graphlets(rowptr, col), G.census(nv, eu, ev))


def test_orbits_by_definition_on_the_generated_graph(hug, hug_census):
    """Sixty vertices whose three-hop ball has at most 1500 vertices: far more and far larger sets than the small graphs have.
    The ball limit is honoured: a vertex beside the hub is refused."""
    want = hug_census[0]["orbit"]
    order = np.random.default_rng(3).permutation(hug["nv"])
    done = 0
    for v in order.tolist():
        vec, ball = O.orbits_by_definition(hug["rowptr"], hug["col"], v, 1500)
        if vec is None:
            continue
        assert ball <= 1500 and np.array_equal(vec, want[:, v]), v
        done += 1
        if done == 60:
            break
    assert done == 60
    assert O.orbits_by_definition(hug["rowptr"], hug["col"], hug["hub"], 1000) == (None, None)


def ordered_items_np(rowptr, col):
    """graphlets_ref.ordered_items -- the sum over v, over the neighbours u of v below v in (d, id) order, of the neighbours
    of u below v -- over whole arrays, for graphs where the Python loop takes too long: every row's ranks are sorted once
    (one global sort of row * nv + rank), and a slot (v, u) with u below v looks up how many of u's are below rank[v]."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    nv = len(rowptr) - 1
    deg = np.diff(rowptr)
    rank = np.empty(nv, np.int64)
    rank[np.lexsort((np.arange(nv), deg))] = np.arange(nv)
    v = np.repeat(np.arange(nv, dtype=np.int64), deg)
    key = np.sort(v * nv + rank[col])
    take = rank[col] < rank[v]
    u = col[take]
    return int((np.searchsorted(key, u * nv + rank[v[take]]) - rowptr[u]).sum())


def test_ordered_items_over_whole_arrays_equal_the_loop(hug):
    eu, ev = O.edge_list(hug["rowptr"], hug["col"])
    assert ordered_items_np(hug["rowptr"], hug["col"]) == G.ordered_items(hug["nv"], eu, ev) > 0
    for nv, edges in small_graphs()[6::3] + [_hub_graph(), (90, _clique(90))]:
        rowptr, col = O.simplify(nv, np.asarray(edges, dtype=np.int64).reshape(-1, 2))
        eu, ev = O.edge_list(rowptr, col)
        assert ordered_items_np(rowptr, col) == G.ordered_items(nv, eu, ev)


def test_graphlets_cross_checks_with_the_clique_census_and_the_support(hug, hug_census):
    got = hug_census[1]
    assert np.array_equal(got["orbit"][3], O.clique_counts(hug["rowptr"], hug["col"], 3)["local"])
    assert np.array_equal(got["orbit"][14], O.clique_counts(hug["rowptr"], hug["col"], 4)["local"])
    sup, triangles = O.support(hug["rowptr"], hug["col"])
    assert np.array_equal(got["sup"], sup) and got["total"]["triangle"] == triangles > 0
    totals = O.clique_counts(hug["rowptr"], hug["col"], 0)["total"]
    assert [got["total"]["edge"], got["total"]["triangle"], got["total"]["clique4"]] == [int(x) for x in totals[2:5]]
