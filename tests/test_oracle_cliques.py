"""CPU tests of the native references of oracle/komb_oracle.c for the clique analyses and the (3,4)-nucleus decomposition --
orc_clique_census, orc_maximal_cliques, orc_nucleus and the numpy / scipy helpers of oracle/oracle.py on top of them, clique
percolation by shared subsets (clique_communities, percolation_pair_tests) among them.  The mid-size GPU tests
(tests/test_gpu_midsize.py, tests/test_gpu_midsize_structure.py) trust them at sizes the Python restatements cannot reach, so
here every output is
tied to what the suite already trusts: on the random and hand graph sets of test_clique_census_ref.py,
test_maximal_cliques_ref.py, test_max_clique_ref.py, test_nucleus_ref.py and test_nucleus_hierarchy_ref.py it equals the Python
restatement's, and networkx's where those files use it; the degenerate inputs and K_70 (saturation) are included; and one
recorded run pins the oracle itself: the k-clique totals of gen_hug_edges(50000, 122500, 2.6, 42), counted once by an
enumeration over std::set_intersection that shares no code with anything here."""
from math import comb

import numpy as np
import pytest

import clique_census_ref as C
import clique_communities_ref as P
import max_clique_ref as Q
import maximal_cliques_ref as M
import nucleus_hierarchy_ref as H
import nucleus_ref as R
import test_clique_census_ref as TC
import test_max_clique_ref as TQ
import test_maximal_cliques_ref as TM
import test_nucleus_ref as TN
from oracle import oracle as O

SAT = 2 ** 64 - 1


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _graph(nv, edges):
    """(rowptr, col, eu, ev) of any simple edge list."""
    rowptr, col = O.simplify(nv, np.asarray(R.canonical(edges), np.int64).reshape(-1, 2))
    return (rowptr, col) + O.edge_list(rowptr, col)


def _tuples(view):
    off, verts = view["offset"], view["verts"]
    return [tuple(verts[off[i]:off[i + 1]].tolist()) for i in range(len(off) - 1)]


# ---- clique census

def _same_census(got, want):
    for name in ("k_lo", "k_hi", "k_local", "t_max", "omega", "flags"):
        assert got[name] == want[name], name
    assert got["total"].dtype == np.uint64 and np.array_equal(got["total"], want["total"])
    if want["local"] is None:
        assert got["local"] is None
    else:
        assert got["local"].dtype == np.uint64 and np.array_equal(got["local"], want["local"])


@pytest.mark.parametrize("seed", range(16))
def test_census_random_graphs(built, seed):
    """The windows of test_clique_census_ref on its random graphs: the Python restatement and networkx, clique by clique."""
    nv, edges = TC._random_graph(seed)
    rowptr, col, eu, ev = _graph(nv, edges)
    by_k = {k_local: TC._by_networkx(nv, edges, k_local) for k_local in (0, 2, 3, 4, 5)}
    t_max = by_k[0][2]
    assert O.t_max(rowptr, col) == t_max
    for k_lo in (2, 4):
        for k_hi in (-1, k_lo + 2):
            used = max(k_lo, t_max if k_hi == -1 else min(k_hi, t_max))
            for k_local in (0, k_lo, k_lo + 1):
                if k_local > used:
                    with pytest.raises(ValueError):
                        O.clique_census(rowptr, col, k_lo, k_hi, k_local)
                    continue
                got = O.clique_census(rowptr, col, k_lo, k_hi, k_local)
                _same_census(got, C.census(nv, eu, ev, k_lo=k_lo, k_hi=k_hi, k_local=k_local))
                total, local, _ = by_k[k_local]
                assert got["total"].tolist() == [total.get(k, 0) for k in range(k_lo, used + 1)]
                if k_local:
                    assert got["local"].tolist() == local
    raw = O.clique_counts(rowptr, col)
    assert raw["clique_number"] == max([k for k in by_k[0][0] if k >= 2], default=0)
    assert raw["nodes"] == sum(n for k, n in by_k[0][0].items() if k >= 2)        # every clique was visited, once


def test_census_degenerate_graphs_and_arguments(built):
    for nv, edges in ((0, []), (5, [])):                                          # no vertices, no edges
        rowptr, col, eu, ev = _graph(nv, edges)
        got = O.clique_census(rowptr, col, 2, -1, 2)
        _same_census(got, C.census(nv, eu, ev, k_local=2))
        assert (got["k_hi"], got["t_max"], got["omega"], got["flags"]) == (2, 0, 0, 1)
        assert got["total"].tolist() == [0] and got["local"].tolist() == [0] * nv
    nv, edges = 6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)]                       # no triangle
    rowptr, col, eu, ev = _graph(nv, edges)
    got = O.clique_census(rowptr, col, 2, -1, 2)
    _same_census(got, C.census(nv, eu, ev, k_local=2))
    assert got["total"].tolist() == [5] and got["local"].tolist() == [1, 3, 2, 2, 1, 1] and got["omega"] == 2
    rowptr, col, eu, ev = _graph(4, [(0, 1), (1, 3), (0, 3)])
    got = O.clique_census(rowptr, col, 4, 9)                                       # a window above t_max: zeros
    _same_census(got, C.census(4, eu, ev, k_lo=4, k_hi=9))
    assert (got["k_hi"], got["total"].tolist(), got["omega"]) == (4, [0], 0)
    for bad in (dict(k_lo=1), dict(k_lo=3, k_hi=2), dict(k_local=-1), dict(k_lo=2, k_hi=3, k_local=4), dict(k_lo=3, k_local=2)):
        with pytest.raises(ValueError):
            O.clique_census(rowptr, col, **bad)


@pytest.mark.parametrize("n", [2, 3, 5, 12, 19, 20, 21, 40])
def test_census_complete_graphs(built, n):
    """K_n on both sides of the size from which a complete candidate set is closed by binomials (20)."""
    rowptr, col, eu, ev = _graph(n, R.clique(range(n)))
    k_local = max(n // 2, 2)
    got = O.clique_census(rowptr, col, 2, -1, k_local, tmax=n)
    assert got["t_max"] == n == got["omega"] == got["k_hi"] and got["flags"] == 1
    assert got["total"].tolist() == [comb(n, k) for k in range(2, n + 1)]
    assert got["local"].tolist() == [comb(n - 1, k_local - 1)] * n
    if n <= 12:
        _same_census(got, C.census(n, eu, ev, k_local=k_local))
        assert O.clique_counts(rowptr, col)["nodes"] == 2 ** n - 1 - n            # every clique was visited


def test_census_closed_sets_inside_a_larger_graph(built):
    """A K_30 with a pendant triangle on two of its vertices and a K_26 sharing five vertices with it: candidate sets that are
    complete and ones of the same size that are not, with held vertices above them."""
    edges = R.clique(range(30)) + [(30, 0), (30, 1)] + R.clique(list(range(25, 30)) + list(range(31, 52)))
    nv = 52
    rowptr, col, eu, ev = _graph(nv, edges)
    for k_local in (3, 17, 26):
        got = O.clique_census(rowptr, col, 2, -1, k_local)
        want = [comb(30, k) + comb(26, k) - comb(5, k) + (1 if k == 3 else 0) + (2 if k == 2 else 0) for k in range(2, 31)]
        assert got["total"].tolist() == want and got["omega"] == 30 and got["t_max"] == 30
        j = k_local - 1
        both = comb(29, j) + comb(25, j) - comb(4, j)
        local = [comb(29, j)] * 25 + [both] * 5 + [0] + [comb(25, j)] * 21
        if k_local == 3:
            local[0] += 1; local[1] += 1; local[30] = 1
        assert got["local"].tolist() == local
        assert int(got["local"].sum()) == k_local * int(got["total"][k_local - 2])


@pytest.mark.parametrize("m", [3, 6, 10, 12])
def test_census_cocktail_party(built, m):
    nv, edges = C.cocktail_party(m)
    rowptr, col, eu, ev = _graph(nv, edges)
    got = O.clique_census(rowptr, col, 2, -1, m)
    assert got["t_max"] == 2 * m - 2 == got["k_hi"] and got["omega"] == m
    assert got["total"].tolist() == [comb(m, k) * 2 ** k for k in range(2, 2 * m - 1)]
    assert got["local"].tolist() == [2 ** (m - 1)] * nv
    if m <= 6:
        _same_census(got, C.census(nv, eu, ev, k_local=m))
    low = O.clique_census(rowptr, col, 3, 5, 3)
    assert low["total"].tolist() == [comb(m, k) * 2 ** k for k in range(3, min(5, 2 * m - 2) + 1)]
    assert int(low["local"].sum()) == 3 * comb(m, 3) * 8


def test_census_k70_saturates_in_the_middle(built):
    n = 70
    edges = R.clique(range(n))
    rowptr, col, eu, ev = _graph(n, edges)
    want = C.census(n, eu, ev, k_local=35, truss=[n] * len(edges))
    got = O.clique_census(rowptr, col, 2, -1, 35, tmax=n)
    _same_census(got, want)
    assert got["flags"] == 3 and got["omega"] == n
    assert got["total"].tolist() == [min(comb(n, k), SAT) for k in range(2, n + 1)]
    assert [k for k in range(2, n + 1) if got["total"][k - 2] == SAT] == list(range(28, 43))
    assert got["local"].tolist() == [SAT] * n
    low = O.clique_census(rowptr, col, 60, -1, 66, tmax=n)
    _same_census(low, C.census(n, eu, ev, k_lo=60, k_local=66, truss=[n] * len(edges)))
    assert low["flags"] == 1 and low["local"].tolist() == [comb(n - 1, 65)] * n


# ---- maximal cliques, and the maximum cliques read off their list

def _same_maximal(got, want):
    for name in ("k_min", "k_hi", "t_max", "omega", "flags", "n_cliques"):
        assert got[name] == want[name], name
    assert got["hist"].dtype == np.int64 and np.array_equal(got["hist"], want["hist"])
    assert got["count"].dtype == np.int32 and np.array_equal(got["count"], want["count"])
    assert got["largest"].dtype == np.int32 and np.array_equal(got["largest"], want["largest"])
    assert _tuples(got) == want["cliques"]


def _check_maximal(nv, edges, k_mins=TM.K_MIN, truss=None):
    """Every k_min: the numpy view of the k_min = 2 list and the native run at that k_min, both against the restatement."""
    rowptr, col, eu, ev = _graph(nv, edges)
    tmax = O.t_max(rowptr, col) if truss is None else (max(truss) if len(truss) else 0)
    everything = O.maximal_cliques_all(rowptr, col, 2)
    out = {}
    for k_min in k_mins:
        want = M.solve(nv, eu, ev, k_min, truss=truss)
        view = O.maximal_view(everything, tmax, k_min)
        _same_maximal(view, want)
        direct = O.maximal_cliques_all(rowptr, col, k_min)                         # orc_maximal_cliques' own k_min
        assert np.array_equal(direct["hist_all"], everything["hist_all"])
        for name in ("count", "largest", "offset", "verts"):
            assert np.array_equal(direct[name], view[name]), name
        assert (direct["omega"], direct["n_cliques"]) == (view["omega"], view["n_cliques"])
        nolist = O.maximal_cliques_all(rowptr, col, k_min, want_list=False)
        assert nolist["offset"] is None and nolist["n_cliques"] == view["n_cliques"] and np.array_equal(nolist["count"], view["count"])
        out[k_min] = view
    return out


@pytest.mark.parametrize("seed", range(24))
def test_maximal_random_graphs(built, seed):
    nv, edges = TM._random_graph(seed)
    cliques, t_max = TM._by_networkx(nv, edges)
    for k_min, view in _check_maximal(nv, edges).items():
        assert view["t_max"] == t_max and _tuples(view) == [c for c in cliques if len(c) >= k_min]


def test_maximal_degenerate_graphs_and_arguments(built):
    for nv, edges in ((0, []), (5, [])):
        view = _check_maximal(nv, edges)[2]
        assert (view["k_hi"], view["t_max"], view["omega"], view["n_cliques"]) == (2, 0, 0, 0) and view["hist"].tolist() == [0]
    view = _check_maximal(6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)])[2]            # no triangle: every edge is maximal
    assert view["hist"].tolist() == [5] and view["count"].tolist() == [1, 3, 2, 2, 1, 1] and view["largest"].tolist() == [2] * 6
    views = _check_maximal(4, [(0, 1), (1, 3), (0, 3)], k_mins=(2, 3, 5))
    assert _tuples(views[2]) == [(0, 1, 3)] and views[2]["largest"].tolist() == [3, 3, 0, 3]
    assert (views[5]["k_hi"], views[5]["hist"].tolist(), views[5]["omega"]) == (5, [0], 0)   # k_min above t_max
    rowptr, col, _, _ = _graph(4, [(0, 1)])
    with pytest.raises(ValueError):
        O.maximal_cliques(rowptr, col, 1)
    with pytest.raises(ValueError):
        O.maximal_cliques_all(rowptr, col, 1)


@pytest.mark.parametrize("n", [2, 3, 5, 12, 18])
def test_maximal_complete_graphs(built, n):
    """(the pivot-free enumeration visits all 2^n cliques of K_n: no K_70 here)"""
    edges = R.clique(range(n))
    view = _check_maximal(n, edges, k_mins=(2, n), truss=[n] * len(edges))[2]
    assert _tuples(view) == [tuple(range(n))] and view["hist"].tolist() == [0] * (n - 2) + [1]
    assert view["count"].tolist() == [1] * n and view["largest"].tolist() == [n] * n


@pytest.mark.parametrize("m", [3, 6, 12])
def test_maximal_cocktail_party(built, m):
    nv, edges = M.cocktail_party(m)
    for k_min, view in _check_maximal(nv, edges, k_mins=(2, m, m + 1)).items():
        n = 2 ** m if k_min <= m else 0
        assert view["t_max"] == 2 * m - 2 and view["n_cliques"] == n
        assert view["count"].tolist() == [n // 2] * nv and view["largest"].tolist() == [m if n else 0] * nv


def test_maximal_complete_five_partite_and_hand_graph(built):
    nv, edges = M.complete_multipartite([3] * 5)
    view = _check_maximal(nv, edges)[2]
    assert view["n_cliques"] == 243 and view["omega"] == 5 and view["count"].tolist() == [81] * 15
    nv, edges = R.hand_graph()
    view = _check_maximal(nv, edges)[2]
    assert _tuples(view) == sorted(tuple(c) for c in (range(7), (5, 6, 7, 8, 9), (9, 10, 11, 12), (12, 13, 14), (3, 14)))


def _check_maximum(nv, edges, networkx=True):
    """The maximum cliques read off the native list against max_clique_ref (and networkx)."""
    rowptr, col, eu, ev = _graph(nv, edges)
    tmax = O.t_max(rowptr, col)
    got = O.maximum_cliques(O.maximal_cliques(rowptr, col, 2, tmax))
    want = Q.solve(nv, eu, ev)
    for name in ("omega", "upper", "flags", "t_max", "n_max_cliques"):
        assert got[name] == want[name], name
    assert got["count"].dtype == np.int32 and np.array_equal(got["count"], want["count"])
    assert [tuple(r) for r in got["list"].tolist()] == want["cliques"]
    if networkx:
        omega, best, t_max = TQ._by_networkx(nv, R.canonical(edges))
        assert (got["omega"], got["t_max"]) == (omega, t_max) and [tuple(r) for r in got["list"].tolist()] == best
    if got["omega"] > 2:                                                           # the same from a list cut at omega
        high = O.maximum_cliques(O.maximal_cliques(rowptr, col, got["omega"], tmax))
        assert np.array_equal(high["list"], got["list"]) and np.array_equal(high["count"], got["count"])
    return got


def test_maximum_small_graphs(K, golden):
    _check_maximum(0, [])
    _check_maximum(5, [])
    _check_maximum(6, [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5)])
    for g in golden:
        _check_maximum(len(g["rowptr"]) - 1, list(zip(g["eu"], g["ev"])))
        _check_maximum(len(g["rowptr"]) - 1, list(zip(g["sub_eu"], g["sub_ev"])))
    _check_maximum(*R.hand_graph())
    _check_maximum(120, R.clique_union(120, 220, 2, 9, 1))
    _check_maximum(300, TQ._canonical(K.gen_hug_edges(300, 735, 2.6, 6)))
    for m in (3, 6, 12):
        got = _check_maximum(*Q.cocktail_party(m), networkx=m < 12)
        assert (got["omega"], got["n_max_cliques"]) == (m, 2 ** m)


# (the rows of 3 000 and 5 000 vertices at alpha 2.2 / 2.1 hold cliques of 18 and 23 vertices inside a truss of 26: tens of
# millions of cliques, minutes for an enumeration that visits each one)
@pytest.mark.parametrize("row", [r for r in TQ.TABLE if r[1] is None or r[1][0] <= 2000], ids=lambda r: "%s%s" % (r[0], r[1] or ""))
def test_maximum_table_of_the_suite_graphs(K, row):
    kind, args, omega, n_max, n_vertices, t_max = row
    if kind == "hand":
        nv, edges = R.hand_graph()
    elif kind == "cascade":
        nv, edges = 120, R.clique_union(120, 220, 2, 9, 1)
    else:
        nv, edges = args[0], TQ._canonical(K.gen_hug_edges(*args))
    got = _check_maximum(nv, edges, networkx=False)
    assert (got["omega"], got["n_max_cliques"], got["t_max"]) == (omega, n_max, t_max)
    assert int(np.count_nonzero(got["count"])) == n_vertices


# ---- (3,4)-nucleus decomposition and the k-nuclei

def _check_nucleus(nv, edges):
    rowptr, col, eu, ev = _graph(nv, edges)
    got = O.nucleus(rowptr, col)
    want = R.decompose(nv, eu, ev)
    for name in ("a", "b", "c", "key0", "theta", "edge_theta", "vertex_theta"):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), name
    assert got["info"] == want["info"]
    assert got["quads"].shape == (len(want["cliques"]), 4) and got["quads"].tolist() == [list(q) for q in want["cliques"]]
    return got, want


@pytest.mark.parametrize("i", range(len(TN.GRAPHS)))
def test_nucleus_random_graphs(built, i):
    nv, edges = TN.GRAPHS[i]
    got, _ = _check_nucleus(nv, edges)
    want = TN.brute_theta(nv, edges)                                              # and the definition itself
    tris = list(zip(got["a"].tolist(), got["b"].tolist(), got["c"].tolist()))
    assert tris == sorted(want) and got["theta"].tolist() == [want[t] for t in tris]


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_nucleus_hand_cases(built, case):
    name, nv, edges, n_tri, n_clq, counts = case
    got, _ = _check_nucleus(nv, edges)
    assert (got["info"]["n_triangles"], got["info"]["n_cliques4"]) == (n_tri, n_clq)
    assert dict(zip(*(x.tolist() for x in np.unique(got["theta"], return_counts=True)))) == counts


def test_nucleus_hand_graph_clique_union_and_empty_inputs(built):
    got, _ = _check_nucleus(*R.hand_graph())
    assert got["vertex_theta"].tolist() == [4, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1, 0, 0]
    got, _ = _check_nucleus(600, R.clique_union(600, 150, 4, 12, 11))
    assert (got["info"]["n_triangles"], got["info"]["n_cliques4"]) == (14223, 25839)
    for nv, edges in ((0, []), (5, []), (4, [(0, 1), (1, 2), (2, 3)])):           # no vertices, no edges, no triangle
        got, _ = _check_nucleus(nv, edges)
        assert got["info"] == {"n_triangles": 0, "n_cliques4": 0, "theta_max": -1, "n_levels": 0}
        assert got["edge_theta"].tolist() == [-1] * len(edges) and got["vertex_theta"].tolist() == [-1] * nv
        assert O.nuclei_labels(got["theta"], got["quads"], 1)[0].tolist() == []


def _check_nuclei(nv, edges):
    """The scipy helper at every k against the walk-up rule on nucleus_hierarchy_ref's forest, and the classes per level
    against the forest's nodes."""
    rowptr, col, eu, ev = _graph(nv, edges)
    got = O.nucleus(rowptr, col)
    h, dec = H.hierarchy(nv, eu, ev, theta=got["theta"])
    top = max(got["info"]["theta_max"], 0)
    classes = {}
    for k in range(1, top + 2):
        label, size = O.nuclei_labels(got["theta"], got["quads"], k)
        wl, ws = H.walk_up(h, dec["theta"], k)
        assert label.dtype == np.int32 and np.array_equal(label, wl) and np.array_equal(size, ws), k
        classes[k] = set(zip(label[label >= 0].tolist(), size[label >= 0].tolist()))
    assert classes[top + 1] == set()
    nodes = set(zip(h["k"].tolist(), h["rep"].tolist(), h["size"].tolist()))
    assert nodes == {(k, r, s) for k in range(1, top + 1) for r, s in classes[k] - classes[k + 1]}   # a node: a class of k, none of k + 1
    return got, h


@pytest.mark.parametrize("i", range(len(TN.GRAPHS)))
def test_nuclei_random_graphs(built, i):
    _check_nuclei(*TN.GRAPHS[i])


def test_nuclei_worked_examples(built):
    for nv, edges in ((4, R.clique(range(4))), (7, R.clique([0, 1, 2, 3, 4]) + R.clique([0, 1, 2, 5, 6])), H.two_k5_sharing_an_edge(),
                      H.k6_plus_vertex(), H.two_k6_joined_by_a_band(), R.hand_graph(), H.clique_chain(9), H.band(2000), H.disjoint_k4(50),
                      H.triangle_in_n_cliques(65), (600, R.clique_union(600, 150, 4, 12, 11)),
                      (0, []), (5, []), (4, [(0, 1), (1, 2), (2, 3)]), (4, [(0, 1), (1, 3), (0, 3)])):
        _check_nuclei(nv, edges)
    got, h = _check_nuclei(*H.two_k5_sharing_an_edge())                            # theta cannot tell these two apart: the classes do
    label, size = O.nuclei_labels(got["theta"], got["quads"], 2)
    assert sorted(set(label.tolist())) == [0, 3] and size.tolist() == [10] * 20


# ---- clique percolation: the subset method and the vectorised pivot rule against the all-pairs restatement

PERCOLATION_FIELDS = ("label", "size", "rep", "n_cliques", "offset", "verts", "n_comm", "first")
PERCOLATION_INFO = ("k", "n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap")
PERCOLATION_HUG = [(500, 1225, 2.6, 6), (600, 1200, 2.2, 11)]                      # 3 128 and 2 283 maximal cliques
PERCOLATION_CASCADE = (200, 90, 2, 9, 1)


def _check_percolation(nv, edges, networkx=True):
    """Every k from 2 to omega + 1 on the native list of the graph: every field of O.clique_communities against
    clique_communities_ref.solve, O.percolation_pair_tests against its pair_tests, the communities against networkx."""
    rowptr, col, _, _ = _graph(nv, edges)
    view = O.maximal_cliques(rowptr, col, 2)
    cliques = _tuples(view)
    if networkx:
        import networkx as nx
        from networkx.algorithms.community import k_clique_communities
        g = nx.Graph()
        g.add_nodes_from(range(nv))
        g.add_edges_from(R.canonical(edges))
    for k in range(2, view["omega"] + 2):
        got = O.clique_communities(nv, view["offset"], view["verts"], k)
        want = P.solve(nv, cliques, k)
        for name in PERCOLATION_FIELDS:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, k)
        for name in PERCOLATION_INFO:
            assert got[name] == want[name], (name, k)
        assert O.percolation_pair_tests(nv, view["offset"], view["verts"], k) == P.pair_tests(cliques, k), k
        if networkx:
            sets = sorted(tuple(got["verts"][got["offset"][c]:got["offset"][c + 1]].tolist()) for c in range(got["n_communities"]))
            assert sets == sorted(tuple(sorted(c)) for c in k_clique_communities(g, k)), k
    above = O.clique_communities(nv, view["offset"], view["verts"], view["omega"] + 1)
    assert (above["n_member_cliques"], above["n_communities"], above["largest"], above["n_covered"], above["n_overlap"]) == (0,) * 5
    assert above["label"].tolist() == [-1] * len(cliques) and above["offset"].tolist() == [0] and above["first"].tolist() == [-1] * nv
    assert O.percolation_pair_tests(nv, view["offset"], view["verts"], view["omega"] + 1) == 0
    return view


@pytest.mark.parametrize("i", range(2), ids=lambda i: "nv %d" % PERCOLATION_HUG[i][0])
def test_percolation_power_law_graphs(K, i):
    nv = PERCOLATION_HUG[i][0]
    view = _check_percolation(nv, TQ._canonical(K.gen_hug_edges(*PERCOLATION_HUG[i])))
    assert view["n_cliques"] == (3128, 2283)[i]


@pytest.mark.parametrize("name", sorted(P.HAND_GRAPHS))
def test_percolation_hand_graphs(built, name):
    nv, edges = P.HAND_GRAPHS[name]
    view = _check_percolation(nv, edges)
    for gname, k, n_comm, tests in P.HAND_TABLE:
        if gname == name:
            assert O.clique_communities(nv, view["offset"], view["verts"], k)["n_communities"] == n_comm
            assert O.percolation_pair_tests(nv, view["offset"], view["verts"], k) == tests


def test_percolation_cascade_of_random_cliques(built):
    view = _check_percolation(PERCOLATION_CASCADE[0], R.clique_union(*PERCOLATION_CASCADE))
    assert O.clique_communities(PERCOLATION_CASCADE[0], view["offset"], view["verts"], 3)["n_overlap"] > 0


def test_percolation_empty_list_and_arguments(built):
    for nv in (0, 5):
        for k in (2, 3):
            got = O.clique_communities(nv, np.zeros(1, np.int64), np.zeros(0, np.int32), k)
            want = P.solve(nv, [], k)
            for name in PERCOLATION_FIELDS:
                assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
            for name in PERCOLATION_INFO:
                assert got[name] == want[name], name
            assert O.percolation_pair_tests(nv, np.zeros(1, np.int64), np.zeros(0, np.int32), k) == 0
    for call in (O.clique_communities, O.percolation_pair_tests):
        with pytest.raises(ValueError):
            call(4, np.asarray([0, 2]), np.asarray([0, 1], np.int32), 1)


# ---- one recorded run

def test_recorded_totals_of_a_power_law_graph(K):
    """gen_hug_edges(50000, 122500, 2.6, 42): 502 700 edges, omega = 16 and these k-clique totals, from an enumeration written
    once for this purpose over std::set_intersection (3.34 M cliques).  The other two references must agree with the census
    where their outputs overlap."""
    nv = 50000
    rowptr, col = O.simplify(nv, K.gen_hug_edges(nv, 122500, 2.6, 42))
    assert len(col) // 2 == 502700
    raw = O.clique_counts(rowptr, col, 3)
    want = [502700, 601248, 447974, 356346, 359629, 365631, 311454, 212731, 115601, 49496, 16410, 4076, 713, 78, 4]
    assert raw["clique_number"] == 16 and raw["total"][2:17].tolist() == want and not raw["total"][17:].any()
    assert raw["nodes"] == sum(want)                                               # every clique was visited, none closed by binomials
    assert int(raw["local"].sum()) == 3 * want[1]
    nuc = O.nucleus(rowptr, col)
    assert (nuc["info"]["n_triangles"], nuc["info"]["n_cliques4"]) == (want[1], want[2])
    tri_at = np.bincount(np.concatenate([nuc["a"], nuc["b"], nuc["c"]]), minlength=nv)
    assert np.array_equal(tri_at.astype(np.uint64), raw["local"])
    mx = O.maximal_cliques_all(rowptr, col, 2)
    assert mx["omega"] == 16 and int(mx["hist_all"][16]) == want[-1] and int(mx["hist_all"][2:].sum()) == mx["n_cliques"]
    assert int(mx["count"].sum()) == int((np.arange(len(mx["hist_all"])) * mx["hist_all"]).sum())
