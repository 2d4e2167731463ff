"""Mid-size GPU tests of the three analyses that tests/test_gpu_midsize.py left out: the biconnected components, the k-clique
communities (with the maximal-clique list above the default MAXIMAL_LIST) and the densest-subgraph search, at the sizes where
their size-dependent paths run together on one graph that a reference can still check.  Every comparison is exact equality of
whole integer arrays and of every integer info field.

The references: tests/biconnected_ref.py (Hopcroft-Tarjan with an edge stack, in Python) and tests/densest_ref.py as they are;
for the percolation oracle.clique_communities and oracle.percolation_pair_tests (every (k - 1)-subset of every clique, numbered
by np.unique, and the components of the clique -- subset graph: no pivots, no pair of cliques), which
tests/test_oracle_cliques.py ties to the all-pairs restatement and to networkx; for the cliques themselves the pivot-free
orc_maximal_cliques.  The block tree (tests/block_tree.py) brings a closed form of its own.

One context and one k-truss run per graph, shared by its tests and never changed; trussness is the library's own, asserted equal
to the oracle's once per graph (test_gpu_midsize.Graph).  A reference is computed once per (graph, k) and shared.

The graphs (m edges; seconds are the reference's CPU time on one thread, as printed by the run RECORDED is from):
  G100  gen_hug_edges(100000, 245000, 2.6, 42): m 1 007 422, largest degree 7 059 (rows of >= 2048 entries go to the workgroup
        walk of k_bc_bfs amid ordinary rows on one frontier, and low[] / high[] are contended on the hubs), t_max 19.
        Biconnected at k = 2, 3, 4 and max, k = 2 again with BICONN_HEAVY = 0 and under POISON: one giant block of 1 005 703 edges
        across every tile of the counting passes beside 1 695 small ones.  Reference: 0.90, 0.78 and 0.66 s at k = 2, 3, 4.
  G50   gen_hug_edges(50000, 122500, 2.6, 42): m 502 700, 204 551 maximal cliques (755 132 words, omega 16): the first list above
        65 536 cliques that is compared, then the percolation at k = 2, 3, 4, 6, 7, 12, 16 and 17 (above omega: nothing): walks
        that start behind the clique in the long rows of the hubs, 10^7 .. 10^9 pair tests, a class of 142 337 cliques at k = 3
        that merges while the walks run.  Reference: orc_maximal_cliques 0.75 s, the percolation 1.63 s for the slowest k (7).
  G50 under a vmask (coreness >= half the largest): biconnected at k = 2, 3, max; the percolation at k = 3, 5, omega on the
        list of maximal_cliques_run(3) (119 589 cliques).  References on the induced subgraph, mapped back: at most 1.13 s each.
  GRID  725 x 725, ids permuted by default_rng(7): m 1 049 800, one block of all edges (every tile of k_bc_edge_blocks adds
        to the LDS partial sum of its first class), a forest of 836 levels.  Reference: 2.10 s.
  TREE  block_tree(**FULL): 576 730 vertices, m 774 542, 6 243 blocks, three of them of 81 333, 85 333 and 93 333 edges -- more
        than 300 tiles each, so a class that is not a workgroup's first crosses many tiles --, 240 rings of 100 .. 5 000 and
        6 000 of 3 .. 30 vertices; no bridge, a forest of 134 levels.  Against the reference (1.64 s) and the closed form.
  ALL   G50, GRID and TREE side by side, ids interleaved: 1 152 355 vertices, m 2 327 042; several roots of the forest, their
        preorder intervals from one cursor.  Reference: 4.58 s.
  HUBS  G(60 000, 900 000) by default_rng(3) with 60 000 more edges among its first 3 000 vertices and four hubs of degree
        exactly 2047, 2048, 2049 and 9000 behind it: k_prune 21, |P| 57 550 > 20 480 (the rounds cannot run in LDS: all three
        settings of DENSEST_LOCAL take the grid), 928 302 pairs; the best core at 0 and 1 rounds, a denser prefix from 7 on.
        Reference: 0.45 s for the four numbers of rounds together.
  K_4096, K_4097: k_max 4095 / 4096, the last profile with LDS histograms and the first without (DenHist<false>); no k-truss
        run on them.  Reference: 0.72 s per graph.

The percolation at k = 2 on G50 (1 130 824 618 pair tests, within the default budget of 2^32) took 57.7 ms on an MI355X, so
the case is kept (test_percolation_g50_k2).  The profile of K_4097 took 95 ms against 0.34 ms for K_4096: without the LDS
histograms every entry of the graph adds to one of two words of global memory.

RECORDED holds what the library reported on an MI355X beyond the contract (depth is fixed by the graph and asserted against
the reference; ms is not asserted)."""
import numpy as np
import pytest

import biconnected_ref as R
import block_tree as BT
import densest_ref as D
import test_gpu_biconnected as TB
import test_gpu_clique_communities as TC
import test_gpu_densest as TD
from oracle import oracle as O
from test_gpu_midsize import HUG, Graph, _set

pytestmark = pytest.mark.gpu

KMAX = -1
MAXIMAL_LIST = "262144"
GRID = 725
LDS_PAIRS = 160 * 1024 // 4 // 2                          # |P| above this: loads and deltas of the local path do not fit LDS
POISON = {"POISON": "0xFFFFFFFF"}

# as printed by a run of this file with -s on an MI355X, default options
RECORDED = {
    "G100": {"biconnected": {2: {"depth": 7, "ms": 12.70}, 3: {"depth": 6, "ms": 11.57}, 4: {"depth": 6, "ms": 11.72}, 19: {"depth": 2, "ms": 0.36}}},
    "G50 vmask": {"biconnected": {2: {"depth": 5, "ms": 12.76}, 3: {"depth": 5, "ms": 10.31}, 17: {"depth": 3, "ms": 0.33}},
                  "maximal": {"max_candidates": 618, "nodes": 451377, "ms": 36.02},
                  "percolation": {3: {"pair_tests": 378750767, "ms": 38.29}, 5: {"pair_tests": 61338535, "ms": 26.13}, 16: {"pair_tests": 2, "ms": 0.70}}},
    "GRID": {"biconnected": {2: {"depth": 836, "ms": 36.71}}},
    "TREE": {"biconnected": {2: {"depth": 134, "ms": 10.49}}},
    "ALL": {"biconnected": {2: {"depth": 836, "ms": 41.65}}},
    "G50": {"maximal": {"max_candidates": 662, "nodes": 826108, "ms": 64.83},
            "percolation": {2: {"pair_tests": 1130824618, "ms": 57.67}, 3: {"pair_tests": 432433457, "ms": 45.46},
                            4: {"pair_tests": 166535918, "ms": 51.69}, 6: {"pair_tests": 28042302, "ms": 21.23},
                            7: {"pair_tests": 12085839, "ms": 6.64}, 12: {"pair_tests": 64291, "ms": 1.40},
                            16: {"pair_tests": 2, "ms": 0.80}, 17: {"pair_tests": 0, "ms": 0.004}}},
    "HUBS": {"densest ms": {0: 0.19, 1: 0.61, 7: 0.86, 64: 3.06}},
    "K_4096": {"densest ms": {0: 0.34, 1: 3.20, 2: 3.49}},
    "K_4097": {"densest ms": {0: 95.43, 1: 98.68, 2: 98.85}},
}


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _graph(K, name, nv, uv, **kw):
    graph = Graph(K, name, nv, uv, **kw)
    graph.bc = {}
    graph.perc = {}
    yield graph
    graph.close()


@pytest.fixture(scope="module")
def g100(K):
    yield from _graph(K, "G100", HUG["G100"][0], K.gen_hug_edges(*HUG["G100"]))


@pytest.fixture(scope="module")
def g50(K):
    yield from _graph(K, "G50", HUG["G50"][0], K.gen_hug_edges(*HUG["G50"]))


@pytest.fixture(scope="module")
def masked(K):
    yield from _graph(K, "G50 vmask", HUG["G50"][0], K.gen_hug_edges(*HUG["G50"]), masked=True)


def grid_edges():
    nv = GRID * GRID
    ids = np.random.default_rng(7).permutation(nv).reshape(GRID, GRID)
    return nv, np.concatenate([np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1), np.stack([ids[:-1].ravel(), ids[1:].ravel()], 1)]).astype(np.int64)


@pytest.fixture(scope="module")
def grid(K):
    yield from _graph(K, "GRID", *grid_edges())


@pytest.fixture(scope="module")
def tree(K):
    t = BT.block_tree(**BT.FULL)
    for graph in _graph(K, "TREE", t["nv"], t["uv"]):
        graph.t = t
        yield graph


def interleave(parts):
    """Disjoint parts (nv, uv) in one graph: the vertices of every part spread evenly over the whole id range."""
    sizes = [nv for nv, _ in parts]
    frac = np.concatenate([(np.arange(nv) + 0.5) / nv for nv in sizes])
    ids = np.empty(len(frac), np.int64)
    ids[np.argsort(frac, kind="stable")] = np.arange(len(frac))
    first = np.concatenate([[0], np.cumsum(sizes)])
    return int(first[-1]), np.concatenate([ids[uv + first[i]] for i, (_, uv) in enumerate(parts)])


@pytest.fixture(scope="module")
def everything(K):
    t = BT.block_tree(**BT.FULL)
    hug = np.asarray(K.gen_hug_edges(*HUG["G50"]), np.int64).reshape(-1, 2)
    for graph in _graph(K, "ALL", *interleave([(HUG["G50"][0], hug), grid_edges(), (t["nv"], t["uv"])])):
        graph.m_parts = (502700, 2 * GRID * (GRID - 1), len(t["uv"]))
        yield graph


# ---- biconnected components

def bc_want(g, k):
    """The reference at threshold k (as resolved) on g's k-truss result, once per graph."""
    import time
    kk = TB._resolve(k, g.tr)
    if kk not in g.bc:
        t0 = time.perf_counter()
        g.bc[kk] = R.biconnected(g.nv, g.eu, g.ev, g.tr, kk)
        g.bc[kk]["seconds"] = time.perf_counter() - t0
    return kk, g.bc[kk]


def check_biconnected(g, k):
    """One run at threshold k: every array of the three fetches, every info field and the count against the reference, and
    the invariants of the block-cut forest from the library's outputs alone."""
    kk, want = bc_want(g, k)
    got = TB._fetch_all(g.a, k)
    info = got["info"]
    print("%s biconnected k %d: %s; reference %.2f s" % (g.name, k, info, want["seconds"]))
    for name in ("block", "size", "n_blocks", "ecc_label", "ecc_size"):
        assert got[name].dtype == np.int32 and len(got[name]) == len(want[name]), (name, k)
        assert np.array_equal(got[name], want[name]), (name, k)
    for name in ("rep", "n_edges", "n_verts"):
        assert got["blocks"][name].dtype == np.int32 and np.array_equal(got["blocks"][name], want["blocks"][name]), (name, k)
    assert tuple(info[x] for x in TB.INFO) == (kk,) + R.summary(want), k
    assert info["ms"] >= 0.0 and got["count"] == want["info"]["n_blocks"]
    TB._invariants(g.a, k, got)
    return got


@pytest.mark.parametrize("k", [2, 3, 4, KMAX], ids=["k 2", "k 3", "k 4", "k max"])
def test_biconnected_g100(g100, k):
    got = check_biconnected(g100, k)
    if k == 2:
        assert len(g100.eu) == 1007422 and int(np.diff(g100.lib_rowptr).max()) == 7059 >= 2048
        assert got["info"]["n_member_edges"] > 2048 * 256 and got["info"]["largest_block"] == 1005703
    if k == KMAX:
        assert got["info"]["k_used"] == g100.tmax == 19


@pytest.mark.parametrize("opts", [{"BICONN_HEAVY": "0"}, POISON], ids=["heavy 0", "poison"])
def test_biconnected_g100_options(g100, monkeypatch, opts):
    """BICONN_HEAVY = 0: every row of the BFS through its wave, the hubs' through the workgroup."""
    _set(monkeypatch, opts)
    check_biconnected(g100, 2)


@pytest.mark.parametrize("k", [2, 3, KMAX], ids=["k 2", "k 3", "k max"])
def test_biconnected_g50_under_a_vmask(masked, k):
    assert 0 < len(masked.inv) < masked.nv and 0 < len(masked.eu) < 502700
    check_biconnected(masked, k)


def test_biconnected_grid(grid):
    got = check_biconnected(grid, 2)
    m = 2 * GRID * (GRID - 1)
    info = got["info"]
    assert m == 1049800 == len(grid.eu) and (info["n_blocks"], info["n_bridges"], info["n_articulation"], info["largest_block"]) == (1, 0, 0, m)
    assert got["blocks"]["rep"].tolist() == [0] and got["blocks"]["n_verts"].tolist() == [GRID * GRID]
    assert info["depth"] == 836 >= GRID                  # (the root is wherever the permutation put id 0; no vertex sees all others in fewer than GRID levels)


def test_biconnected_block_tree(tree):
    got = check_biconnected(tree, 2)
    want = BT.closed_form(tree.t)
    for name, value in want["info"].items():
        assert got["info"][name] == value, name
    assert np.array_equal(BT.sorted_pairs(got["blocks"]["n_edges"], got["blocks"]["n_verts"]), want["pairs"])
    assert np.array_equal(np.sort(got["blocks"]["n_edges"]), want["n_edges"]) and np.array_equal(np.sort(got["blocks"]["n_verts"]), want["n_verts"])
    assert np.array_equal(got["n_blocks"], want["n_blocks"]) and np.array_equal(np.flatnonzero(got["n_blocks"] >= 2), want["articulation"])
    assert int((want["n_edges"] > 256 * 300).sum()) >= 3 and want["info"]["n_member_edges"] > 2048 * 256
    assert (got["ecc_label"] == 0).all() and (got["ecc_size"] == tree.nv).all()


def test_biconnected_disjoint_parts_with_interleaved_ids(everything):
    got = check_biconnected(everything, 2)
    assert len(everything.eu) == sum(everything.m_parts) == got["info"]["n_member_edges"]
    assert got["info"]["largest_block"] == everything.m_parts[1]                          # the grid's one block
    a = everything.a
    a.components_run("truss", 2)
    assert a.components_info()["n_components"] > 2       # several roots of the forest


# ---- the maximal-clique list above 65 536 cliques, and the k-clique communities on it

def _list_cliques(g, monkeypatch, k_min):
    """maximal_cliques_run(k_min) with a list that holds every clique, asserted equal to the oracle's list; (offset, verts) in
    original ids.  Once per graph: the list stays on the context (no other test of this file runs the cliques on it)."""
    if "list" not in g.perc:
        _set(monkeypatch, {"MAXIMAL_LIST": MAXIMAL_LIST})
        g.a.maximal_cliques_run(k_min)
        info = g.a.maximal_cliques_info()
        want = g.view(k_min)
        print("%s maximal cliques k_min %d: %s; oracle %.2f s" % (g.name, k_min, info, g.maximal_all()["seconds"]))
        assert info["flags"] == 3 and info["n_cliques"] == want["n_cliques"] and info["omega"] == want["omega"]
        offset, verts = g.a.maximal_cliques_list()
        assert offset.dtype == np.int64 and np.array_equal(offset, want["offset"])
        assert verts.dtype == np.int32 and np.array_equal(verts, g.inv[want["verts"]])
        g.perc["list"] = (want["offset"], g.inv[want["verts"]].astype(np.int32), want["omega"])
    return g.perc["list"]


def perc_want(g, k):
    """The references of one k on g's list (the ORACLE's list), once per graph."""
    import time
    if k not in g.perc:
        offset, verts, _ = g.perc["list"]
        t0 = time.perf_counter()
        want = O.clique_communities(g.nv, offset, verts, k)
        g.perc[k] = (want, O.percolation_pair_tests(g.nv, offset, verts, k), time.perf_counter() - t0)
    return g.perc[k]


def check_percolation(g, k, budget=0):
    want, tests, seconds = perc_want(g, k)
    g.a.clique_communities_run(k, budget)
    print("%s clique communities k %d: %s; reference %.2f s" % (g.name, k, g.a.clique_communities_info(), seconds))
    return TC._compare(g.a, want, tests)


def test_maximal_clique_list_above_the_default(g50, monkeypatch):
    offset, verts, omega = _list_cliques(g50, monkeypatch, 2)
    assert len(offset) - 1 == 204551 > 65536 and len(verts) == 755132 and omega == 16


@pytest.mark.parametrize("k", [3, 4, 6, 7, 12, 16, 17])
def test_percolation_g50(g50, monkeypatch, k):
    _list_cliques(g50, monkeypatch, 2)
    info = check_percolation(g50, k)
    if k == 3:
        assert info["n_member_cliques"] > 65536
    if k == 17:                                          # above omega: nothing
        assert (info["n_member_cliques"], info["n_communities"], info["largest"], info["n_covered"], info["pair_tests"]) == (0,) * 5


def test_percolation_g50_k2(g50, monkeypatch):
    """1.13 x 10^9 pair tests, within the default budget of 2^32; nearly every clique ends in one class."""
    _list_cliques(g50, monkeypatch, 2)
    info = check_percolation(g50, 2)
    assert info["pair_tests"] > 10 ** 9 and info["n_overlap"] == 0


@pytest.mark.parametrize("opts", [{"PERC_GROUP": "4"}, {"PERC_GROUP": "16"}, {"PERC_GROUP": "64"}, POISON],
                         ids=["group 4", "group 16", "group 64", "poison"])
def test_percolation_g50_options(g50, monkeypatch, opts):
    _list_cliques(g50, monkeypatch, 2)
    _set(monkeypatch, opts)
    check_percolation(g50, 4)


def test_percolation_budget_at_mid_size(g50, K, monkeypatch):
    """budget = pair_tests succeeds; one less answers KOMB_ERR_LIMIT and leaves the previous result in place."""
    _list_cliques(g50, monkeypatch, 2)
    before = check_percolation(g50, 6)
    want7, tests7, _ = perc_want(g50, 7)
    assert tests7 > 10 ** 7
    assert TC._code(K, lambda: g50.a.clique_communities_run(7, tests7 - 1)) == K._lib.KOMB_ERR_LIMIT
    want6, tests6, _ = perc_want(g50, 6)
    assert TC._compare(g50.a, want6, tests6) == before
    assert check_percolation(g50, 7, tests7)["pair_tests"] == tests7


def test_percolation_results_replace_each_other_and_repeat(g50, monkeypatch):
    _list_cliques(g50, monkeypatch, 2)
    a = g50.a
    check_percolation(g50, 3)
    first = a.clique_communities_fetch() + a.clique_communities_fetch_communities() + a.clique_communities_fetch_vertices()
    n_comm = first[6]
    _, count, largest = a.maximal_cliques_fetch()
    assert np.array_equal(n_comm >= 1, largest >= 3) and (n_comm <= count).all()      # in a community: in a clique of >= 3 vertices
    check_percolation(g50, 12)                           # another k replaces the result
    assert a.clique_communities_info()["k"] == 12 and a.clique_communities_count()[0] == perc_want(g50, 12)[0]["n_communities"]
    check_percolation(g50, 3)                            # and k = 3 again: bit-equal, whatever the schedule of the links was
    again = a.clique_communities_fetch() + a.clique_communities_fetch_communities() + a.clique_communities_fetch_vertices()
    assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(first, again))


@pytest.mark.parametrize("k", [3, 5, "omega"])
def test_percolation_g50_under_a_vmask(masked, monkeypatch, k):
    offset, verts, omega = _list_cliques(masked, monkeypatch, 3)
    assert omega == 16 and int(np.diff(offset).min()) >= 3 and not np.array_equal(verts, masked.view(3)["verts"])
    info = check_percolation(masked, omega if k == "omega" else k)
    assert info["k_min"] == 3 and info["n_communities"] > 0


# ---- densest subgraph

def _densest_runs(a, case, monkeypatch, name, iters_list, local):
    if local is None:
        monkeypatch.delenv("KOMB_DENSEST_LOCAL", raising=False)
    else:
        monkeypatch.setenv("KOMB_DENSEST_LOCAL", local)
    for iters in iters_list:
        a.densest_subgraph_run(iters)
        got = TD._fetch_all(a)
        print("%s densest, DENSEST_LOCAL %s, iters %d: %s" % (name, local, iters, a.densest_subgraph_info()))
        TD._same(got, case.ref(iters), (name, local, iters))


def hub_edges():
    rng = np.random.default_rng(3)
    n = 60000
    parts = [rng.integers(0, n, (900000, 2)), rng.integers(0, 3000, (60000, 2))]
    for h, d in enumerate(HUB_DEGREES):
        parts.append(np.stack([np.full(d, n + h), rng.choice(n, d, replace=False)], 1))
    return n + len(HUB_DEGREES), np.concatenate(parts).astype(np.int64)


HUB_DEGREES = (2047, 2048, 2049, 9000)                    # around kDenHeavy = 2048: k_den_rows decides on the full row


@pytest.fixture(scope="module")
def hubs(K):
    nv, uv = hub_edges()
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        case = TD._Case(a)
        rowptr, col = O.simplify(nv, uv)
        assert np.array_equal(case.rowptr, rowptr) and np.array_equal(case.col, col) and np.array_equal(case.core, O.coreness(rowptr, col))
        yield case


@pytest.mark.parametrize("local", [None, "0", "1"], ids=["auto", "local 0", "local 1"])
def test_densest_hubs(hubs, monkeypatch, local):
    import time
    t0 = time.perf_counter()
    want = {iters: hubs.ref(iters) for iters in (0, 1, 7, 64)}
    print("HUBS reference: %.2f s for the four" % (time.perf_counter() - t0))
    assert np.diff(hubs.rowptr)[-4:].tolist() == list(HUB_DEGREES)
    assert want[64]["n_pruned"] > LDS_PAIRS == 20480 and (hubs.core[-4:] >= want[64]["k_prune"]).all()      # (the hubs are in P)
    assert (want[1]["source"], want[7]["source"]) == (D.SOURCE_CORE, D.SOURCE_PREFIX)      # both outcomes of the final decision
    assert want[0]["load_max"] == 0 < want[1]["load_max"] < want[7]["load_max"]
    _densest_runs(hubs.a, hubs, monkeypatch, "HUBS", (0, 1, 7, 64), local)


@pytest.mark.parametrize("n", [4096, 4097])
def test_densest_complete_graphs_around_the_lds_histograms(K, monkeypatch, n):
    """k_max + 1 = n bins: 4096 is the last profile with its two histograms in LDS, 4097 the first that adds to global memory."""
    import time
    col = np.ascontiguousarray(np.broadcast_to(np.arange(n, dtype=np.int32), (n, n))[~np.eye(n, dtype=bool)])
    rowptr = np.arange(n + 1, dtype=np.int64) * (n - 1)
    with K.KombAccel() as a:
        a.from_csr(rowptr, col)
        case = TD._Case(a)
        assert (case.core == n - 1).all() and len(case.col) == n * (n - 1)
        t0 = time.perf_counter()
        want = {iters: case.ref(iters) for iters in (0, 1, 2)}
        print("K_%d reference: %.2f s for the three" % (n, time.perf_counter() - t0))
        m = n * (n - 1) // 2
        for iters in (0, 1, 2):
            w = want[iters]
            assert (w["k_max"], w["k_best"], w["source"], w["n_sub"], w["m_sub"]) == (n - 1, n - 1, D.SOURCE_CORE, n, m)
            assert w["n_k"].tolist() == [n] * n and w["m_k"].tolist() == [m] * n                 # single steps
        _densest_runs(a, case, monkeypatch, "K_%d" % n, (0, 1, 2), None)
