"""GPU tests of komb_clique_census_run / _fetch / _info: every complete result -- the window as used, t_max, omega, flags, every
total and every local count -- is compared exactly with the restatement of tests/clique_census_ref.py, which is fed the
library's own run_truss() edge list (whose parity other tests own).  A result the budget cut short is checked against the
closed form as a lower bound."""
from math import comb

import numpy as np
import pytest

import clique_census_ref as C
import nucleus_ref as R

pytestmark = pytest.mark.gpu

SAT = 2 ** 64 - 1
LDS = [{}, {"CENSUS_LDS": "0"}, {"CENSUS_LDS": "64"}]
LDS_IDS = ["lds default", "lds 0", "lds 64"]
PIVOT = [{}, {"CENSUS_PIVOT": "first"}]
PIVOT_IDS = ["pivot max", "pivot first"]
WINDOWS = [(2, -1), (4, -1), (3, 5)]


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


_WANT = {}


def _want(key, nv, eu, ev, tr, k_lo, k_hi, k_local, own_truss=True):
    """The restatement of one census of one k-truss result, computed once per module and never changed."""
    truss = None if own_truss else tr
    if key is None:
        return C.census(nv, eu, ev, k_lo, k_hi, k_local, truss=truss)
    key = (key, k_lo, k_hi, k_local)
    if key not in _WANT:
        _WANT[key] = (eu.copy(), ev.copy(), C.census(nv, eu, ev, k_lo, k_hi, k_local, truss=truss))
    seu, sev, want = _WANT[key]
    assert np.array_equal(seu, eu) and np.array_equal(sev, ev)
    return want


def _compare(a, want):
    info = a.clique_census_info()
    for name in ("k_lo", "k_hi", "k_local", "t_max", "omega", "flags"):
        assert info[name] == want[name], name
    total, local = a.clique_census_fetch()
    assert total.dtype == np.uint64 and np.array_equal(total, want["total"])
    if want["k_local"]:
        assert local.dtype == np.uint64 and len(local) == max(a.nv, 0) and np.array_equal(local, want["local"])
        if not want["flags"] & C.SATURATED:
            assert sum(local.tolist()) == want["k_local"] * int(total[want["k_local"] - want["k_lo"]])
    else:
        assert local is None
    assert info["nodes"] >= 0 and info["n_roots"] >= 0 and info["ms"] >= 0.0 and 0 <= info["max_candidates"] <= 4096
    return info


def _check(a, k_lo=2, k_hi=-1, k_local=0, key=None, own_truss=True, edges=None, budget=0):
    """One census of the k-truss result the context holds (edges: what run_truss returned) against the restatement."""
    eu, ev, tr = edges
    a.clique_census_run(k_lo, k_hi, k_local, budget)
    return _compare(a, _want(key, a.nv, eu, ev, tr, k_lo, k_hi, k_local, own_truss))


def _check_windows(a, vmask=None, key=None, own_truss=True, windows=WINDOWS):
    """k-truss (whole graph or vmask), then every window with k_local in {0, k_lo, k_hi as used}."""
    edges = a.run_truss(vmask)
    t_max = int(edges[2].max()) if len(edges[2]) else 0
    for k_lo, k_hi in windows:
        used = max(k_lo, t_max if k_hi == -1 else min(k_hi, t_max))
        for k_local in sorted({0, k_lo, used}):
            _check(a, k_lo, k_hi, k_local, key, own_truss, edges)
    return edges


def _load(K, nv, uv):
    a = K.KombAccel()
    a.from_edges(nv, _i64(uv))
    return a


def _set(monkeypatch, *opts):
    for o in opts:
        for k, v in o.items():
            monkeypatch.setenv("KOMB_" + k, v)


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_degenerate_graphs(K):
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))                                        # the empty graph is not an error
        _check_windows(a)
        total, local, info = a.run_clique_census(2, -1, 2)
        assert total.tolist() == [0] and local.tolist() == []
        assert (info["k_hi"], info["t_max"], info["omega"], info["flags"], info["nodes"]) == (2, 0, 0, 1, 0)
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges
        _check_windows(a)
        total, local, info = a.run_clique_census(2, 9, 2)
        assert total.tolist() == [0] and local.tolist() == [0] * 7 and (info["k_hi"], info["omega"], info["flags"]) == (2, 0, 1)
        a.from_edges(6, [[0, 1], [1, 2], [2, 3], [3, 4], [1, 5]])                # a path: five 2-cliques
        _check_windows(a)
        total, local, info = a.run_clique_census(2, -1, 2)
        assert total.tolist() == [5] and local.tolist() == [1, 3, 2, 2, 1, 1] and (info["omega"], info["flags"]) == (2, 1)
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        _check_windows(a, vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        assert a.run_clique_census()[0].tolist() == [0]
        a.from_edges(4, [[0, 1], [1, 3], [0, 3]])                                # one triangle (and an isolated vertex)
        _check_windows(a)
        total, local, info = a.run_clique_census(2, -1, 3)
        assert total.tolist() == [3, 1] and local.tolist() == [1, 1, 0, 1] and (info["omega"], info["t_max"]) == (3, 3)


@pytest.mark.parametrize("pivot", PIVOT, ids=PIVOT_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
@pytest.mark.parametrize("n", [2, 3, 5, 40, 66, 130])
def test_complete_graphs(K, monkeypatch, n, lds, pivot):
    """K_n against C(n, k): K_66 and K_130 have candidate sets of one and two words and a bit, and K_130 saturates."""
    _set(monkeypatch, lds, pivot)
    with _load(K, n, R.clique(range(n))) as a:
        edges = a.run_truss()
        k_local = max(n // 2, 2)
        info = _check(a, 2, -1, k_local, ("K", n), n < 100, edges)
        total, local = a.clique_census_fetch()
        assert total.tolist() == [min(comb(n, k), SAT) for k in range(2, n + 1)]
        assert local.tolist() == [min(comb(n - 1, k_local - 1), SAT)] * n
        assert (info["omega"], info["t_max"], info["flags"], info["max_candidates"]) == (n, n, 3 if n == 130 else 1, n - 2)


@pytest.mark.parametrize("pivot", PIVOT, ids=PIVOT_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
def test_k70_saturates_in_the_middle(K, monkeypatch, lds, pivot):
    _set(monkeypatch, lds, pivot)
    n = 70
    with _load(K, n, R.clique(range(n))) as a:
        edges = a.run_truss()
        info = _check(a, 2, -1, 35, ("K", n), True, edges)
        total, local = a.clique_census_fetch()
        assert info["flags"] == 3 and info["omega"] == n
        assert total.tolist() == [min(comb(n, k), SAT) for k in range(2, n + 1)]
        assert [k for k in range(2, n + 1) if int(total[k - 2]) == SAT] == list(range(28, 43))
        assert local.tolist() == [SAT] * n
        info = _check(a, 60, -1, 66, ("K", n), True, edges)                      # nothing saturates up here
        assert info["flags"] == 1 and a.clique_census_fetch()[1].tolist() == [comb(n - 1, 65)] * n


def test_k515_in_global_scratch_through_the_filter(K):
    """K_515, k_lo = k_hi = 514: candidate sets of up to 513 (the bit matrix in global scratch whatever CENSUS_LDS says), three
    roots that can reach 514 vertices, 515 cliques of 514."""
    n = 515
    with _load(K, n, R.clique(range(n))) as a:
        edges = a.run_truss()
        info = _check(a, 514, 514, 514, ("K", n), False, edges)
        total, local = a.clique_census_fetch()
        assert total.tolist() == [515] and local.tolist() == [514] * n and info["max_candidates"] == 513
        info = _check(a, 515, -1, 0, ("K", n), False, edges)
        assert a.clique_census_fetch()[0].tolist() == [1] and info["omega"] == 515


@pytest.mark.parametrize("pivot", PIVOT, ids=PIVOT_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
@pytest.mark.parametrize("m", [6, 12])
def test_cocktail_party_in_full(K, monkeypatch, m, lds, pivot):
    _set(monkeypatch, lds, pivot)
    nv, edges = C.cocktail_party(m)
    with _load(K, nv, edges) as a:
        _check_windows(a, key=("CP", m))
        total, local, info = a.run_clique_census(2, -1, m)
        assert total.tolist() == [comb(m, k) * 2 ** k for k in range(2, 2 * m - 1)]
        assert local.tolist() == [2 ** (m - 1)] * nv and (info["omega"], info["t_max"], info["flags"]) == (m, 2 * m - 2, 1)


def test_hand_graph_its_reversed_labelling_and_a_vmask(K):
    nv, edges = R.hand_graph()
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        with _load(K, nv, ids[_i64(edges)]) as a:
            _check_windows(a)
            total, local, info = a.run_clique_census(2, -1, 7)
            assert info["omega"] == 7 and int(total[-1]) == 1 and local[ids].tolist() == [1] * 7 + [0] * 8
            _check_windows(a, vmask=(np.arange(nv) != ids[0]).astype(np.uint8))  # without a K_7 vertex: a K_6 is left
            assert a.run_clique_census()[2]["omega"] == 6


HUG = [(300, 735, 2.6, 6), (2000, 4900, 2.2, 11)]


@pytest.mark.parametrize("i", range(2), ids=lambda i: "nv %d" % HUG[i][0])
def test_power_law_graphs(K, monkeypatch, i):
    nv = HUG[i][0]
    with K.KombAccel() as a:
        a.from_edges(nv, K.gen_hug_edges(*HUG[i]))
        _check_windows(a, key=("hug", nv))
        if nv == 2000:
            _set(monkeypatch, {"CENSUS_LDS": "0", "CENSUS_PIVOT": "first"})
            _check_windows(a, key=("hug", nv), windows=WINDOWS[:1])
            monkeypatch.delenv("KOMB_CENSUS_LDS")
            monkeypatch.delenv("KOMB_CENSUS_PIVOT")
            core = a.run_core()[1]
            _check_windows(a, vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8), key=("hug, vmask", nv))


def test_cascade_of_random_cliques(K):
    with _load(K, 120, R.clique_union(120, 220, 2, 9, 1)) as a:
        _check_windows(a, key="cascade")
        assert a.run_clique_census()[2]["omega"] == 11


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            eu, ev, _ = _check_windows(a)
            assert (eu.tolist(), ev.tolist()) == (g["eu"], g["ev"]), g["name"]
            eu, ev, _ = _check_windows(a, vmask=np.asarray(g["maxcore_mask"], np.uint8))
            assert (eu.tolist(), ev.tolist()) == (g["sub_eu"], g["sub_ev"]), g["name"]


@pytest.mark.parametrize("graph", ["hug", "cascade", "CP 6"])
def test_identities_with_the_nucleus_counts_and_the_maximum_cliques(K, graph):
    """On one k-truss result, without the restatement: total[3] and total[4] are the triangles and 4-cliques of the nucleus
    decomposition, omega and total[omega] are the maximum-clique search's, local at k_local = omega is its count."""
    a = K.KombAccel()
    if graph == "hug":
        a.from_edges(2000, K.gen_hug_edges(*HUG[1]))
    elif graph == "cascade":
        a.from_edges(120, _i64(R.clique_union(120, 220, 2, 9, 1)))
    else:
        a.from_edges(12, _i64(C.cocktail_party(6)[1]))
    with a:
        a.truss_run()
        a.run_nucleus()
        minfo, count, _ = a.run_max_clique()
        assert minfo["flags"] == 7
        total, local, info = a.run_clique_census(2, -1, minfo["omega"])
        assert info["flags"] & K._lib.KOMB_CENSUS_COMPLETE and info["k_hi"] == info["t_max"] == minfo["t_max"]
        assert int(total[3 - 2]) == a.nucleus_info()["n_triangles"]
        assert int(total[4 - 2]) == a.nucleus_info()["n_cliques4"]
        assert info["omega"] == minfo["omega"] and int(total[info["omega"] - 2]) == minfo["n_max_cliques"]
        assert np.array_equal(local, count.astype(np.uint64))
        assert sum(local.tolist()) == info["omega"] * int(total[info["omega"] - 2])
        assert a.max_clique_info() == minfo and np.array_equal(a.max_clique_fetch()[0], count)   # (the census left them alone)


def test_budget_that_runs_out(K):
    """CP(33): 2^33 maximal cliques, one leaf each at the least.  What 1 000 nodes count is a lower bound of the closed form."""
    m = 33
    nv, edges = C.cocktail_party(m)
    with _load(K, nv, edges) as a:
        a.truss_run()
        total, local, info = a.run_clique_census(2, -1, 3, budget=1000)
        assert info["flags"] == 0 and (info["k_lo"], info["k_hi"], info["t_max"]) == (2, 64, 64)
        assert info["nodes"] <= 1000 + K._lib.KOMB_MAXCLQ_OVERSHOOT
        closed = [comb(m, k) * 2 ** k for k in range(2, 65)]
        assert all(int(x) <= y for x, y in zip(total.tolist(), closed))
        assert all(int(x) <= comb(m - 1, 2) * 4 for x in local.tolist())        # the 3-cliques through a vertex
        assert info["omega"] <= m
        assert _code(K, lambda: a.clique_census_run(2, -1, 0, -1)) == K._lib.KOMB_ERR_ARG   # refused: the result stays
        assert a.clique_census_info() == info


def _path_k3(n_path):
    """A path joined to a K_3 (vertices 0, 1, 2), with a K_6 on six path vertices: the K_3's edges have n_path + 1 common
    neighbours at trussness 2, and seven at trussness 6 (the K_9)."""
    path = np.arange(3, 3 + n_path)
    edges = R.clique([0, 1, 2]) + [(int(path[i]), int(path[i + 1])) for i in range(n_path - 1)]
    edges += [(x, int(v)) for x in (0, 1, 2) for v in path]
    edges += R.clique([int(v) for v in path[100:200:20]] + [int(path[300])])
    return 3 + n_path, edges


def test_more_than_4096_candidates(K):
    nv, uv = _path_k3(4200)
    with _load(K, nv, uv) as a:
        edges = a.run_truss()
        a.clique_census_run(6, -1, 0)                                            # a first result, to be kept
        info = a.clique_census_info()
        assert _code(K, lambda: a.clique_census_run(2, -1, 0)) == K._lib.KOMB_ERR_LIMIT
        assert _code(K, lambda: a.clique_census_run(3, 4, 3)) == K._lib.KOMB_ERR_LIMIT
        assert b"4096" in K._lib.load().komb_last_error(a._ctx)
        assert a.clique_census_info() == info                                    # refused before anything was counted
        info = _check(a, 6, -1, 9, "path + K_3", False, edges)
        assert (info["omega"], info["t_max"], info["max_candidates"]) == (9, 9, 7)
        assert a.clique_census_fetch()[0].tolist() == [comb(9, k) for k in range(6, 10)]


def test_arguments(K):
    ARG = K._lib.KOMB_ERR_ARG
    nv, edges = R.hand_graph()                                                   # t_max 7
    with _load(K, nv, edges) as a:
        a.truss_run()
        total, local, info = a.run_clique_census(3, 20, 7)                       # k_hi is clamped, k_local = 7 is inside
        assert (info["k_lo"], info["k_hi"], info["k_local"]) == (3, 7, 7) and len(total) == 5
        for args in ((1, -1, 0), (0, 5, 0), (-3, -1, 0), (5, 4, 0), (3, 2, 0), (3, -2, 0), (2, -1, -1), (3, -1, 2), (2, 4, 5),
                     (2, 20, 8), (2, -1, 8)):
            assert _code(K, lambda: a.clique_census_run(*args)) == ARG, args
        assert _code(K, lambda: a.clique_census_run(2, -1, 0, -5)) == ARG
        assert a.clique_census_info() == info                                    # every refusal left the result alone
        total, local, info = a.run_clique_census(9, -1, 9)                       # a window above t_max: one entry, zero
        assert (info["k_lo"], info["k_hi"], info["omega"], info["flags"]) == (9, 9, 0, 1)
        assert total.tolist() == [0] and local.tolist() == [0] * nv


def test_call_order_and_lifetime(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, edges = R.hand_graph()
    want = C.census_edges(nv, edges, k_local=3)
    readers = lambda a: (a.clique_census_fetch, a.clique_census_info)
    run = lambda a: a.clique_census_run(2, -1, 3)
    with K.KombAccel() as a:
        for call in (a.clique_census_run,) + readers(a):                         # no graph
            assert _code(K, call) == ARG
        a.from_edges(nv, _i64(edges))
        assert _code(K, a.clique_census_run) == STATE                            # no k-truss result
        a.run_core(); a.run_onion(); a.run_components("core", 0)
        assert _code(K, a.clique_census_run) == STATE
        a.truss_run()
        for call in readers(a):                                                  # fetch / info before a run
            assert _code(K, call) == STATE
        run(a)                                                                   # (makes the canonical endpoints nobody has fetched yet)
        _compare(a, want)
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core); a.run_structural_clusters(1, 2, 3); a.run_community_hierarchy()
        a.run_nucleus(); a.run_nucleus_hierarchy(); a.run_max_clique()
        _compare(a, want)
        # NULL outputs are allowed; local after a run without a k_local is not there
        assert lib.komb_clique_census_fetch(a._ctx, None, None) == 0
        assert lib.komb_clique_census_info(a._ctx, *([None] * 10)) == 0
        a.clique_census_run()
        buf = np.full(nv, 7, np.uint64)
        assert lib.komb_clique_census_fetch(a._ctx, None, K._lib.ptr(buf)) == STATE and buf.tolist() == [7] * nv
        assert lib.komb_clique_census_fetch(a._ctx, None, None) == 0
        # a new k-truss run of any kind drops it
        a.truss_run()
        for call in readers(a):
            assert _code(K, call) == STATE
        run(a)
        _compare(a, want)
        a.truss_run(np.asarray([1] * 7 + [0] * 8, np.uint8))
        assert _code(K, a.clique_census_info) == STATE
        assert a.run_clique_census(2, -1, 7)[1].tolist() == [1] * 7 + [0] * 8
        # a slice of the canonical edges is no k-truss result to count in
        a.truss_run_slice(0, 2)
        assert _code(K, a.clique_census_fetch) == STATE and _code(K, a.clique_census_run) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, a.clique_census_run) == STATE
        a.truss_run_slice(0, 1)                                                  # the whole range
        run(a)
        _compare(a, want)
        # komb_truss_unprepare drops the k-truss result and the census with it
        a.truss_unprepare()
        for call in (a.clique_census_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        run(a)
        _compare(a, want)
        # a new graph drops it
        a.from_edges(4, [[0, 1], [1, 2], [0, 2]])
        for call in (a.clique_census_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        assert a.run_clique_census(2, -1, 3)[1].tolist() == [1, 1, 1, 0]
        with pytest.raises(K.KombError):                                         # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.clique_census_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            for k_lo, k_local in ((2, 4), (5, 0)):
                total, local, info = a.run_clique_census(k_lo, -1, k_local)
                assert info["flags"] == 1
                out += [total, np.zeros(0) if local is None else local, np.asarray([info[k] for k in ("k_hi", "t_max", "omega", "max_candidates")])]
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "CENSUS_LDS": "0"},
                                  {"POISON": "0x7FFFFFFF", "CENSUS_DEBUG": "1", "CENSUS_PIVOT": "first"}])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, opts):
    graphs = [(2000, K.gen_hug_edges(*HUG[1])), (300, K.gen_hug_edges(*HUG[0])), (3000, K.gen_hug_edges(3000, 7350, 2.2, 5))]
    want = [_all_results(K, nv, uv) for nv, uv in graphs]
    _set(monkeypatch, opts)
    with K.KombAccel() as a:                     # one context across the three graphs: larger, smaller, larger
        for (nv, uv), w in zip(graphs, want):
            got = _all_results(K, nv, uv, a)
            assert len(got) == len(w)
            for x, y in zip(got, w):
                assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """A run changes no k-core, onion, components, communities, densest, structural, nucleus, maximum-clique or k-truss
    result and no komb_stats field, and the resident k-truss preparation survives it."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv = 2000
    uv = K.gen_hug_edges(*HUG[1])
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        layer, ocore = a.run_onion()
        eu, ev, tr = a.run_truss()
        clabel, csize = a.run_components("truss", 3)
        mlabel, msize = a.run_truss_communities(3)
        member, load, _ = a.run_densest_subgraph(8)
        slabel, ssize, srole, ssim = a.run_structural_clusters(1, 2, 3)
        tris, etheta, vtheta = a.run_nucleus()
        qinfo, qcount, qwitness = a.run_max_clique()
        cinfo, minfo, dinfo, sinfo = a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()
        ninfo = a.nucleus_info()
        st = a.stats()
        for _ in range(2):
            a.clique_census_run(2, -1, 3)
            assert a.stats() == st
            a.clique_census_fetch(); a.clique_census_info()
            assert a.stats() == st
        _compare(a, _want(("hug", nv), nv, eu, ev, tr, 2, -1, 3))
        got = (a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch()
               + a.densest_subgraph_fetch() + a.structural_clusters_fetch()
               + (a.nucleus_fetch()["theta"], a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()) + a.max_clique_fetch())
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load, slabel, ssize, srole, ssim,
                         tris["theta"], etheta, vtheta, qcount, qwitness), got):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()) == (cinfo, minfo, dinfo, sinfo)
        assert a.nucleus_info() == ninfo and a.max_clique_info() == qinfo
        assert a.stats() == st
        e3 = a.run_truss()                                                       # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr), e3):
            assert np.array_equal(x, y)
