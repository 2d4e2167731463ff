"""GPU tests of komb_max_clique_run / _fetch / _list / _info: every complete result (flags == 7) -- omega, upper, t_max,
n_max_cliques, count, the whole list and witness == list[0] -- is compared exactly with the restatement of
tests/max_clique_ref.py, which is fed the library's own run_truss() edge list (whose parity other tests own).  A result the
budget cut short is checked against the invariants the header states."""
import ctypes

import numpy as np
import pytest

import max_clique_ref as M
import nucleus_ref as R

pytestmark = pytest.mark.gpu

LDS = [{}, {"MAXCLQ_LDS": "0"}, {"MAXCLQ_LDS": "64"}]
LDS_IDS = ["lds default", "lds 0", "lds 64"]
SEED = [{}, {"MAXCLQ_SEED": "0"}]
SEED_IDS = ["seed", "no seed"]


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


_WANT = {}


def _want(key, nv, eu, ev, tr, own_truss=True):
    """The restatement of one k-truss result, computed once per module and never changed."""
    truss = None if own_truss else tr
    if key is None:
        return M.solve(nv, eu, ev, truss=truss)
    if key not in _WANT:
        _WANT[key] = (eu.copy(), ev.copy(), M.solve(nv, eu, ev, truss=truss))
    seu, sev, want = _WANT[key]
    assert np.array_equal(seu, eu) and np.array_equal(sev, ev)
    return want


def _compare(a, want):
    info = a.max_clique_info()
    assert info["flags"] == 7 == want["flags"]
    for name in ("omega", "upper", "t_max", "n_max_cliques"):
        assert info[name] == want[name], name
    count, witness = a.max_clique_fetch()
    assert count.dtype == np.int32 and len(count) == max(a.nv, 0)
    assert np.array_equal(count, want["count"])
    cliques = a.max_clique_list()
    assert cliques.dtype == np.int32 and cliques.shape == (want["n_max_cliques"], want["omega"])
    assert [tuple(c) for c in cliques.tolist()] == want["cliques"]
    assert tuple(witness.tolist()) == tuple(want["witness"])
    if want["omega"]:
        assert witness.tolist() == cliques[0].tolist()
    assert info["nodes"] >= info["n_max_cliques"] and info["n_roots"] >= min(info["n_max_cliques"], 1) and info["ms"] >= 0.0
    return info


def _check(a, vmask=None, key=None, own_truss=True, budget=0):
    """k-truss (whole graph or vmask), then the search: everything against the restatement."""
    eu, ev, tr = a.run_truss(vmask)
    a.max_clique_run(budget)
    want = _want(key, a.nv, eu, ev, tr, own_truss)
    _compare(a, want)
    return eu, ev, want


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


def _is_clique(witness, eu, ev):
    edges = set(zip(eu.tolist(), ev.tolist()))
    w = sorted(witness.tolist())
    return len(set(w)) == len(w) and all((w[i], w[j]) in edges for i in range(len(w)) for j in range(i + 1, len(w)))


def test_degenerate_graphs(K):
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))                                        # the empty graph is not an error
        _check(a)
        info = a.max_clique_info()
        assert (info["omega"], info["upper"], info["flags"], info["t_max"], info["n_max_cliques"], info["nodes"]) == (0, 0, 7, 0, 0, 0)
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges
        _check(a)
        assert a.max_clique_fetch()[0].tolist() == [0] * 7 and a.max_clique_info()["omega"] == 0
        a.from_edges(6, [[0, 1], [1, 2], [2, 3], [3, 4], [1, 5]])                # a path: every edge is a maximum clique
        _check(a)
        assert a.max_clique_list().tolist() == [[0, 1], [1, 2], [1, 5], [2, 3], [3, 4]]
        assert a.max_clique_fetch()[0].tolist() == [1, 3, 2, 2, 1, 1]
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        _check(a, vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        assert a.max_clique_info()["omega"] == 0 and a.max_clique_info()["flags"] == 7
        a.from_edges(4, [[0, 1], [1, 3], [0, 3]])                                # one triangle (and an isolated vertex)
        _check(a)
        assert a.max_clique_list().tolist() == [[0, 1, 3]] and a.max_clique_fetch()[0].tolist() == [1, 1, 0, 1]
        info = a.max_clique_info()
        assert (info["omega"], info["upper"], info["t_max"], info["n_max_cliques"]) == (3, 3, 3, 1)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 12, 40])
def test_complete_graphs(K, n):
    with _load(K, n, R.clique(range(n))) as a:
        _check(a)
        info = a.max_clique_info()
        assert (info["omega"], info["t_max"], info["n_max_cliques"]) == (n, n, 1)
        assert a.max_clique_list().tolist() == [list(range(n))]


def test_hand_graph_and_its_reversed_labelling(K):
    nv, edges = R.hand_graph()
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        with _load(K, nv, ids[_i64(edges)]) as a:
            _check(a)
            info = a.max_clique_info()
            assert (info["omega"], info["n_max_cliques"], info["t_max"]) == (7, 1, 7)
            assert a.max_clique_fetch()[0][ids].tolist() == [1] * 7 + [0] * 8
            _check(a, vmask=(np.arange(nv) != ids[0]).astype(np.uint8))         # without a K_7 vertex: a K_6 is left
            info = a.max_clique_info()
            assert (info["omega"], info["n_max_cliques"]) == (6, 1) and a.max_clique_fetch()[0][ids[0]] == 0


@pytest.mark.parametrize("seed", SEED, ids=SEED_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
@pytest.mark.parametrize("n", [65, 66, 67, 130, 515])
def test_candidate_sets_across_word_and_path_boundaries(K, monkeypatch, n, lds, seed):
    """K_n: without the seed the search itself walks a candidate set of n - 2 (one, two, three and nine words; above 512 the
    bit matrix is in global scratch whatever MAXCLQ_LDS says)."""
    _set(monkeypatch, lds, seed)
    with _load(K, n, R.clique(range(n))) as a:
        _check(a, key=("K", n), own_truss=n < 100)
        info = a.max_clique_info()
        assert (info["omega"], info["t_max"], info["n_max_cliques"]) == (n, n, 1)


@pytest.mark.parametrize("seed", SEED, ids=SEED_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
@pytest.mark.parametrize("m", [6, 12])
def test_cocktail_party_in_full(K, monkeypatch, m, lds, seed):
    _set(monkeypatch, lds, seed)
    nv, edges = M.cocktail_party(m)
    with _load(K, nv, edges) as a:
        _check(a, key=("CP", m))
        info = a.max_clique_info()
        assert (info["omega"], info["t_max"], info["n_max_cliques"]) == (m, 2 * m - 2, 2 ** m)
        assert a.max_clique_fetch()[0].tolist() == [2 ** (m - 1)] * nv


@pytest.mark.parametrize("seed", SEED, ids=SEED_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
def test_cocktail_party_33_is_proven_and_not_enumerated(K, monkeypatch, lds, seed):
    """CP(33): candidate sets of up to 64; 2^33 maximum cliques are beyond any budget, omega = 33 is not (the colouring
    closes every root after the first dive)."""
    _set(monkeypatch, lds, seed)
    nv, edges = M.cocktail_party(33)
    with _load(K, nv, edges) as a:
        eu, ev, _ = a.run_truss()
        a.max_clique_run(200000)
        info = a.max_clique_info()
        assert (info["flags"], info["omega"], info["upper"], info["t_max"], info["n_max_cliques"]) == (1, 33, 33, 64, -1)
        assert info["nodes"] <= 200000 + K._lib.KOMB_MAXCLQ_OVERSHOOT
        count, witness = a.max_clique_fetch()
        assert _is_clique(witness, eu, ev) and sorted(np.flatnonzero(count).tolist()) == witness.tolist() and int(count.sum()) == 33
        assert _code(K, a.max_clique_list) == K._lib.KOMB_ERR_LIMIT


def _hub_graph(hub_first):
    """A vertex joined to all of 3 000 others, which carry a few K_5: the hub's row (id 0) or column (the largest id) is long."""
    n = 3001
    others = np.arange(1, n) if hub_first else np.arange(0, n - 1)
    hub = 0 if hub_first else n - 1
    edges = [(hub, int(v)) for v in others]
    for s in (0, 5, 700, 1500, 2990):
        edges += R.clique(others[s:s + 5])
    edges += R.clique(others[[3, 800, 1600, 2500]])
    return n, edges


def _path_k3(k3_first):
    """A path of 3 000 vertices joined to a K_3: the K_3's edges have 3 001 common neighbours, every two next to each other on
    the path close a maximum clique with it."""
    n = 3003
    k3 = [0, 1, 2] if k3_first else [n - 3, n - 2, n - 1]
    path = np.arange(3, n) if k3_first else np.arange(0, n - 3)
    edges = R.clique(k3) + [(int(path[i]), int(path[i + 1])) for i in range(len(path) - 1)]
    edges += [(x, int(v)) for x in k3 for v in path]
    return n, edges


LONG = {"star": lambda: (5001, [(0, i) for i in range(1, 5001)]),
        "star, centre last": lambda: (5001, [(5000, i) for i in range(5000)]),
        "hub row": lambda: _hub_graph(True), "hub column": lambda: _hub_graph(False),
        "path + K_3 first": lambda: _path_k3(True), "path + K_3 last": lambda: _path_k3(False)}


@pytest.mark.parametrize("seed", SEED, ids=SEED_IDS)
@pytest.mark.parametrize("name", list(LONG))
def test_long_rows(K, monkeypatch, name, seed):
    _set(monkeypatch, seed)
    nv, edges = LONG[name]()
    with _load(K, nv, edges) as a:
        _, _, want = _check(a, key=name)
        if name.startswith("star"):
            assert (want["omega"], want["n_max_cliques"]) == (2, 5000)
        if name.startswith("hub"):
            assert (want["omega"], want["n_max_cliques"]) == (6, 5)              # a K_5 and the hub: a K_6
        if name.startswith("path"):
            assert (want["omega"], want["n_max_cliques"]) == (5, 2999)


HUG = [(300, 735, 2.6, 6), (2000, 4900, 2.2, 11), (3000, 7350, 2.2, 5), (5000, 12250, 2.1, 7)]
HUG_WANT = [(9, 2, 9), (17, 8, 17), (18, 9, 19), (23, 14, 26)]


@pytest.mark.parametrize("i", range(4), ids=lambda i: "nv %d" % HUG[i][0])
def test_power_law_graphs(K, monkeypatch, i):
    nv = HUG[i][0]
    with K.KombAccel() as a:
        a.from_edges(nv, K.gen_hug_edges(*HUG[i]))
        _check(a, key=("hug", nv))
        info = a.max_clique_info()
        assert (info["omega"], info["n_max_cliques"], info["t_max"]) == HUG_WANT[i]
        if nv == 2000:
            monkeypatch.setenv("KOMB_MAXCLQ_LDS", "0")
            _check(a, key=("hug", nv))
            monkeypatch.delenv("KOMB_MAXCLQ_LDS")
            core = a.run_core()[1]
            _check(a, vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8), key=("hug, vmask", nv))


def test_cascade_of_random_cliques(K):
    with _load(K, 120, R.clique_union(120, 220, 2, 9, 1)) as a:
        _, _, want = _check(a, key="cascade")
        assert (want["omega"], want["t_max"]) == (11, 15)
        assert a.max_clique_list().tolist() == [[16, 24, 32, 51, 68, 71, 78, 96, 99, 105, 117]]


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            eu, ev, _ = _check(a)
            assert (eu.tolist(), ev.tolist()) == (g["eu"], g["ev"]), g["name"]
            eu, ev, _ = _check(a, vmask=np.asarray(g["maxcore_mask"], np.uint8))
            assert (eu.tolist(), ev.tolist()) == (g["sub_eu"], g["sub_ev"]), g["name"]


def test_budget_that_runs_out_in_the_search(K):
    nv, edges = M.cocktail_party(40)
    with _load(K, nv, edges) as a:
        eu, ev, _ = a.run_truss()
        a.max_clique_run(1000)
        info = a.max_clique_info()
        assert not info["flags"] & K._lib.KOMB_MAXCLQ_ENUMERATED and info["n_max_cliques"] == -1
        assert info["omega"] <= 40 <= info["upper"] <= 78 and info["t_max"] == 78
        count, witness = a.max_clique_fetch()
        assert len(witness) == info["omega"] >= 2 and _is_clique(witness, eu, ev)
        assert sorted(np.flatnonzero(count).tolist()) == sorted(witness.tolist()) and int(count.sum()) == info["omega"]
        if info["flags"] & K._lib.KOMB_MAXCLQ_EXACT:
            assert info["omega"] == 40 == info["upper"]
        else:
            assert info["upper"] == 78
        assert _code(K, a.max_clique_list) == K._lib.KOMB_ERR_LIMIT
        assert info["nodes"] <= 1000 + K._lib.KOMB_MAXCLQ_OVERSHOOT


def test_list_cap_and_negative_budget(K, monkeypatch):
    nv, edges = M.cocktail_party(12)
    with _load(K, nv, edges) as a:
        eu, ev, tr = a.run_truss()
        want = _want(("CP", 12), nv, eu, ev, tr)
        monkeypatch.setenv("KOMB_MAXCLQ_LIST", "1000")
        a.max_clique_run()
        info = a.max_clique_info()
        assert (info["flags"], info["omega"], info["upper"], info["n_max_cliques"]) == (3, 12, 12, 4096)
        count, witness = a.max_clique_fetch()
        assert count.tolist() == [2048] * nv and _is_clique(witness, eu, ev) and len(witness) == 12
        assert _code(K, a.max_clique_list) == K._lib.KOMB_ERR_LIMIT
        monkeypatch.delenv("KOMB_MAXCLQ_LIST")
        a.max_clique_run()
        _compare(a, want)
        assert _code(K, lambda: a.max_clique_run(-1)) == K._lib.KOMB_ERR_ARG      # refused: the previous result stays readable
        _compare(a, want)
        lib = K._lib.load()
        n = ctypes.c_int64(-7)
        small = np.full(12, -7, np.int32)
        assert lib.komb_max_clique_list(a._ctx, 1, ctypes.byref(n), K._lib.ptr(small)) == K._lib.KOMB_ERR_ARG
        assert n.value == -7 and small.tolist() == [-7] * 12                     # too little room: nothing written


def test_call_order_and_lifetime(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, edges = R.hand_graph()
    want = M.solve_edges(nv, edges)
    readers = lambda a: (a.max_clique_fetch, a.max_clique_list, a.max_clique_info)
    with K.KombAccel() as a:
        for call in (a.max_clique_run,) + readers(a):                            # no graph
            assert _code(K, call) == ARG
        a.from_edges(nv, _i64(edges))
        assert _code(K, a.max_clique_run) == STATE                               # no k-truss result
        a.run_core(); a.run_onion(); a.run_components("core", 0)
        assert _code(K, a.max_clique_run) == STATE
        a.truss_run()
        for call in readers(a):                                                  # fetch / list / info before a run
            assert _code(K, call) == STATE
        a.max_clique_run()                                                       # (makes the canonical endpoints nobody has fetched yet)
        _compare(a, want)
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core); a.run_structural_clusters(1, 2, 3); a.run_community_hierarchy()
        a.run_nucleus(); a.run_nucleus_hierarchy()
        _compare(a, want)
        # NULL outputs are allowed
        assert lib.komb_max_clique_fetch(a._ctx, None, None) == 0
        assert lib.komb_max_clique_list(a._ctx, 0, None, None) == 0
        assert lib.komb_max_clique_info(a._ctx, *([None] * 8)) == 0
        # a new k-truss run of any kind drops it
        a.truss_run()
        for call in readers(a):
            assert _code(K, call) == STATE
        a.max_clique_run()
        _compare(a, want)
        a.truss_run(np.asarray([1] * 7 + [0] * 8, np.uint8))
        assert _code(K, a.max_clique_info) == STATE
        a.max_clique_run()
        assert a.max_clique_fetch()[0].tolist() == [1] * 7 + [0] * 8
        # a slice of the canonical edges is no k-truss result to search
        a.truss_run_slice(0, 2)
        assert _code(K, a.max_clique_fetch) == STATE and _code(K, a.max_clique_run) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, a.max_clique_run) == STATE
        a.truss_run_slice(0, 1)                                                  # the whole range
        a.max_clique_run()
        _compare(a, want)
        # komb_truss_unprepare drops the k-truss result and the cliques with it
        a.truss_unprepare()
        for call in (a.max_clique_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        a.max_clique_run()
        _compare(a, want)
        # a new graph drops it
        a.from_edges(4, [[0, 1], [1, 2], [0, 2]])
        for call in (a.max_clique_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        assert a.run_max_clique()[1].tolist() == [1, 1, 1, 0]
        with pytest.raises(K.KombError):                                         # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.max_clique_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            info, count, witness = a.run_max_clique()
            assert info["flags"] == 7
            out += [count, witness, a.max_clique_list(), np.asarray([info[k] for k in ("omega", "upper", "flags", "t_max", "n_max_cliques")])]
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "MAXCLQ_LDS": "0"},
                                  {"POISON": "0x7FFFFFFF", "MAXCLQ_DEBUG": "1"}])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, opts):
    graphs = [(3000, K.gen_hug_edges(3000, 7350, 2.2, 5)), (300, K.gen_hug_edges(300, 735, 2.6, 6)), (5000, K.gen_hug_edges(5000, 12250, 2.1, 7))]
    want = [_all_results(K, nv, uv) for nv, uv in graphs]
    _set(monkeypatch, opts)
    with K.KombAccel() as a:                     # one context across the three graphs: larger, smaller, larger
        for (nv, uv), w in zip(graphs, want):
            got = _all_results(K, nv, uv, a)
            assert len(got) == len(w)
            for x, y in zip(got, w):
                assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """A run changes no k-core, onion, components, communities, densest, structural, nucleus or k-truss result and no
    komb_stats field, and the resident k-truss preparation survives it."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv = 2000
    uv = K.gen_hug_edges(nv, int(2.45 * nv), 2.2, 11)
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
        cinfo, minfo, dinfo, sinfo = a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()
        ninfo = a.nucleus_info()
        st = a.stats()
        for _ in range(2):
            a.max_clique_run()
            assert a.stats() == st
            a.max_clique_fetch(); a.max_clique_list(); a.max_clique_info()
            assert a.stats() == st
        _compare(a, _want(("hug", nv), nv, eu, ev, tr))
        got = (a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch()
               + a.densest_subgraph_fetch() + a.structural_clusters_fetch() + (a.nucleus_fetch()["theta"], a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()))
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load, slabel, ssize, srole, ssim,
                         tris["theta"], etheta, vtheta), got):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()) == (cinfo, minfo, dinfo, sinfo)
        assert a.nucleus_info() == ninfo
        assert a.stats() == st
        e3 = a.run_truss()                                                       # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr), e3):
            assert np.array_equal(x, y)
