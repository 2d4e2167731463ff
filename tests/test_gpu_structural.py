"""GPU tests of komb_structural_clusters_run / _fetch / _fetch_edges / _info: every label, size, role, sim_deg and similar
entry and every count of info is compared exactly with the restatement of tests/structural_ref.py, which is fed the
library's own run_truss(with_support=True) (whose parity other tests own)."""
import numpy as np
import pytest

import components_ref as CR
import structural_ref as R

pytestmark = pytest.mark.gpu

COUNTS = ("eps_num", "eps_den", "mu", "n_similar_edges", "n_cores", "n_borders", "n_hubs", "n_outliers", "n_clusters", "largest")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _expect(a, eu, ev, sup, params):
    """Run params on a's last k-truss result (eu, ev, sup) and compare everything with the restatement."""
    a.structural_clusters_run(*params)
    return _compare(a, eu, ev, sup, params)


def _compare(a, eu, ev, sup, params, want=None):
    """The held clustering of params of the k-truss result (eu, ev, sup): everything against the restatement."""
    label, size, role, sim_deg = a.structural_clusters_fetch()
    similar = a.structural_clusters_fetch_edges()
    info = a.structural_clusters_info()
    want = R.clusters(a.nv, eu, ev, sup, *params) if want is None else want
    for x in (label, size, role, sim_deg, similar):
        assert x.dtype == np.int32
    assert len(similar) == len(eu) and all(len(x) == a.nv for x in (label, size, role, sim_deg))
    assert np.array_equal(similar, want["similar"]), params
    assert np.array_equal(sim_deg, want["sim_deg"]), params
    assert np.array_equal(label, want["label"]), params
    assert np.array_equal(size, want["size"]), params
    assert np.array_equal(role, want["role"]), params
    assert {k: info[k] for k in COUNTS} == want["info"], params
    assert info["ms"] >= 0.0
    return want


def _check(a, params_list, vmask=None):
    eu, ev, tr, sup = a.run_truss(vmask, with_support=True)
    return eu, ev, sup, [_expect(a, eu, ev, sup, p) for p in params_list]


def _load(K, nv, uv):
    a = K.KombAccel()
    a.from_edges(nv, _i64(uv))
    return a


SOME = [(3, 10, 2), (1, 2, 3), (7, 10, 3), (7, 10, 4), (1, 1, 2), (1, 100, 2), (999999, 1000000, 2)]


def _clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


def test_degenerate_graphs(K):
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))                                        # the empty graph is not an error
        _check(a, [(1, 2, 2), (1, 1, 5)])
        assert a.structural_clusters_info()["n_outliers"] == 0
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges: all outliers, zero counts
        _check(a, [(1, 2, 2)])
        label, size, role, sim_deg = a.structural_clusters_fetch()
        assert label.tolist() == [-1] * 7 and size.tolist() == [0] * 7 and role.tolist() == [0] * 7 and sim_deg.tolist() == [0] * 7
        info = a.structural_clusters_info()
        assert [info[k] for k in COUNTS[3:]] == [0, 0, 0, 0, 7, 0, 0]
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        _check(a, [(1, 2, 2)], vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        assert a.structural_clusters_info()["n_outliers"] == 6
        a.from_edges(3, [[0, 2]])                                                # one edge (and an isolated vertex)
        _check(a, SOME)
        assert a.run_structural_clusters(1, 1, 2)[0].tolist() == [0, -1, 0]
        a.from_edges(3, [[0, 1], [1, 2], [0, 2]])                                # one triangle
        _check(a, SOME)
        assert a.run_structural_clusters(1, 1, 3)[2].tolist() == [3, 3, 3]


def test_hand_graph(K):
    nv, edges = R.hand_graph()
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        with _load(K, nv, ids[_i64(edges)]) as a:
            _check(a, SOME + [(8, 10, 4), (6, 10, 3), (5, 10, 2)])
            label, size, role, _ = a.run_structural_clusters(7, 10, 3)
            info = a.structural_clusters_info()
            assert info["n_similar_edges"] == 21 and info["n_clusters"] == 2
            assert role[ids].tolist() == [3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 0, 2, 1]
            if ids[0] == 0:
                assert label.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, -1, -1, 0, -1]
            label, size, role, _ = a.run_structural_clusters(8, 10, 4)
            assert a.structural_clusters_info()["n_similar_edges"] == 18
            assert role[ids[3]] == R.BORDER and role[ids[12]] == R.OUTLIER


def test_path_star_clique(K):
    n = 3000
    with _load(K, n, np.stack([np.arange(n - 1), np.arange(1, n)], 1)) as a:     # a path: one long chain of hooks
        _check(a, [(1, 2, 2), (2, 3, 2), (2, 3, 3), (7, 10, 3), (1, 1, 2)])
    n = 5001
    for centre in (0, n - 1):                                                    # the centre's counts arrive by runs / by atomics on one word
        leaves = np.setdiff1d(np.arange(n), [centre])
        with _load(K, n, np.stack([np.full(n - 1, centre), leaves], 1)) as a:
            _check(a, [(1, 100, 2), (1, 2, 2), (1, 100, 3)])
            label, size, role, sim_deg = a.run_structural_clusters(1, 100, 2)    # everything similar: one cluster
            info = a.structural_clusters_info()
            assert sim_deg[centre] == 5000 and np.all(label == 0) and np.all(size == n) and np.all(role == R.CORE)
            assert [info[k] for k in COUNTS[3:]] == [5000, n, 0, 0, 0, 1, n]
            label, size, role, sim_deg = a.run_structural_clusters(1, 2, 2)      # nothing similar: all outliers, the centre included
            info = a.structural_clusters_info()
            assert not sim_deg.any() and np.all(label == -1) and not role.any() and not size.any()
            assert [info[k] for k in COUNTS[3:]] == [0, 0, 0, 0, n, 0, 0]
    with _load(K, 40, _clique(range(40))) as a:                                  # K_40
        _check(a, SOME + [(1, 1, 40), (1, 1, 41)])
        assert a.run_structural_clusters(1, 1, 40)[1].tolist() == [40] * 40
        assert a.run_structural_clusters(1, 1, 41)[2].tolist() == [0] * 40


def test_border_of_two_clusters_takes_the_smaller_label(K):
    """Two K_5 and a vertex x of degree 2 with one edge into each: sigma = 2 / sqrt(3 * 6) = 0.47 on both, so at eps = 2/5 and
    mu = 4 x is no core (sim_deg + 1 = 3) and a border of both clusters."""
    base = np.concatenate([_clique(range(5)), _clique(range(5, 10)), [[10, 4], [10, 9]]])
    rng = np.random.default_rng(4)
    for ids in (np.arange(11), 10 - np.arange(11), rng.permutation(11), rng.permutation(11)):
        with _load(K, 11, ids[base]) as a:
            eu, ev, sup, (want,) = _check(a, [(2, 5, 4)])
            assert R.multi_borders(11, eu, ev, want) == 1
            label, size, role, sim_deg = a.structural_clusters_fetch()
            x = ids[10]
            la, lb = int(ids[:5].min()), int(ids[5:10].min())
            assert role[x] == R.BORDER and sim_deg[x] == 2 and label[x] == min(la, lb)
            assert size[min(la, lb)] == 6 and size[max(la, lb)] == 5
            assert a.structural_clusters_info()["n_hubs"] == 0


def test_exact_tie(K):
    """Edge (0, 1): common neighbour 2, d(0) = 3, d(1) = 8, so sigma = 3 / sqrt(4 * 9) = 1/2 exactly."""
    edges = [[0, 1], [0, 2], [1, 2], [0, 3]] + [[1, w] for w in range(4, 10)]
    with _load(K, 10, edges) as a:
        eu, ev, sup, _ = _check(a, [(1, 2, 2), (500001, 1000000, 2), (499999, 1000000, 2)])
        assert (eu[0], ev[0], sup[0]) == (0, 1, 1)
        a.structural_clusters_run(1, 2, 2)
        assert a.structural_clusters_fetch_edges()[0] == 1
        a.structural_clusters_run(500001, 1000000, 2)
        assert a.structural_clusters_fetch_edges()[0] == 0


def test_wide_arithmetic(K):
    """Two adjacent vertices with 5 000 common neighbours: that edge has sigma = 5002 / 5002 = 1, and (sup + 2)^2 eps_den^2 is
    above 2^64 at eps_den = 10^6: a 64-bit product gets it wrong."""
    w = np.arange(2, 5002)
    edges = np.concatenate([[[0, 1]], np.stack([np.zeros(5000, np.int64), w], 1), np.stack([np.ones(5000, np.int64), w], 1)])
    assert 5002 ** 2 * 1000000 ** 2 > 2 ** 64
    for ids in (np.arange(5002), 5001 - np.arange(5002)):
        with _load(K, 5002, ids[edges]) as a:
            eu, ev, sup, _ = _check(a, [(999999, 1000000, 2), (1, 1, 2), (1, 100, 3)])
            assert len(eu) == 10001
            a.structural_clusters_run(999999, 1000000, 2)
            similar = a.structural_clusters_fetch_edges()
            i = int(np.flatnonzero((eu == min(ids[0], ids[1])) & (ev == max(ids[0], ids[1])))[0])
            assert sup[i] == 5000 and similar[i] == 1 and similar.sum() == 1


def _tri_paths(ne, lead):
    """`lead` path edges, then as many disjoint triangles as fit, then a path for the rest: ne edges in all.  A triangle's
    first two canonical edges share eu: with lead = 0, 1, 2 such a run starts at every residue of 3."""
    edges, v = [], 0
    for _ in range(lead):
        edges.append((v, v + 1)); v += 1
    v += 1
    while len(edges) + 3 <= ne:
        edges += [(v, v + 1), (v, v + 2), (v + 1, v + 2)]; v += 3
    while len(edges) < ne:
        edges.append((v, v + 1)); v += 1
    return v + 1, edges


@pytest.mark.parametrize("ne", [63, 64, 65, 1023, 1024, 1025])
def test_runs_across_wave_and_workgroup_boundaries(K, ne):
    for lead in (0, 1, 2):
        nv, edges = _tri_paths(ne, lead)
        with _load(K, nv, edges) as a:
            eu, ev, sup, _ = _check(a, [(1, 2, 2), (7, 10, 3), (1, 1, 3)])
            assert len(eu) == ne
    # a run of equal eu that starts in one wave / workgroup and ends in the next: a fan of 40 behind ne - 20 path edges
    p = ne - 20
    edges = [(i, i + 1) for i in range(p)] + [(p + 1, p + 2 + j) for j in range(40)] + [(p + 2 + j, p + 3 + j) for j in range(0, 39, 2)]
    with _load(K, p + 43, edges) as a:
        eu, ev, sup, _ = _check(a, [(1, 3, 2), (1, 2, 2), (1, 2, 4)])
        assert np.all(eu[p:p + 40] == p + 1)


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            eu, ev, _, _ = _check(a, SOME)
            assert (eu.tolist(), ev.tolist()) == (g["eu"], g["ev"]), g["name"]
            eu, ev, _, _ = _check(a, SOME, vmask=np.asarray(g["maxcore_mask"], np.uint8))
            assert (eu.tolist(), ev.tolist()) == (g["sub_eu"], g["sub_ev"]), g["name"]


@pytest.mark.parametrize("nv,alpha", [(20000, 2.2), (200000, 2.6)])
def test_power_law_graphs(K, nv, alpha):
    uv = K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        params = [(3, 10, 2), (1, 2, 3), (7, 10, 4), (1, 1, 2), (2, 5, 4), (1, 100, int(deg.max()) + 2)]
        eu, ev, sup, wants = _check(a, params)
        # the cases show something: all four roles (mu = 2 leaves no border: a non-core has no similar edge then), borders of
        # several clusters (a non-core has at most mu - 2 similar edges: mu = 4 at the least), and no core at all for the last
        for i in (1, 2, 4):
            assert all(wants[i]["info"][k] > 0 for k in ("n_cores", "n_borders", "n_hubs", "n_outliers")), params[i]
        assert all(wants[i]["info"][k] > 0 for i in (0, 3) for k in ("n_cores", "n_hubs", "n_outliers"))
        assert R.multi_borders(nv, eu, ev, wants[4]) > 0
        assert wants[5]["info"]["n_cores"] == 0 and wants[5]["info"]["n_outliers"] == nv
        _check(a, params[:5], vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8))


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, edges = R.hand_graph()
    with _load(K, nv, edges) as b:                                             # what the calls below must give
        want = _check(b, [(7, 10, 3)])[3][0]
    with K.KombAccel() as a:
        assert _code(K, a.structural_clusters_run) == ARG                        # no graph
        assert _code(K, a.structural_clusters_fetch) == ARG
        assert _code(K, a.structural_clusters_fetch_edges) == ARG
        assert _code(K, a.structural_clusters_info) == ARG
        a.from_edges(nv, _i64(edges))
        # no k-truss result; fetch / info before a run
        assert _code(K, a.structural_clusters_run) == STATE
        a.run_core(); a.run_onion(); a.run_components("core", 0)
        assert _code(K, a.structural_clusters_run) == STATE
        a.truss_run()
        assert _code(K, a.structural_clusters_fetch) == STATE
        assert _code(K, a.structural_clusters_fetch_edges) == STATE
        assert _code(K, a.structural_clusters_info) == STATE
        # parameters outside their ranges (checked before the state)
        bad = [(0, 10, 3), (-1, 10, 3), (11, 10, 3), (1, 1000001, 3), (1000001, 1000001, 3), (7, 10, 1), (7, 10, 0), (7, 10, -5), (1, 0, 2)]
        for p in bad:
            assert _code(K, lambda: a.structural_clusters_run(*p)) == ARG, p
        assert _code(K, a.structural_clusters_fetch) == STATE
        # the run makes the canonical endpoints and supports nobody has fetched yet
        label, size, role, sim_deg = a.run_structural_clusters(7, 10, 3)
        assert np.array_equal(label, want["label"]) and np.array_equal(role, want["role"]) and np.array_equal(size, want["size"])
        assert np.array_equal(a.structural_clusters_fetch_edges(), want["similar"])
        assert a.run_structural_clusters(1000000, 1000000, 2) is not None and a.structural_clusters_info()["eps_den"] == 1000000
        a.structural_clusters_run(7, 10, 3)
        # a refused call leaves the last result readable
        for p in bad:
            assert _code(K, lambda: a.structural_clusters_run(*p)) == ARG
        assert np.array_equal(a.structural_clusters_fetch()[0], want["label"])
        assert {k: a.structural_clusters_info()[k] for k in COUNTS} == want["info"]
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core)
        assert np.array_equal(a.structural_clusters_fetch()[2], want["role"])
        assert np.array_equal(a.structural_clusters_fetch_edges(), want["similar"])
        # NULL outputs are allowed
        assert lib.komb_structural_clusters_fetch(a._ctx, None, None, None, None) == 0
        assert lib.komb_structural_clusters_fetch_edges(a._ctx, None) == 0
        assert lib.komb_structural_clusters_info(a._ctx, *([None] * 11)) == 0
        # a new k-truss run of any kind drops it
        a.truss_run()
        assert _code(K, a.structural_clusters_fetch) == STATE
        assert _code(K, a.structural_clusters_fetch_edges) == STATE
        assert _code(K, a.structural_clusters_info) == STATE
        assert np.array_equal(a.run_structural_clusters(7, 10, 3)[0], want["label"])
        a.truss_run(np.asarray([1] * 10 + [0] * 4, np.uint8))
        assert _code(K, a.structural_clusters_info) == STATE
        assert a.run_structural_clusters(7, 10, 3)[0].tolist() == [0] * 5 + [5] * 5 + [-1] * 4
        # a slice of the canonical edges is not a k-truss result to cluster
        a.truss_run_slice(0, 2)
        assert _code(K, a.structural_clusters_fetch) == STATE
        assert _code(K, a.structural_clusters_run) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, a.structural_clusters_run) == STATE
        a.truss_run_slice(0, 1)                                                  # the whole range
        assert np.array_equal(a.run_structural_clusters(7, 10, 3)[0], want["label"])
        # komb_truss_unprepare drops the k-truss result and the clustering with it
        a.truss_unprepare()
        assert _code(K, a.structural_clusters_fetch) == STATE
        assert _code(K, a.structural_clusters_info) == STATE
        assert _code(K, a.structural_clusters_run) == STATE
        a.truss_run()
        assert np.array_equal(a.run_structural_clusters(7, 10, 3)[2], want["role"])
        # a new graph drops it
        a.from_edges(3, [[0, 1]])
        assert _code(K, a.structural_clusters_fetch) == STATE
        assert _code(K, a.structural_clusters_info) == STATE
        assert _code(K, a.structural_clusters_run) == STATE
        a.truss_run()
        assert a.run_structural_clusters(1, 1, 2)[0].tolist() == [0, 0, -1]
        with pytest.raises(K.KombError):                                         # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.structural_clusters_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            for p in ((3, 10, 2), (1, 2, 3), (7, 10, 4)):
                out += list(a.run_structural_clusters(*p))
                out.append(a.structural_clusters_fetch_edges())
                info = a.structural_clusters_info()
                out.append(np.asarray([info[k] for k in COUNTS]))
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001"}, {"POISON": "0x7FFFFFFF", "STRUCT_DEBUG": "1"}])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, opts):
    graphs = [(30000, K.gen_hug_edges(30000, 73500, 2.2, 5)), (900, K.gen_hug_edges(900, 2200, 2.6, 6)), (50000, K.gen_hug_edges(50000, 122500, 2.1, 7))]
    want = [_all_results(K, nv, uv) for nv, uv in graphs]
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)
    with K.KombAccel() as a:                     # one context across the three graphs: larger, smaller, larger
        for (nv, uv), w in zip(graphs, want):
            got = _all_results(K, nv, uv, a)
            assert len(got) == len(w)
            for x, y in zip(got, w):
                assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """A run changes no k-core, onion, components, communities, densest or k-truss result and no komb_stats field, and the
    resident k-truss preparation survives it."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv, uv = CR.composite(K.gen_hug_edges, 5)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        layer, ocore = a.run_onion()
        eu, ev, tr = a.run_truss()                                               # (no support fetched: the first run puts it in order)
        clabel, csize = a.run_components("truss", 3)
        mlabel, msize = a.run_truss_communities(3)
        member, load, _ = a.run_densest_subgraph(8)
        cinfo, minfo, dinfo = a.components_info(), a.truss_communities_info(), a.densest_subgraph_info()
        st = a.stats()
        for p in ((1, 2, 3), (3, 10, 2), (1, 1, 2), (1, 2, 100000)):
            a.structural_clusters_run(*p)
            assert a.stats() == st
            a.structural_clusters_fetch(); a.structural_clusters_fetch_edges(); a.structural_clusters_info()
            assert a.stats() == st
        sup = a.truss_fetch(with_support=True)[3]
        _expect(a, eu, ev, sup, (1, 2, 3))
        got = a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch() + a.densest_subgraph_fetch()
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load), got):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info()) == (cinfo, minfo, dinfo) and a.stats() == st
        e3 = a.run_truss(with_support=True)                                      # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr, sup), e3):
            assert np.array_equal(x, y)
