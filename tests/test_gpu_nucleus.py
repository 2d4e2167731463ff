"""GPU tests of komb_nucleus_run / _count / _fetch / _fetch_edges / _fetch_vertices / _info: every triangle, key0, theta,
edge_theta and vertex_theta entry and every count of info is compared exactly with the restatement of tests/nucleus_ref.py,
which is fed the library's own run_truss() edge list (whose parity other tests own)."""
import numpy as np
import pytest

import nucleus_ref as R

pytestmark = pytest.mark.gpu

COUNTS = ("n_triangles", "n_cliques4", "theta_max", "n_levels")
FIELDS = ("a", "b", "c", "key0", "theta")
# the three ways a walked side is enumerated: its lane, its wave, several workgroups (triangle pass) -- and the defaults
PATHS = [{}, {"NUC_SHORT": "1000000000", "NUC_HEAVY": "2000000000"}, {"NUC_SHORT": "1", "NUC_HEAVY": "1000000000"},
         {"NUC_SHORT": "1", "NUC_HEAVY": "2"}]
PATH_IDS = ["default", "lane", "wave", "queued"]


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


_WANT = {}


def _want(key, nv, eu, ev):
    """The restatement of one k-truss result, computed once per module and never changed."""
    if key is None:
        return R.decompose(nv, eu, ev)
    if key not in _WANT:
        _WANT[key] = (eu.copy(), ev.copy(), R.decompose(nv, eu, ev))
    seu, sev, want = _WANT[key]
    assert np.array_equal(seu, eu) and np.array_equal(sev, ev)
    return want


def _compare(a, n_edges, want):
    tris, edge_theta, vertex_theta = a.nucleus_fetch(), a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()
    info = a.nucleus_info()
    assert {k: info[k] for k in COUNTS} == want["info"]
    for name in FIELDS:
        assert tris[name].dtype == np.int32 and len(tris[name]) == want["info"]["n_triangles"], name
        assert np.array_equal(tris[name], want[name]), name
    assert edge_theta.dtype == np.int32 and len(edge_theta) == n_edges
    assert vertex_theta.dtype == np.int32 and len(vertex_theta) == max(a.nv, 0)
    assert np.array_equal(edge_theta, want["edge_theta"])
    assert np.array_equal(vertex_theta, want["vertex_theta"])
    assert info["n_subrounds"] >= info["n_levels"] and info["n_subrounds"] <= max(info["n_triangles"], 0)
    assert info["ms"] >= 0.0


def _check(a, vmask=None, key=None):
    """k-truss (whole graph or vmask), then the nucleus run: everything against the restatement."""
    eu, ev, _ = a.run_truss(vmask)
    a.nucleus_run()
    want = _want(key, a.nv, eu, ev)
    _compare(a, len(eu), want)
    return eu, ev, want


def _load(K, nv, uv):
    a = K.KombAccel()
    a.from_edges(nv, _i64(uv))
    return a


def _set(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)


def test_degenerate_graphs(K):
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))                                        # the empty graph is not an error
        _check(a)
        assert a.nucleus_info()["theta_max"] == -1 and a.nucleus_info()["n_subrounds"] == 0
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges
        _check(a)
        assert a.nucleus_fetch_vertices().tolist() == [-1] * 7
        a.from_edges(6, [[0, 1], [1, 2], [2, 3], [3, 4], [1, 5]])                # edges without a triangle
        _check(a)
        assert a.nucleus_fetch_edges().tolist() == [-1] * 5 and a.nucleus_info()["n_triangles"] == 0
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        _check(a, vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        assert a.nucleus_info()["n_triangles"] == 0
        a.from_edges(4, [[0, 1], [1, 3], [0, 3]])                                # one triangle (and an isolated vertex)
        _check(a)
        t = a.nucleus_fetch()
        assert [t[k].tolist() for k in FIELDS] == [[0], [1], [3], [0], [0]]
        assert a.nucleus_fetch_vertices().tolist() == [0, 0, -1, 0] and a.nucleus_fetch_edges().tolist() == [0, 0, 0]
        info = a.nucleus_info()
        assert [info[k] for k in COUNTS] == [1, 0, 0, 1] and info["n_subrounds"] == 1


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(K, case):
    name, nv, edges, n_tri, n_clq, counts = case
    with _load(K, nv, edges) as a:
        _, _, want = _check(a)
        info = a.nucleus_info()
        assert info["n_triangles"] == n_tri and info["n_cliques4"] == n_clq and info["theta_max"] == max(counts)
        theta = a.nucleus_fetch()["theta"]
        assert {int(k): int(v) for k, v in zip(*np.unique(theta, return_counts=True))} == counts


def test_k40(K):
    with _load(K, 40, R.clique(range(40))) as a:
        _check(a)
        info = a.nucleus_info()
        assert [info[k] for k in COUNTS] == [9880, 91390, 37, 1] and info["n_subrounds"] == 1
        assert np.all(a.nucleus_fetch()["theta"] == 37) and np.all(a.nucleus_fetch_edges() == 37)


def test_hand_graph_and_its_reversed_labelling(K):
    nv, edges = R.hand_graph()
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        with _load(K, nv, ids[_i64(edges)]) as a:
            _check(a)
            assert a.nucleus_fetch_vertices()[ids].tolist() == [4, 4, 4, 4, 4, 4, 4, 2, 2, 2, 1, 1, 1, 0, 0]
            assert a.nucleus_info()["n_levels"] == 4
            _check(a, vmask=(np.arange(nv) != ids[0]).astype(np.uint8))         # without a K_7 vertex: a K_6 is left
            assert a.nucleus_info()["theta_max"] == 3 and a.nucleus_fetch_vertices()[ids[0]] == -1


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
    """A path of 3 000 vertices joined to a K_3: the K_3's triangle lies in 3 000 4-cliques."""
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


@pytest.mark.parametrize("paths", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("name", list(LONG))
def test_long_rows(K, monkeypatch, name, paths):
    _set(monkeypatch, paths)
    nv, edges = LONG[name]()
    with _load(K, nv, edges) as a:
        _, _, want = _check(a, key=name)
        if name.startswith("path"):
            assert int(want["key0"].max()) == 3000                               # thousands of decrements on one word
        if name.startswith("star"):
            assert want["info"]["n_triangles"] == 0
        if name.startswith("hub"):
            assert want["info"]["theta_max"] == 3                                # a K_5 and the hub: a K_6


def _fan(n, edge_first):
    """An edge with n common neighbours, which form a path: n triangles on one edge, two 4-cliques through each but the ends'."""
    nv = n + 2
    u, v = (0, 1) if edge_first else (nv - 2, nv - 1)
    rest = np.arange(2, nv) if edge_first else np.arange(0, n)
    edges = [(u, v)] + [(u, int(w)) for w in rest] + [(v, int(w)) for w in rest]
    edges += [(int(rest[i]), int(rest[i + 1])) for i in range(n - 1)]
    return nv, edges


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1025])
def test_triangle_lists_across_wave_and_workgroup_boundaries(K, monkeypatch, n):
    for edge_first in (True, False):
        nv, edges = _fan(n, edge_first)
        want = None
        for paths in PATHS:
            with monkeypatch.context() as mp:
                _set(mp, paths)
                with _load(K, nv, edges) as a:
                    _, _, want = _check(a, key=("fan", n, edge_first))
        assert want["info"]["n_triangles"] == 3 * n - 2 and want["info"]["n_cliques4"] == n - 1 and int(want["key0"].max()) == 2
        if edge_first:
            assert want["b"][:n].tolist() == [1] * n and want["c"][:n].tolist() == list(range(2, n + 2))


def test_cascade_of_random_cliques(K):
    """A union of random cliques on 120 vertices: many levels, and levels that take many sub-rounds to drain."""
    edges = R.clique_union(120, 220, 2, 9, 1)
    with _load(K, 120, edges) as a:
        _, _, want = _check(a, key="cascade")
        assert max(want["subrounds"]) >= 8 and len(want["levels"]) >= 6          # (asserted on the restatement's side)
        assert (want["info"]["n_triangles"], len(want["levels"]), sum(want["subrounds"])) == (20032, 9, 130)
        info = a.nucleus_info()
        assert info["n_levels"] == len(want["levels"]) and info["n_subrounds"] >= info["n_levels"]
        core = a.run_core()[1]
        _check(a, vmask=(core >= int(np.median(core))).astype(np.uint8))


@pytest.mark.parametrize("paths", [PATHS[0], PATHS[3]], ids=["default", "queued"])
def test_power_law_graph(K, monkeypatch, paths):
    _set(monkeypatch, paths)
    nv = 2000
    uv = K.gen_hug_edges(nv, int(2.45 * nv), 2.2, 11)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _, _, want = _check(a, key="power law")
        assert want["info"] == {"n_triangles": 50852, "n_cliques4": 115979, "theta_max": 14, "n_levels": 15}   # (DESIGN.md 4.6h quotes these)
        assert sum(want["subrounds"]) == 76
        core = a.run_core()[1]
        _check(a, vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8), key="power law, vmask")


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            eu, ev, _ = _check(a)
            assert (eu.tolist(), ev.tolist()) == (g["eu"], g["ev"]), g["name"]
            eu, ev, _ = _check(a, vmask=np.asarray(g["maxcore_mask"], np.uint8))
            assert (eu.tolist(), ev.tolist()) == (g["sub_eu"], g["sub_ev"]), g["name"]


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_clique_limit_refuses_and_keeps_the_previous_result(K, monkeypatch):
    LIMIT = K._lib.KOMB_ERR_LIMIT
    with _load(K, 12, R.clique(range(12))) as a:
        eu, ev, want = _check(a)
        assert want["info"]["n_cliques4"] == 495
        monkeypatch.setenv("KOMB_NUC_CAP", "100")
        assert _code(K, a.nucleus_run) == LIMIT
        _compare(a, len(eu), want)                                               # the previous result is still readable
        a.truss_run()                                                            # ... and gone with its k-truss result
        assert _code(K, a.nucleus_info) == K._lib.KOMB_ERR_STATE
        assert _code(K, a.nucleus_run) == LIMIT
        assert _code(K, a.nucleus_fetch) == K._lib.KOMB_ERR_STATE                # a refused first run leaves none
        monkeypatch.setenv("KOMB_NUC_CAP", "495")                                # at the limit, not above it
        a.nucleus_run()
        _compare(a, len(eu), want)
        monkeypatch.delenv("KOMB_NUC_CAP")
        a.nucleus_run()
        _compare(a, len(eu), want)


def test_call_order_and_lifetime(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, edges = R.hand_graph()
    want = R.decompose_edges(nv, edges)
    readers = lambda a: (a.nucleus_fetch, a.nucleus_fetch_edges, a.nucleus_fetch_vertices, a.nucleus_info,
                         lambda: a._check(lib.komb_nucleus_count(a._ctx, None)))
    with K.KombAccel() as a:
        for call in (a.nucleus_run,) + readers(a):                               # no graph
            assert _code(K, call) == ARG
        a.from_edges(nv, _i64(edges))
        assert _code(K, a.nucleus_run) == STATE                                  # no k-truss result
        a.run_core(); a.run_onion(); a.run_components("core", 0)
        assert _code(K, a.nucleus_run) == STATE
        a.truss_run()
        for call in readers(a):                                                  # count / fetch / info before a run
            assert _code(K, call) == STATE
        # the run makes the canonical endpoints nobody has fetched yet
        a.nucleus_run()
        _compare(a, len(want["edge_theta"]), want)
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core); a.run_structural_clusters(1, 2, 3); a.run_community_hierarchy()
        _compare(a, len(want["edge_theta"]), want)
        # NULL outputs are allowed
        assert lib.komb_nucleus_count(a._ctx, None) == 0
        assert lib.komb_nucleus_fetch(a._ctx, None, None, None, None, None) == 0
        assert lib.komb_nucleus_fetch_edges(a._ctx, None) == 0 and lib.komb_nucleus_fetch_vertices(a._ctx, None) == 0
        assert lib.komb_nucleus_info(a._ctx, *([None] * 6)) == 0
        # a new k-truss run of any kind drops it
        a.truss_run()
        for call in readers(a):
            assert _code(K, call) == STATE
        a.nucleus_run()
        _compare(a, len(want["edge_theta"]), want)
        a.truss_run(np.asarray([1] * 7 + [0] * 8, np.uint8))
        assert _code(K, a.nucleus_info) == STATE
        a.nucleus_run()
        assert a.nucleus_fetch_vertices().tolist() == [4] * 7 + [-1] * 8
        # a slice of the canonical edges is no k-truss result to decompose
        a.truss_run_slice(0, 2)
        assert _code(K, a.nucleus_fetch) == STATE and _code(K, a.nucleus_run) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, a.nucleus_run) == STATE
        a.truss_run_slice(0, 1)                                                  # the whole range
        a.nucleus_run()
        _compare(a, len(want["edge_theta"]), want)
        # komb_truss_unprepare drops the k-truss result and the decomposition with it
        a.truss_unprepare()
        for call in (a.nucleus_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        a.nucleus_run()
        _compare(a, len(want["edge_theta"]), want)
        # a new graph drops it
        a.from_edges(4, [[0, 1], [1, 2], [0, 2]])
        for call in (a.nucleus_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        assert a.run_nucleus()[2].tolist() == [0, 0, 0, -1]
        with pytest.raises(K.KombError):                                         # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.nucleus_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            tris, edge_theta, vertex_theta = a.run_nucleus()
            info = a.nucleus_info()
            out += [tris[k] for k in FIELDS] + [edge_theta, vertex_theta, np.asarray([info[k] for k in COUNTS])]
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "NUC_SHORT": "1", "NUC_HEAVY": "2"},
                                  {"POISON": "0x7FFFFFFF", "NUC_DEBUG": "1"}])
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
    """A run changes no k-core, onion, components, communities, densest, structural or k-truss result and no komb_stats field,
    and the resident k-truss preparation survives it."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv = 2000
    uv = K.gen_hug_edges(nv, int(2.45 * nv), 2.2, 11)                            # (the power-law graph above)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        layer, ocore = a.run_onion()
        eu, ev, tr = a.run_truss()
        clabel, csize = a.run_components("truss", 3)
        mlabel, msize = a.run_truss_communities(3)
        member, load, _ = a.run_densest_subgraph(8)
        slabel, ssize, srole, ssim = a.run_structural_clusters(1, 2, 3)
        cinfo, minfo, dinfo, sinfo = a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()
        st = a.stats()
        for _ in range(2):
            a.nucleus_run()
            assert a.stats() == st
            a.nucleus_fetch(); a.nucleus_fetch_edges(); a.nucleus_fetch_vertices(); a.nucleus_info()
            assert a.stats() == st
        _compare(a, len(eu), _want("power law", nv, eu, ev))
        got = (a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch()
               + a.densest_subgraph_fetch() + a.structural_clusters_fetch())
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load, slabel, ssize, srole, ssim), got):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()) == (cinfo, minfo, dinfo, sinfo)
        assert a.stats() == st
        e3 = a.run_truss()                                                       # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr), e3):
            assert np.array_equal(x, y)
