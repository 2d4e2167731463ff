"""GPU tests of komb_nucleus_hierarchy_run / _count / _fetch_nodes / _fetch_triangles / _labels / _nuclei / _info: every node
field, every node[] entry, every label and size of every threshold, every row of the nuclei of every populated level and every
count of info is compared exactly with tests/nucleus_hierarchy_ref.py, which is fed the library's own run_truss() edge list
and nucleus_fetch() (whose parity other tests own)."""
import ctypes

import numpy as np
import pytest

import nucleus_hierarchy_ref as R
import nucleus_ref as N

pytestmark = pytest.mark.gpu

INFO = ("n_nodes", "n_roots", "theta_max", "depth", "n_member_triangles")
LANE, WAVE = {"NUC_SHORT": "1000000000"}, {"NUC_SHORT": "1"}     # the two ways a walked tail is enumerated


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


_WANT = {}


def _want(key, nv, eu, ev, theta):
    """(forest, decomposition) of one k-truss result, computed once per module and never changed."""
    if key is None:
        return R.hierarchy(nv, eu, ev, theta)
    if key not in _WANT:
        _WANT[key] = (eu.copy(), ev.copy(), R.hierarchy(nv, eu, ev, theta))
    seu, sev, want = _WANT[key]
    assert np.array_equal(seu, eu) and np.array_equal(sev, ev) and np.array_equal(want[1]["theta"], theta)
    return want


def _nodes(h):
    return [tuple(int(h[f][i]) for f in R.FIELDS) for i in range(len(h["k"]))]


def _compare_forest(a, h, dec):
    nodes, node, info = a.nucleus_hierarchy_fetch_nodes(), a.nucleus_hierarchy_fetch_triangles(), a.nucleus_hierarchy_info()
    assert tuple(info[k] for k in INFO) == R.info(h, dec["theta"])
    assert info["ms"] >= 0.0
    for name in R.FIELDS:
        assert nodes[name].dtype == np.int32 and len(nodes[name]) == len(h["k"]), name
        assert np.array_equal(nodes[name], h[name]), name
    assert node.dtype == np.int32 and len(node) == len(dec["theta"])
    assert np.array_equal(node, h["node"])


def _compare_levels(K, a, h, dec):
    lib = K._lib.load()
    top = int(dec["theta"].max()) if len(dec["theta"]) else -1
    for k in [-1, 0] + list(range(1, max(top, 1) + 2)):                  # every k up to theta_max + 1
        label, size = a.nucleus_hierarchy_labels(k)
        wl, ws = R.walk_up(h, dec["theta"], k)
        assert label.dtype == np.int32 and size.dtype == np.int32
        assert np.array_equal(label, wl) and np.array_equal(size, ws), k
    for k in [-1, 0, top + 1] + sorted(set(h["k"].tolist())):            # every populated level
        got, want = a.nucleus_hierarchy_nuclei(k), R.nuclei(h, dec, k)
        for name in R.NUCLEI_FIELDS:
            assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (k, name)
        n = ctypes.c_int64(-7)
        assert lib.komb_nucleus_hierarchy_nuclei(a._ctx, k, 0, ctypes.byref(n), None, None, None, None) == 0     # count only
        assert n.value == len(want["rep"])
        if n.value:                                                      # too little room: refused, nothing written
            bufs = [np.full(n.value, -7, np.int32) for _ in range(4)]
            m = ctypes.c_int64(-7)
            assert lib.komb_nucleus_hierarchy_nuclei(a._ctx, k, n.value - 1, ctypes.byref(m), *(K._lib.ptr(b) for b in bufs)) == K._lib.KOMB_ERR_ARG
            assert m.value == -7 and all((b == -7).all() for b in bufs)
            one = np.full(n.value, -7, np.int32)                         # any subset of the arrays
            assert lib.komb_nucleus_hierarchy_nuclei(a._ctx, k, n.value, None, None, None, K._lib.ptr(one), None) == 0
            assert np.array_equal(one, want["n_edges"])


def _check(K, a, vmask=None, key=None):
    """k-truss (whole graph or vmask), the nucleus decomposition, the hierarchy: everything against the reference."""
    eu, ev, _ = a.run_truss(vmask)
    a.nucleus_run()
    h, dec = _want(key, a.nv, eu, ev, a.nucleus_fetch()["theta"])
    a.nucleus_hierarchy_run()
    _compare_forest(a, h, dec)
    _compare_levels(K, a, h, dec)
    R.check_invariants(h, dec["theta"])
    return h, dec


def _load(K, nv, uv):
    a = K.KombAccel()
    a.from_edges(nv, _i64(uv))
    return a


def _set(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)


def test_degenerate_graphs(K):
    with K.KombAccel() as a:
        for nv, edges, vmask, top in ((0, np.zeros((0, 2)), None, -1),                        # the empty graph is not an error
                                      (7, np.zeros((0, 2)), None, -1),                        # vertices without edges
                                      (6, [[0, 1], [1, 2], [2, 3], [3, 4], [1, 5]], None, -1),  # edges without a triangle
                                      (6, [[0, 1], [1, 2], [0, 2], [4, 5]], np.asarray([1, 0, 0, 1, 1, 0], np.uint8), -1),   # a vmask that keeps no edge
                                      (4, [[0, 1], [1, 3], [0, 3]], None, 0),                 # one triangle: theta 0, no nucleus
                                      (6, [[0, 1], [1, 2], [0, 2], [2, 3], [3, 4], [2, 4]], None, 0)):
            a.from_edges(nv, edges)
            h, dec = _check(K, a, vmask)
            info = a.nucleus_hierarchy_info()
            assert [info[k] for k in INFO] == [0, 0, top, 0, 0]
            assert a.nucleus_hierarchy_fetch_triangles().tolist() == [-1] * len(dec["theta"])


WORKED = {
    "K_4": (lambda: (4, N.clique(range(4))), [(1, 0, -1, 4, 4)]),
    "two K_5 sharing a triangle": (lambda: (7, N.clique([0, 1, 2, 3, 4]) + N.clique([0, 1, 2, 5, 6])), [(2, 0, -1, 19, 19)]),
    "two K_5 sharing an edge": (R.two_k5_sharing_an_edge, [(2, 0, -1, 10, 10), (2, 3, -1, 10, 10)]),
    "K_6 plus a vertex on three of its vertices": (R.k6_plus_vertex, [(1, 0, -1, 23, 3), (3, 0, 0, 20, 20)]),
}


@pytest.mark.parametrize("name", list(WORKED))
def test_worked_examples(K, name):
    make, nodes = WORKED[name]
    nv, edges = make()
    with _load(K, nv, edges) as a:
        _check(K, a)
        assert _nodes(a.nucleus_hierarchy_fetch_nodes()) == nodes


def test_two_k6_joined_by_a_band(K):
    with _load(K, *R.two_k6_joined_by_a_band()) as a:
        h, dec = _check(K, a)
        nodes = _nodes(a.nucleus_hierarchy_fetch_nodes())
        assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (48, 33)
        assert len(nodes) == 3 and nodes[0][0] == 1 and nodes[0][2:] == (-1, 48, 8)
        assert [(n[0], n[2], n[3], n[4]) for n in nodes[1:]] == [(3, 0, 20, 20)] * 2


def test_hand_graph_and_its_reversed_labelling(K):
    nv, edges = N.hand_graph()
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        with _load(K, nv, ids[_i64(edges)]) as a:
            h, dec = _check(K, a)
            nodes = _nodes(a.nucleus_hierarchy_fetch_nodes())
            assert sorted((n[0], n[2], n[3]) for n in nodes) == [(1, -1, 4), (2, -1, 10), (4, -1, 35)]
            assert (a.nucleus_hierarchy_fetch_triangles() < 0).sum() == 1
            if ids[0] == 0:
                assert [n[1] for n in nodes] == [45, 35, 0] and a.nucleus_hierarchy_fetch_triangles()[-1] == -1
            _check(K, a, vmask=(np.arange(nv) != ids[0]).astype(np.uint8))         # without a K_7 vertex: a K_6 is left
            assert a.nucleus_hierarchy_info()["theta_max"] == 3


@pytest.mark.parametrize("n", [63, 64, 65, 1025])
def test_one_triangle_in_n_cliques(K, monkeypatch, n):
    """The per-wave slot reservation of the record stream at the wave boundary, through the wave and the lane path."""
    nv, edges = R.triangle_in_n_cliques(n)
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        for paths in (WAVE, LANE, {}):
            with monkeypatch.context() as mp:
                _set(mp, paths)
                with _load(K, nv, ids[_i64(edges)]) as a:
                    h, dec = _check(K, a, key=("k3", n, int(ids[0])))
                    assert int(dec["key0"].max()) == n and dec["info"]["n_cliques4"] == n
                    assert _nodes(a.nucleus_hierarchy_fetch_nodes()) == [(1, 0, -1, 3 * n + 1, 3 * n + 1)]


def test_k40(K):
    """One class: the hot-root LDS sums."""
    with _load(K, 40, N.clique(range(40))) as a:
        h, dec = _check(K, a)
        assert dec["info"]["n_cliques4"] == 91390
        assert _nodes(a.nucleus_hierarchy_fetch_nodes()) == [(37, 0, -1, 9880, 9880)]
        got = a.nucleus_hierarchy_nuclei(-1)
        assert [got[f].tolist() for f in R.NUCLEI_FIELDS] == [[0], [9880], [780], [40]]


def test_disjoint_k4(K):
    """All roots: the log cursor and the node sort across workgroups."""
    with _load(K, *R.disjoint_k4(5000)) as a:
        _check(K, a)
        assert _nodes(a.nucleus_hierarchy_fetch_nodes()) == [(1, 4 * i, -1, 4, 4) for i in range(5000)]
        assert a.nucleus_hierarchy_info()["n_roots"] == 5000


def test_band(K):
    """Long hook chains."""
    with _load(K, *R.band(20000)) as a:
        h, dec = _check(K, a)
        assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (59992, 19997)
        assert _nodes(a.nucleus_hierarchy_fetch_nodes()) == [(1, 0, -1, 59992, 59992)]


def test_clique_chain(K):
    """K_4 ... K_24: 21 levels, depth 21, three launches per level."""
    with _load(K, *R.clique_chain(24)) as a:
        h, dec = _check(K, a)
        nodes = a.nucleus_hierarchy_fetch_nodes()
        assert nodes["k"].tolist() == list(range(1, 22)) and nodes["parent"].tolist() == list(range(-1, 20))
        info = a.nucleus_hierarchy_info()
        assert (info["n_nodes"], info["n_roots"], info["depth"], info["theta_max"]) == (21, 1, 21, 21)
    with _load(K, *R.clique_chain(9)) as a:
        _check(K, a)
        assert a.nucleus_hierarchy_fetch_nodes()["size"].tolist() == [204, 201, 192, 173, 139, 84]


@pytest.mark.parametrize("paths", [{}, WAVE, LANE], ids=["default", "wave", "lane"])
def test_clique_union(K, monkeypatch, paths):
    _set(monkeypatch, paths)
    with _load(K, 600, N.clique_union(600, 150, 4, 12, 11)) as a:
        h, dec = _check(K, a, key="union")
        assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (14223, 25839)
        info = a.nucleus_hierarchy_info()
        assert (info["n_nodes"], info["n_roots"], info["depth"]) == (161, 79, 4)
        core = a.run_core()[1]
        _check(K, a, vmask=(core >= int(np.median(core))).astype(np.uint8), key="union, vmask")


def test_power_law_graph(K):
    nv = 5000
    uv = K.gen_hug_edges(nv, 12250, 2.1, 7)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        h, dec = _check(K, a, key="power law")
        assert len(h["k"]) > 1 and dec["info"]["n_cliques4"] > 0
        core = a.run_core()[1]
        _check(K, a, vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8), key="power law, vmask")


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            _check(K, a)
            _check(K, a, vmask=np.asarray(g["maxcore_mask"], np.uint8))


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_lifetime(K, monkeypatch):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, edges = N.hand_graph()
    h, dec = R.hierarchy_edges(nv, edges)
    readers = lambda a: (a.nucleus_hierarchy_fetch_nodes, a.nucleus_hierarchy_fetch_triangles, a.nucleus_hierarchy_labels,
                         a.nucleus_hierarchy_nuclei, a.nucleus_hierarchy_info,
                         lambda: a._check(lib.komb_nucleus_hierarchy_count(a._ctx, None)))
    with K.KombAccel() as a:
        for call in (a.nucleus_hierarchy_run,) + readers(a):                     # no graph
            assert _code(K, call) == ARG
        a.from_edges(nv, _i64(edges))
        assert _code(K, a.nucleus_hierarchy_run) == STATE                        # no k-truss result, no decomposition
        a.truss_run()
        assert _code(K, a.nucleus_hierarchy_run) == STATE                        # _run before komb_nucleus_run
        for call in readers(a):
            assert _code(K, call) == STATE
        a.nucleus_run()
        for call in readers(a):                                                  # readers before a run
            assert _code(K, call) == STATE
        a.nucleus_hierarchy_run()
        _compare_forest(a, h, dec)
        first = (a.nucleus_hierarchy_fetch_nodes(), a.nucleus_hierarchy_fetch_triangles())
        a.nucleus_hierarchy_run()                                                # a second run gives identical arrays
        again = (a.nucleus_hierarchy_fetch_nodes(), a.nucleus_hierarchy_fetch_triangles())
        assert all(np.array_equal(first[0][f], again[0][f]) for f in R.FIELDS) and np.array_equal(first[1], again[1])
        # a bad threshold is refused and changes nothing
        assert _code(K, lambda: a.nucleus_hierarchy_labels(-2)) == ARG and _code(K, lambda: a.nucleus_hierarchy_nuclei(-2)) == ARG
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core); a.run_structural_clusters(1, 2, 3); a.run_community_hierarchy()
        _compare_forest(a, h, dec)
        _compare_levels(K, a, h, dec)
        # NULL outputs are allowed
        assert lib.komb_nucleus_hierarchy_count(a._ctx, None) == 0
        assert lib.komb_nucleus_hierarchy_fetch_nodes(a._ctx, None, None, None, None, None) == 0
        assert lib.komb_nucleus_hierarchy_fetch_triangles(a._ctx, None) == 0
        assert lib.komb_nucleus_hierarchy_labels(a._ctx, 1, None, None) == 0
        assert lib.komb_nucleus_hierarchy_nuclei(a._ctx, 1, 0, None, None, None, None, None) == 0
        assert lib.komb_nucleus_hierarchy_info(a._ctx, *([None] * 6)) == 0
        # a refused komb_nucleus_run keeps the decomposition, and so the hierarchy that indexes it
        monkeypatch.setenv("KOMB_NUC_CAP", "10")
        assert _code(K, a.nucleus_run) == K._lib.KOMB_ERR_LIMIT
        monkeypatch.delenv("KOMB_NUC_CAP")
        _compare_forest(a, h, dec)
        # a new komb_nucleus_run drops it
        a.nucleus_run()
        for call in readers(a):
            assert _code(K, call) == STATE
        a.nucleus_hierarchy_run()
        _compare_forest(a, h, dec)
        # a new k-truss run of any kind drops it (with the decomposition)
        a.truss_run()
        for call in (a.nucleus_hierarchy_run,) + readers(a):
            assert _code(K, call) == STATE
        a.nucleus_run(); a.nucleus_hierarchy_run()
        _compare_forest(a, h, dec)
        a.truss_run(np.asarray([1] * 7 + [0] * 8, np.uint8))
        assert _code(K, a.nucleus_hierarchy_info) == STATE
        a.nucleus_run(); a.nucleus_hierarchy_run()
        assert _nodes(a.nucleus_hierarchy_fetch_nodes()) == [(4, 0, -1, 35, 35)]
        # komb_truss_unprepare drops the k-truss result and everything that indexes it
        a.truss_unprepare()
        for call in (a.nucleus_hierarchy_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run(); a.nucleus_run(); a.nucleus_hierarchy_run()
        _compare_forest(a, h, dec)
        # a new graph drops it
        a.from_edges(4, N.clique(range(4)))
        for call in (a.nucleus_hierarchy_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run(); a.nucleus_run()
        nodes, node = a.run_nucleus_hierarchy()
        assert _nodes(nodes) == [(1, 0, -1, 4, 4)] and node.tolist() == [0] * 4
        with pytest.raises(K.KombError):                                         # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.nucleus_hierarchy_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            a.nucleus_run()
            nodes, node = a.run_nucleus_hierarchy()
            info = a.nucleus_hierarchy_info()
            out += [nodes[k] for k in R.FIELDS] + [node, np.asarray([info[k] for k in INFO])]
            for k in (1, 2, -1):
                out += list(a.nucleus_hierarchy_labels(k)) + list(a.nucleus_hierarchy_nuclei(k).values())
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "NUC_SHORT": "1"}, {"POISON": "0x7FFFFFFF"}])
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
    nv = 5000
    uv = K.gen_hug_edges(nv, 12250, 2.1, 7)                                      # (the power-law graph above)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        layer, ocore = a.run_onion()
        eu, ev, tr = a.run_truss()
        clabel, csize = a.run_components("truss", 3)
        mlabel, msize = a.run_truss_communities(3)
        member, load, _ = a.run_densest_subgraph(8)
        slabel, ssize, srole, ssim = a.run_structural_clusters(1, 2, 3)
        hnodes, hnode = a.run_community_hierarchy()
        tris, etheta, vtheta = a.run_nucleus()
        infos = lambda: (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info(),
                         a.community_hierarchy_info(), a.nucleus_info())
        before = infos()
        st = a.stats()
        h, dec = _want("power law", nv, eu, ev, tris["theta"])
        for _ in range(2):
            a.nucleus_hierarchy_run()
            assert a.stats() == st
            a.nucleus_hierarchy_fetch_nodes(); a.nucleus_hierarchy_fetch_triangles(); a.nucleus_hierarchy_labels(2)
            a.nucleus_hierarchy_nuclei(2); a.nucleus_hierarchy_info()
            assert a.stats() == st
        _compare_forest(a, h, dec)
        got = (a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch()
               + a.densest_subgraph_fetch() + a.structural_clusters_fetch() + (a.community_hierarchy_fetch_edges(),)
               + tuple(a.nucleus_fetch()[k] for k in a.NUCLEUS_FIELDS) + (a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()))
        was = (deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load, slabel, ssize, srole, ssim, hnode) \
            + tuple(tris[k] for k in a.NUCLEUS_FIELDS) + (etheta, vtheta)
        assert len(got) == len(was)
        for x, y in zip(was, got):
            assert np.array_equal(x, y)
        now = a.community_hierarchy_fetch_nodes()
        assert all(np.array_equal(hnodes[f], now[f]) for f in R.FIELDS)
        assert infos() == before
        assert a.stats() == st
        e3 = a.run_truss()                                                       # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr), e3):
            assert np.array_equal(x, y)
