"""GPU tests of komb_community_hierarchy_run / _count / _fetch_nodes / _fetch_edges / _labels / _info: every array compared
exactly, every entry, with the reference of tests/community_hierarchy_ref.py (trussness taken from the library's own
run_truss, whose parity other tests own), info with the figures recomputed from the reference forest, and the walk-up
labels with the library's own komb_truss_communities_run for every k."""
import ctypes

import numpy as np
import pytest

import community_hierarchy_ref as CH
import components_ref as CR

pytestmark = pytest.mark.gpu
KMAX = -1
INFO = ("n_nodes", "n_roots", "k_max", "depth", "n_member_edges")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


def _expect(a, want):
    """Run the community hierarchy on a's k-truss result and compare nodes, node[] and info with the reference forest."""
    a.community_hierarchy_run()
    return _compare(a, want)


def _compare(a, want):
    """The held community hierarchy: nodes, node[] and info against the reference forest."""
    nodes, node = a.community_hierarchy_fetch_nodes(), a.community_hierarchy_fetch_edges()
    info = a.community_hierarchy_info()
    for f in CH.FIELDS:
        assert nodes[f].dtype == np.int32 and len(nodes[f]) == len(want[f]), f
        assert np.array_equal(nodes[f], want[f]), f
    assert node.dtype == np.int32 and np.array_equal(node, want["node"])
    assert tuple(info[f] for f in INFO) == CH.info(want) and info["ms"] >= 0.0
    return nodes, node, info


def _check(a, vmask=None, want_truss=None):
    eu, ev, tr = a.run_truss(vmask)
    if want_truss is not None:
        assert (eu.tolist(), ev.tolist(), tr.tolist()) == tuple(list(w) for w in want_truss)
    want = CH.community_hierarchy(a.nv, eu, ev, tr)
    CH.check_invariants(want)
    return _expect(a, want) + (want, tr)


def _check_graph(K, nv, uv):
    with K.KombAccel() as a:
        a.from_edges(nv, _i64(uv))
        return _check(a)


def _fields(nodes):
    return tuple(nodes[f].tolist() for f in CH.FIELDS)


def test_golden_graphs(K, golden):
    for g in golden:
        for load in ("raw", "csr"):
            with K.KombAccel() as a:
                if load == "raw":
                    a.from_edges(g["nv"], _i64(g["raw"]))
                else:
                    a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
                _check(a, want_truss=(g["eu"], g["ev"], g["trussness"]))
                _check(a, vmask=np.asarray(g["maxcore_mask"], np.uint8), want_truss=(g["sub_eu"], g["sub_ev"], g["sub_trussness"]))


EXAMPLE_A = (10, np.concatenate([_clique(range(5)), [[5, 0], [5, 1]], _clique([4, 6, 7, 8]), [[8, 9]]]))
EXAMPLE_B = (11, np.concatenate([_clique(range(5)), _clique(range(5, 10)), [[10, 0], [10, 1], [10, 5], [10, 6]], [[0, 5]]]))


def test_worked_examples(K):
    """The two examples of the definition, as stated and with their ids permuted."""
    nodes, node, info, _, tr = _check_graph(K, *EXAMPLE_A)
    assert tr.tolist() == [5, 5, 5, 5, 3, 5, 5, 5, 3, 5, 5, 5, 4, 4, 4, 4, 4, 4, 2]
    assert _fields(nodes) == ([3, 4, 5], [0, 12, 0], [-1, -1, 0], [12, 6, 10], [2, 6, 10])
    assert node.tolist() == [2, 2, 2, 2, 0, 2, 2, 2, 0, 2, 2, 2, 1, 1, 1, 1, 1, 1, -1]
    assert tuple(info[f] for f in INFO) == (3, 2, 5, 2, 18)
    nodes, node, info, _, _ = _check_graph(K, *EXAMPLE_B)
    assert _fields(nodes) == ([3, 5, 5], [0, 0, 13], [-1, 0, 0], [25, 10, 10], [5, 10, 10])
    assert tuple(info[f] for f in INFO) == (3, 1, 5, 2, 25)
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        for nv, uv in (EXAMPLE_A, EXAMPLE_B):
            _check_graph(K, nv, rng.permutation(nv)[uv])


def _two_k40(how):
    a, b = _clique(range(40)), _clique(range(40, 80))
    if how == "vertex":
        return 79, np.concatenate([a, _clique(range(39, 79))])
    if how == "edge":
        return 78, np.concatenate([a, _clique(range(38, 78))])
    # a strip of triangles 38-39-80, 39-80-40, 80-40-41: each shares an edge with the next
    return 81, np.concatenate([a, b, [[80, 38], [80, 39], [39, 40], [80, 40], [80, 41]]])


def test_edge_cases(K):
    with K.KombAccel() as a:
        for nv, uv, ne in ((0, [], 0), (7, [], 0), (4, [[3, 1]], 1), (6, [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]], 5)):
            a.from_edges(nv, _i64(uv))                   # empty, isolated vertices, one edge, a path
            nodes, node, info, _, _ = _check(a)
            assert all(len(nodes[f]) == 0 for f in CH.FIELDS) and node.tolist() == [-1] * ne
            assert tuple(info[f] for f in INFO) == (0, 0, 2, 0, 0)
            for k in (0, 2, KMAX):
                label, size = a.community_hierarchy_labels(k)
                assert label.tolist() == list(range(ne)) and size.tolist() == [1] * ne
            label, size = a.community_hierarchy_labels(3)
            assert label.tolist() == [-1] * ne and size.tolist() == [0] * ne
        a.from_edges(3, [[0, 1], [1, 2], [0, 2]])        # one triangle
        nodes, node, info, _, _ = _check(a)
        assert _fields(nodes) == ([3], [0], [-1], [3], [3]) and node.tolist() == [0, 0, 0]
        assert tuple(info[f] for f in INFO) == (1, 1, 3, 1, 3)
    nodes, _, info, _, _ = _check_graph(K, *_two_k40("vertex"))
    assert _fields(nodes) == ([40, 40], [0, 780], [-1, -1], [780, 780], [780, 780]) and info["depth"] == 1
    nodes, _, info, _, _ = _check_graph(K, *_two_k40("edge"))
    assert _fields(nodes) == ([40], [0], [-1], [2 * 780 - 1], [2 * 780 - 1])
    nodes, _, info, _, _ = _check_graph(K, *_two_k40("strip"))
    assert (nodes["k"].tolist(), nodes["parent"].tolist(), nodes["size"].tolist(), nodes["shell"].tolist()) == (
        [3, 40, 40], [-1, 0, 0], [2 * 780 + 5, 780, 780], [5, 780, 780])
    assert tuple(info[f] for f in INFO) == (3, 1, 40, 2, 2 * 780 + 5)
    # raw input with loops and duplicates
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 300, (1200, 2))
    _check_graph(K, 310, np.concatenate([raw, raw[:100], raw[:100, ::-1], np.stack([np.arange(50)] * 2, 1)]))


def test_many_levels(K):
    """The chain K3, K4, ..., K40 in which consecutive cliques share an edge: 38 levels, one node per level, depth 38."""
    parts, off = [], 0
    for n in range(3, 41):
        parts.append(_clique(range(off, off + n)))
        off += n - 2
    nv, uv = off + 2, np.concatenate(parts)
    for ids in (np.arange(nv), np.random.default_rng(8).permutation(nv)):
        nodes, _, info, _, _ = _check_graph(K, nv, ids[uv])
        assert nodes["k"].tolist() == list(range(3, 41)) and nodes["parent"].tolist() == list(range(-1, 37))
        assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == (38, 1, 40, 38)


def _book(pages):
    p = np.arange(2, 2 + pages)
    return 2 + pages, np.concatenate([[[0, 1]], np.stack([np.zeros(pages, np.int64), p], 1), np.stack([np.ones(pages, np.int64), p], 1)])


def _strip(n):
    i = np.arange(n + 1)
    return n + 2, np.concatenate([np.stack([i, i + 1], 1), np.stack([i[:-1], i[:-1] + 2], 1)])


@pytest.mark.parametrize("shape", ["strip", "book"])
def test_deep_trees_and_the_hot_root(K, shape):
    """A strip of 100 000 triangles: one node, reached through long parent chains.  A book of 5 000 pages: every link goes
    into one root, and the spine's walked side is past the heavy class boundary.  Ids in construction order and scattered."""
    nv, uv = _strip(100000) if shape == "strip" else _book(5000)
    ne = 200001 if shape == "strip" else 10001
    for ids in (np.arange(nv), np.random.default_rng(9).permutation(nv)):
        nodes, node, info, _, _ = _check_graph(K, nv, ids[uv])
        assert _fields(nodes) == ([3], [0], [-1], [ne], [ne]) and not node.any()
        assert tuple(info[f] for f in INFO) == (1, 1, 3, 1, ne)


CLASSES = [{}, {"COMM_SHORT": "1000000000", "COMM_HEAVY": "2000000000"}, {"COMM_SHORT": "1", "COMM_HEAVY": "1000000000"},
           {"COMM_SHORT": "1", "COMM_HEAVY": "2"}]


@pytest.mark.parametrize("seed", [1, 2])
def test_length_classes(K, monkeypatch, seed):
    """The defaults, then every edge through its lane, through its wave (walked sides of one entry stay with the lane) and
    through the queued workgroup path: identical to one another and to the reference."""
    nv, uv = CR.composite(K.gen_hug_edges, seed)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        eu, ev, tr = a.run_truss()
        want = CH.community_hierarchy(nv, eu, ev, tr)
        CH.check_invariants(want)
        for opts in CLASSES:
            for o in ("COMM_SHORT", "COMM_HEAVY"):
                if o in opts:
                    monkeypatch.setenv("KOMB_" + o, opts[o])
                else:
                    monkeypatch.delenv("KOMB_" + o, raising=False)
            _expect(a, want)


@pytest.fixture(scope="module")
def generated(K):
    """The generated graphs, each made once."""
    cache = {}

    def get(nv, alpha):
        if (nv, alpha) not in cache:
            cache[nv, alpha] = K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11)
        return cache[nv, alpha]
    return get


def _walk_up_equals_single_k(a, tr):
    """community_hierarchy_labels(k) against komb_truss_communities_run(k) + fetch, for every k; the forest's invariants."""
    nodes, node = a.run_community_hierarchy()
    CH.check_invariants(dict(nodes, node=node))
    tmax = int(tr.max()) if len(tr) else 2
    for k in list(range(0, tmax + 2)) + [KMAX]:
        want_label, want_size = a.run_truss_communities(k)
        label, size = a.community_hierarchy_labels(k)
        assert np.array_equal(label, want_label) and np.array_equal(size, want_size), k
        again = a.truss_communities_fetch()              # the stored result of the single-k path is not touched
        assert np.array_equal(again[0], want_label) and np.array_equal(again[1], want_size), k


@pytest.mark.parametrize("nv", [1000, 20000])
@pytest.mark.parametrize("alpha", [2.1, 2.2, 2.6])
def test_generated_graphs(K, generated, nv, alpha):
    with K.KombAccel() as a:
        a.from_edges(nv, generated(nv, alpha))
        _, _, _, _, tr = _check(a)
        _walk_up_equals_single_k(a, tr)


def test_walk_up_equals_communities_run_200k(K):
    nv = 200000
    with K.KombAccel() as a:
        a.from_edges(nv, K.gen_hug_edges(nv, 490000, 2.6, 11))
        _, _, tr = a.run_truss()
        _walk_up_equals_single_k(a, tr)


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    reads = lambda a: (a.community_hierarchy_fetch_nodes, a.community_hierarchy_fetch_edges, lambda: a.community_hierarchy_labels(3),
                       a.community_hierarchy_info)
    lib = K._lib.load()
    with K.KombAccel() as a:
        for call in (a.community_hierarchy_run,) + reads(a):                # no graph
            assert _code(K, call) == ARG
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [2, 3], [4, 5]])
        for call in (a.community_hierarchy_run,) + reads(a):                # before any truss run
            assert _code(K, call) == STATE
        a.truss_run_slice(0, 2)                                             # a slice is not a complete k-truss result
        assert _code(K, a.community_hierarchy_run) == STATE
        a.truss_run_slice(0, 1)                                             # the whole range
        nodes, node = a.run_community_hierarchy()
        assert _fields(nodes) == ([3], [0], [-1], [3], [3]) and node.tolist() == [0, 0, 0, -1, -1]
        # argument errors of _labels; NULL outputs
        assert lib.komb_community_hierarchy_labels(a._ctx, -2, None, None) == ARG
        assert lib.komb_community_hierarchy_labels(a._ctx, -5, None, None) == ARG
        for k in (KMAX, 0, 3, 4):
            assert lib.komb_community_hierarchy_labels(a._ctx, k, None, None) == 0
        size = np.full(5, -9, np.int32)
        assert lib.komb_community_hierarchy_labels(a._ctx, 2, None, K._lib.ptr(size)) == 0 and size.tolist() == [3, 3, 3, 1, 1]
        assert a.community_hierarchy_labels(KMAX)[0].tolist() == [0, 0, 0, -1, -1]
        assert a.community_hierarchy_labels(4)[0].tolist() == [-1] * 5 and a.community_hierarchy_labels(4)[1].tolist() == [0] * 5
        n = ctypes.c_int64(-1)
        assert lib.komb_community_hierarchy_count(a._ctx, None) == 0
        assert lib.komb_community_hierarchy_count(a._ctx, ctypes.byref(n)) == 0 and n.value == 1
        assert lib.komb_community_hierarchy_fetch_nodes(a._ctx, None, None, None, None, None) == 0
        one = np.full(1, -9, np.int32)
        assert lib.komb_community_hierarchy_fetch_nodes(a._ctx, None, None, None, K._lib.ptr(one), None) == 0 and one.tolist() == [3]
        assert lib.komb_community_hierarchy_fetch_edges(a._ctx, None) == 0
        assert lib.komb_community_hierarchy_info(a._ctx, None, None, None, None, None, None) == 0
        # a new truss run of any kind drops the result
        a.truss_run()
        for call in reads(a):
            assert _code(K, call) == STATE
        assert a.run_community_hierarchy()[1].tolist() == [0, 0, 0, -1, -1]   # (endpoints nobody has fetched yet)
        a.truss_run_slice(1, 2)
        for call in (a.community_hierarchy_run,) + reads(a):
            assert _code(K, call) == STATE
        a.truss_run()
        a.community_hierarchy_run()
        a.truss_unprepare()
        for call in (a.community_hierarchy_run,) + reads(a):
            assert _code(K, call) == STATE
        # a k-truss result under a vmask, in its own canonical order
        a.truss_run(np.asarray([1, 1, 1, 0, 1, 1], np.uint8))
        nodes, node = a.run_community_hierarchy()
        assert _fields(nodes) == ([3], [0], [-1], [3], [3]) and node.tolist() == [0, 0, 0, -1]
        # calls that fail leave it readable
        assert lib.komb_community_hierarchy_labels(a._ctx, -2, None, None) == ARG
        assert a.community_hierarchy_fetch_edges().tolist() == [0, 0, 0, -1] and a.community_hierarchy_info()["n_nodes"] == 1
        # a new graph drops it
        a.from_edges(3, [[0, 1]])
        for call in (a.community_hierarchy_run,) + reads(a):
            assert _code(K, call) == STATE
        with pytest.raises(K.KombError):                                    # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        for call in (a.community_hierarchy_run,) + reads(a):
            assert _code(K, call) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        for vmask in (None, (np.arange(nv) % 3 != 0).astype(np.uint8)):
            _, _, tr = a.run_truss(vmask)
            nodes, node = a.run_community_hierarchy()
            info = a.community_hierarchy_info()
            out += [nodes[f] for f in CH.FIELDS] + [node, np.asarray([info[f] for f in INFO])]
            for k in (2, 3, max(int(tr.max()) // 2, 3) if len(tr) else 3, KMAX):
                out += list(a.community_hierarchy_labels(k))
        return out
    finally:
        if own:
            a.close()


@pytest.fixture(scope="module")
def three_graphs(K):
    """Larger, smaller, larger -- and their results on fresh contexts without options, computed once."""
    graphs = [CR.composite(K.gen_hug_edges, 3), (900, K.gen_hug_edges(900, 2200, 2.6, 6)), (50000, K.gen_hug_edges(50000, 122500, 2.1, 7))]
    return graphs, [_all_results(K, nv, uv) for nv, uv in graphs]


@pytest.mark.parametrize("poison", [None, "0xFFFFFFFF", "0x00000001", "0x7FFFFFFF", "0xA5A5A5A5"])
def test_poison_and_reuse_change_nothing(K, monkeypatch, three_graphs, poison):
    graphs, want = three_graphs
    if poison:
        monkeypatch.setenv("KOMB_POISON", poison)
    with K.KombAccel() as a:                     # one context across the three graphs
        for (nv, uv), w in zip(graphs, want):
            for _ in range(2 if poison is None else 1):
                got = _all_results(K, nv, uv, a)
                assert len(got) == len(w)
                for x, y in zip(got, w):
                    assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """A run changes no k-core, onion, k-truss, components, vertex-hierarchy, communities or CoreA result and no komb_stats
    field; none of their calls changes or drops this result."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv, uv = CR.composite(K.gen_hug_edges, 5)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)

        def others():
            h = a.hierarchy_fetch_nodes()
            return (a.core_fetch() + a.onion_fetch() + a.truss_fetch(with_support=True) + a.components_fetch()
                    + a.truss_communities_fetch() + (a.truss_communities_fetch_vertices(), a.hierarchy_fetch_vertices())
                    + tuple(h[f] for f in CH.FIELDS))

        deg, core = a.run_core()
        a.run_onion()
        a.run_truss()
        a.run_components("core", 2)
        a.run_truss_communities(4)
        a.run_hierarchy("truss")
        score = a.get_anomaly_score(deg, core)
        cinfo, minfo, hinfo = a.components_info(), a.truss_communities_info(), a.hierarchy_info()
        before, st = others(), a.stats()
        for _ in range(2):
            a.community_hierarchy_run()
            a.community_hierarchy_labels(3)
            assert a.stats() == st
        for x, y in zip(others(), before):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.hierarchy_info(), a.stats()) == (cinfo, minfo, hinfo, st)
        assert np.array_equal(a.get_anomaly_score(deg, core), score)
        # the result survives runs of everything that does not replace the k-truss result
        nodes, node = a.run_community_hierarchy()
        info, labels = a.community_hierarchy_info(), a.community_hierarchy_labels(4)
        a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_components("core", 1); a.run_truss_communities(3)
        a.run_hierarchy("core"); a.run_hierarchy("truss"); a.get_anomaly_score(deg, core)
        again = a.community_hierarchy_fetch_nodes()
        assert all(np.array_equal(again[f], nodes[f]) for f in CH.FIELDS)
        assert np.array_equal(a.community_hierarchy_fetch_edges(), node) and a.community_hierarchy_info() == info
        assert all(np.array_equal(x, y) for x, y in zip(a.community_hierarchy_labels(4), labels))
