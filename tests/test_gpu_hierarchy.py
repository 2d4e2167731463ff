"""GPU tests of komb_hierarchy_run / _count / _fetch_nodes / _fetch_vertices / _info: every array compared exactly, every
entry, with the reference of tests/hierarchy_ref.py (coreness / trussness taken from the library's own run_core / run_truss,
whose parity other tests own), and info with the figures recomputed from the reference forest."""
import ctypes

import numpy as np
import pytest

import components_ref as R
import hierarchy_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _expect(a, kind, want):
    """Run the hierarchy of `kind` on a and compare the node arrays, node[] and info with the reference forest."""
    a.hierarchy_run(kind)
    return _compare(a, kind, want)


def _compare(a, kind, want):
    """The held hierarchy of `kind`: the node arrays, node[] and info against the reference forest."""
    nodes, node = a.hierarchy_fetch_nodes(), a.hierarchy_fetch_vertices()
    info = a.hierarchy_info()
    for f in H.FIELDS:
        assert nodes[f].dtype == np.int32 and len(nodes[f]) == len(want[f]), (kind, f)
        assert np.array_equal(nodes[f], want[f]), (kind, f)
    assert node.dtype == np.int32 and np.array_equal(node, want["node"]), kind
    assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == H.info(want, kind), kind
    assert info["kind"] == {"core": 0, "truss": 1}[kind] and info["ms"] >= 0.0
    return nodes, node, info


def _check_core(a, want_core=None):
    rowptr, col = a.get_csr()
    _, core = a.run_core()
    if want_core is not None:
        assert core.tolist() == list(want_core)
    want = H.core_hierarchy(rowptr, col, core)
    H.check_invariants(want, True)
    return _expect(a, "core", want)


def _check_truss(a, vmask=None, want_truss=None):
    eu, ev, tr = a.run_truss(vmask)
    if want_truss is not None:
        assert (eu.tolist(), ev.tolist(), tr.tolist()) == tuple(list(w) for w in want_truss)
    want = H.truss_hierarchy(a.nv, eu, ev, tr)
    H.check_invariants(want, False)
    return _expect(a, "truss", want)


def _check_both(K, nv, uv):
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        return _check_core(a), _check_truss(a)


def test_golden_graphs(K, golden):
    for g in golden:
        for load in ("raw", "csr"):
            with K.KombAccel() as a:
                if load == "raw":
                    a.from_edges(g["nv"], _i64(g["raw"]))
                else:
                    a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
                _check_core(a, g["coreness"])
                _check_truss(a, want_truss=(g["eu"], g["ev"], g["trussness"]))
                _check_truss(a, vmask=np.asarray(g["maxcore_mask"], np.uint8), want_truss=(g["sub_eu"], g["sub_ev"], g["sub_trussness"]))


def _k4(off):
    return [[off + a, off + b] for a in range(4) for b in range(a + 1, 4)]


def test_worked_examples(K):
    """The two examples of the definition, as stated and with their ids permuted."""
    nv, uv = 11, _i64(_k4(0) + _k4(4) + [[8, 0], [8, 4], [9, 8]])
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        nodes, node, info = _check_core(a, [3] * 8 + [2, 1, 0])
        assert {f: nodes[f].tolist() for f in H.FIELDS} == {"k": [0, 1, 2, 3, 3], "rep": [10, 0, 0, 0, 4], "parent": [-1, -1, 1, 2, 2],
                                                            "size": [1, 10, 9, 4, 4], "shell": [1, 1, 1, 4, 4]}
        assert node.tolist() == [3, 3, 3, 3, 4, 4, 4, 4, 2, 1, 0]
        assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == (5, 2, 3, 3)
    tnv, tuv = 8, _i64(_k4(0) + _k4(4) + [[0, 4]])
    with K.KombAccel() as a:
        a.from_edges(tnv, tuv)
        nodes, node, info = _check_truss(a)
        assert {f: nodes[f].tolist() for f in H.FIELDS} == {"k": [2, 4, 4], "rep": [0, 0, 4], "parent": [-1, 0, 0], "size": [8, 4, 4],
                                                            "shell": [0, 4, 4]}
        assert node.tolist() == [1, 1, 1, 1, 2, 2, 2, 2]
        assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == (3, 1, 4, 2)
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        _check_both(K, nv, rng.permutation(nv)[uv])
        _check_both(K, tnv, rng.permutation(tnv)[tuv])


def _two_k40(bridge_vertex):
    n = 40
    iu = np.stack(np.triu_indices(n, 1), 1)
    link = [[0, 2 * n], [2 * n, n]] if bridge_vertex else [[0, n]]
    return 2 * n + (1 if bridge_vertex else 0), np.concatenate([iu, iu + n, np.asarray(link)])


def test_edge_cases(K):
    with K.KombAccel() as a:
        # the empty graph
        a.from_edges(0, np.zeros((0, 2)))
        a.run_core(); a.run_truss()
        for kind, kmax in (("core", 0), ("truss", 2)):
            nodes, node = a.run_hierarchy(kind)
            assert all(len(nodes[f]) == 0 for f in H.FIELDS) and len(node) == 0
            info = a.hierarchy_info()
            assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == (0, 0, kmax, 0)
        # only isolated vertices: 7 nodes at k = 0
        a.from_edges(7, np.zeros((0, 2)))
        nodes, node, info = _check_core(a)
        assert nodes["k"].tolist() == [0] * 7 and nodes["rep"].tolist() == list(range(7)) and nodes["parent"].tolist() == [-1] * 7
        assert nodes["size"].tolist() == [1] * 7 and nodes["shell"].tolist() == [1] * 7 and node.tolist() == list(range(7))
        assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == (7, 7, 0, 1)
        nodes, node, info = _check_truss(a)             # a result with no edges: nobody is a member
        assert info["n_nodes"] == 0 and info["k_max"] == 2 and node.tolist() == [-1] * 7
        # one edge and a bystander
        a.from_edges(4, [[3, 1]])
        nodes, node, _ = _check_core(a)
        assert (nodes["k"].tolist(), nodes["rep"].tolist(), nodes["size"].tolist()) == ([0, 0, 1], [0, 2, 1], [1, 1, 2])
        assert node.tolist() == [0, 2, 1, 2] and nodes["parent"].tolist() == [-1, -1, -1]
        nodes, node, _ = _check_truss(a)
        assert (nodes["k"].tolist(), nodes["rep"].tolist(), nodes["size"].tolist()) == ([2], [1], [2]) and node.tolist() == [-1, 0, -1, 0]
        # a triangle with a tail: the tail's vertices have level 2, the triangle's 3
        a.from_edges(5, [[0, 1], [1, 2], [0, 2], [2, 3], [3, 4]])
        _check_core(a)
        nodes, node, _ = _check_truss(a)
        assert (nodes["k"].tolist(), nodes["rep"].tolist(), nodes["parent"].tolist()) == ([2, 3], [0, 0], [-1, 0])
        assert (nodes["size"].tolist(), nodes["shell"].tolist(), node.tolist()) == ([5, 3], [2, 3], [1, 1, 1, 0, 0])
    # two K_40 joined by a bridge edge: the truss kind has a root that only merges, and two children
    nv, uv = _two_k40(False)
    (cn, _, _), (tn, tnode, tinfo) = _check_both(K, nv, uv)
    assert (cn["k"].tolist(), cn["size"].tolist()) == ([39], [80])
    assert (tn["k"].tolist(), tn["rep"].tolist(), tn["parent"].tolist()) == ([2, 40, 40], [0, 0, 40], [-1, 0, 0])
    assert (tn["size"].tolist(), tn["shell"].tolist()) == ([80, 40, 40], [0, 40, 40])
    assert tnode.tolist() == [1] * 40 + [2] * 40 and tinfo["depth"] == 2
    # the same two joined through a vertex of degree 2
    nv, uv = _two_k40(True)
    (cn, cnode, _), _ = _check_both(K, nv, uv)
    assert (cn["k"].tolist(), cn["rep"].tolist(), cn["parent"].tolist()) == ([2, 39, 39], [0, 0, 40], [-1, 0, 0])
    assert (cn["size"].tolist(), cn["shell"].tolist()) == ([81, 40, 40], [1, 40, 40]) and cnode.tolist() == [1] * 40 + [2] * 40 + [0]
    # raw input with loops and duplicates
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 300, (400, 2))
    raw = np.concatenate([raw, raw[:100], raw[:100, ::-1], np.stack([np.arange(50)] * 2, 1)])
    _check_both(K, 310, raw)


def test_level_gaps(K):
    """A K_40 and a 100 000-path: only the levels 1 and 39 (truss: 2 and 40) are populated."""
    n = 100000
    iu = np.stack(np.triu_indices(40, 1), 1)
    path = np.stack([np.arange(n - 1), np.arange(1, n)], 1) + 40
    uv = np.concatenate([iu, path])
    for ids in (np.arange(n + 40), np.random.default_rng(5).permutation(n + 40)):
        (cn, _, cinfo), (tn, _, _) = _check_both(K, n + 40, ids[uv])
        assert (cn["k"].tolist(), sorted(cn["size"].tolist())) == ([1, 39], [40, n]) and cinfo["n_roots"] == 2
        assert (tn["k"].tolist(), sorted(tn["size"].tolist())) == ([2, 40], [40, n])


def test_many_levels(K):
    """A chain of cliques K_3 .. K_40, each joined to the next by one edge: 38 core levels, a path of 38 nodes."""
    parts, first, off = [], [], 0
    for n in range(3, 41):
        parts.append(np.stack(np.triu_indices(n, 1), 1) + off)
        first.append(off)
        off += n
    parts.append(np.stack([first[:-1], first[1:]], 1))
    uv = np.concatenate(parts)
    for ids in (np.arange(off), np.random.default_rng(8).permutation(off)):
        (cn, _, cinfo), (tn, _, tinfo) = _check_both(K, off, ids[uv])
        assert cn["k"].tolist() == list(range(2, 40)) and cn["parent"].tolist() == list(range(-1, 37))
        assert (cinfo["n_nodes"], cinfo["n_roots"], cinfo["k_max"], cinfo["depth"]) == (38, 1, 39, 38)
        assert tn["k"].tolist() == [2] + list(range(3, 41)) and tn["parent"].tolist() == [-1] + [0] * 38
        assert tn["shell"].tolist() == [0] + list(range(3, 41)) and tinfo["depth"] == 2


def test_long_rows(K):
    """Rows of every class of the linking pass (short, wave-wide, grid-wide: the boundaries are 16 and 2048, as in
    komb_components_run), ids in order and scattered."""
    parts, off = [], 0
    for n in (10, 16, 17, 64, 65, 700, 2047, 2048, 2049, 9000, 70000):  # stars: the hub's row has n entries
        parts.append(np.stack([np.full(n, off), np.arange(off + 1, off + n + 1)], 1))
        off += n + 1
    for n in (5, 30):                                                   # cliques hanging on a long row
        iu = np.stack(np.triu_indices(n, 1), 1) + off
        parts.append(np.concatenate([iu, np.stack([np.full(3000, off), np.arange(off + n, off + n + 3000)], 1)]))
        off += n + 3000
    hub = off                                                           # a long row at a higher level: a hub joined to every vertex of three cliques
    for n in (20, 2100, 40):
        iu = np.stack(np.triu_indices(min(n, 60), 1), 1) + off + 1
        ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1) + off + 1
        parts += [iu, ring, np.stack([np.full(n, hub), np.arange(off + 1, off + n + 1)], 1)]
        off += n
    nv = off + 4
    uv = np.concatenate(parts)
    for ids in (np.arange(nv), np.random.default_rng(9).permutation(nv)):
        _check_both(K, nv, ids[uv])


@pytest.mark.parametrize("nv", [255, 256, 257, 513])
def test_isolated_vertices(K, nv):
    """No edges, up to and past one and two workgroups of CLAIM / ADOPT: every vertex makes its own node, and only a
    workgroup's first lane has the root whose counts are summed in LDS."""
    with K.KombAccel() as a:
        a.from_edges(nv, np.zeros((0, 2)))
        nodes, node, info = _check_core(a, [0] * nv)
        assert nodes["k"].tolist() == [0] * nv and nodes["rep"].tolist() == list(range(nv)) and nodes["parent"].tolist() == [-1] * nv
        assert nodes["size"].tolist() == [1] * nv and nodes["shell"].tolist() == [1] * nv and node.tolist() == list(range(nv))
        assert (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == (nv, nv, 0, 1)
        _check_truss(a)


def test_strided_claim(K):
    """Level 0 takes the most workgroups CLAIM / ADOPT get, and the first two go round a second time."""
    nv, uv = H.strided_claim_graph()
    (cn, cnode, cinfo), (tn, _, _) = _check_both(K, nv, uv)
    n = H.STRIDE_ISOLATED
    assert (cinfo["n_nodes"], cinfo["n_roots"], cinfo["k_max"], cinfo["depth"]) == (n + 1, n + 1, 3, 1)
    assert (cn["size"][:n] == 1).all() and (cn["shell"][:n] == 1).all() and (cn["size"][n], cn["shell"][n]) == (4, 4)
    assert np.array_equal(cnode, np.minimum(np.arange(nv), n)) and tn["size"].tolist() == [4]


def test_shell_before_hooks_and_heavy_rows_at_two_levels(K):
    """A level with more vertices than hooks (workgroups whose first root comes from the vertex list), and rows of the
    grid-wide class at two core levels (each level's rows queued behind the earlier levels'), ids in order and permuted."""
    nv, uv = H.shell_first_graph()
    for ids in (np.arange(nv), np.random.default_rng(12).permutation(nv)):
        (cn, _, _), (tn, _, _) = _check_both(K, nv, ids[uv])
        assert cn["k"].tolist() == [1] * 302 + [5, 30] and sorted(cn["size"].tolist()[:302]) == [2] * 300 + [2106, 2131]
        assert sorted(tn["k"].tolist()) == [2] * 302 + [6, 31]


@pytest.mark.parametrize("seed", [1, 2])
def test_composite(K, seed):
    nv, uv = R.composite(K.gen_hug_edges, seed)
    (cn, _, cinfo), (tn, _, _) = _check_both(K, nv, uv)
    if seed == 1:
        assert cinfo["n_roots"] == 3949 and cinfo["k_max"] == 63      # the components of the whole graph (test_components_ref.py)
        assert (tn["shell"] == 0).any()


@pytest.mark.parametrize("nv", [1000, 20000, 200000])
@pytest.mark.parametrize("alpha", [2.1, 2.2, 2.6])
def test_generated_graphs(K, nv, alpha):
    _check_both(K, nv, K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11))


def test_walk_up_equals_components_run(K):
    """The consequence that ties the forest to komb_components_run, against the product's own labels, for every k."""
    nv, uv = R.composite(K.gen_hug_edges, 3)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _, core = a.run_core()
        eu, ev, tr = a.run_truss()
        for kind, lvl, ks in (("core", core, range(0, int(core.max()) + 2)),
                              ("truss", H.truss_levels(nv, eu, ev, tr), range(2, int(tr.max()) + 2))):
            nodes, node = a.run_hierarchy(kind)
            h = dict(nodes, node=node)
            H.check_invariants(h, kind == "core")
            for k in ks:
                label, _ = a.run_components(kind, k)
                assert np.array_equal(H.walk_up_labels(h, lvl, k), label), (kind, k)


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    reads = lambda a: (a.hierarchy_fetch_nodes, a.hierarchy_fetch_vertices, a.hierarchy_info)
    with K.KombAccel() as a:
        # no graph
        for call in (lambda: a.hierarchy_run("core"), lambda: a.hierarchy_run("truss")) + reads(a):
            assert _code(K, call) == ARG
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])
        # count / fetch / info before a run
        for call in reads(a):
            assert _code(K, call) == STATE
        # unknown kinds
        assert _code(K, lambda: a.hierarchy_run(2)) == ARG
        assert _code(K, lambda: a.hierarchy_run(-1)) == ARG
        # results that are not there: k-core is never run here
        assert _code(K, lambda: a.hierarchy_run("core")) == STATE
        assert _code(K, lambda: a.hierarchy_run("truss")) == STATE
        for call in reads(a):
            assert _code(K, call) == STATE                             # none of these made a result
        a.run_core()
        nodes, node = a.run_hierarchy("core")
        assert (nodes["k"].tolist(), nodes["rep"].tolist(), node.tolist()) == ([0, 1, 2], [3, 4, 0], [2, 2, 2, 0, 1, 1])
        # a failed call leaves the last result readable
        assert _code(K, lambda: a.hierarchy_run(7)) == ARG
        assert _code(K, lambda: a.hierarchy_run("truss")) == STATE
        assert a.hierarchy_fetch_vertices().tolist() == [2, 2, 2, 0, 1, 1] and a.hierarchy_info()["kind"] == 0
        # a slice of the canonical edges is not a complete k-truss result
        a.truss_run_slice(0, 2)
        assert _code(K, lambda: a.hierarchy_run("truss")) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, lambda: a.hierarchy_run("truss")) == STATE
        assert a.hierarchy_fetch_vertices().tolist() == [2, 2, 2, 0, 1, 1]
        a.truss_run_slice(0, 1)                                        # the whole range
        nodes, node = a.run_hierarchy("truss")
        assert (nodes["k"].tolist(), nodes["rep"].tolist(), node.tolist()) == ([2, 3], [4, 0], [1, 1, 1, -1, 0, 0])
        a.truss_run()
        assert a.run_hierarchy("truss")[1].tolist() == [1, 1, 1, -1, 0, 0]
        a.truss_unprepare()
        assert _code(K, lambda: a.hierarchy_run("truss")) == STATE
        assert a.hierarchy_fetch_vertices().tolist() == [1, 1, 1, -1, 0, 0]   # the snapshot stays
        assert a.hierarchy_info()["kind"] == 1
        # the endpoints of a whole-graph result nobody has fetched yet
        a.truss_run()
        assert a.run_hierarchy("truss")[0]["rep"].tolist() == [4, 0]
        # a k-truss result under a vmask, in original ids
        a.truss_run(np.asarray([1, 1, 1, 1, 0, 0], np.uint8))
        nodes, node = a.run_hierarchy("truss")
        assert (nodes["k"].tolist(), nodes["rep"].tolist(), node.tolist()) == ([3], [0], [0, 0, 0, -1, -1, -1])
        # NULL outputs are allowed
        lib = K._lib.load()
        n = ctypes.c_int64(-1)
        assert lib.komb_hierarchy_count(a._ctx, None) == 0
        assert lib.komb_hierarchy_count(a._ctx, ctypes.byref(n)) == 0 and n.value == 1
        assert lib.komb_hierarchy_fetch_nodes(a._ctx, None, None, None, None, None) == 0
        size = np.full(1, -9, np.int32)
        assert lib.komb_hierarchy_fetch_nodes(a._ctx, None, None, None, K._lib.ptr(size), None) == 0 and size.tolist() == [3]
        assert lib.komb_hierarchy_fetch_vertices(a._ctx, None) == 0
        assert lib.komb_hierarchy_info(a._ctx, None, None, None, None, None, None) == 0
        # a new graph drops the result (and the coreness)
        a.from_edges(3, [[0, 1]])
        for call in reads(a):
            assert _code(K, call) == STATE
        assert _code(K, lambda: a.hierarchy_run("core")) == STATE
        assert _code(K, lambda: a.hierarchy_run("truss")) == STATE
        a.run_core()
        assert a.run_hierarchy("core")[1].tolist() == [1, 1, 0]
        # a failed graph load leaves no graph
        with pytest.raises(K.KombError):
            a.from_edges(3, [[0, 5]])
        for call in reads(a):
            assert _code(K, call) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        a.run_core()
        a.run_truss()
        for kind in ("core", "truss", "core"):
            nodes, node = a.run_hierarchy(kind)
            info = a.hierarchy_info()
            out += [nodes[f] for f in H.FIELDS] + [node, np.asarray([info[f] for f in ("kind", "n_nodes", "n_roots", "k_max", "depth")])]
        a.run_truss((np.arange(nv) % 3 != 0).astype(np.uint8))
        nodes, node = a.run_hierarchy("truss")
        return out + [nodes[f] for f in H.FIELDS] + [node]
    finally:
        if own:
            a.close()


@pytest.fixture(scope="module")
def three_graphs(K):
    """Larger, smaller, larger -- and their results on fresh contexts without options, computed once."""
    graphs = [R.composite(K.gen_hug_edges, 3), (900, K.gen_hug_edges(900, 2200, 2.6, 6)), (50000, K.gen_hug_edges(50000, 122500, 2.1, 7))]
    return graphs, [_all_results(K, nv, uv) for nv, uv in graphs]


@pytest.mark.parametrize("poison", [None, "0xFFFFFFFF", "0x00000001", "0x7FFFFFFF", "0xA5A5A5A5"])
def test_poison_and_reuse_change_nothing(K, monkeypatch, three_graphs, poison):
    graphs, want = three_graphs
    if poison:
        monkeypatch.setenv("KOMB_POISON", poison)
    with K.KombAccel() as a:                     # one context across the three graphs, each run twice
        for (nv, uv), w in zip(graphs, want):
            for _ in range(2 if poison is None else 1):
                got = _all_results(K, nv, uv, a)
                assert len(got) == len(w)
                for x, y in zip(got, w):
                    assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """A hierarchy run changes no k-core, onion, k-truss, components or communities result and no komb_stats field; later runs
    of those neither change nor drop its snapshot."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv, uv = R.composite(K.gen_hug_edges, 5)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)

        def others():
            return (a.core_fetch() + a.onion_fetch() + a.truss_fetch(with_support=True) + a.components_fetch()
                    + a.truss_communities_fetch() + (a.truss_communities_fetch_vertices(),))

        deg, core = a.run_core()
        a.run_onion()
        a.run_truss()
        a.run_components("core", 2)
        a.run_truss_communities(4)
        cinfo, minfo = a.components_info(), a.truss_communities_info()
        before, st = others(), a.stats()
        for kind in ("core", "truss", "truss", "core"):
            a.hierarchy_run(kind)
            assert a.stats() == st
        for x, y in zip(others(), before):
            assert np.array_equal(x, y)
        assert a.components_info() == cinfo and a.truss_communities_info() == minfo and a.stats() == st
        # the same results once more, made after the hierarchy runs
        a.run_core(); a.run_onion(); a.run_truss(); a.run_components("core", 2); a.run_truss_communities(4)
        for x, y in zip(others(), before):
            assert np.array_equal(x, y)
        # a snapshot survives later runs of everything else
        nodes, node = a.run_hierarchy("truss")
        info = a.hierarchy_info()
        vmask = (core >= int(core.max()) // 2).astype(np.uint8)
        su, sv, st_ = a.run_truss(vmask)
        a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3)
        again = a.hierarchy_fetch_nodes()
        assert all(np.array_equal(again[f], nodes[f]) for f in H.FIELDS)
        assert np.array_equal(a.hierarchy_fetch_vertices(), node) and a.hierarchy_info() == info
        # ... and the vmask result gets a forest of its own
        _expect(a, "truss", H.truss_hierarchy(nv, su, sv, st_))
