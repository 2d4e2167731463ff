"""GPU tests of komb_biconnected_run / _count / _fetch_edges / _fetch_vertices / _fetch_blocks / _info: every array and
every info field is compared exactly with the Hopcroft-Tarjan reference of tests/biconnected_ref.py (trussness taken from
the library's own run_truss, whose parity other tests own), and the invariants of the block-cut forest are asserted from
the library's outputs alone."""
import numpy as np
import pytest

import biconnected_ref as R
import components_ref as CR

pytestmark = pytest.mark.gpu

KMAX = -1
INFO = ("k_used",) + R.INFO_FIELDS


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _resolve(k, tr):
    tmax = int(tr.max()) if len(tr) else 2
    return max(tmax, 2) if k == KMAX else max(k, 2)


def _fetch_all(a, k):
    a.biconnected_run(k)
    return _fetch_held(a)


def _fetch_held(a):
    block, size = a.biconnected_fetch_edges()
    n_blocks, ecc_label, ecc_size = a.biconnected_fetch_vertices()
    return {"block": block, "size": size, "n_blocks": n_blocks, "ecc_label": ecc_label, "ecc_size": ecc_size,
            "blocks": a.biconnected_fetch_blocks(), "info": a.biconnected_info(), "count": a.biconnected_count()}


def _invariants(a, k, got):
    """What holds for any graph, from the library's outputs alone (the block-cut structure is a forest)."""
    info, nb, blocks = got["info"], got["n_blocks"].astype(np.int64), got["blocks"]
    a.components_run("truss", k)
    n_comp = a.components_info()["n_components"]
    assert int(nb[nb >= 2].sum()) == info["n_blocks"] + info["n_articulation"] - n_comp
    assert int(blocks["n_edges"].sum()) == info["n_member_edges"]
    assert int(blocks["n_verts"].sum()) == int(nb.sum())
    assert info["n_bridges"] == int((blocks["n_edges"] == 1).sum())
    assert np.array_equal(got["block"][blocks["rep"]], blocks["rep"])
    assert got["count"] == info["n_blocks"] == len(blocks["rep"])


def _expect(a, k, eu, ev, tr, invariants=True):
    """Run threshold k on a's last k-truss result (eu, ev, tr) and compare everything with the reference."""
    got = _compare(a, k, eu, ev, tr, _fetch_all(a, k))
    if invariants:
        _invariants(a, k, got)
    return got


def _compare(a, k, eu, ev, tr, got=None, want=None):
    """The held blocks of threshold k of the k-truss result (eu, ev, tr): everything against the reference."""
    got = _fetch_held(a) if got is None else got
    kk = _resolve(k, tr)
    want = R.biconnected(a.nv, eu, ev, tr, kk) if want is None else want
    for name in ("block", "size", "n_blocks", "ecc_label", "ecc_size"):
        assert got[name].dtype == np.int32 and len(got[name]) == len(want[name]), (name, k)
        assert np.array_equal(got[name], want[name]), (name, k)
    for name in ("rep", "n_edges", "n_verts"):
        assert got["blocks"][name].dtype == np.int32
        assert np.array_equal(got["blocks"][name], want["blocks"][name]), (name, k)
    assert tuple(got["info"][x] for x in INFO) == (kk,) + R.summary(want), k
    assert got["info"]["ms"] >= 0.0
    return got


def _check(a, ks, vmask=None, want_truss=None):
    eu, ev, tr = a.run_truss(vmask)
    if want_truss is not None:
        assert (eu.tolist(), ev.tolist(), tr.tolist()) == tuple(list(w) for w in want_truss)
    for k in ks:
        _expect(a, k, eu, ev, tr)
    return int(tr.max()) if len(tr) else 2


def test_golden_graphs(K, golden):
    for g in golden:
        nv = g["nv"]
        kt = max(g["trussness"]) if g["trussness"] else 2
        kts = max(g["sub_trussness"]) if g["sub_trussness"] else 2
        for load in ("raw", "csr"):
            with K.KombAccel() as a:
                if load == "raw":
                    a.from_edges(nv, _i64(g["raw"]))
                else:
                    a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
                assert _check(a, list(range(2, kt + 2)) + [KMAX], want_truss=(g["eu"], g["ev"], g["trussness"])) == kt, g["name"]
                assert _check(a, list(range(2, kts + 2)) + [KMAX], vmask=np.asarray(g["maxcore_mask"], np.uint8),
                              want_truss=(g["sub_eu"], g["sub_ev"], g["sub_trussness"])) == kts, g["name"]


@pytest.mark.parametrize("seed", [1, 2])
def test_composite(K, seed):
    nv, uv = CR.composite(K.gen_hug_edges, seed)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _check(a, [2, 3, 4, KMAX])


@pytest.mark.parametrize("nv", [1000, 20000])
@pytest.mark.parametrize("alpha", [2.1, 2.6])
def test_generated_graphs(K, nv, alpha):
    uv = K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _check(a, [2, 3, KMAX])
        core = a.run_core()[1]
        _check(a, [2, 3, KMAX], vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8))


# ---- closed forms: the smallest shapes at which each rule can go wrong.  Ids go through a fixed random permutation, so that
# the roots of the forest and of the union-finds are not vertex 0.

def _clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


def _two_k40(bridge_vertex):
    n = 40
    iu = np.stack(np.triu_indices(n, 1), 1)
    link = [[0, 2 * n], [2 * n, n]] if bridge_vertex else [[0, n]]
    return 2 * n + (1 if bridge_vertex else 0), np.concatenate([iu, iu + n, np.asarray(link)])


def _grid(n):
    g = np.arange(n * n).reshape(n, n)
    return n * n, np.concatenate([np.stack([g[:, :-1].ravel(), g[:, 1:].ravel()], 1), np.stack([g[:-1].ravel(), g[1:].ravel()], 1)])


def _closed(K, nv, pairs, k=2, permute=True):
    """The library's result at threshold k on the graph of `pairs`, checked against the reference: (info, got, ids)."""
    ids = np.random.default_rng(17).permutation(nv) if permute else np.arange(nv)
    with K.KombAccel() as a:
        a.from_edges(nv, ids[_i64(pairs)])
        eu, ev, tr = a.run_truss()
        got = _expect(a, k, eu, ev, tr)
    i = got["info"]
    return (i["n_blocks"], i["n_articulation"], i["n_bridges"]), got, ids


def test_closed_forms_small(K):
    assert _closed(K, 5, [[i, i + 1] for i in range(4)])[0] == (4, 3, 4)                          # a path: all bridges
    for n in (5, 6):             # the non-tree edge joins equal levels in one cycle and adjacent levels in the other
        counts, got, _ = _closed(K, n, [[i, (i + 1) % n] for i in range(n)])
        assert counts == (1, 0, 0) and got["info"]["largest_block"] == n and got["info"]["depth"] == n // 2 + 1
    # a triangle: the root of the forest has two children joined only by the cross edge, and is no cut vertex
    counts, got, _ = _closed(K, 3, [[0, 1], [0, 2], [1, 2]], permute=False)
    assert counts == (1, 0, 0) and got["n_blocks"].tolist() == [1, 1, 1] and got["info"]["depth"] == 2
    counts, got, ids = _closed(K, 5, [[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]])             # two triangles, one vertex
    assert counts == (2, 1, 0) and got["n_blocks"][ids[2]] == 2 and got["info"]["n_ecc"] == 1
    assert _closed(K, 4, [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]])[0] == (1, 0, 0)                 # two triangles, one edge
    assert _closed(K, 7, [[0, 1], [1, 2], [2, 3], [0, 4], [4, 3], [0, 5], [5, 6], [6, 3]])[0] == (1, 0, 0)     # a theta graph
    for bridge_vertex in (False, True):                          # two K40 joined by a bridge edge / through a vertex
        counts, got, ids = _closed(K, *_two_k40(bridge_vertex))
        assert counts == ((4, 3, 2) if bridge_vertex else (3, 2, 1))
        assert got["info"]["largest_block"] == 780 and got["info"]["largest_ecc"] == 40
        assert got["n_blocks"][ids[0]] == 2 and got["n_blocks"][ids[40]] == 2
    # a cactus of 50 triangles in a chain
    counts, got, _ = _closed(K, 101, [e for i in range(50) for e in ([2 * i, 2 * i + 1], [2 * i, 2 * i + 2], [2 * i + 1, 2 * i + 2])])
    assert counts == (50, 49, 0) and np.all(got["blocks"]["n_verts"] == 3) and got["info"]["largest_ecc"] == 101
    # a grid: one block, a deep forest, many cross edges
    counts, got, _ = _closed(K, *_grid(30))
    assert counts == (1, 0, 0) and got["info"]["largest_block"] == 2 * 30 * 29


@pytest.mark.parametrize("heavy", [None, "1"])
def test_star(K, monkeypatch, heavy):
    """A hub of degree 3000: its row goes to the workgroup; with BICONN_HEAVY = 1 every other row of two entries or more
    goes to its wave."""
    if heavy:
        monkeypatch.setenv("KOMB_BICONN_HEAVY", heavy)
    counts, got, ids = _closed(K, 3001, [[0, i] for i in range(1, 3001)])
    assert counts == (3000, 1, 3000) and got["n_blocks"][ids[0]] == 3000 and got["info"]["n_ecc"] == 3001
    assert _closed(K, *_two_k40(True))[0] == (4, 3, 2)
    assert _closed(K, *_grid(30))[0] == (1, 0, 0)


def test_long_path(K):
    """A path of 20 000 vertices beside a K5: one level per vertex of the path, and the result still exact."""
    k5 = _clique(np.arange(20000, 20005))
    counts, got, _ = _closed(K, 20005, np.concatenate([np.stack([np.arange(19999), np.arange(1, 20000)], 1), k5]), permute=False)
    assert counts == (20000, 19998, 19999) and got["info"]["depth"] == 20000 and got["info"]["largest_block"] == 10
    counts, got, _ = _closed(K, 20005, np.concatenate([np.stack([np.arange(19999), np.arange(1, 20000)], 1), k5]))
    assert counts == (20000, 19998, 19999) and 10000 <= got["info"]["depth"] <= 20000


def test_members_and_edge_cases(K):
    with K.KombAccel() as a:
        # isolated vertices and non-member edges at k = 3: a triangle with a pendant path, vertex 5 alone
        a.from_edges(6, [[0, 1], [0, 2], [1, 2], [2, 3], [3, 4]])
        eu, ev, tr = a.run_truss()
        assert tr.tolist() == [3, 3, 3, 2, 2]
        got = _expect(a, 2, eu, ev, tr)
        assert got["block"].tolist() == [0, 0, 0, 3, 4] and got["size"].tolist() == [3, 3, 3, 1, 1]
        assert got["n_blocks"].tolist() == [1, 1, 2, 2, 1, 0] and got["ecc_label"].tolist() == [0, 0, 0, 3, 4, -1]
        for k in (3, KMAX):
            got = _expect(a, k, eu, ev, tr)
            assert got["block"].tolist() == [0, 0, 0, -1, -1] and got["n_blocks"].tolist() == [1, 1, 1, 0, 0, 0]
            assert got["ecc_size"].tolist() == [3, 3, 3, 0, 0, 0] and got["info"]["k_used"] == 3
        for k in (0, 1):                                         # 0 <= k <= 2 are the same call
            assert _expect(a, k, eu, ev, tr)["info"]["k_used"] == 2
        # k above the maximum: no members, not an error
        got = _expect(a, 4, eu, ev, tr)
        assert got["block"].tolist() == [-1] * 5 and got["size"].tolist() == [0] * 5 and got["count"] == 0
        assert got["ecc_label"].tolist() == [-1] * 6 and got["info"]["depth"] == 0
        # an empty k-truss result: a vmask that keeps no edge, only isolated vertices, the empty graph
        eu, ev, tr = a.run_truss(np.asarray([1, 0, 0, 1, 0, 1], np.uint8))
        assert len(tr) == 0
        got = _expect(a, KMAX, eu, ev, tr)
        assert len(got["block"]) == 0 and got["n_blocks"].tolist() == [0] * 6 and got["info"]["k_used"] == 2
        a.from_edges(7, np.zeros((0, 2)))
        _expect(a, 2, *a.run_truss())
        a.from_edges(0, np.zeros((0, 2)))
        got = _expect(a, 3, *a.run_truss())
        assert len(got["n_blocks"]) == 0 and got["count"] == 0
    # raw input with loops and duplicates
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 300, (420, 2))
    raw = np.concatenate([raw, raw[:100], raw[:100, ::-1], np.stack([np.arange(50)] * 2, 1)])
    with K.KombAccel() as a:
        a.from_edges(310, raw)
        _check(a, [2, 3, 4, KMAX])


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    tri6 = [[0, 1], [1, 2], [0, 2], [4, 5]]
    fetches = ("biconnected_count", "biconnected_fetch_edges", "biconnected_fetch_vertices", "biconnected_fetch_blocks", "biconnected_info")
    with K.KombAccel() as a:
        assert _code(K, lambda: a.biconnected_run(2)) == ARG                  # no graph
        a.from_edges(6, tri6)
        # no k-truss result; fetch / info before a run
        assert _code(K, lambda: a.biconnected_run(2)) == STATE
        assert _code(K, lambda: a.biconnected_run(KMAX)) == STATE
        a.run_core(); a.run_components("core", 0)
        assert _code(K, lambda: a.biconnected_run(2)) == STATE
        a.truss_run()
        for f in fetches:
            assert _code(K, getattr(a, f)) == STATE, f
        # bad thresholds (the argument is checked before the state)
        assert _code(K, lambda: a.biconnected_run(-2)) == ARG
        assert _code(K, lambda: a.biconnected_run(-100)) == ARG
        # the endpoints of a whole-graph result nobody has fetched yet
        assert a.run_biconnected(2)[0].tolist() == [0, 0, 0, 3]
        assert a.run_biconnected(KMAX)[0].tolist() == [0, 0, 0, -1] and a.biconnected_info()["k_used"] == 3
        # a failed call leaves the last result readable
        assert _code(K, lambda: a.biconnected_run(-7)) == ARG
        assert a.biconnected_fetch_edges()[1].tolist() == [3, 3, 3, 0]
        # NULL outputs are allowed
        assert lib.komb_biconnected_count(a._ctx, None) == 0
        assert lib.komb_biconnected_fetch_edges(a._ctx, None, None) == 0
        assert lib.komb_biconnected_fetch_vertices(a._ctx, None, None, None) == 0
        assert lib.komb_biconnected_fetch_blocks(a._ctx, None, None, None) == 0
        assert lib.komb_biconnected_info(a._ctx, *([None] * 11)) == 0
        # a later k-truss run of any kind drops it
        a.truss_run()
        for f in fetches:
            assert _code(K, getattr(a, f)) == STATE, f
        assert a.run_biconnected(2)[1].tolist() == [3, 3, 3, 1]
        a.truss_run(np.asarray([1, 1, 1, 0, 0, 0], np.uint8))
        assert _code(K, a.biconnected_fetch_vertices) == STATE
        assert a.run_biconnected(2)[0].tolist() == [0, 0, 0]
        # a slice of the canonical edges is not a k-truss result to split
        a.truss_run_slice(0, 2)
        assert _code(K, a.biconnected_fetch_edges) == STATE
        assert _code(K, lambda: a.biconnected_run(2)) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, lambda: a.biconnected_run(KMAX)) == STATE
        a.truss_run_slice(0, 1)                                    # the whole range
        assert a.run_biconnected(3)[0].tolist() == [0, 0, 0, -1]
        a.truss_unprepare()
        assert _code(K, a.biconnected_info) == STATE
        a.truss_run()
        assert a.run_biconnected(2)[0].tolist() == [0, 0, 0, 3]
        # loading a graph drops it
        a.from_edges(3, [[0, 1]])
        for f in fetches:
            assert _code(K, getattr(a, f)) == STATE, f
        assert _code(K, lambda: a.biconnected_run(2)) == STATE
        a.truss_run()
        assert a.run_biconnected(0)[0].tolist() == [0]


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            for k in (2, 3, KMAX):
                got = _fetch_all(a, k)
                out += [got[x] for x in ("block", "size", "n_blocks", "ecc_label", "ecc_size")] + list(got["blocks"].values())
                out.append(np.asarray([got["info"][x] for x in INFO]))
        return out
    finally:
        if own:
            a.close()


def test_repeated_runs_and_poisoned_memory(K, monkeypatch):
    """Two runs in one context, and one with every allocation filled with garbage first, give identical arrays."""
    graphs = [(20000, K.gen_hug_edges(20000, 49000, 2.2, 5)), (900, K.gen_hug_edges(900, 2200, 2.6, 6))]
    want = [_all_results(K, nv, uv) for nv, uv in graphs]
    with K.KombAccel() as a:                     # one context across the graphs, twice: larger, smaller, larger, smaller
        for (nv, uv), w in list(zip(graphs, want)) * 2:
            for x, y in zip(_all_results(K, nv, uv, a), w):
                assert np.array_equal(x, y)
    monkeypatch.setenv("KOMB_POISON", "0xFFFFFFFF")
    with K.KombAccel() as a:
        for (nv, uv), w in zip(graphs, want):
            for x, y in zip(_all_results(K, nv, uv, a), w):
                assert np.array_equal(x, y)


def test_independence(K):
    """A run changes no k-core, components, communities or k-truss result and no komb_stats field."""
    nv, uv = CR.composite(K.gen_hug_edges, 5)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        eu, ev, tr = a.run_truss()
        clabel, csize = a.run_components("truss", 3)
        cinfo = a.components_info()
        mlabel, msize = a.run_truss_communities(3)
        minfo = a.truss_communities_info()
        st = a.stats()
        for k in (3, 2, KMAX, 1000):
            a.biconnected_run(k)
            assert a.stats() == st
            a.biconnected_fetch_edges(); a.biconnected_fetch_vertices(); a.biconnected_fetch_blocks(); a.biconnected_info()
            assert a.stats() == st
        got = a.core_fetch() + a.truss_fetch() + a.components_fetch() + a.truss_communities_fetch()
        for x, y in zip((deg, core, eu, ev, tr, clabel, csize, mlabel, msize), got):
            assert np.array_equal(x, y)
        assert a.components_info() == cinfo and a.truss_communities_info() == minfo and a.stats() == st
        a.truss_run()
        assert a.stats()["truss_prepared"] == 0              # the resident k-truss preparation is still there
