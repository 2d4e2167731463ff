"""GPU tests of komb_maximal_cliques_run / _fetch / _list / _info: every complete result -- k_min, k_hi, t_max, omega, flags,
n_cliques, the histogram, both per-vertex arrays and the full sorted list -- is compared exactly with the restatement of
tests/maximal_cliques_ref.py, which is fed the library's own run_truss() edge list (whose parity other tests own).  A result
the budget cut short is checked against the closed form as a lower bound.  No node count is asserted other than by bounds: it
depends on pivot ties."""
import ctypes

import numpy as np
import pytest

import maximal_cliques_ref as M
import nucleus_ref as R

pytestmark = pytest.mark.gpu

LDS = [{}, {"MAXIMAL_LDS": "0"}, {"MAXIMAL_LDS": "64"}]
LDS_IDS = ["lds default", "lds 0", "lds 64"]
PIVOT = [{}, {"MAXIMAL_PIVOT": "first"}]
PIVOT_IDS = ["pivot max", "pivot first"]
K_MIN = (2, 3, 4)


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


_WANT = {}


def _want(key, nv, eu, ev, tr, k_min, own_truss=True):
    """The restatement of one run on one k-truss result, computed once per module and never changed."""
    truss = None if own_truss else tr
    if key is None:
        return M.solve(nv, eu, ev, k_min, truss=truss)
    key = (key, k_min)
    if key not in _WANT:
        _WANT[key] = (eu.copy(), ev.copy(), M.solve(nv, eu, ev, k_min, truss=truss))
    seu, sev, want = _WANT[key]
    assert np.array_equal(seu, eu) and np.array_equal(sev, ev)
    return want


def _cliques(a):
    offset, verts = a.maximal_cliques_list()
    assert offset.dtype == np.int64 and verts.dtype == np.int32 and int(offset[0]) == 0 and int(offset[-1]) == len(verts)
    return [tuple(verts[offset[i]:offset[i + 1]].tolist()) for i in range(len(offset) - 1)]


def _compare(a, want):
    info = a.maximal_cliques_info()
    for name in ("k_min", "k_hi", "t_max", "omega", "flags", "n_cliques"):
        assert info[name] == want[name], name
    hist, count, largest = a.maximal_cliques_fetch()
    assert hist.dtype == np.int64 and np.array_equal(hist, want["hist"])
    assert count.dtype == np.int32 and len(count) == max(a.nv, 0) and np.array_equal(count, want["count"])
    assert largest.dtype == np.int32 and np.array_equal(largest, want["largest"])
    assert int(count.sum()) == int((np.arange(info["k_min"], info["k_hi"] + 1) * hist).sum())
    if want["flags"] & M.LISTED:
        assert _cliques(a) == want["cliques"]
    assert info["n_roots"] >= 0 and info["ms"] >= 0.0 and 0 <= info["max_candidates"] <= 4096
    assert info["n_cliques"] <= info["nodes"] or info["n_cliques"] == 0
    return info


def _check(a, k_min=2, key=None, own_truss=True, edges=None, budget=0):
    """One run on the k-truss result the context holds (edges: what run_truss returned) against the restatement."""
    eu, ev, tr = edges
    a.maximal_cliques_run(k_min, budget)
    return _compare(a, _want(key, a.nv, eu, ev, tr, k_min, own_truss))


def _check_all(a, vmask=None, key=None, own_truss=True, k_mins=K_MIN):
    """k-truss (whole graph or vmask), then every k_min of the list and one above t_max."""
    edges = a.run_truss(vmask)
    t_max = int(edges[2].max()) if len(edges[2]) else 0
    for k_min in tuple(k_mins) + (max(t_max, max(k_mins)) + 1,):
        info = _check(a, k_min, key, own_truss, edges)
        if k_min > t_max:
            assert (info["n_cliques"], info["omega"], info["flags"], info["nodes"]) == (0, 0, 3, 0)
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
        _check_all(a)
        hist, count, largest, info = a.run_maximal_cliques()
        assert hist.tolist() == [0] and count.tolist() == [] and largest.tolist() == [] and _cliques(a) == []
        assert (info["k_hi"], info["t_max"], info["omega"], info["flags"], info["n_cliques"], info["nodes"]) == (2, 0, 0, 3, 0, 0)
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges
        _check_all(a)
        hist, count, largest, info = a.run_maximal_cliques(5)
        assert hist.tolist() == [0] and count.tolist() == [0] * 7 and largest.tolist() == [0] * 7
        assert (info["k_min"], info["k_hi"], info["omega"], info["flags"]) == (5, 5, 0, 3) and _cliques(a) == []
        a.from_edges(3, [[0, 2]])                                                # one edge
        _check_all(a)
        hist, count, largest, info = a.run_maximal_cliques()
        assert hist.tolist() == [1] and count.tolist() == [1, 0, 1] and largest.tolist() == [2, 0, 2] and _cliques(a) == [(0, 2)]
        a.from_edges(6, [[0, 1], [1, 2], [2, 3], [3, 4], [1, 5]])                # a path: every edge is a maximal clique
        _check_all(a)
        hist, count, largest, info = a.run_maximal_cliques()
        assert hist.tolist() == [5] and count.tolist() == [1, 3, 2, 2, 1, 1] and largest.tolist() == [2] * 6
        assert _cliques(a) == [(0, 1), (1, 2), (1, 5), (2, 3), (3, 4)] and (info["omega"], info["flags"]) == (2, 3)
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        _check_all(a, vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        assert a.run_maximal_cliques()[0].tolist() == [0]
        a.from_edges(4, [[0, 1], [1, 3], [0, 3]])                                # one triangle (and an isolated vertex): no edge is maximal
        _check_all(a)
        hist, count, largest, info = a.run_maximal_cliques()
        assert hist.tolist() == [0, 1] and count.tolist() == [1, 1, 0, 1] and largest.tolist() == [3, 3, 0, 3]
        assert _cliques(a) == [(0, 1, 3)] and (info["omega"], info["t_max"]) == (3, 3)


@pytest.mark.parametrize("pivot", PIVOT, ids=PIVOT_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 65, 66, 67, 129, 130, 131])
def test_complete_graphs(K, monkeypatch, n, lds, pivot):
    """K_n: one maximal clique, candidate lists of n - 2 -- one word, one word and a bit, two words and a bit."""
    _set(monkeypatch, lds, pivot)
    with _load(K, n, R.clique(range(n))) as a:
        edges = a.run_truss()
        for k_min in sorted({2, min(n, 4), n}):
            info = _check(a, k_min, ("K", n), n < 100, edges)
            hist, count, largest = a.maximal_cliques_fetch()
            assert hist.tolist() == [0] * (n - k_min) + [1] and count.tolist() == [1] * n and largest.tolist() == [n] * n
            assert _cliques(a) == [tuple(range(n))]
            assert (info["omega"], info["t_max"], info["flags"], info["max_candidates"]) == (n, n, 3, n - 2)
        info = _check(a, n + 1, ("K", n), n < 100, edges)
        assert (info["n_cliques"], info["flags"]) == (0, 3)


def test_k515_in_global_scratch_through_the_filter(K):
    """K_515 at k_min = 514: candidate lists of 513 (the bit matrix in global scratch whatever MAXIMAL_LDS says), three roots that
    can reach 514 vertices, one maximal clique."""
    n = 515
    with _load(K, n, R.clique(range(n))) as a:
        edges = a.run_truss()
        info = _check(a, 514, ("K", n), False, edges)
        hist, count, largest = a.maximal_cliques_fetch()
        assert hist.tolist() == [0, 1] and count.tolist() == [1] * n and largest.tolist() == [n] * n
        assert _cliques(a) == [tuple(range(n))] and info["max_candidates"] == 513


@pytest.mark.parametrize("pivot", PIVOT, ids=PIVOT_IDS)
@pytest.mark.parametrize("lds", LDS, ids=LDS_IDS)
@pytest.mark.parametrize("m", [6, 12])
def test_cocktail_party_in_full(K, monkeypatch, m, lds, pivot):
    _set(monkeypatch, lds, pivot)
    nv, edges = M.cocktail_party(m)
    with _load(K, nv, edges) as a:
        _check_all(a, key=("CP", m))
        hist, count, largest, info = a.run_maximal_cliques()
        assert hist.tolist() == [2 ** m if k == m else 0 for k in range(2, 2 * m - 1)]
        assert count.tolist() == [2 ** (m - 1)] * nv and largest.tolist() == [m] * nv
        assert (info["omega"], info["t_max"], info["flags"], info["n_cliques"]) == (m, 2 * m - 2, 3, 2 ** m)


@pytest.mark.parametrize("pivot", PIVOT, ids=PIVOT_IDS)
def test_complete_five_partite(K, monkeypatch, pivot):
    _set(monkeypatch, pivot)
    nv, edges = M.complete_multipartite([3] * 5)
    with _load(K, nv, edges) as a:
        _check_all(a, key="3,3,3,3,3")
        hist, count, largest, info = a.run_maximal_cliques(5)
        assert int(hist[0]) == 243 == info["n_cliques"] and count.tolist() == [81] * nv and info["omega"] == 5


@pytest.mark.parametrize("low", [False, True], ids=["the extra vertex last", "the extra vertex first"])
def test_k_min_filter(K, low):
    """K_5 and a vertex joined to two of its vertices: the K_5 is always reported, the triangle at k_min <= 3 only."""
    five = [1, 2, 3, 4, 5] if low else [0, 1, 2, 3, 4]
    x = 0 if low else 5
    tri = tuple(sorted([x, five[0], five[1]]))
    with _load(K, 6, R.clique(five) + [(x, five[0]), (x, five[1])]) as a:
        edges = a.run_truss()
        for k_min in (2, 3, 4, 5, 6):
            _check(a, k_min, ("K_5 + 1", low), True, edges)
            want = sorted(c for c in (tri, tuple(five)) if len(c) >= k_min)
            assert _cliques(a) == want
            assert a.maximal_cliques_fetch()[2].tolist() == [max([len(c) for c in want if v in c], default=0) for v in range(6)]


def test_hand_graph_its_reversed_labelling_and_a_vmask(K):
    nv, edges = R.hand_graph()
    for ids in (np.arange(nv), nv - 1 - np.arange(nv)):
        with _load(K, nv, ids[_i64(edges)]) as a:
            _check_all(a)
            hist, count, largest, info = a.run_maximal_cliques()
            want = sorted(tuple(sorted(int(ids[v]) for v in c)) for c in
                          (range(7), (5, 6, 7, 8, 9), (9, 10, 11, 12), (12, 13, 14), (3, 14)))
            assert _cliques(a) == want and info["omega"] == 7 and hist.tolist() == [1, 1, 1, 1, 0, 1]
            assert largest[ids].tolist() == [7] * 7 + [5, 5, 5, 4, 4, 4, 3, 3]
            _check_all(a, vmask=(np.arange(nv) != ids[0]).astype(np.uint8))      # without a K_7 vertex: a K_6 is left
            assert a.run_maximal_cliques()[3]["omega"] == 6


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_two_k6_sharing_a_triangle(K, where):
    """The shared vertices carry the smallest, the middle or the largest ids: the roots of the two cliques are two shared
    vertices, one shared and one own, or two own, and the other clique's vertices are excluded below a, between a and b, or candidates."""
    shared = {"first": [0, 1, 2], "middle": [3, 4, 5], "last": [6, 7, 8]}[where]
    rest = [v for v in range(9) if v not in shared]
    one, two = sorted(shared + rest[:3]), sorted(shared + rest[3:])
    with _load(K, 9, R.clique(one) + R.clique(two)) as a:
        _check_all(a, k_mins=(2, 3, 4, 6))
        hist, count, largest, info = a.run_maximal_cliques()
        assert _cliques(a) == sorted([tuple(one), tuple(two)]) and info["n_cliques"] == 2
        assert count.tolist() == [2 if v in shared else 1 for v in range(9)] and largest.tolist() == [6] * 9


def _fan(n_common):
    """An edge (u, v) with n_common common neighbours, u and v carrying the two largest ids, and a disjoint K_6 on the first ids."""
    u, v = 6 + n_common, 7 + n_common
    edges = R.clique(range(6)) + [(u, v)]
    for w in range(6, 6 + n_common):
        edges += [(w, u), (w, v)]
    return 8 + n_common, edges


def test_more_than_4096_excluded_vertices(K):
    """The limit through X alone: the root (u, v) has no candidate and 4201 excluded vertices."""
    nv, uv = _fan(4201)
    with _load(K, nv, uv) as a:
        edges = a.run_truss()
        info = _check(a, 4, "fan", False, edges)                                 # accepted: the K_6 alone
        assert _cliques(a) == [tuple(range(6))] and info["max_candidates"] == 4
        assert _code(K, lambda: a.maximal_cliques_run(2)) == K._lib.KOMB_ERR_LIMIT
        assert b"4096" in K._lib.load().komb_last_error(a._ctx)
        assert _code(K, lambda: a.maximal_cliques_run(3)) == K._lib.KOMB_ERR_LIMIT
        assert a.maximal_cliques_info() == info and _cliques(a) == [tuple(range(6))]   # refused before anything was reported
        total, _, cinfo = a.run_clique_census(2, -1, 0)                          # the census counts candidates only: the limit is this call's own
        assert cinfo["flags"] == 1 and total.tolist()[:2] == [15 + 2 * 4201 + 1, 20 + 4201]
    nv, uv = _fan(4094)                                                          # at the limit: accepted
    with _load(K, nv, uv) as a:
        edges = a.run_truss()
        hist, count, largest, info = a.run_maximal_cliques()
        assert info["max_candidates"] == 4094 and hist.tolist()[:2] == [0, 4094] and info["n_cliques"] == 4095
        assert count[-2:].tolist() == [4094, 4094] and largest.tolist() == [6] * 6 + [3] * 4096


HUG = [(300, 735, 2.6, 6), (2000, 4900, 2.2, 11)]


@pytest.mark.parametrize("i", range(2), ids=lambda i: "nv %d" % HUG[i][0])
def test_power_law_graphs(K, monkeypatch, i):
    nv = HUG[i][0]
    with K.KombAccel() as a:
        a.from_edges(nv, K.gen_hug_edges(*HUG[i]))
        _check_all(a, key=("hug", nv))
        if nv == 2000:
            _set(monkeypatch, {"MAXIMAL_LDS": "0", "MAXIMAL_PIVOT": "first"})
            _check_all(a, key=("hug", nv), k_mins=K_MIN[:1])
            monkeypatch.delenv("KOMB_MAXIMAL_LDS")
            monkeypatch.delenv("KOMB_MAXIMAL_PIVOT")
            core = a.run_core()[1]
            _check_all(a, vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8), key=("hug, vmask", nv))


def test_cascade_of_random_cliques(K):
    with _load(K, 120, R.clique_union(120, 220, 2, 9, 1)) as a:
        _check_all(a, key="cascade", k_mins=K_MIN + (6,))
        assert a.run_maximal_cliques()[3]["omega"] == 11


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            eu, ev, _ = _check_all(a)
            assert (eu.tolist(), ev.tolist()) == (g["eu"], g["ev"]), g["name"]
            eu, ev, _ = _check_all(a, vmask=np.asarray(g["maxcore_mask"], np.uint8))
            assert (eu.tolist(), ev.tolist()) == (g["sub_eu"], g["sub_ev"]), g["name"]


@pytest.mark.parametrize("graph", ["hug", "cascade", "CP 6"])
def test_identities_with_the_maximum_cliques(K, graph):
    """On one k-truss result, without the restatement: omega, hist[omega] and the cliques of omega vertices are the
    maximum-clique search's, and the counts add up."""
    a = K.KombAccel()
    if graph == "hug":
        a.from_edges(2000, K.gen_hug_edges(*HUG[1]))
    elif graph == "cascade":
        a.from_edges(120, _i64(R.clique_union(120, 220, 2, 9, 1)))
    else:
        a.from_edges(12, _i64(M.cocktail_party(6)[1]))
    with a:
        a.truss_run()
        minfo, mcount, _ = a.run_max_clique()
        assert minfo["flags"] == 7
        mlist = a.max_clique_list()
        hist, count, largest, info = a.run_maximal_cliques()
        assert info["flags"] == 3 and info["k_hi"] == info["t_max"] == minfo["t_max"]
        omega = info["omega"]
        assert omega == minfo["omega"] and int(hist[omega - 2]) == minfo["n_max_cliques"]
        assert [c for c in _cliques(a) if len(c) == omega] == [tuple(r) for r in mlist.tolist()]
        assert np.array_equal(largest == omega, mcount > 0)
        assert int(count.sum()) == int((np.arange(2, info["k_hi"] + 1) * hist).sum()) and info["n_cliques"] == int(hist.sum())
        assert a.max_clique_info() == minfo and np.array_equal(a.max_clique_fetch()[0], mcount)   # (the run left them alone)


def test_budget_that_runs_out(K):
    """CP(33): 2^33 maximal cliques, one leaf each.  What 1 000 nodes report is a lower bound of the closed form."""
    m = 33
    nv, edges = M.cocktail_party(m)
    with _load(K, nv, edges) as a:
        a.truss_run()
        hist, count, largest, info = a.run_maximal_cliques(2, budget=1000)
        assert info["flags"] == 0 and (info["k_min"], info["k_hi"], info["t_max"]) == (2, 64, 64)
        assert info["nodes"] <= 1000 + K._lib.KOMB_MAXCLQ_OVERSHOOT
        assert all(int(x) <= (2 ** m if k == m else 0) for k, x in zip(range(2, 65), hist.tolist()))
        assert info["n_cliques"] == int(hist.sum()) <= info["nodes"] and info["omega"] in (0, m)
        assert all(0 <= int(x) <= 2 ** (m - 1) for x in count.tolist()) and set(largest.tolist()) <= {0, m}
        assert int(count.sum()) == m * info["n_cliques"]
        assert _code(K, a.maximal_cliques_list) == K._lib.KOMB_ERR_LIMIT
        assert _code(K, lambda: a.maximal_cliques_run(2, -1)) == K._lib.KOMB_ERR_ARG   # refused: the result stays
        assert a.maximal_cliques_info() == info


def test_list_caps(K, monkeypatch):
    LIMIT, ARG = K._lib.KOMB_ERR_LIMIT, K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    nv, edges = M.cocktail_party(6)
    with _load(K, nv, edges) as a:
        e = a.run_truss()
        want = _want(("CP", 6), nv, *e, 2)
        monkeypatch.setenv("KOMB_MAXIMAL_LIST", "10")                            # 64 cliques: the list is not kept, the rest is exact
        hist, count, largest, info = a.run_maximal_cliques()
        assert info["flags"] == 1 and info["n_cliques"] == 64
        assert np.array_equal(hist, want["hist"]) and np.array_equal(count, want["count"]) and np.array_equal(largest, want["largest"])
        assert _code(K, a.maximal_cliques_list) == LIMIT
        n, nw = ctypes.c_int64(-7), ctypes.c_int64(-7)
        assert lib.komb_maximal_cliques_list(a._ctx, 0, 0, ctypes.byref(n), ctypes.byref(nw), None, None) == LIMIT
        assert (n.value, nw.value) == (-7, -7)
        monkeypatch.setenv("KOMB_MAXIMAL_LIST", "64")                            # exactly enough
        _check(a, 2, ("CP", 6), True, e)
        monkeypatch.setenv("KOMB_MAXIMAL_LIST", "0")                             # no list at all
        assert a.run_maximal_cliques()[3]["flags"] == 1
        assert a.run_maximal_cliques(7)[3]["flags"] == 3 and _cliques(a) == []   # (nothing to list is a list)
        monkeypatch.delenv("KOMB_MAXIMAL_LIST")
        _check(a, 2, ("CP", 6), True, e)
        # the caps and the NULL outputs of the call itself
        assert lib.komb_maximal_cliques_list(a._ctx, 0, 0, ctypes.byref(n), ctypes.byref(nw), None, None) == 0
        assert (n.value, nw.value) == (64, 384)
        assert lib.komb_maximal_cliques_list(a._ctx, 0, 0, None, None, None, None) == 0
        offset, verts = np.full(65, -7, np.int64), np.full(384, -7, np.int32)
        n.value = nw.value = -7
        for cap_c, cap_v, o, v in ((63, 384, offset, verts), (64, 383, offset, verts), (63, 0, offset, None), (0, 383, None, verts)):
            assert lib.komb_maximal_cliques_list(a._ctx, cap_c, cap_v, ctypes.byref(n), ctypes.byref(nw), K._lib.ptr(o), K._lib.ptr(v)) == ARG
        assert (n.value, nw.value) == (-7, -7) and set(offset.tolist()) == {-7} and set(verts.tolist()) == {-7}   # nothing was written
        assert lib.komb_maximal_cliques_list(a._ctx, 64, 0, None, None, K._lib.ptr(offset), None) == 0
        assert offset.tolist() == list(range(0, 385, 6)) and set(verts.tolist()) == {-7}
        assert lib.komb_maximal_cliques_list(a._ctx, 0, 400, None, None, None, K._lib.ptr(verts)) == 0
        assert [tuple(verts[i:i + 6].tolist()) for i in range(0, 384, 6)] == want["cliques"]


def test_call_order_and_lifetime(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, edges = R.hand_graph()
    want = M.solve_edges(nv, edges, k_min=3)
    readers = lambda a: (a.maximal_cliques_fetch, a.maximal_cliques_list, a.maximal_cliques_info)
    run = lambda a: a.maximal_cliques_run(3)
    with K.KombAccel() as a:
        for call in (a.maximal_cliques_run,) + readers(a):                       # no graph
            assert _code(K, call) == ARG
        a.from_edges(nv, _i64(edges))
        assert _code(K, a.maximal_cliques_run) == STATE                          # no k-truss result
        a.run_core(); a.run_onion(); a.run_components("core", 0)
        assert _code(K, a.maximal_cliques_run) == STATE
        a.truss_run()
        for call in readers(a):                                                  # fetch / list / info before a run
            assert _code(K, call) == STATE
        for args in ((1, 0), (0, 0), (-3, 0), (2, -1), (2, -5)):
            assert _code(K, lambda: a.maximal_cliques_run(*args)) == ARG, args
        for call in readers(a):                                                  # (a refused run is no run)
            assert _code(K, call) == STATE
        run(a)                                                                   # (makes the canonical endpoints nobody has fetched yet)
        _compare(a, want)
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core); a.run_structural_clusters(1, 2, 3); a.run_community_hierarchy()
        a.run_nucleus(); a.run_nucleus_hierarchy(); a.run_max_clique(); a.run_clique_census(2, -1, 3)
        _compare(a, want)
        # NULL outputs are allowed
        assert lib.komb_maximal_cliques_fetch(a._ctx, None, None, None) == 0
        assert lib.komb_maximal_cliques_info(a._ctx, *([None] * 10)) == 0
        # a new k-truss run of any kind drops it
        a.truss_run()
        for call in readers(a):
            assert _code(K, call) == STATE
        run(a)
        _compare(a, want)
        a.truss_run(np.asarray([1] * 7 + [0] * 8, np.uint8))
        assert _code(K, a.maximal_cliques_info) == STATE
        assert a.run_maximal_cliques()[1].tolist() == [1] * 7 + [0] * 8
        # a slice of the canonical edges is no k-truss result to walk
        a.truss_run_slice(0, 2)
        assert _code(K, a.maximal_cliques_fetch) == STATE and _code(K, a.maximal_cliques_run) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, a.maximal_cliques_run) == STATE
        a.truss_run_slice(0, 1)                                                  # the whole range
        run(a)
        _compare(a, want)
        # komb_truss_unprepare drops the k-truss result and the cliques with it
        a.truss_unprepare()
        for call in (a.maximal_cliques_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        run(a)
        _compare(a, want)
        # a new graph drops it
        a.from_edges(4, [[0, 1], [1, 2], [0, 2]])
        for call in (a.maximal_cliques_run,) + readers(a):
            assert _code(K, call) == STATE
        a.truss_run()
        assert a.run_maximal_cliques()[2].tolist() == [3, 3, 3, 0]
        with pytest.raises(K.KombError):                                         # a failed graph load leaves no graph
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.maximal_cliques_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            for k_min in (2, 5):
                hist, count, largest, info = a.run_maximal_cliques(k_min)
                assert info["flags"] == 3
                out += [hist, count, largest, np.asarray([info[k] for k in ("k_hi", "t_max", "omega", "n_cliques", "max_candidates")])]
                out += list(a.maximal_cliques_list())
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "MAXIMAL_LDS": "0"},
                                  {"POISON": "0x7FFFFFFF", "MAXIMAL_DEBUG": "1", "MAXIMAL_PIVOT": "first"}])
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
    """A run changes no k-core, onion, components, communities, densest, structural, nucleus, maximum-clique, census or k-truss
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
        ctotal, clocal, ccinfo = a.run_clique_census(2, -1, 3)
        cinfo, minfo, dinfo, sinfo = a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()
        ninfo = a.nucleus_info()
        st = a.stats()
        for _ in range(2):
            a.maximal_cliques_run(2)
            assert a.stats() == st
            a.maximal_cliques_fetch(); a.maximal_cliques_list(); a.maximal_cliques_info()
            assert a.stats() == st
        _compare(a, _want(("hug", nv), nv, eu, ev, tr, 2))
        got = (a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch()
               + a.densest_subgraph_fetch() + a.structural_clusters_fetch()
               + (a.nucleus_fetch()["theta"], a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()) + a.max_clique_fetch()
               + a.clique_census_fetch())
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load, slabel, ssize, srole, ssim,
                         tris["theta"], etheta, vtheta, qcount, qwitness, ctotal, clocal), got):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()) == (cinfo, minfo, dinfo, sinfo)
        assert a.nucleus_info() == ninfo and a.max_clique_info() == qinfo and a.clique_census_info() == ccinfo
        assert a.stats() == st
        e3 = a.run_truss()                                                       # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr), e3):
            assert np.array_equal(x, y)
