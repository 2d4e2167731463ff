"""GPU tests of komb_clique_communities_run / _count / _fetch / _fetch_communities / _fetch_vertices / _info: every output --
labels, sizes, reps, clique counts, offsets, vertices, per-vertex counts and first communities, the info fields -- is compared
exactly with the restatement of tests/clique_communities_ref.py, which tests all pairs of cliques and is fed the library's own
maximal_cliques_list() (whose parity tests/test_gpu_maximal_cliques.py owns); pair_tests with the restatement of the pivot rule.
No time is asserted."""
import numpy as np
import pytest

import clique_communities_ref as C
import maximal_cliques_ref as M
import nucleus_ref as R

pytestmark = pytest.mark.gpu

GROUP = [{}, {"PERC_GROUP": "4"}, {"PERC_GROUP": "16"}, {"PERC_GROUP": "64"}]
GROUP_IDS = ["group default", "group 4", "group 16", "group 64"]


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


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


def _cliques(a):
    offset, verts = a.maximal_cliques_list()
    return [tuple(verts[offset[i]:offset[i + 1]].tolist()) for i in range(len(offset) - 1)]


_WANT = {}


def _want(key, nv, cliques, k):
    """The restatement of one run on one list, computed once per module and never changed."""
    if key is None:
        return C.solve(nv, cliques, k), C.pair_tests(cliques, k)
    key = (key, k)
    if key not in _WANT:
        _WANT[key] = (list(cliques), C.solve(nv, cliques, k), C.pair_tests(cliques, k))
    kept, want, tests = _WANT[key]
    assert kept == cliques
    return want, tests


def _compare(a, want, tests):
    info = a.clique_communities_info()
    for name in ("k", "n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap"):
        assert info[name] == want[name], name
    assert info["pair_tests"] == tests and info["ms"] >= 0.0 and info["k_min"] == a.maximal_cliques_info()["k_min"]
    label, size = a.clique_communities_fetch()
    assert label.dtype == np.int32 and size.dtype == np.int32
    assert np.array_equal(label, want["label"]) and np.array_equal(size, want["size"])
    assert a.clique_communities_count() == (want["n_communities"], len(want["verts"]))
    rep, ncl, offset, verts = a.clique_communities_fetch_communities()
    assert offset.dtype == np.int64 and verts.dtype == np.int32
    assert np.array_equal(rep, want["rep"]) and np.array_equal(ncl, want["n_cliques"])
    assert np.array_equal(offset, want["offset"]) and np.array_equal(verts, want["verts"])
    n_comm, first = a.clique_communities_fetch_vertices()
    assert len(n_comm) == max(a.nv, 0) and np.array_equal(n_comm, want["n_comm"]) and np.array_equal(first, want["first"])
    return info


def _check(a, k, key=None, budget=0):
    """One run on the list the context holds against the restatement."""
    a.clique_communities_run(k, budget)
    want, tests = _want(key, max(a.nv, 0), _cliques(a), k)
    return _compare(a, want, tests)


def _check_all(a, ks, vmask=None, key=None, k_min=2):
    """k-truss (whole graph or vmask), the maximal cliques from k_min, then every k of the list and one above t_max."""
    a.truss_run(vmask)
    a.maximal_cliques_run(k_min)
    t_max = a.maximal_cliques_info()["t_max"]
    for k in tuple(ks) + (max(t_max, max(ks)) + 1,):
        info = _check(a, k, key)
        if k > t_max:
            assert (info["n_member_cliques"], info["n_communities"], info["largest"], info["n_covered"], info["pair_tests"]) == (0, 0, 0, 0, 0)
    return t_max


def _sets(a):
    rep, ncl, offset, verts = a.clique_communities_fetch_communities()
    return sorted(tuple(verts[offset[c]:offset[c + 1]].tolist()) for c in range(len(rep)))


def test_degenerate_graphs(K):
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))                                        # the empty graph is not an error
        _check_all(a, (2, 3))
        out = a.run_clique_communities(3)
        assert [x.tolist() for x in out[:8]] == [[], [], [], [], [0], [], [], []]
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges
        _check_all(a, (2, 3))
        out = a.run_clique_communities(2)
        assert out[6].tolist() == [0] * 7 and out[7].tolist() == [-1] * 7 and out[4].tolist() == [0]
        a.from_edges(3, [[0, 2]])                                                # one edge
        _check_all(a, (2, 3))
        out = a.run_clique_communities(2)
        assert out[0].tolist() == [0] and out[1].tolist() == [1] and out[5].tolist() == [0, 2] and out[6].tolist() == [1, 0, 1]
        a.from_edges(6, [[0, 1], [1, 2], [2, 3], [3, 4], [1, 5]])                # a path: one community at k = 2, none at 3
        _check_all(a, (2, 3))
        out = a.run_clique_communities(2)
        assert out[0].tolist() == [0] * 5 and out[1].tolist() == [5] * 5 and out[5].tolist() == [0, 1, 2, 3, 4, 5]
        assert a.run_clique_communities(3)[8]["n_communities"] == 0
        a.from_edges(4, [[0, 1], [1, 3], [0, 3]])                                # one triangle (and an isolated vertex)
        _check_all(a, (2, 3))
        out = a.run_clique_communities(3)
        assert out[5].tolist() == [0, 1, 3] and out[6].tolist() == [1, 1, 0, 1] and out[7].tolist() == [0, 0, -1, 0]
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        _check_all(a, (2, 3), vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        info = a.run_clique_communities(2)[8]
        assert (info["n_member_cliques"], info["n_communities"]) == (0, 0)


@pytest.mark.parametrize("group", GROUP, ids=GROUP_IDS)
@pytest.mark.parametrize("name", sorted(C.HAND_GRAPHS))
def test_hand_graphs(K, monkeypatch, name, group):
    _set(monkeypatch, group)
    nv, edges = C.HAND_GRAPHS[name]
    with _load(K, nv, edges) as a:
        _check_all(a, (2, 3, 4, 5), key=name)
        for gname, k, n_comm, tests in C.HAND_TABLE:
            if gname == name:
                a.clique_communities_run(k)
                info = a.clique_communities_info()
                assert (info["n_communities"], info["pair_tests"]) == (n_comm, tests), k
        if name == "two K_4 sharing one vertex":
            n_comm, first = a.run_clique_communities(3)[6:8]
            assert n_comm.tolist() == [1, 1, 1, 2, 1, 1, 1] and first.tolist() == [0, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("name", sorted(C.HAND_GRAPHS))
def test_hand_graphs_reversed_and_under_a_vmask(K, name):
    nv, edges = C.HAND_GRAPHS[name]
    ids = nv - 1 - np.arange(nv)
    with _load(K, nv, ids[_i64(edges)]) as a:
        _check_all(a, (2, 3, 4, 5))
        for gname, k, n_comm, _ in C.HAND_TABLE:                                 # (pair_tests depends on the labelling; the communities do not)
            if gname == name:
                assert a.run_clique_communities(k)[8]["n_communities"] == n_comm
        _check_all(a, (2, 3, 4), vmask=(np.arange(nv) != 1).astype(np.uint8))
    with _load(K, nv, edges) as a:
        _check_all(a, (2, 3, 4), vmask=(np.arange(nv) != nv - 1).astype(np.uint8))


@pytest.mark.parametrize("group", GROUP, ids=GROUP_IDS)
@pytest.mark.parametrize("n", [4, 63, 64, 65, 66, 130])
def test_intersection_trip_boundaries(K, monkeypatch, n, group):
    """Two K_n sharing n - 2 vertices: adjacent exactly when k - 1 <= n - 2."""
    _set(monkeypatch, group)
    nv, edges = C.two_cliques(n, n - 2)
    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(max(n - 1, 2))
        assert _cliques(a) == [tuple(range(n)), tuple(range(2, n + 2))]
        info = _check(a, n - 1, ("two K", n))
        assert (info["n_communities"], info["largest"], info["n_overlap"], info["pair_tests"]) == (1, n + 2, 0, 1)
        assert _sets(a) == [tuple(range(n + 2))]
        info = _check(a, n, ("two K", n))
        assert (info["n_communities"], info["largest"], info["n_overlap"]) == (2, n, n - 2)
        info = _check(a, n + 1, ("two K", n))
        assert (info["n_communities"], info["n_member_cliques"]) == (0, 0)


@pytest.mark.parametrize("group", GROUP, ids=GROUP_IDS)
def test_row_trips_and_contention(K, monkeypatch, group):
    _set(monkeypatch, group)
    nv, edges = C.book(200)                                                      # rows of 200 entries at both ends of the spine
    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(2)
        info = _check(a, 3, "book")
        assert (info["n_communities"], info["largest"], info["pair_tests"], info["n_member_cliques"]) == (1, 202, 19900, 200)
        assert a.clique_communities_fetch()[1].tolist() == [200] * 200
        assert _check(a, 2, "book")["n_communities"] == 1
    nv, edges = C.windmill(200)
    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(2)
        info = _check(a, 3, "windmill")
        assert (info["n_communities"], info["pair_tests"], info["n_overlap"], info["largest"]) == (200, 0, 1, 3)
        n_comm, first = a.clique_communities_fetch_vertices()
        assert int(n_comm[0]) == 200 and int(first[0]) == 0 and set(n_comm[1:].tolist()) == {1}
        assert _check(a, 2, "windmill")["n_communities"] == 1


@pytest.mark.parametrize("group", GROUP, ids=GROUP_IDS)
def test_cocktail_party_and_five_partite(K, monkeypatch, group):
    _set(monkeypatch, group)
    nv, edges = M.cocktail_party(8)
    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(2)
        for k in (2, 3, 5, 8):
            info = _check(a, k, "CP 8")
            assert (info["n_communities"], info["largest"], info["n_member_cliques"]) == (1, 16, 256)
        assert _check(a, 9, "CP 8")["n_communities"] == 0
    nv, edges = M.complete_multipartite([3] * 5)
    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(2)
        for k in (2, 4, 5):
            info = _check(a, k, "3,3,3,3,3")
            assert (info["n_communities"], info["largest"], info["n_member_cliques"]) == (1, 15, 243)


def test_budget_refusal(K):
    LIMIT = K._lib.KOMB_ERR_LIMIT
    nv, edges = M.cocktail_party(12)
    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(2)
        assert _code(K, lambda: a.clique_communities_run(3, 1000000)) == LIMIT   # refused before anything is linked: no result yet
        msg = K._lib.load().komb_last_error(a._ctx)
        assert b"46114816" in msg and b"1000000" in msg
        assert _code(K, a.clique_communities_info) == K._lib.KOMB_ERR_STATE
        out = a.run_clique_communities(12)                                       # the default budget: completes
        info = out[8]
        assert (info["n_communities"], info["largest"], info["n_member_cliques"], info["pair_tests"]) == (1, 24, 4096, 8384512)
        assert out[0].tolist() == [0] * 4096 and out[1].tolist() == [4096] * 4096 and out[5].tolist() == list(range(24))
        assert out[2].tolist() == [0] and out[3].tolist() == [4096] and out[4].tolist() == [0, 24]
        assert _code(K, lambda: a.clique_communities_run(3, 1000000)) == LIMIT   # a refused run leaves the previous result readable
        again = a.clique_communities_fetch() + a.clique_communities_fetch_communities() + a.clique_communities_fetch_vertices()
        assert a.clique_communities_info() == info and all(np.array_equal(x, y) for x, y in zip(again, out[:8]))
        a.clique_communities_run(3, 46114816)                                    # exactly enough
        assert a.clique_communities_info()["pair_tests"] == 46114816 and a.clique_communities_info()["n_communities"] == 1


# (sized for the restatement, which tests all pairs of cliques: 3 128 and 2 283 maximal cliques, under two seconds per k)
HUG = [(500, 1225, 2.6, 6), (600, 1200, 2.2, 11)]
BIG = (2000, 4900, 2.2, 11)                                                      # 11 396 maximal cliques: compared between runs and results only
CASCADE = (200, 90, 2, 9, 1)


@pytest.mark.parametrize("i", range(2), ids=lambda i: "nv %d" % HUG[i][0])
def test_power_law_graphs(K, monkeypatch, i):
    nv = HUG[i][0]
    with K.KombAccel() as a:
        a.from_edges(nv, K.gen_hug_edges(*HUG[i]))
        t_max = _check_all(a, (3, 4), key=("hug", nv), k_min=3)
        _check(a, max(t_max - 1, 3), ("hug", nv))
        if nv == 600:
            _set(monkeypatch, {"PERC_GROUP": "64"})
            _check(a, 3, ("hug", nv))
            monkeypatch.delenv("KOMB_PERC_GROUP")
            core = a.run_core()[1]
            _check_all(a, (3, 4), vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8), key=("hug, vmask", nv), k_min=3)


@pytest.mark.parametrize("group", GROUP, ids=GROUP_IDS)
def test_cascade_of_random_cliques(K, monkeypatch, group):
    _set(monkeypatch, group)
    with _load(K, CASCADE[0], R.clique_union(*CASCADE)) as a:
        t_max = _check_all(a, (2, 3, 4, 6), key="cascade")
        _check(a, t_max - 1, "cascade")
        assert a.run_clique_communities(3)[8]["n_overlap"] > 0


def test_golden_graphs(K, golden):
    for g in golden:
        with K.KombAccel() as a:
            a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
            t_max = _check_all(a, (3, 4), k_min=3)
            _check(a, max(t_max - 1, 3))
            t_max = _check_all(a, (3, 4), vmask=np.asarray(g["maxcore_mask"], np.uint8), k_min=3)
            _check(a, max(t_max - 1, 3))


@pytest.mark.parametrize("graph", ["hug", "cascade", "hand"])
def test_cross_results_on_one_context(K, graph):
    """Without the restatement: k = 3 against the k-truss communities, k = 4 against the 1-nuclei, k = 2 against the components."""
    a = K.KombAccel()
    if graph == "hug":
        a.from_edges(BIG[0], K.gen_hug_edges(*BIG))
    elif graph == "cascade":
        a.from_edges(120, _i64(R.clique_union(120, 220, 2, 9, 1)))
    else:
        a.from_edges(15, _i64(R.hand_graph()[1]))
    with a:
        eu, ev, tr = a.run_truss()
        a.maximal_cliques_run(2)
        # k = 3: the vertex sets of the triangle-connected edge classes
        label, _ = a.run_truss_communities(3)
        sets = {}
        for u, v, l in zip(eu.tolist(), ev.tolist(), label.tolist()):
            if l >= 0:
                sets.setdefault(l, set()).update((u, v))
        a.clique_communities_run(3)
        assert _sets(a) == sorted(tuple(sorted(s)) for s in sets.values())
        # k = 4: the 1-nuclei
        a.run_nucleus()
        a.nucleus_hierarchy_run()
        nuclei = a.nucleus_hierarchy_nuclei(1)
        a.clique_communities_run(4)
        rep, ncl, offset, verts = a.clique_communities_fetch_communities()
        assert len(rep) == len(nuclei["rep"]) and sorted(np.diff(offset).tolist()) == sorted(nuclei["n_vertices"].tolist())
        # k = 2: the components of the non-isolated vertices
        clabel, _ = a.run_components("truss", 2)
        deg = np.bincount(np.concatenate([eu, ev]), minlength=a.nv)
        comps = {}
        for v in np.flatnonzero(deg > 0).tolist():
            comps.setdefault(int(clabel[v]), []).append(v)
        a.clique_communities_run(2)
        assert _sets(a) == sorted(tuple(c) for c in comps.values())
        assert a.clique_communities_info()["n_overlap"] == 0


def test_errors(K, monkeypatch):
    ARG, STATE, LIMIT = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE, K._lib.KOMB_ERR_LIMIT
    lib = K._lib.load()
    nv, edges = R.hand_graph()
    with _load(K, nv, edges) as a:
        assert _code(K, a.clique_communities_run) == STATE                       # no k-truss result, so no maximal cliques
        a.truss_run()
        assert _code(K, a.clique_communities_run) == STATE                       # no maximal cliques
        a.maximal_cliques_run(4)
        assert _code(K, lambda: a.clique_communities_run(3)) == STATE            # the list lacks the cliques of 3 vertices
        msg = lib.komb_last_error(a._ctx)
        assert b"k_min 4" in msg and b"k 3" in msg
        for args in ((1, 0), (0, 0), (-2, 0), (4, -1), (4, -5)):
            assert _code(K, lambda: a.clique_communities_run(*args)) == ARG, args
        assert _code(K, a.clique_communities_info) == STATE                      # (a refused run is no run)
        _check(a, 4)
        _check(a, 5)
        monkeypatch.setenv("KOMB_MAXIMAL_LIST", "1")                             # two cliques, a list that holds one
        a.maximal_cliques_run(5)
        assert a.maximal_cliques_info()["n_cliques"] == 2 and not a.maximal_cliques_info()["flags"] & 2
        assert _code(K, lambda: a.clique_communities_run(5)) == LIMIT
        monkeypatch.delenv("KOMB_MAXIMAL_LIST")
        assert lib.komb_clique_communities_run(a._ctx, 5, 0) == LIMIT            # (the option is read by the cliques' run)
        a.maximal_cliques_run(4)
        _check(a, 4)
        # NULL outputs are allowed
        assert lib.komb_clique_communities_count(a._ctx, None, None) == 0
        assert lib.komb_clique_communities_fetch(a._ctx, None, None) == 0
        assert lib.komb_clique_communities_fetch_communities(a._ctx, None, None, None, None) == 0
        assert lib.komb_clique_communities_fetch_vertices(a._ctx, None, None) == 0
        assert lib.komb_clique_communities_info(a._ctx, *([None] * 9)) == 0


def test_lifetime(K):
    STATE = K._lib.KOMB_ERR_STATE
    nv, edges = R.hand_graph()
    readers = lambda a: (a.clique_communities_count, a.clique_communities_fetch, a.clique_communities_fetch_communities,
                         a.clique_communities_fetch_vertices, a.clique_communities_info)

    def gone(a):
        for call in readers(a):
            assert _code(K, call) == STATE

    with _load(K, nv, edges) as a:
        a.truss_run()
        a.maximal_cliques_run(2)
        gone(a)                                                                  # before a run
        info = _check(a, 3, "hand")
        # the other analyses neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("truss", 3); a.run_truss_communities(3); a.run_hierarchy("core")
        a.run_densest_subgraph(4); a.get_anomaly_score(deg, core); a.run_structural_clusters(1, 2, 3); a.run_community_hierarchy()
        a.run_nucleus(); a.run_nucleus_hierarchy(); a.run_max_clique(); a.run_clique_census(2, -1, 3)
        want, tests = _want("hand", nv, _cliques(a), 3)
        assert _compare(a, want, tests) == info
        a.maximal_cliques_run(2)                                                 # another run of the cliques drops it
        gone(a)
        _check(a, 3, "hand")
        assert _code(K, lambda: a.maximal_cliques_run(2, -1)) == K._lib.KOMB_ERR_ARG   # a refused one does not
        _compare(a, want, tests)
        a.truss_run()                                                            # a new k-truss run
        gone(a)
        a.maximal_cliques_run(2)
        _check(a, 3, "hand")
        a.truss_run(np.asarray([1] * 7 + [0] * 8, np.uint8))
        gone(a)
        a.maximal_cliques_run(2)
        assert _check(a, 7)["n_communities"] == 1
        a.truss_unprepare()                                                      # komb_truss_unprepare
        gone(a)
        a.truss_run()
        a.maximal_cliques_run(2)
        _check(a, 3, "hand")
        a.from_edges(4, [[0, 1], [1, 2], [0, 2]])                                # a new graph
        gone(a)
        a.truss_run()
        a.maximal_cliques_run(2)
        assert a.run_clique_communities(3)[5].tolist() == [0, 1, 2]


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            a.maximal_cliques_run(2)
            for k in (2, 3, 5):
                res = a.run_clique_communities(k)
                out += list(res[:8]) + [np.asarray([res[8][f] for f in ("n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap", "pair_tests")])]
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "PERC_GROUP": "4"},
                                  {"POISON": "0x7FFFFFFF", "PERC_DEBUG": "1", "PERC_GROUP": "64"}])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, opts):
    graphs = [(600, K.gen_hug_edges(*HUG[1])), (300, K.gen_hug_edges(300, 735, 2.6, 6)), (900, K.gen_hug_edges(900, 2205, 2.2, 5))]
    want = [_all_results(K, nv, uv) for nv, uv in graphs]
    _set(monkeypatch, opts)
    with K.KombAccel() as a:                     # one context across the three graphs: larger, smaller, larger
        for (nv, uv), w in zip(graphs, want):
            got = _all_results(K, nv, uv, a)
            assert len(got) == len(w)
            for x, y in zip(got, w):
                assert np.array_equal(x, y)


def test_independence_and_running_twice(K, monkeypatch):
    """A run changes no other result and no komb_stats field, the resident k-truss preparation survives it, and a second run gives
    the same output."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv = HUG[1][0]
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
        xhist, xcount, xlargest, xinfo = a.run_maximal_cliques(3)
        xlist = a.maximal_cliques_list()
        cinfo, minfo, dinfo, sinfo = a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()
        ninfo = a.nucleus_info()
        st = a.stats()
        runs = []
        for _ in range(2):
            res = a.run_clique_communities(3)
            assert a.stats() == st
            runs.append(res)
        assert all(np.array_equal(x, y) for x, y in zip(runs[0][:8], runs[1][:8]))
        assert {k: v for k, v in runs[0][8].items() if k != "ms"} == {k: v for k, v in runs[1][8].items() if k != "ms"}
        want, tests = _want(("hug", nv), nv, _cliques(a), 3)
        _compare(a, want, tests)
        got = (a.core_fetch() + a.onion_fetch() + tuple(a.truss_fetch()) + a.components_fetch() + a.truss_communities_fetch()
               + a.densest_subgraph_fetch() + a.structural_clusters_fetch()
               + (a.nucleus_fetch()["theta"], a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()) + a.max_clique_fetch()
               + a.clique_census_fetch() + a.maximal_cliques_fetch() + a.maximal_cliques_list())
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, clabel, csize, mlabel, msize, member, load, slabel, ssize, srole, ssim,
                         tris["theta"], etheta, vtheta, qcount, qwitness, ctotal, clocal, xhist, xcount, xlargest) + tuple(xlist), got):
            assert np.array_equal(x, y)
        assert (a.components_info(), a.truss_communities_info(), a.densest_subgraph_info(), a.structural_clusters_info()) == (cinfo, minfo, dinfo, sinfo)
        assert a.nucleus_info() == ninfo and a.max_clique_info() == qinfo and a.clique_census_info() == ccinfo
        assert a.maximal_cliques_info() == xinfo and a.stats() == st
        e3 = a.run_truss()                                                       # the preparation of the graph is still there
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr), e3):
            assert np.array_equal(x, y)
