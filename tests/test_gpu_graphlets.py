"""GPU tests of komb_graphlets_run / _fetch_vertices / _fetch_edges / _info: every orbit of every vertex, cycles4 and
cliques4 of every edge and every total is compared exactly with census() of tests/graphlets_ref.py (closed forms, or the
tile's own census on a replica, where the graph is too large for it), which is fed the library's own
run_truss(with_support=True) edge list (whose parity other tests own).  On every graph the 4-cycle pass must not walk more
entries than the degree-ordered algorithm needs: info["cycle_items"] <= ordered_items()."""
from itertools import combinations
from math import comb

import numpy as np
import pytest

import replica as RP
from graphlets_ref import ORBITS, TYPES, brute, census, check_identities, ordered_items
from test_gpu_alloc_failure import Case, E, ENDPOINTS, F, NV, SUPPORT, dropped, load_truss, run_state, truss_exact
from test_gpu_replicas import N, _padded, _truss
from test_graphlets_ref import FOUR

pytestmark = pytest.mark.gpu

U64 = 0xA5A5A5A5A5A5A5A5
TILE = RP.tile()
K2, K3, K5 = (RP.filler(x) for x in ("K2", "K3", "K5"))
FORCED = [{}, {"GRAPHLET_LDS": "0"}, {"GRAPHLET_LDS": "64"}, {"GRAPHLET_SHORT": "0"}, {"GRAPHLET_SHORT": "100000"}]


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


def _clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


def _set(monkeypatch, opts):
    for name in ("GRAPHLET_LDS", "GRAPHLET_SHORT"):
        monkeypatch.delenv("KOMB_" + name, raising=False)
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)


def _compare(a, eu, ev, sup, want, items=None):
    """The census of a's last k-truss result (eu, ev, sup), run now, against `want`."""
    orbit, cyc, clq, info = a.run_graphlets()
    assert orbit.dtype == cyc.dtype == clq.dtype == np.uint64
    assert orbit.shape == (ORBITS, a.nv) and len(cyc) == len(clq) == len(eu)
    assert np.array_equal(sup, want["sup"])
    assert np.array_equal(cyc, want["cycles4"])
    assert np.array_equal(clq, want["cliques4"])
    for o in range(ORBITS):
        assert np.array_equal(orbit[o], want["orbit"][o]), o
    assert info["total"] == want["total"] and info["flags"] == 0
    assert info["n_triangles"] == want["total"]["triangle"] and info["n_cliques4"] == want["total"]["clique4"]
    assert info["max_degree"] == int(want["orbit"][0].max(initial=0)) and info["ms"] >= 0.0
    items = ordered_items(a.nv, eu, ev) if items is None else items
    assert 0 <= info["cycle_items"] <= items, (info["cycle_items"], items)
    return orbit, cyc, clq, info


def _check(a, vmask=None):
    eu, ev, tr, sup = a.run_truss(vmask, with_support=True)
    want = census(a.nv, eu, ev)
    return (eu, ev, sup, want) + _compare(a, eu, ev, sup, want)


def test_degenerate_graphs(K):
    zero = {t: 0 for t in TYPES}
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))                                        # the empty graph is not an error
        info = _check(a)[-1]
        assert info["total"] == zero and info["cycle_items"] == 0
        a.from_edges(7, np.zeros((0, 2)))                                        # vertices without edges
        orbit, info = _check(a)[4], _check(a)[-1]
        assert not orbit.any() and info["total"] == zero and info["max_degree"] == 0
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])                        # a vmask that keeps no edge
        orbit, info = _check(a, vmask=np.asarray([1, 0, 0, 1, 1, 0], np.uint8))[4::3]
        assert not orbit.any() and info["total"] == zero
        a.from_edges(3, [[0, 2]])                                                # one edge (and an isolated vertex)
        orbit, cyc, clq, info = _check(a)[4:]
        assert orbit[0].tolist() == [1, 0, 1] and not orbit[1:].any() and info["total"] == dict(zero, edge=1)
        assert cyc.tolist() == [0] and clq.tolist() == [0]
        a.from_edges(3, [[0, 1], [1, 2], [0, 2]])                                # one triangle
        orbit, cyc, clq, info = _check(a)[4:]
        assert orbit[3].tolist() == [1, 1, 1] and info["total"] == dict(zero, edge=3, triangle=1)


def test_every_graphlet_under_id_permutations(K):
    """The six 4-vertex graphlets and the two 3-vertex ones as components of one graph: every orbit is populated, and among
    the many vertices of equal degree the (d, id) order is decided by the ids."""
    edges, base = [(0, 1), (1, 2), (3, 4), (4, 5), (3, 5)], 6
    for name in sorted(FOUR):
        edges += [(base + u, base + v) for u, v in FOUR[name][0]]
        base += 4
    edges = _i64(edges)
    rng = np.random.default_rng(17)
    for ids in (np.arange(base), base - 1 - np.arange(base), rng.permutation(base), rng.permutation(base)):
        with _load(K, base, ids[edges]) as a:
            eu, ev, sup, want, orbit, cyc, clq, info = _check(a)
            b = brute(base, list(zip(eu.tolist(), ev.tolist())))
            assert np.array_equal(orbit, b["orbit"]) and np.array_equal(cyc, b["cycles4"]) and np.array_equal(clq, b["cliques4"])
            assert orbit.any(axis=1).all()                                       # every orbit occurs
            assert info["total"] == {"edge": len(edges), "wedge": 1 + 2 + 3 + 4 + 2 + 2, "triangle": 1 + 1 + 2 + 4, "path4": 1, "claw": 1,
                                     "cycle4": 1, "paw": 1, "diamond": 1, "clique4": 1}
            check_identities(orbit)


def test_closed_forms(K):
    with _load(K, 40, _clique(range(40))) as a:                                  # K_40
        orbit, cyc, clq, info = _check(a)[4:]
        assert orbit[14].tolist() == [comb(39, 3)] * 40 and cyc.tolist() == [2 * comb(38, 2)] * 780 and clq.tolist() == [comb(38, 2)] * 780
        assert info["total"] == {"edge": 780, "wedge": 0, "triangle": comb(40, 3), "path4": 0, "claw": 0, "cycle4": 0, "paw": 0,
                                 "diamond": 0, "clique4": comb(40, 4)}
    with _load(K, 70, [(u, 30 + v) for u in range(30) for v in range(40)]) as a:   # K_{30,40}
        orbit, cyc, clq, info = _check(a)[4:]
        assert cyc.tolist() == [29 * 39] * 1200 and not clq.any() and info["n_triangles"] == 0
        assert info["total"]["cycle4"] == comb(30, 2) * comb(40, 2)
    for n in (4, 5):                                                             # C_4, C_5
        with _load(K, n, [(i, (i + 1) % n) for i in range(n)]) as a:
            orbit, cyc, clq, info = _check(a)[4:]
            assert info["total"]["cycle4"] == (1 if n == 4 else 0) and info["total"]["path4"] == (0 if n == 4 else 5)
    n = 3000
    with _load(K, n, np.stack([np.arange(n - 1), np.arange(1, n)], 1)) as a:     # a path
        orbit, cyc, clq, info = _check(a)[4:]
        assert info["total"] == {"edge": n - 1, "wedge": n - 2, "triangle": 0, "path4": n - 3, "claw": 0, "cycle4": 0, "paw": 0,
                                 "diamond": 0, "clique4": 0}


@pytest.mark.parametrize("n", [18, 19])
def test_triangle_pass_lane_wave_boundary(K, n):
    """The triangle pass keeps a walked side of up to 16 entries with the edge's lane and hands longer ones to the wave; the
    threshold has no option.  In K_n the longest walked side is that of edge (0, 1), n - 2 entries: K_18 is the largest clique
    that stays with the lanes, K_19 the smallest with a wave unit."""
    with _load(K, n, _clique(range(n))) as a:
        orbit, cyc, clq, info = _check(a)[4:]
        m = comb(n, 2)
        assert clq.tolist() == [comb(n - 2, 2)] * m and cyc.tolist() == [2 * comb(n - 2, 2)] * m
        assert orbit[3].tolist() == [comb(n - 1, 2)] * n and orbit[14].tolist() == [comb(n - 1, 3)] * n
        assert info["total"]["triangle"] == comb(n, 3) and info["total"]["clique4"] == comb(n, 4)


@pytest.mark.parametrize("centre", [0, 5000])
def test_star(K, centre):
    """K_{1,5000}: the centre's claw count is above 2^32, and nothing is walked (a leaf has no neighbour below the centre)."""
    n = 5001
    leaves = np.setdiff1d(np.arange(n), [centre])
    with _load(K, n, np.stack([np.full(n - 1, centre), leaves], 1)) as a:
        eu, ev, tr, sup = a.run_truss(with_support=True)
        orbit, cyc, clq, info = a.run_graphlets()
        want = np.zeros((ORBITS, n), np.uint64)
        want[0, leaves], want[0, centre] = 1, 5000
        want[1, leaves], want[2, centre] = 4999, comb(5000, 2)
        want[6, leaves], want[7, centre] = comb(4999, 2), comb(5000, 3)
        assert comb(5000, 3) > 2 ** 32
        assert np.array_equal(orbit, want) and not cyc.any() and not clq.any() and not sup.any()
        assert info["cycle_items"] == 0 == ordered_items(n, eu, ev)
        assert info["total"] == {"edge": 5000, "wedge": comb(5000, 2), "triangle": 0, "path4": 0, "claw": comb(5000, 3), "cycle4": 0,
                                 "paw": 0, "diamond": 0, "clique4": 0}
        assert info["max_degree"] == 5000


def _hub_graph():
    """K_60 and a hub joined to all of it and to 1940 leaves: degree 2000"""
    return 2001, np.concatenate([_clique(range(60)), [[60, v] for v in range(60)], [[60, 61 + v] for v in range(1940)]])


@pytest.fixture(scope="module")
def tier_graphs(K):
    """(nv, pairs) and, filled by the first run, what census() and ordered_items() say: computed once."""
    return {"hug": [3000, K.gen_hug_edges(3000, 7350, 2.2, 5), None], "hub": list(_hub_graph()) + [None],
            "k90": [90, _clique(range(90)), None]}


@pytest.mark.parametrize("opts", FORCED, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()) or "default")
@pytest.mark.parametrize("which", ["hug", "hub", "k90"])
def test_tiers(K, monkeypatch, tier_graphs, which, opts):
    """Every root on every kind of table.  K_90 under the default options has 25 roots that walk more than 4096 entries (the
    root of rank r walks r (r - 1)): more than the 8 dense tables of a batch; under GRAPHLET_LDS=0 every root of every graph
    here goes that way."""
    nv, uv, cached = tier_graphs[which]
    _set(monkeypatch, opts)
    with _load(K, nv, uv) as a:
        eu, ev, tr, sup = a.run_truss(with_support=True)
        if cached is None:
            cached = tier_graphs[which][2] = (census(nv, eu, ev), ordered_items(nv, eu, ev))
        want, items = cached
        info = _compare(a, eu, ev, sup, want, items)[-1]
        assert info["cycle_items"] == items                                      # (the tiers walk the same entries)
        if which == "k90":
            assert sum(1 for r in range(90) if r * (r - 1) > 4096) == 25 > 8
            assert items == sum(r * (r - 1) for r in range(90))


def _roots_with_work(nv, edges):
    """the vertices v with a neighbour u below them in (d, id) order that has a neighbour below v: the roots the pass queues"""
    adj = [set() for _ in range(nv)]
    for u, v in edges.tolist():
        adj[u].add(v); adj[v].add(u)
    rank = {v: i for i, v in enumerate(sorted(range(nv), key=lambda v: (len(adj[v]), v)))}
    return sum(1 for v in range(nv) if any(rank[u] < rank[v] and any(rank[w] < rank[v] for w in adj[u]) for u in adj[v]))


def _replica_want(f):
    """census() of the union from the tiles' own: every count is local to a component, and so is the (d, id) order's effect
    on the work (ids ascend inside a copy)."""
    t = [f.tile_result(p, "graphlets", census) for p in f.parts()]
    items = [f.tile_result(p, "graphlet_items", ordered_items) for p in f.parts()]
    orbit = np.stack([f.per_vertex([t[p]["orbit"][o].astype(np.int64) for p in f.parts()]) for o in range(ORBITS)]).astype(np.uint64)
    want = {"orbit": orbit, "sup": f.per_edge([t[p]["sup"] for p in f.parts()]),
            "cycles4": f.per_edge([t[p]["cycles4"].astype(np.int64) for p in f.parts()]).astype(np.uint64),
            "cliques4": f.per_edge([t[p]["cliques4"].astype(np.int64) for p in f.parts()]).astype(np.uint64),
            "total": {x: f.total([t[p]["total"][x] for p in f.parts()]) for x in TYPES}}
    return want, f.total(items)


@pytest.mark.parametrize("opts", [{}, {"GRAPHLET_SHORT": "0"}], ids=["default", "lds"])
def test_past_one_tile_per_workgroup(K, monkeypatch, opts):
    """The two queue kernels of the 4-cycle pass launch at most 2048 workgroups of four wavefronts (a root each) and at most
    1024 workgroups (a root each): 1500 tile copies have more roots than either, N + 1 vertices and more than N edges and
    triangles are past 2048 * 256 of everything else."""
    _set(monkeypatch, opts)
    u = _padded("interleaved", N + 1, [(TILE, 1500), (K2, 7), (K3, 5), (K5, 3)])
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u, with_support=True)
        want, items = _replica_want(f)
        assert f.nv > N and f.m > N and want["total"]["triangle"] > N
        assert 1500 * _roots_with_work(*TILE) > 4 * 2048
        info = _compare(a, f.eu, f.ev, want["sup"], want, items)[-1]
        assert info["cycle_items"] == items


def test_vmask_result(K):
    nv, e = TILE
    with _load(K, nv, e) as a:
        _, core = a.run_core()
        mask = (core >= 3).astype(np.uint8)
        eu, ev, sup, want, orbit, cyc, clq, info = _check(a, vmask=mask)
        assert 0 < len(eu) < len(e) and not orbit[:, mask == 0].any() and orbit[0, mask == 1].all()
        _check(a)                                                               # and the whole tile


def test_cross_checks_with_the_clique_analyses(K):
    for nv, uv in (TILE, (3000, K.gen_hug_edges(3000, 7350, 2.2, 5))):
        with _load(K, nv, uv) as a:
            a.truss_run()
            info = a.run_graphlets()[-1]
            total, _, _ = a.run_clique_census(3, 4)
            assert [int(x) for x in total] == [info["total"]["triangle"], info["total"]["clique4"]]
            a.nucleus_run()
            nuc = a.nucleus_info()
            assert nuc["n_cliques4"] == info["n_cliques4"] > 0 and nuc["n_triangles"] == info["n_triangles"]
            orbit, cyc, clq = a.graphlets_fetch_vertices(), *a.graphlets_fetch_edges()   # (neither dropped it)
            check_identities(orbit)
            assert int(cyc.sum()) == 4 * (info["total"]["cycle4"] + info["total"]["diamond"] + 3 * info["total"]["clique4"])


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order(K):
    STATE = K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, e = TILE
    with _load(K, nv, e) as a:
        assert _code(K, a.graphlets_run) == STATE                                # no k-truss result
        a.run_core()
        assert _code(K, a.graphlets_run) == STATE
        a.truss_run()
        for fn in (a.graphlets_fetch_vertices, a.graphlets_fetch_edges, a.graphlets_info):
            assert _code(K, fn) == STATE                                         # fetch / info before a run
        first = a.run_graphlets()                                                # (makes the endpoints and supports nobody fetched)
        eu, ev, tr, sup = a.truss_fetch(with_support=True)
        want = census(nv, eu, ev)
        assert np.array_equal(first[0], want["orbit"]) and np.array_equal(first[1], want["cycles4"]) and np.array_equal(first[2], want["cliques4"])
        assert lib.komb_graphlets_fetch_vertices(a._ctx, None) == 0              # NULL outputs are allowed
        assert lib.komb_graphlets_fetch_edges(a._ctx, None, None) == 0
        assert lib.komb_graphlets_info(a._ctx, *([None] * 7)) == 0
        cyc_only = np.full(len(eu), U64, np.uint64)
        assert lib.komb_graphlets_fetch_edges(a._ctx, K._lib.ptr(cyc_only), None) == 0 and np.array_equal(cyc_only, want["cycles4"])
        a.run_core(); a.run_onion(); a.run_structural_clusters(); a.nucleus_run()   # the other analyses neither change nor drop it
        assert np.array_equal(a.graphlets_fetch_vertices(), want["orbit"])
        second = a.run_graphlets()                                               # two runs on one context
        for x, y in zip(first[:3], second[:3]):
            assert np.array_equal(x, y)
        assert first[3]["total"] == second[3]["total"]
        a.truss_run()                                                            # a new k-truss run drops it
        for fn in (a.graphlets_fetch_vertices, a.graphlets_fetch_edges, a.graphlets_info):
            assert _code(K, fn) == STATE
        a.truss_run_slice(0, 2)                                                  # a slice is no result to count in
        assert _code(K, a.graphlets_run) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, a.graphlets_run) == STATE
        a.truss_run_slice(0, 1)
        assert np.array_equal(a.run_graphlets()[0], want["orbit"])
        a.truss_unprepare()
        assert _code(K, a.graphlets_info) == STATE and _code(K, a.graphlets_run) == STATE
        a.from_edges(3, [[0, 1]])                                                # a new graph
        assert _code(K, a.graphlets_info) == STATE
        a.truss_run()
        assert a.run_graphlets()[0][0].tolist() == [1, 1, 0]


@pytest.mark.parametrize("word", ["0xFFFFFFFF", "0x00000001", "0x7FFFFFFF"])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, word, tier_graphs):
    graphs = [tuple(tier_graphs["hug"][:2]), TILE, _hub_graph()]
    def results(a):
        out = []
        for nv, uv in graphs:
            a.from_edges(nv, _i64(uv))
            core = a.run_core()[1]
            for vmask in (None, (core >= 3).astype(np.uint8)):
                a.truss_run(vmask)
                orbit, cyc, clq, info = a.run_graphlets()
                out += [orbit, cyc, clq, np.asarray([info["total"][t] for t in TYPES] + [info["cycle_items"], info["max_degree"]])]
        return out
    with K.KombAccel() as a:
        want = results(a)
    monkeypatch.setenv("KOMB_POISON", word)
    monkeypatch.setenv("KOMB_GRAPHLET_DEBUG", "1")
    with K.KombAccel() as a:
        for turn in range(2):
            got = results(a)
            assert len(got) == len(want)
            for x, y in zip(got, want):
                assert np.array_equal(x, y)


def _star(K, leaves):
    a = K.KombAccel()
    a.from_edges(leaves + 1, np.stack([np.zeros(leaves, np.int64), np.arange(1, leaves + 1)], 1))
    a.truss_run()
    return a


def test_degree_limit(K):
    LIMIT = K._lib.KOMB_ERR_LIMIT
    lib = K._lib.load()
    with _star(K, 2 ** 20) as a:
        assert _code(K, a.graphlets_run) == LIMIT
        assert b"2^20" in lib.komb_last_error(a._ctx)
        out = np.full(ORBITS * a.nv, U64, np.uint64)
        assert lib.komb_graphlets_fetch_vertices(a._ctx, K._lib.ptr(out)) == K._lib.KOMB_ERR_STATE     # nothing installed, nothing written
        assert (out == U64).all()
    n = 2 ** 20 - 1
    with _star(K, n) as a:
        orbit, cyc, clq, info = a.run_graphlets()
        assert int(orbit[7, 0]) == comb(n, 3) and int(orbit[2, 0]) == comb(n, 2) and int(orbit[0, 0]) == n
        assert (orbit[6, 1:] == comb(n - 1, 2)).all() and (orbit[1, 1:] == n - 1).all() and not orbit[[3, 4, 5, 8, 9, 10, 11, 12, 13, 14]].any()
        assert info["total"]["claw"] == comb(n, 3) and info["max_degree"] == n and info["cycle_items"] == 0 and info["flags"] == 0
        assert not cyc.any() and not clq.any()


class Graphlets(Case):
    """komb_graphlets_run on the tile: a failed run leaves the previous census (warm) or none (cold), the k-truss result exact."""
    want = None

    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS + SUPPORT

    def setup(self, a):
        load_truss(a)

    def exact(self, a):
        if Graphlets.want is None:
            Graphlets.want = census(NV, F.eu, F.ev)
        w = Graphlets.want
        cyc, clq = a.graphlets_fetch_edges()
        assert np.array_equal(a.graphlets_fetch_vertices(), w["orbit"]) and np.array_equal(cyc, w["cycles4"]) and np.array_equal(clq, w["cliques4"])
        assert a.graphlets_info()["total"] == w["total"]

    def earlier(self, a):
        a.graphlets_run()
        self.exact(a)

    def call(self, a, out):
        return a._lib.komb_graphlets_run(a._ctx)

    def after(self, a, warm):
        if warm:
            self.exact(a)
        else:
            dropped(a.graphlets_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a)


@pytest.mark.parametrize("opts", [{}, {"GRAPHLET_LDS": "0"}], ids=["default", "dense"])
def test_every_request_fails_once(K, monkeypatch, opts):
    """Every device allocation request of a cold and of a warm run fails once (tests/test_gpu_alloc_failure.py has the
    protocol); with GRAPHLET_LDS=0 the dense tables of the heavy tier are among the requests."""
    _set(monkeypatch, opts)
    case = Graphlets()
    with K.KombAccel() as a:
        for warm in case.states:
            n = run_state(a, case, warm)
            print("alloc failure sweep: graphlets_run, %s: N = %d" % ("warm" if warm else "cold", n))
