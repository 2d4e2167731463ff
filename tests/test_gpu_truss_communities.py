"""GPU tests of komb_truss_communities_run / _fetch / _fetch_vertices / _info: every label, size and n_comm entry is
compared exactly with the numpy / scipy reference of tests/truss_communities_ref.py (trussness taken from the library's
own run_truss, whose parity other tests own), and info with the reference's summary."""
import hashlib

import numpy as np
import pytest

import components_ref as CR
import truss_communities_ref as R

pytestmark = pytest.mark.gpu

KMAX = -1


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _resolve(k, tr):
    tmax = int(tr.max()) if len(tr) else 2
    return max(tmax, 2) if k == KMAX else max(k, 2)


def _expect(a, k, eu, ev, tr, tri=None, want=None):
    """Run threshold k on a's last k-truss result (eu, ev, tr) and compare everything with the reference."""
    a.truss_communities_run(k)
    return _compare(a, k, eu, ev, tr, tri, want)


def _compare(a, k, eu, ev, tr, tri=None, want=None):
    """The held communities of threshold k of the k-truss result (eu, ev, tr): everything against the reference."""
    label, size = a.truss_communities_fetch()
    info = a.truss_communities_info()
    n_comm = a.truss_communities_fetch_vertices()
    kk = _resolve(k, tr)
    if want is None:
        want = R.communities(a.nv, eu, ev, tr, kk, tri)
    assert label.dtype == np.int32 and size.dtype == np.int32 and n_comm.dtype == np.int32
    assert len(label) == len(tr) and len(size) == len(tr) and len(n_comm) == a.nv
    assert np.array_equal(label, want), k
    assert np.array_equal(size, R.sizes(want)), k
    assert np.array_equal(n_comm, R.vertex_multiplicity(a.nv, eu, ev, want)), k
    got = (info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"])
    assert got == R.summary(a.nv, eu, ev, want), k
    assert info["k_used"] == kk, k
    assert info["ms"] >= 0.0
    return label, size, n_comm, info


def _check(a, ks, vmask=None, want_truss=None):
    eu, ev, tr = a.run_truss(vmask)
    if want_truss is not None:
        assert (eu.tolist(), ev.tolist(), tr.tolist()) == tuple(list(w) for w in want_truss)
    tri = R.triangles(a.nv, eu, ev)
    for k in ks:
        _expect(a, k, eu, ev, tr, tri)
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
        _check(a, [2, 3, 4, 6, KMAX])
        if seed == 1:
            a.truss_communities_run(3)
            info = a.truss_communities_info()
            assert (info["n_member_edges"], info["n_communities"], info["largest"]) == (801610, 24553, 352381)
            assert info["n_multi_vertices"] == 38888


@pytest.mark.parametrize("nv", [1000, 20000, 200000])
@pytest.mark.parametrize("alpha", [2.1, 2.2, 2.6])
def test_generated_graphs(K, nv, alpha):
    uv = K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _check(a, [2, 3, KMAX])
        core = a.run_core()[1]
        a.run_truss()
        _check(a, [2, 3, KMAX], vmask=(core >= max(int(core.max()) // 2, 1)).astype(np.uint8))


def _clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


def _hub_of_cliques():
    """A hub of degree 3000 (above the 2048 entries from which a row is split over workgroups) whose neighbours form
    cliques of 2..6 vertices: one community per clique (n_cl of them), every one of them through the hub."""
    parts, v, n_cl = [], 1, 0
    while v < 3001:
        s = min(2 + n_cl % 5, 3001 - v)
        ids = np.arange(v, v + s)
        parts.append(np.stack([np.zeros(s, np.int64), ids], 1))
        if s > 1:
            parts.append(_clique(ids))
        v += s; n_cl += 1 if s > 1 else 0
    return 3001, np.concatenate(parts), n_cl


def _book(pages):
    p = np.arange(2, 2 + pages)
    return 2 + pages, np.concatenate([[[0, 1]], np.stack([np.zeros(pages, np.int64), p], 1), np.stack([np.ones(pages, np.int64), p], 1)])


def _strip(n):
    i = np.arange(n + 1)
    return n + 2, np.concatenate([np.stack([i, i + 1], 1), np.stack([i[:-1], i[:-1] + 2], 1)])


@pytest.mark.parametrize("paths", [{}, {"COMM_SHORT": "1", "COMM_HEAVY": "2"}, {"COMM_SHORT": "2", "COMM_HEAVY": "64"}])
def test_shapes_that_stress_the_kernels(K, monkeypatch, paths):
    """Every class of the triangle pass (the edge's lane, its wave, several workgroups), all links into one root, deep
    trees; ids in construction order and scattered."""
    for k, v in paths.items():
        monkeypatch.setenv("KOMB_" + k, v)
    nv_h, uv_h, n_cl = _hub_of_cliques()
    shapes = [("hub", nv_h, uv_h), ("book", *_book(5000)), ("strip", *_strip(100000)), ("K200", 200, _clique(range(200)))]
    for name, nv, uv in shapes:
        for ids in (np.arange(nv), np.random.default_rng(9).permutation(nv)):
            with K.KombAccel() as a:
                a.from_edges(nv, ids[uv])
                eu, ev, tr = a.run_truss()
                tri = R.triangles(nv, eu, ev)
                for k in (2, 3, KMAX):
                    label, size, n_comm, info = _expect(a, k, eu, ev, tr, tri)
                if name == "hub":
                    _, _, n_comm, info = _expect(a, 3, eu, ev, tr, tri)
                    assert info["n_communities"] == n_cl and n_comm[ids[0]] == n_cl and info["n_multi_vertices"] == 1
                elif name == "book":
                    _, size, _, info = _expect(a, 3, eu, ev, tr, tri)
                    assert (info["n_member_edges"], info["n_communities"], info["largest"]) == (10001, 1, 10001)
                elif name == "strip":
                    label, _, n_comm, info = _expect(a, 3, eu, ev, tr, tri)
                    assert (info["n_member_edges"], info["n_communities"], info["n_multi_vertices"]) == (200001, 1, 0)
                    assert not label.any() and np.all(n_comm == 1)
                else:
                    _, _, _, info = _expect(a, 200, eu, ev, tr, tri)
                    assert (info["n_member_edges"], info["n_communities"], info["largest"]) == (19900, 1, 19900)
                    assert _expect(a, 201, eu, ev, tr, tri)[3]["n_member_edges"] == 0


def test_edge_cases(K):
    with K.KombAccel() as a:
        # the empty graph
        a.from_edges(0, np.zeros((0, 2)))
        a.run_truss()
        for k in (0, 3, KMAX):
            label, size = a.run_truss_communities(k)
            info = a.truss_communities_info()
            assert len(label) == 0 and len(size) == 0 and len(a.truss_communities_fetch_vertices()) == 0
            assert (info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"]) == (0, 0, 0, 0)
            assert info["k_used"] == max(k, 2)
        # only isolated vertices: a result with no edges
        a.from_edges(7, np.zeros((0, 2)))
        a.run_truss()
        label, size = a.run_truss_communities(KMAX)
        assert len(label) == 0 and a.truss_communities_fetch_vertices().tolist() == [0] * 7
        assert a.truss_communities_info()["k_used"] == 2 and a.truss_communities_info()["n_communities"] == 0
        # a vmask that keeps no edge
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])
        a.run_truss(np.asarray([1, 0, 0, 1, 1, 0], np.uint8))
        label, size = a.run_truss_communities(KMAX)
        assert len(label) == 0 and a.truss_communities_fetch_vertices().tolist() == [0] * 6
        assert a.truss_communities_info()["k_used"] == 2
        # one triangle, one edge, an isolated vertex: k in {0, 1, 2} are the same call
        eu, ev, tr = a.run_truss()
        assert (eu.tolist(), ev.tolist(), tr.tolist()) == ([0, 0, 1, 4], [1, 2, 2, 5], [3, 3, 3, 2])
        for k in (0, 1, 2):
            label, size = a.run_truss_communities(k)
            assert label.tolist() == [0, 0, 0, 3] and size.tolist() == [3, 3, 3, 1]
            assert a.truss_communities_fetch_vertices().tolist() == [1, 1, 1, 0, 1, 1]
            info = a.truss_communities_info()
            assert (info["k_used"], info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"]) == (2, 4, 2, 3, 0)
        for k in (3, KMAX):
            label, size = a.run_truss_communities(k)
            assert label.tolist() == [0, 0, 0, -1] and size.tolist() == [3, 3, 3, 0]
            assert a.truss_communities_fetch_vertices().tolist() == [1, 1, 1, 0, 0, 0]
            assert a.truss_communities_info()["k_used"] == 3
        # k above the maximum: no members, not an error
        label, size = a.run_truss_communities(4)
        assert label.tolist() == [-1] * 4 and size.tolist() == [0] * 4
        assert a.truss_communities_fetch_vertices().tolist() == [0] * 6
        info = a.truss_communities_info()
        assert (info["k_used"], info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"]) == (4, 0, 0, 0, 0)
        # the bow-tie: the centre is in two communities
        a.from_edges(5, [[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]])
        a.run_truss()
        label, size = a.run_truss_communities(3)
        assert label.tolist() == [0, 0, 0, 3, 3, 3] and size.tolist() == [3] * 6
        assert a.truss_communities_fetch_vertices().tolist() == [1, 1, 2, 1, 1]
        assert a.truss_communities_info()["n_multi_vertices"] == 1
    # two K5 sharing a vertex / an edge; two cliques and a bridge; raw input with loops and duplicates
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 300, (1200, 2))
    raw = np.concatenate([raw, raw[:100], raw[:100, ::-1], np.stack([np.arange(50)] * 2, 1)])
    for nv, uv in ((9, np.concatenate([_clique(range(5)), _clique(range(4, 9))])),
                   (8, np.concatenate([_clique(range(5)), _clique(range(3, 8))])),
                   (8, np.concatenate([_clique(range(4)), _clique(range(4, 8)), [[3, 4]]])), (310, raw)):
        with K.KombAccel() as a:
            a.from_edges(nv, uv)
            _check(a, [2, 3, 4, 5, 6, KMAX])


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    tri6 = [[0, 1], [1, 2], [0, 2], [4, 5]]
    with K.KombAccel() as a:
        # no graph
        assert _code(K, lambda: a.truss_communities_run(3)) == ARG
        assert lib.komb_truss_communities_fetch(a._ctx, None, None) == ARG
        assert _code(K, a.truss_communities_fetch_vertices) == ARG
        assert _code(K, a.truss_communities_info) == ARG
        a.from_edges(6, tri6)
        # no k-truss result; fetch / info before a run
        assert _code(K, lambda: a.truss_communities_run(3)) == STATE
        assert _code(K, lambda: a.truss_communities_run(KMAX)) == STATE
        a.run_core(); a.run_onion(); a.run_components("core", 0)
        assert _code(K, lambda: a.truss_communities_run(2)) == STATE
        a.truss_run()
        assert _code(K, a.truss_communities_fetch) == STATE
        assert _code(K, a.truss_communities_fetch_vertices) == STATE
        assert _code(K, a.truss_communities_info) == STATE
        # bad thresholds (the argument is checked before the state)
        assert _code(K, lambda: a.truss_communities_run(-2)) == ARG
        assert _code(K, lambda: a.truss_communities_run(-100)) == ARG
        assert _code(K, a.truss_communities_fetch) == STATE
        # the endpoints of a whole-graph result nobody has fetched yet
        assert a.run_truss_communities(KMAX)[0].tolist() == [0, 0, 0, -1]
        assert a.truss_communities_info()["k_used"] == 3
        # a failed call leaves the last result readable
        assert _code(K, lambda: a.truss_communities_run(-7)) == ARG
        assert a.truss_communities_fetch()[0].tolist() == [0, 0, 0, -1]
        # k-core, onion, components and CoreA calls neither change nor drop it
        deg, core = a.run_core(); a.run_onion(); a.run_components("core", 1); a.run_components("truss", 3)
        a.get_anomaly_score(deg, core)
        assert a.truss_communities_fetch()[0].tolist() == [0, 0, 0, -1]
        assert a.truss_communities_fetch_vertices().tolist() == [1, 1, 1, 0, 0, 0]
        # NULL outputs are allowed
        assert lib.komb_truss_communities_fetch(a._ctx, None, None) == 0
        assert lib.komb_truss_communities_fetch_vertices(a._ctx, None) == 0
        assert lib.komb_truss_communities_info(a._ctx, None, None, None, None, None, None) == 0
        # a new k-truss run of any kind drops it
        a.truss_run()
        assert _code(K, a.truss_communities_fetch) == STATE
        assert _code(K, a.truss_communities_info) == STATE
        assert a.run_truss_communities(2)[0].tolist() == [0, 0, 0, 3]
        a.truss_run(np.asarray([1, 1, 1, 0, 0, 0], np.uint8))
        assert _code(K, a.truss_communities_fetch_vertices) == STATE
        assert a.run_truss_communities(2)[0].tolist() == [0, 0, 0]
        # a slice of the canonical edges is not a k-truss result to split
        a.truss_run_slice(0, 2)
        assert _code(K, a.truss_communities_fetch) == STATE
        assert _code(K, lambda: a.truss_communities_run(2)) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, lambda: a.truss_communities_run(KMAX)) == STATE
        a.truss_run_slice(0, 1)                                    # the whole range
        assert a.run_truss_communities(3)[0].tolist() == [0, 0, 0, -1]
        # komb_truss_unprepare drops the k-truss result and the communities with it
        a.truss_unprepare()
        assert _code(K, a.truss_communities_fetch) == STATE
        assert _code(K, a.truss_communities_info) == STATE
        assert _code(K, lambda: a.truss_communities_run(3)) == STATE
        a.truss_run()
        assert a.run_truss_communities(3)[1].tolist() == [3, 3, 3, 0]
        # a new graph drops it
        a.from_edges(3, [[0, 1]])
        assert _code(K, a.truss_communities_fetch) == STATE
        assert _code(K, a.truss_communities_fetch_vertices) == STATE
        assert _code(K, a.truss_communities_info) == STATE
        assert _code(K, lambda: a.truss_communities_run(2)) == STATE
        a.truss_run()
        assert a.run_truss_communities(0)[0].tolist() == [0]
        # a failed graph load leaves no graph
        with pytest.raises(K.KombError):
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.truss_communities_info) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        core = a.run_core()[1]
        for vmask in (None, (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)):
            a.truss_run(vmask)
            for k in (2, 3, 4, KMAX):
                out += list(a.run_truss_communities(k))
                out.append(a.truss_communities_fetch_vertices())
                info = a.truss_communities_info()
                out.append(np.asarray([info[x] for x in ("k_used", "n_member_edges", "n_communities", "largest", "n_multi_vertices")]))
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"COMP_SAMPLE": "0"}, {"COMP_SAMPLE": "1"}, {"COMM_SHORT": "1", "COMM_HEAVY": "2"},
                                  {"COMM_SHORT": "3", "COMM_HEAVY": "9"}, {"COMM_SHORT": "64", "COMM_HEAVY": "1000000000"},
                                  {"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "COMM_HEAVY": "40"}])
def test_options_change_nothing(K, monkeypatch, opts):
    graphs = [CR.composite(K.gen_hug_edges, 3), (900, K.gen_hug_edges(900, 2200, 2.6, 6)), (50000, K.gen_hug_edges(50000, 122500, 2.1, 7))]
    want = [_all_results(K, nv, uv) for nv, uv in graphs]
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)
    with K.KombAccel() as a:                     # one context across the three graphs: larger, smaller, larger
        for (nv, uv), w in zip(graphs, want):
            got = _all_results(K, nv, uv, a)
            assert len(got) == len(w)
            for x, y in zip(got, w):
                assert np.array_equal(x, y)


def test_repeated_calls_identical(K):
    nv, uv = CR.composite(K.gen_hug_edges, 4)
    first = _all_results(K, nv, uv)
    for _ in range(2):
        for x, y in zip(_all_results(K, nv, uv), first):
            assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """A communities run changes no k-core, onion, components or k-truss result and no komb_stats field, and the resident
    k-truss preparation survives it."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv, uv = CR.composite(K.gen_hug_edges, 5)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        layer, ocore = a.run_onion()
        eu, ev, tr, sup = a.run_truss(with_support=True)
        clabel, csize = a.run_components("truss", 3)
        cinfo = a.components_info()
        st = a.stats()
        for k in (3, 2, KMAX, 4, 1000):
            a.truss_communities_run(k)
            assert a.stats() == st
            a.truss_communities_fetch(); a.truss_communities_fetch_vertices(); a.truss_communities_info()
            assert a.stats() == st
        d2, c2 = a.core_fetch()
        l2, o2 = a.onion_fetch()
        e2 = a.truss_fetch(with_support=True)
        cl2, cs2 = a.components_fetch()
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, sup, clabel, csize), (d2, c2, l2, o2) + tuple(e2) + (cl2, cs2)):
            assert np.array_equal(x, y)
        assert a.components_info() == cinfo and a.stats() == st
        # the preparation of the graph is still there: the next k-truss run does not make one
        e3 = a.run_truss(with_support=True)
        assert a.stats()["truss_prepared"] == 0
        for x, y in zip((eu, ev, tr, sup), e3):
            assert np.array_equal(x, y)
        # under a vmask the communities are those of the subgraph's result, and the resident preparation stays
        vmask = (core >= int(core.max()) // 2).astype(np.uint8)
        su, sv, st_ = a.run_truss(vmask)
        _expect(a, 3, su, sv, st_)
        _expect(a, KMAX, su, sv, st_)
        a.truss_run()
        assert a.stats()["truss_prepared"] == 0


def _sha(x):
    return hashlib.sha256(np.ascontiguousarray(x, np.int32).tobytes()).hexdigest()[:16]


def test_full_size_c2(K):
    nv = 1_000_000
    uv = K.gen_hug_edges(nv, 2_425_000, 2.6, 42)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        del uv
        eu, ev, tr = a.run_truss()
        assert len(eu) == 9_998_435 and int(tr.max()) == 26
        tri = R.triangles(nv, eu, ev)
        assert len(tri[0]) == 9_597_768
        label, _, _, info = _expect(a, 3, eu, ev, tr, tri)
        print("C2 k=3:", info, _sha(label))
        assert (info["n_member_edges"], info["n_communities"], info["largest"]) == (9_019_096, 863_764, 3_969_947)
        assert _sha(label) == "f55c813dc95dc030"
        label, _, _, info = _expect(a, KMAX, eu, ev, tr, tri)
        print("C2 k=max:", info)
        assert (info["k_used"], info["n_member_edges"], info["n_communities"], info["largest"]) == (26, 1149, 1, 1149)


# k = 3 at C3: 89 697 942 member edges (of 100 120 558; 88 336 441 triangles, largest trussness 40) in 10 889 087 communities,
# the largest of 21 431 671 edges, 8 122 421 vertices in more than one.  The SHA-256 prefix of the int32 labels and the counts are
# those of the full CPU reference (tests/manual/c3_communities_check.py's computation: 12 min, oracle trussness included).
C3_K3 = {"hash": "d6d55a7399ecbbae", "counts": (89_697_942, 10_889_087, 21_431_671), "n_multi_vertices": 8_122_421}


def _c3_invariants(nv, eu, ev, tr, labels, sizes_):
    """The invariants of tests/test_truss_communities_ref.py, computed from the outputs alone."""
    idx = np.arange(len(tr))
    for k in sorted(labels):
        lab, sz = labels[k], sizes_[k]
        mem = lab >= 0
        assert np.array_equal(mem, tr >= k), k
        assert not np.any(sz[mem] == 1) and not np.any(sz[~mem]), k
        assert np.array_equal(lab[lab[mem]], lab[mem]) and np.all(lab[mem] <= idx[mem]), k
        cnt = np.bincount(lab[mem], minlength=len(tr))
        assert np.array_equal(sz[mem], cnt[lab[mem]]), k
        del cnt
        if k + 1 in labels:
            up = labels[k + 1]
            sel = up >= 0
            assert np.array_equal(lab[up[sel]], lab[sel]), k
        comp = CR.truss_components(nv, eu, ev, tr, k)
        assert np.array_equal(comp[eu[mem]], comp[ev[mem]]) and np.array_equal(comp[eu[mem]], comp[eu[lab[mem]]]), k


def test_full_size_c3(K):
    """No CPU reference of the whole graph here (tests/manual/c3_communities_check.py runs it by hand): the invariants,
    equality across the option variants, K_MAX against the reference on the max-truss subgraph, and the pinned hash."""
    nv = 10_000_000
    uv = K.gen_hug_edges(nv, 24_250_000, 2.6, 42)
    got = {}
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        del uv
        assert a.ne == 100_120_558
        eu, ev, tr = a.run_truss()
        tmax = int(tr.max())
        for name, opts in (("default", {}), ("wave", {"COMM_SHORT": "1", "COMM_HEAVY": "1000000000"}), ("split", {"COMM_HEAVY": "256"})):
            for o in ("COMM_SHORT", "COMM_HEAVY"):
                a.set_option(o, opts.get(o))
            for k in ((3, 4, KMAX) if name == "default" else (3, KMAX)):
                label, size = a.run_truss_communities(k)
                info = a.truss_communities_info()
                n_comm = a.truss_communities_fetch_vertices() if k != 4 else None
                if name == "default":
                    got[k] = (label, size, n_comm, info)
                    print("C3 k =", k, info, _sha(label))
                else:
                    info.pop("ms"); ref = dict(got[k][3]); ref.pop("ms")
                    assert np.array_equal(label, got[k][0]) and np.array_equal(size, got[k][1]) and info == ref, (name, k)
                    assert n_comm is None or np.array_equal(n_comm, got[k][2]), (name, k)
    _c3_invariants(nv, eu, ev, tr, {3: got[3][0], 4: got[4][0]}, {3: got[3][1], 4: got[4][1]})
    # n_comm from the outputs
    for k in (3,):
        assert np.array_equal(got[k][2], R.vertex_multiplicity(nv, eu, ev, got[k][0]))
        assert got[k][3]["n_multi_vertices"] == int((got[k][2] > 1).sum())
    # K_MAX: the reference on the max-truss subgraph (small)
    sel = np.flatnonzero(tr >= tmax)
    sub = R.communities(nv, eu[sel], ev[sel], tr[sel], tmax)
    want = np.full(len(tr), -1, np.int64)
    want[sel] = sel[sub]
    label, size, n_comm, info = got[KMAX]
    assert info["k_used"] == tmax
    assert np.array_equal(label, want) and np.array_equal(size, R.sizes(want))
    assert np.array_equal(n_comm, R.vertex_multiplicity(nv, eu, ev, want))
    assert (info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"]) == R.summary(nv, eu, ev, want)
    info = got[3][3]
    assert (_sha(got[3][0]), (info["n_member_edges"], info["n_communities"], info["largest"])) == (C3_K3["hash"], C3_K3["counts"])
    assert info["n_multi_vertices"] == C3_K3["n_multi_vertices"]
