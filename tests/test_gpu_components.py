"""GPU tests of komb_components_run / _fetch / _info: labels and sizes compared exactly, every entry, with the scipy
reference of tests/components_ref.py (coreness / trussness taken from the library's own run_core / run_truss, whose
parity other tests own), and info with the counts recomputed from the reference labels."""
import hashlib

import numpy as np
import pytest

import components_ref as R

pytestmark = pytest.mark.gpu

KMAX = -1


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _expect(a, kind, k, want, k_used=None):
    """Run (kind, k) on a and compare label, size and info with the reference labels `want`."""
    a.components_run(kind, k)
    return _compare(a, kind, k, want, k_used)


def _compare(a, kind, k, want, k_used=None):
    """The held result of a run (kind, k): label, size and info against the reference labels `want`."""
    label, size = a.components_fetch()
    info = a.components_info()
    tag = (kind, k)
    assert label.dtype == np.int32 and size.dtype == np.int32
    assert np.array_equal(label, want), tag
    assert np.array_equal(size, R.sizes(want)), tag
    mem, comp, big = R.summary(want)
    assert (info["n_members"], info["n_components"], info["largest"]) == (mem, comp, big), tag
    assert info["kind"] == {"core": 0, "truss": 1}[kind], tag
    if k_used is not None:
        assert info["k_used"] == k_used, tag
    assert info["ms"] >= 0.0
    return label, size


def _check_core(a, ks, want_core=None):
    rowptr, col = a.get_csr()
    _, core = a.run_core()
    if want_core is not None:
        assert core.tolist() == list(want_core)
    kmax = int(core.max()) if len(core) else 0
    for k in ks:
        kk = kmax if k == KMAX else k
        _expect(a, "core", k, R.core_components(rowptr, col, core, kk), k_used=kk)
    return kmax


def _check_truss(a, ks, vmask=None, want=None):
    eu, ev, tr = a.run_truss(vmask)
    if want is not None:
        assert (eu.tolist(), ev.tolist(), tr.tolist()) == tuple(list(w) for w in want)
    tmax = int(tr.max()) if len(tr) else 2
    for k in ks:
        kk = tmax if k == KMAX else k
        _expect(a, "truss", k, R.truss_components(a.nv, eu, ev, tr, kk), k_used=kk)
    return tmax


def test_golden_graphs(K, golden):
    for g in golden:
        nv = g["nv"]
        kc = max(g["coreness"]) if nv else 0
        kt = max(g["trussness"]) if g["trussness"] else 2
        kts = max(g["sub_trussness"]) if g["sub_trussness"] else 2
        for load in ("raw", "csr"):
            with K.KombAccel() as a:
                if load == "raw":
                    a.from_edges(nv, _i64(g["raw"]))
                else:
                    a.from_csr(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int32))
                assert _check_core(a, list(range(0, kc + 2)) + [KMAX], g["coreness"]) == kc, g["name"]
                assert _check_truss(a, list(range(2, kt + 2)) + [KMAX], want=(g["eu"], g["ev"], g["trussness"])) == kt, g["name"]
                assert _check_truss(a, list(range(2, kts + 2)) + [KMAX], vmask=np.asarray(g["maxcore_mask"], np.uint8),
                                    want=(g["sub_eu"], g["sub_ev"], g["sub_trussness"])) == kts, g["name"]


@pytest.mark.parametrize("seed", [1, 2])
def test_composite(K, seed):
    nv, uv = R.composite(K.gen_hug_edges, seed)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _check_core(a, [0, 1, 2, 3, 5, KMAX])
        _check_truss(a, [2, 3, 4, 6, KMAX])
        if seed == 1:
            a.components_run("core", 2)
            info = a.components_info()
            assert (info["n_members"], info["n_components"], info["largest"]) == (84671, 15, 48304)


@pytest.mark.parametrize("nv", [1000, 20000, 200000])
@pytest.mark.parametrize("alpha", [2.1, 2.2, 2.6])
def test_generated_graphs(K, nv, alpha):
    uv = K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        _check_core(a, [0, 1, 2, KMAX])
        _check_truss(a, [2, 3, KMAX])


def _two_k40(bridge_vertex):
    n = 40
    iu = np.stack(np.triu_indices(n, 1), 1)
    link = [[0, 2 * n], [2 * n, n]] if bridge_vertex else [[0, n]]
    return 2 * n + (1 if bridge_vertex else 0), np.concatenate([iu, iu + n, np.asarray(link)])


def _count_tiles():
    """577 vertices, ids as given: three tiles of 256 for the counting kernel.  Tile 0 starts with a vertex without a label
    (0 is isolated), has two waves of 64 different labels each (the pairs 64+i -- 128+i) and one alternating between two
    labels that are not the tile's first (192.., step 2).  Tile 1 alternates between its first label, 256, and label 1, which
    tile 0 owns (the even and the odd chain of 256..511; 1 -- 257 joins the odd one to the path 1..63).  Tile 2 is one
    label, 512, and its last wave has one active lane (576)."""
    r = np.arange
    path = lambda a, b: np.stack([r(a, b), r(a + 1, b + 1)], 1)          # a - a+1 - ... - b
    step2 = lambda a, b: np.stack([r(a, b), r(a + 2, b + 2)], 1)         # (i, i + 2) for a <= i < b
    return 577, np.concatenate([path(1, 63), np.stack([64 + r(64), 128 + r(64)], 1), step2(192, 254), step2(256, 510),
                                [[1, 257]], path(512, 576)])


def test_edge_cases(K):
    # what the counting kernel meets in three tiles, both kinds
    nv, uv = _count_tiles()
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        rowptr, col = a.get_csr()
        _, core = a.run_core()
        want = R.core_components(rowptr, col, core, 1)
        assert R.summary(want) == (576, 69, 191)
        for sample in ("0", "1"):
            a.set_option("COMP_SAMPLE", sample)
            _expect(a, "core", 1, want, k_used=1)
        eu, ev, tr = a.run_truss()
        _expect(a, "truss", 2, R.truss_components(nv, eu, ev, tr, 2), k_used=2)
    with K.KombAccel() as a:
        # the empty graph
        a.from_edges(0, np.zeros((0, 2)))
        label, size = a.run_components("core", 0)
        info = a.components_info()
        assert len(label) == 0 and len(size) == 0
        assert (info["n_members"], info["n_components"], info["largest"], info["k_used"]) == (0, 0, 0, 0)
        a.run_core(); a.run_truss()
        for kind in ("core", "truss"):
            a.components_run(kind, KMAX)
            assert a.components_info()["n_components"] == 0
        assert a.components_info()["k_used"] == 2
        # only isolated vertices
        a.from_edges(7, np.zeros((0, 2)))
        label, size = a.run_components("core", 0)
        assert label.tolist() == list(range(7)) and size.tolist() == [1] * 7
        assert a.components_info()["n_components"] == 7 and a.components_info()["largest"] == 1
        a.run_core()
        label, size = a.run_components("core", 1)
        assert label.tolist() == [-1] * 7 and size.tolist() == [0] * 7
        info = a.components_info()
        assert (info["n_members"], info["n_components"], info["largest"]) == (0, 0, 0)
        label, _ = a.run_components("core", KMAX)               # the largest coreness is 0: everyone
        assert label.tolist() == list(range(7)) and a.components_info()["k_used"] == 0
        a.run_truss()
        label, size = a.run_components("truss", KMAX)           # a result with no edges
        assert label.tolist() == [-1] * 7 and size.tolist() == [0] * 7 and a.components_info()["k_used"] == 2
        # one edge (and a bystander)
        a.from_edges(4, [[3, 1]])
        label, size = a.run_components("core", 0)
        assert label.tolist() == [0, 1, 2, 1] and size.tolist() == [1, 2, 1, 2]
        a.run_core(); a.run_truss()
        label, size = a.run_components("core", 1)
        assert label.tolist() == [-1, 1, -1, 1] and size.tolist() == [0, 2, 0, 2]
        label, size = a.run_components("truss", 2)
        assert label.tolist() == [-1, 1, -1, 1] and size.tolist() == [0, 2, 0, 2]
        label, size = a.run_components("truss", 3)
        assert label.tolist() == [-1] * 4
    # the 100 000-path alone, ids in path order and scattered
    n = 100000
    path = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    for uv in (path, np.random.default_rng(5).permutation(n)[path]):
        with K.KombAccel() as a:
            a.from_edges(n, uv)
            for sample in ("0", "1"):
                a.set_option("COMP_SAMPLE", sample)
                label, size = a.run_components("core", 0)
                assert not label.any() and np.all(size == n)
            a.run_core()
            label, size = a.run_components("core", 1)
            assert not label.any() and np.all(size == n)
            label, size = a.run_components("core", 2)
            assert np.all(label == -1) and not size.any()
            a.run_truss()
            label, size = a.run_components("truss", 2)
            assert not label.any() and np.all(size == n)
    # two K_40 joined by a direct bridge edge
    nv, uv = _two_k40(False)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        a.run_core(); a.run_truss()
        for k in (1, 39, KMAX):
            label, size = a.run_components("core", k)
            assert not label.any() and np.all(size == 80), k
        assert a.components_info()["k_used"] == 39
        label, size = a.run_components("core", 40)
        assert np.all(label == -1) and a.components_info()["n_components"] == 0
        for k in (3, 40, KMAX):
            label, size = a.run_components("truss", k)
            assert label.tolist() == [0] * 40 + [40] * 40 and np.all(size == 40), k
            assert a.components_info()["n_components"] == 2
        assert a.components_info()["k_used"] == 40
        label, size = a.run_components("truss", 2)
        assert not label.any() and np.all(size == 80)
        label, size = a.run_components("truss", 41)
        assert np.all(label == -1) and not size.any()
        info = a.components_info()
        assert (info["n_members"], info["n_components"], info["largest"]) == (0, 0, 0)
    # the same two joined through a vertex of degree 2
    nv, uv = _two_k40(True)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        a.run_core()
        for k in (1, 2):
            label, size = a.run_components("core", k)
            assert not label.any() and np.all(size == 81), k
        for k in (3, 20, 39):
            label, size = a.run_components("core", k)
            assert label.tolist() == [0] * 40 + [40] * 40 + [-1] and size.tolist() == [40] * 80 + [0], k
    # raw input with loops and duplicates
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 300, (400, 2))
    raw = np.concatenate([raw, raw[:100], raw[:100, ::-1], np.stack([np.arange(50)] * 2, 1)])
    with K.KombAccel() as a:
        a.from_edges(310, raw)
        _check_core(a, [0, 1, 2, KMAX])
        _check_truss(a, [2, 3, KMAX])
    # a vertex whose only incident edges fall below the truss threshold is no member: a triangle with a tail
    with K.KombAccel() as a:
        a.from_edges(5, [[0, 1], [1, 2], [0, 2], [2, 3], [3, 4]])
        a.run_truss()
        label, size = a.run_components("truss", 3)
        assert label.tolist() == [0, 0, 0, -1, -1] and size.tolist() == [3, 3, 3, 0, 0]
        label, size = a.run_components("truss", 2)
        assert label.tolist() == [0] * 5 and size.tolist() == [5] * 5


def test_long_rows(K):
    """Rows of every class of the linking pass: short, wave-wide and grid-wide ones, members and not, giant and not."""
    parts, off = [], 0
    for n in (10, 17, 64, 65, 700, 2047, 2048, 2049, 9000, 70000):      # stars: the hub's row has n entries
        parts.append(np.stack([np.full(n, off), np.arange(off + 1, off + n + 1)], 1))
        off += n + 1
    for n in (5, 30):                                                   # cliques hanging on a long row
        iu = np.stack(np.triu_indices(n, 1), 1) + off
        parts.append(np.concatenate([iu, np.stack([np.full(3000, off), np.arange(off + n, off + n + 3000)], 1)]))
        off += n + 3000
    nv = off + 3
    uv = np.concatenate(parts)
    for ids in (np.arange(nv), np.random.default_rng(9).permutation(nv)):
        with K.KombAccel() as a:
            a.from_edges(nv, ids[uv])
            for sample in ("0", "1"):
                a.set_option("COMP_SAMPLE", sample)
                _check_core(a, [0, 1, 2, 4, KMAX])
            _check_truss(a, [2, 3, KMAX])


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


def test_call_order_and_arguments(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    with K.KombAccel() as a:
        # no graph
        assert _code(K, lambda: a.components_run("core", 0)) == ARG
        assert _code(K, a.components_fetch) == ARG
        assert _code(K, a.components_info) == ARG
        a.from_edges(6, [[0, 1], [1, 2], [0, 2], [4, 5]])
        # fetch / info before a run
        assert _code(K, a.components_fetch) == STATE
        assert _code(K, a.components_info) == STATE
        # bad arguments
        assert _code(K, lambda: a.components_run("core", -2)) == ARG
        assert _code(K, lambda: a.components_run("truss", -2)) == ARG
        assert _code(K, lambda: a.components_run(2, 0)) == ARG
        assert _code(K, lambda: a.components_run(-1, 0)) == ARG
        # results that are not there
        assert _code(K, lambda: a.components_run("core", 1)) == STATE
        assert _code(K, lambda: a.components_run("core", KMAX)) == STATE
        assert _code(K, lambda: a.components_run("truss", 2)) == STATE
        assert _code(K, lambda: a.components_run("truss", KMAX)) == STATE
        assert _code(K, a.components_fetch) == STATE               # none of these made a result
        # k = 0 needs nothing but the graph
        label, size = a.run_components("core", 0)
        assert label.tolist() == [0, 0, 0, 3, 4, 4] and size.tolist() == [3, 3, 3, 1, 2, 2]
        # a failed call leaves the last result readable, with the graph still there
        assert _code(K, lambda: a.components_run("core", -7)) == ARG
        assert a.components_fetch()[0].tolist() == [0, 0, 0, 3, 4, 4]
        a.run_core()
        assert a.run_components("core", 2)[0].tolist() == [0, 0, 0, -1, -1, -1]
        # a slice of the canonical edges is not a k-truss result to split
        a.truss_run_slice(0, 2)
        assert _code(K, lambda: a.components_run("truss", 2)) == STATE
        a.truss_run_slice(1, 2)
        assert _code(K, lambda: a.components_run("truss", KMAX)) == STATE
        a.truss_run_slice(0, 1)                                    # the whole range
        assert a.run_components("truss", 3)[0].tolist() == [0, 0, 0, -1, -1, -1]
        a.truss_run()
        assert a.run_components("truss", 2)[0].tolist() == [0, 0, 0, -1, 4, 4]
        a.truss_unprepare()
        assert _code(K, lambda: a.components_run("truss", 2)) == STATE
        assert a.components_fetch()[0].tolist() == [0, 0, 0, -1, 4, 4]      # the snapshot stays
        # the endpoints of a whole-graph result nobody has fetched yet
        a.truss_run()
        assert a.run_components("truss", KMAX)[0].tolist() == [0, 0, 0, -1, -1, -1]
        assert a.components_info()["k_used"] == 3
        # a new graph drops the result (and the coreness)
        a.from_edges(3, [[0, 1]])
        assert _code(K, a.components_fetch) == STATE
        assert _code(K, a.components_info) == STATE
        assert _code(K, lambda: a.components_run("core", 1)) == STATE
        assert _code(K, lambda: a.components_run("truss", 2)) == STATE
        assert a.run_components("core", 0)[0].tolist() == [0, 0, 2]
        # NULL outputs are allowed
        lib = K._lib.load()
        assert lib.komb_components_fetch(a._ctx, None, None) == 0
        assert lib.komb_components_info(a._ctx, None, None, None, None, None, None) == 0
        # a failed graph load leaves no graph
        with pytest.raises(K.KombError):
            a.from_edges(3, [[0, 5]])
        assert _code(K, a.components_fetch) == ARG


def _all_results(K, nv, uv, a=None):
    own = a is None
    a = a or K.KombAccel()
    try:
        a.from_edges(nv, uv)
        out = []
        a.run_core()
        for k in (0, 1, 2, 3, KMAX):
            out += list(a.run_components("core", k))
        a.run_truss()
        for k in (2, 3, 4, KMAX):
            out += list(a.run_components("truss", k))
        return out
    finally:
        if own:
            a.close()


@pytest.mark.parametrize("opts", [{"COMP_SAMPLE": "0"}, {"COMP_SAMPLE": "1"}, {"POISON": "0xFFFFFFFF"},
                                  {"POISON": "0x00000001", "COMP_SAMPLE": "0"}, {"POISON": "0x7FFFFFFF", "COMP_SAMPLE": "1"}])
def test_options_change_nothing(K, monkeypatch, opts):
    graphs = [R.composite(K.gen_hug_edges, 3), (900, K.gen_hug_edges(900, 2200, 2.6, 6)), (50000, K.gen_hug_edges(50000, 122500, 2.1, 7))]
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
    nv, uv = R.composite(K.gen_hug_edges, 4)
    first = _all_results(K, nv, uv)
    for _ in range(2):
        for x, y in zip(_all_results(K, nv, uv), first):
            assert np.array_equal(x, y)


def test_independence(K, monkeypatch):
    """Components calls change no k-core, onion or k-truss result and no komb_stats field; a later k-truss run under a
    vmask does not change an earlier snapshot."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv, uv = R.composite(K.gen_hug_edges, 5)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        deg, core = a.run_core()
        layer, ocore = a.run_onion()
        eu, ev, tr, sup = a.run_truss(with_support=True)
        st = a.stats()
        for kind, k in (("core", 0), ("truss", 3), ("core", 2), ("core", KMAX), ("truss", KMAX), ("truss", 2), ("core", 5)):
            a.components_run(kind, k)
            assert a.stats() == st
        d2, c2 = a.core_fetch()
        l2, o2 = a.onion_fetch()
        e2 = a.truss_fetch(with_support=True)
        for x, y in zip((deg, core, layer, ocore, eu, ev, tr, sup), (d2, c2, l2, o2) + tuple(e2)):
            assert np.array_equal(x, y)
        assert a.stats() == st
        # the same results once more, made after the components calls
        d3, c3 = a.run_core()
        e3 = a.run_truss(with_support=True)
        for x, y in zip((deg, core, eu, ev, tr, sup), (d3, c3) + tuple(e3)):
            assert np.array_equal(x, y)
        # a snapshot survives later runs
        label, size = a.run_components("truss", 4)
        info = a.components_info()
        vmask = (core >= int(core.max()) // 2).astype(np.uint8)
        su, sv, st_ = a.run_truss(vmask)
        a.run_core(); a.run_onion()
        l_after, s_after = a.components_fetch()
        assert np.array_equal(l_after, label) and np.array_equal(s_after, size) and a.components_info() == info
        # ... and the vmask result is split on its own terms
        _expect(a, "truss", 4, R.truss_components(nv, su, sv, st_, 4), k_used=4)
        _expect(a, "truss", KMAX, R.truss_components(nv, su, sv, st_, int(st_.max())), k_used=int(st_.max()))


def test_full_size_c2(K):
    nv = 1_000_000
    uv = K.gen_hug_edges(nv, 2_425_000, 2.6, 42)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        del uv
        for sample in ("0", "1"):
            a.set_option("COMP_SAMPLE", sample)
            kmax = _check_core(a, [0, 1, KMAX])
        _check_truss(a, [3])
        a.components_run("core", 0)
        info = a.components_info()
    print("C2 core k=0:", info, "max coreness", kmax)
    assert (info["n_components"], info["largest"], kmax) == (18758, 981159, 46)   # one giant component, small ones, isolated vertices


C3_HASH = {0: "174fd17eea1a33fe", KMAX: "ccede861725755c2"}      # (187 943 components, the largest 9 811 236; one of 354 at k = 72)


def test_full_size_c3(K):
    """Core k = 0 and K_MAX in full against scipy; the SHA-256 prefixes of both label vectors are the reference's."""
    nv = 10_000_000
    uv = K.gen_hug_edges(nv, 24_250_000, 2.6, 42)
    got = {}
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        del uv
        assert a.ne == 100_120_558
        _, core = a.run_core()
        assert hashlib.sha256(core.tobytes()).hexdigest()[:16] == "120d47bf172d8b8f"
        for sample in ("0", "1"):
            a.set_option("COMP_SAMPLE", sample)
            for k in (0, KMAX):
                label, size = a.run_components("core", k)
                got[(sample, k)] = (label, size, a.components_info())
        rowptr, col = a.get_csr()
    kmax = int(core.max())
    for k in (0, KMAX):
        want = R.core_components(rowptr, col, core, kmax if k == KMAX else k)
        mem, comp, big = R.summary(want)
        want_size = R.sizes(want)
        for sample in ("0", "1"):
            label, size, info = got[(sample, k)]
            print("C3 core k =", k, "sample", sample, info, hashlib.sha256(label.tobytes()).hexdigest()[:16])
            assert np.array_equal(label, want) and np.array_equal(size, want_size)
            assert (info["n_members"], info["n_components"], info["largest"]) == (mem, comp, big)
            assert info["k_used"] == (kmax if k == KMAX else 0)
            assert hashlib.sha256(label.tobytes()).hexdigest()[:16] == C3_HASH[k]
        del want, want_size
