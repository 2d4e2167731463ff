"""GPU tests of komb_betweenness_run / _fetch / _fetch_sources / _info: bc is compared with tests/betweenness_ref.py as raw
64-bit patterns, the per-source integers and every info field except ms exactly.  The reference is fed the library's own CSR
(komb_graph_get_csr, whose parity other tests own).  tests/test_betweenness_ref.py shows that the stored fixture tells a fused
multiply-add and a different row order from the definition, so bit equality here says something about both."""
import ctypes

import numpy as np
import pytest

import betweenness_ref as R
from test_betweenness_ref import bits, load_fixture

pytestmark = pytest.mark.gpu

INFO = ("n_sources", "flags", "depth_max", "n_batches", "n_level_steps")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _load(K, nv, uv):
    a = K.KombAccel()
    a.from_edges(nv, np.asarray(uv, dtype=np.int64).reshape(-1, 2))
    return a


def _rows(a):
    rowptr, col = a.get_csr()
    return R.rows_of_csr(rowptr.tolist(), col.tolist())


def _same(got, want):
    bc, per, info = got
    assert bc.dtype == np.float64 and len(bc) == len(want["bc"])
    diff = np.flatnonzero(bits(bc) != bits(want["bc"]))
    assert len(diff) == 0, (len(diff), diff[:5], bc[diff[:5]], want["bc"][diff[:5]])
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert per[name].dtype == want[name].dtype and np.array_equal(per[name], want[name]), name
    assert {k: info[k] for k in INFO} == {k: want[k] for k in INFO}
    assert info["ms"] >= 0.0


def _check(a, sources=None, rows=None):
    want = R.betweenness(_rows(a) if rows is None else rows, sources)
    got = a.run_betweenness(sources)
    _same(got, want)
    return got, want


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


@pytest.fixture(scope="module")
def hug(K):
    """A generated graph of 3000 vertices with a hub of more than a thousand neighbours (the kernels read a row 64 entries at
    a time), its rows, and the references of the source lists, each computed once."""
    nv, uv = 3000, K.gen_hug_edges(3000, 7350, 2.2, 5)
    rows = R.adjacency(nv, uv)
    assert max(len(r) for r in rows) > 1000
    return {"nv": nv, "uv": uv, "rows": rows, "want": {}}


def _hug_sources(hug, which):
    rows, nv = hug["rows"], hug["nv"]
    rng = np.random.default_rng(11)
    hub = max(range(nv), key=lambda v: len(rows[v]))
    isolated = [v for v in range(nv) if not rows[v]]
    return {"1": [hub], "63": rng.permutation(nv)[:63].tolist(), "64": rng.permutation(nv)[:64].tolist(),
            "65": rng.permutation(nv)[:65].tolist(), "130": rng.permutation(nv)[:130].tolist(),
            "duplicates": [7, 7, hub, 2999, 7, hub] * 12, "unsorted": list(range(140, 0, -2)),
            "isolated": (isolated[:3] + [hub] + isolated[:1]) if isolated else [hub]}[which]


def _hug_want(hug, which):
    if which not in hug["want"]:
        hug["want"][which] = R.betweenness(hug["rows"], _hug_sources(hug, which))
    return hug["want"][which]


def test_golden_graphs_from_every_vertex(K, golden):
    for g in golden:
        with _load(K, g["nv"], g["raw"]) as a:
            rows = _rows(a)
            assert rows == R.rows_of_csr(g["rowptr"], g["col"])
            if g["nv"] <= 300:
                _check(a, None, rows)
            _check(a, list(range(g["nv"] - 1, -1, -3)), rows)


def test_the_stored_fixture_bit_for_bit(K):
    nv, pairs, stored = load_fixture()
    with _load(K, nv, pairs) as a:
        (bc, per, info), want = _check(a)
        assert np.array_equal(bits(bc), stored)
        assert np.array_equal(a.run_betweenness(halve=True)[0], bc / 2)
        _check(a, [48, 0, 17, 17, 3])


@pytest.mark.parametrize("which", ["1", "63", "64", "65", "130", "duplicates", "unsorted", "isolated"])
def test_source_lists(K, hug, which):
    """A partial last batch, exactly one batch, more than two batches, repeated sources, sources in descending order, sources
    without a neighbour beside one with a thousand."""
    with _load(K, hug["nv"], hug["uv"]) as a:
        _same(a.run_betweenness(_hug_sources(hug, which)), _hug_want(hug, which))


def test_past_one_pass_of_the_grid(K, hug, monkeypatch):
    """BTW_GRID=2: eight waves take the 3000 vertices in turns."""
    monkeypatch.setenv("KOMB_BTW_GRID", "2")
    monkeypatch.setenv("KOMB_BTW_DEBUG", "1")
    with _load(K, hug["nv"], hug["uv"]) as a:
        for which in ("65", "duplicates"):
            _same(a.run_betweenness(_hug_sources(hug, which)), _hug_want(hug, which))


def test_components_and_degenerate_graphs(K):
    with _load(K, 9, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (4, 6)]) as a:   # a path, a triangle, two isolated vertices
        (bc, per, info), _ = _check(a, [0, 4, 8, 2, 7, 5])                     # unreached lanes beside reached ones
        assert per["n_reached"].tolist() == [4, 3, 1, 4, 1, 3] and per["ecc"].tolist() == [3, 1, 0, 2, 0, 1]
        _check(a)
        (bc, per, info), _ = _check(a, [])                                     # no source: a valid run with zeros everywhere
        assert bc.tolist() == [0.0] * 9 and info["n_sources"] == 0 and info["n_level_steps"] == 0 and len(per["ecc"]) == 0
        _check(a, [8, 7])                                                      # isolated sources only
    with _load(K, 1, np.zeros((0, 2))) as a:
        (bc, per, info), _ = _check(a)
        assert bc.tolist() == [0.0] and per["n_reached"].tolist() == [1]
        _check(a, [0, 0, 0])
    with _load(K, 70, np.zeros((0, 2))) as a:                                  # no edges, more than one batch
        (bc, per, info), _ = _check(a)
        assert not bc.any() and info["n_batches"] == 2 and info["depth_max"] == 0


def test_a_long_path_from_its_end(K):
    n = 3000
    with _load(K, n, np.stack([np.arange(n - 1), np.arange(1, n)], 1)) as a:
        (bc, per, info), _ = _check(a, [0])
        assert info["depth_max"] == n - 1 and info["n_level_steps"] == n + n - 2
        assert bc.tolist() == [0.0] + [float(n - 1 - v) for v in range(1, n)]
        _check(a, [n - 1, 1500, 0])


@pytest.mark.parametrize("k", [52, 53])
def test_diamond_chain_rounded_flag(K, k):
    nv, pairs = R.diamond_chain(k)
    with _load(K, nv, pairs) as a:
        (bc, per, info), _ = _check(a, [0, nv - 1, nv // 2])
        assert info["flags"] == (K._lib.KOMB_BETWEENNESS_ROUNDED if k == 53 else 0)


def test_overflow_is_a_limit_and_keeps_the_previous_result(K):
    LIMIT = K._lib.KOMB_ERR_LIMIT
    nv, pairs = R.layered(256)
    with _load(K, nv, pairs) as a:
        (bc, per, info), _ = _check(a, [0])
        assert info["flags"] == K._lib.KOMB_BETWEENNESS_ROUNDED and info["depth_max"] == 256
    nv, pairs = R.layered(258)
    with _load(K, nv, pairs) as a:
        first, _ = _check(a, [17, 40])                                         # (from layers 2 and 3 the counts stay finite)
        assert _code(K, lambda: a.betweenness_run([0])) == LIMIT
        assert b"binary64" in a._lib.komb_last_error(a._ctx)
        assert _code(K, lambda: a.betweenness_run([3, 0, 4])) == LIMIT
        again = (a.betweenness_fetch(), a.betweenness_fetch_sources(), a.betweenness_info())
        assert np.array_equal(bits(again[0]), bits(first[0])) and again[2] == first[2]
        for name in first[1]:
            assert np.array_equal(again[1][name], first[1][name])


def test_errors_and_state(K, hug):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    nv, pairs, stored = load_fixture()
    with _load(K, nv, pairs) as a:
        for fn in (a.betweenness_fetch, a.betweenness_fetch_sources, a.betweenness_info):
            assert _code(K, fn) == STATE                                       # fetch / info before a run
        out = np.full(nv, -7.0)
        assert lib.komb_betweenness_fetch(a._ctx, K._lib.ptr(out)) == STATE and (out == -7.0).all()
        first, _ = _check(a, [3, 1, 4, 1, 5])
        src = np.asarray([0, nv, 1], np.int32)
        assert lib.komb_betweenness_run(a._ctx, 3, K._lib.ptr(src)) == ARG     # an id out of range
        src = np.asarray([0, -1], np.int32)
        assert lib.komb_betweenness_run(a._ctx, 2, K._lib.ptr(src)) == ARG
        assert lib.komb_betweenness_run(a._ctx, -1, K._lib.ptr(src)) == ARG    # a negative count
        assert np.array_equal(bits(a.betweenness_fetch()), bits(first[0])) and a.betweenness_info() == first[2]
        assert lib.komb_betweenness_run(a._ctx, -5, None) == 0                 # NULL: every vertex, the count is ignored
        assert np.array_equal(bits(a.betweenness_fetch()), stored)
        assert lib.komb_betweenness_fetch(a._ctx, None) == 0                   # NULL outputs are allowed
        assert lib.komb_betweenness_fetch_sources(a._ctx, None, None, None, None) == 0
        assert lib.komb_betweenness_info(a._ctx, *([None] * 6)) == 0
        ecc = np.full(nv, -7, np.int32)
        assert lib.komb_betweenness_fetch_sources(a._ctx, None, None, None, K._lib.ptr(ecc)) == 0 and (ecc >= 0).all()
        a.from_edges(3, [[0, 1], [1, 2]])                                      # a graph load drops it
        assert _code(K, a.betweenness_info) == STATE and _code(K, a.betweenness_fetch) == STATE
        assert a.run_betweenness()[0].tolist() == [0.0, 2.0, 0.0]


def test_the_other_analyses_and_this_one_leave_each_other_alone(K, hug):
    with _load(K, hug["nv"], hug["uv"]) as a:
        want = _hug_want(hug, "65")
        a.betweenness_run(_hug_sources(hug, "65"))
        deg, core = a.run_core()
        eu, ev, tr, sup = a.run_truss(with_support=True)
        stats = a.stats()
        _same((a.betweenness_fetch(), a.betweenness_fetch_sources(), a.betweenness_info()), want)   # neither changed it
        a.betweenness_run(_hug_sources(hug, "1"))
        assert a.stats() == stats                                              # no komb_stats field moves
        deg2, core2 = a.core_fetch()
        eu2, ev2, tr2, sup2 = a.truss_fetch(with_support=True)
        for x, y in ((deg, deg2), (core, core2), (eu, eu2), (ev, ev2), (tr, tr2), (sup, sup2)):
            assert np.array_equal(x, y)
        eu3, ev3, tr3, sup3 = a.run_truss(with_support=True)                   # the resident k-truss preparation still serves
        assert np.array_equal(tr, tr3) and np.array_equal(sup, sup3)
        _same((a.betweenness_fetch(), a.betweenness_fetch_sources(), a.betweenness_info()), _hug_want(hug, "1"))


@pytest.mark.parametrize("word", ["0xFFFFFFFF", "0x00000001", "0x7FF00000"])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, word, hug):
    """Nothing of the [vertex][64] state is initialised: every read of it must be of what the run wrote.  0x7FF00000 repeated
    is a NaN as a double and a large level as a distance."""
    nv, pairs, stored = load_fixture()
    k52 = R.diamond_chain(52)
    monkeypatch.setenv("KOMB_POISON", word)
    with K.KombAccel() as a:
        for turn in range(2):
            a.from_edges(nv, pairs)
            assert np.array_equal(bits(a.run_betweenness()[0]), stored)
            _check(a, [48, 0, 17, 17, 3])
            a.from_edges(hug["nv"], np.asarray(hug["uv"], dtype=np.int64).reshape(-1, 2))
            for which in ("65", "isolated"):
                _same(a.run_betweenness(_hug_sources(hug, which)), _hug_want(hug, which))
            a.from_edges(k52[0], k52[1])
            _check(a, [0, k52[0] - 1, 7])


def test_every_allocation_request_fails_once(K):
    NOMEM = K._lib.KOMB_ERR_NOMEM
    nv, pairs, stored = load_fixture()
    with _load(K, nv, pairs) as a:
        first, _ = _check(a, [9, 2, 30])
        in_use = a.alloc_info()["pool_blocks_in_use"]
        a.set_option("ALLOC_FAIL_AT", "0")                                     # only count
        a.betweenness_run()
        n = a.alloc_info()["requests"]
        assert n >= 8                                                          # bc, the three [vertex][64] arrays, the masks, ...
        assert np.array_equal(bits(a.betweenness_fetch()), stored)
        a.betweenness_run([9, 2, 30])
        held = a.betweenness_info()
        assert {k: held[k] for k in INFO} == {k: first[2][k] for k in INFO}
        for i in range(1, n + 1):
            a.set_option("ALLOC_FAIL_AT", str(i))
            assert _code(K, lambda: a.betweenness_run()) == NOMEM, i
            info = a.alloc_info()
            assert info["fired"] == 1 and info["pool_blocks_in_use"] == in_use, i
            assert np.array_equal(bits(a.betweenness_fetch()), bits(first[0])) and a.betweenness_info() == held
            assert np.array_equal(a.betweenness_fetch_sources()["sum_dist"], first[1]["sum_dist"])
        a.set_option("ALLOC_FAIL_AT", str(n + 1))                              # one past the last: the run succeeds
        a.betweenness_run()
        assert a.alloc_info()["fired"] == 0
        a.set_option("ALLOC_FAIL_AT", None)
        assert np.array_equal(bits(a.run_betweenness()[0]), stored)
        assert a.alloc_info()["pool_blocks_in_use"] == in_use
