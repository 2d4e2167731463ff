"""GPU tests of komb_distances_run / _fetch / _fetch_sources / _histogram / _info: every output is compared with
tests/distances_ref.py exactly, harmonic[] as raw 64-bit patterns, and every info field except ms.  The reference is fed the
library's own CSR (komb_graph_get_csr, whose parity other tests own).  tests/test_distances_ref.py shows that the stored fixture
tells the defined order of the harmonic sum from two others, so bit equality here says something about the order."""
import ctypes

import numpy as np
import pytest

import distances_ref as R

pytestmark = pytest.mark.gpu

INFO = ("n_sources", "flags", "depth_max", "depth_min", "n_pairs", "sum_all", "n_batches", "n_level_steps")
VERTEX = ("n_reached", "sum_dist", "ecc")
WORDS = (1, 2, 4)
DEFAULT_WORDS = 4


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
    vert, per, pairs, info = got
    assert vert["harmonic"].dtype == np.float64 and len(vert["harmonic"]) == len(want["harmonic"])
    diff = np.flatnonzero(R.bits(vert["harmonic"]) != R.bits(want["harmonic"]))
    assert len(diff) == 0, (len(diff), diff[:5], vert["harmonic"][diff[:5]], want["harmonic"][diff[:5]])
    for name in VERTEX:
        assert vert[name].dtype == want[name].dtype and np.array_equal(vert[name], want[name]), name
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert per[name].dtype == want["sources"][name].dtype and np.array_equal(per[name], want["sources"][name]), name
    assert pairs.dtype == np.int64 and np.array_equal(pairs, want["pairs"])
    assert {k: info[k] for k in INFO} == want["info"]
    assert info["ms"] >= 0.0


def _equal(x, y):
    """two results of the library, every array and every info field but ms"""
    for a, b in ((x[0], y[0]), (x[1], y[1])):
        for name in a:
            assert np.array_equal(R.bits(a[name]) if a[name].dtype == np.float64 else a[name], R.bits(b[name]) if b[name].dtype == np.float64 else b[name]), name
    assert np.array_equal(x[2], y[2])
    return {k: x[3][k] for k in INFO} == {k: y[3][k] for k in INFO}


def _check(a, sources=None, rows=None, words=DEFAULT_WORDS, cache=None):
    want = R.distances(_rows(a) if rows is None else rows, sources, words, cache=cache)
    got = a.run_distances(sources)
    _same(got, want)
    return got, want


def _code(K, call):
    with pytest.raises(K.KombError) as e:
        call()
    return e.value.code


@pytest.fixture(scope="module")
def hug(K):
    """The generated graph of test_gpu_betweenness.py: 3000 vertices, a hub of more than a thousand neighbours (far past the 64
    entries up to which eight lanes share a row), isolated vertices.  `master` is one list of 513 entries drawn from 150
    vertices -- repeats everywhere, no order -- that starts at the hub and has isolated vertices among its first entries; the
    lists of the tests are its prefixes, so one search per distinct vertex serves them all (`cache`)."""
    nv, uv = 3000, K.gen_hug_edges(3000, 7350, 2.2, 5)
    rows = R.adjacency(nv, uv)
    assert max(len(r) for r in rows) > 1000
    rng = np.random.default_rng(11)
    hub = max(range(nv), key=lambda v: len(rows[v]))
    isolated = [v for v in range(nv) if not rows[v]]
    assert len(isolated) >= 2
    pool = rng.permutation(nv)[:150]
    master = rng.choice(pool, size=513).tolist()
    master[0], master[5], master[40], master[41], master[70] = hub, isolated[0], isolated[1], isolated[0], hub
    return {"nv": nv, "uv": uv, "rows": rows, "master": master, "cache": {}, "want": {}}


def _hug_want(hug, n, words):
    if (n, words) not in hug["want"]:
        hug["want"][(n, words)] = R.distances(hug["rows"], hug["master"][:n], words, cache=hug["cache"])
    return hug["want"][(n, words)]


def test_golden_graphs(K, golden):
    for g in golden:
        with _load(K, g["nv"], g["raw"]) as a:
            rows = _rows(a)
            assert rows == R.rows_of_csr(g["rowptr"], g["col"])
            cache = {}
            if g["nv"] <= 300:
                _check(a, None, rows, cache=cache)
            _check(a, list(range(g["nv"] - 1, -1, -3)), rows, cache=cache)


@pytest.mark.parametrize("words", WORDS)
def test_the_stored_fixture_bit_for_bit(K, monkeypatch, words):
    monkeypatch.setenv("KOMB_DIST_WORDS", str(words))
    nv, pairs, sources, stored = R.load_fixture()
    with _load(K, nv, pairs) as a:
        (vert, per, hist, info), want = _check(a, sources, words=words)
        assert np.array_equal(R.bits(vert["harmonic"]), stored)
        assert info["n_batches"] == -(-300 // (64 * words)) and info["flags"] == 0


@pytest.mark.parametrize("words", WORDS)
def test_source_lists(K, hug, monkeypatch, words):
    """One entry, a partial batch, exactly one batch, one entry more, more than two batches -- at every width; the lists repeat
    vertices, have no order, and hold isolated vertices beside the hub."""
    monkeypatch.setenv("KOMB_DIST_WORDS", str(words))
    per = 64 * words
    with _load(K, hug["nv"], hug["uv"]) as a:
        for n in (1, per - 1, per, per + 1, 2 * per + 1):
            _same(a.run_distances(hug["master"][:n]), _hug_want(hug, n, words))
            assert a.distances_info()["n_batches"] == -(-n // per)


def test_every_vertex_as_a_source(K):
    """sources == NULL: KOMB_DISTANCES_ALL, and the per-vertex view is the per-source view."""
    nv, uv = 400, K.gen_hug_edges(400, 900, 2.2, 3)
    with _load(K, nv, uv) as a:
        (vert, per, pairs, info), want = _check(a)
        assert info["flags"] == K._lib.KOMB_DISTANCES_ALL and info["n_sources"] == nv
        for name in VERTEX:
            assert np.array_equal(vert[name], per[name]), name
        assert per["source"].tolist() == list(range(nv))
        assert info["depth_max"] == vert["ecc"].max() and info["depth_min"] == vert["ecc"].min()
        assert pairs[0] == nv and pairs.sum() == vert["n_reached"].sum() == info["n_pairs"]
        assert info["sum_all"] == vert["sum_dist"].sum()
        got = a.run_distances(list(range(nv)))                               # the same list, spelled out: only the flag differs
        assert got[3]["flags"] == 0
        for name in VERTEX + ("harmonic",):
            assert np.array_equal(R.bits(got[0][name]) if name == "harmonic" else got[0][name],
                                  R.bits(vert[name]) if name == "harmonic" else vert[name])


@pytest.mark.parametrize("words", (1, 4))
def test_past_one_pass_of_the_grid(K, hug, monkeypatch, words):
    """DIST_GRID=2: eight waves take the 3000 vertices in 47 turns of eight vertices each."""
    monkeypatch.setenv("KOMB_DIST_GRID", "2")
    monkeypatch.setenv("KOMB_DIST_DEBUG", "1")
    monkeypatch.setenv("KOMB_DIST_WORDS", str(words))
    with _load(K, hug["nv"], hug["uv"]) as a:
        for n in (64 * words + 1, 1):
            _same(a.run_distances(hug["master"][:n]), _hug_want(hug, n, words))


@pytest.mark.parametrize("words", WORDS)
def test_rows_on_both_sides_of_the_short_long_split(K, monkeypatch, words):
    """Centres with 1, 7, 8, 9, 63, 64, 65, 128 and 129 neighbours among the vertices of a long path: rows of exactly one trip of a
    group, of the last length eight lanes share, of the first the whole wave walks, and of two and three trips of the wave."""
    monkeypatch.setenv("KOMB_DIST_WORDS", str(words))
    leaves = 300
    pairs = [(v, v + 1) for v in range(leaves - 1)]
    degrees = (1, 7, 8, 9, 63, 64, 65, 128, 129)
    for i, d in enumerate(degrees):
        pairs += [(leaves + i, (37 * i + 2 * j) % leaves) for j in range(d)]
    nv = leaves + len(degrees) + 2                                           # and two isolated vertices
    with _load(K, nv, pairs) as a:
        rows = _rows(a)
        assert [len(rows[leaves + i]) for i in range(len(degrees))] == list(degrees)
        cache = {}
        _check(a, None, rows, words, cache)
        _check(a, [leaves + 5, 0, leaves + 8, nv - 1, 150, leaves + 5], rows, words, cache)


def test_components_and_degenerate_graphs(K):
    with _load(K, 9, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (4, 6)]) as a:   # a path, a triangle, two isolated vertices
        (vert, per, pairs, info), _ = _check(a, [0, 4, 8, 2, 7, 5])
        assert per["n_reached"].tolist() == [4, 3, 1, 4, 1, 3] and per["ecc"].tolist() == [3, 1, 0, 2, 0, 1]
        assert vert["n_reached"].tolist() == [2, 2, 2, 2, 2, 2, 2, 1, 1] and vert["ecc"].tolist() == [2, 1, 2, 3, 1, 1, 1, 0, 0]
        _check(a)
        (vert, per, pairs, info), _ = _check(a, [])                            # no source: a valid run with nothing reached
        assert vert["ecc"].tolist() == [-1] * 9 and not vert["n_reached"].any() and vert["harmonic"].tolist() == [0.0] * 9
        assert pairs.tolist() == [0] and info["n_sources"] == 0 and info["n_level_steps"] == 0 and len(per["ecc"]) == 0
        (vert, per, pairs, info), _ = _check(a, [8, 7])                        # isolated sources only
        assert pairs.tolist() == [2] and info["depth_max"] == 0 and vert["ecc"].tolist() == [-1] * 7 + [0, 0]
    with _load(K, 1, np.zeros((0, 2))) as a:
        (vert, per, pairs, info), _ = _check(a)
        assert vert["n_reached"].tolist() == [1] and vert["ecc"].tolist() == [0] and pairs.tolist() == [1]
        _check(a, [0, 0, 0])
    with _load(K, 300, np.zeros((0, 2))) as a:                                 # no edges, more than one batch
        (vert, per, pairs, info), _ = _check(a)
        assert info["n_batches"] == 2 and info["depth_max"] == 0 and info["depth_min"] == 0 and pairs.tolist() == [300]


def test_a_long_path(K):
    n = 3000
    with _load(K, n, np.stack([np.arange(n - 1), np.arange(1, n)], 1)) as a:
        rows, cache = _rows(a), {}
        (vert, per, pairs, info), _ = _check(a, [0], rows, cache=cache)
        assert info["depth_max"] == n - 1 and info["n_level_steps"] == n and pairs.tolist() == [1] * n
        assert vert["ecc"].tolist() == list(range(n)) and vert["harmonic"][2] == 0.5
        (vert, per, pairs, info), _ = _check(a, [n - 1, 1500, 0], rows, cache=cache)
        assert per["ecc"].tolist() == [n - 1, 1500, n - 1] and info["depth_min"] == 1500


def test_identical_across_words_and_grid(K, hug, monkeypatch):
    results = []
    for words, grid in ((1, None), (2, None), (4, None), (1, 3), (4, 5)):
        monkeypatch.setenv("KOMB_DIST_WORDS", str(words))
        if grid is None:
            monkeypatch.delenv("KOMB_DIST_GRID", raising=False)
        else:
            monkeypatch.setenv("KOMB_DIST_GRID", str(grid))
        with _load(K, hug["nv"], hug["uv"]) as a:
            results.append(a.run_distances(hug["master"][:257]))
    for other in results[1:]:
        _equal(results[0], other)                                            # (batches and level steps follow the words)
    assert _equal(results[0], results[3]) and _equal(results[2], results[4])   # the grid changes nothing at all


def test_the_integers_of_betweenness_from_the_same_list(K, hug):
    with _load(K, hug["nv"], hug["uv"]) as a:
        sources = hug["master"][:130]
        a.distances_run(sources)
        a.betweenness_run(sources)
        ours, theirs = a.distances_fetch_sources(), a.betweenness_fetch_sources()
        for name in ("source", "n_reached", "sum_dist", "ecc"):
            assert np.array_equal(ours[name], theirs[name]), name
        assert a.distances_info()["depth_max"] == a.betweenness_info()["depth_max"]


def test_errors_and_state(K):
    ARG, STATE = K._lib.KOMB_ERR_ARG, K._lib.KOMB_ERR_STATE
    lib = K._lib.load()
    ptr = K._lib.ptr
    nv, pairs, sources, stored = R.load_fixture()
    with _load(K, nv, pairs) as a:
        for fn in (a.distances_fetch, a.distances_fetch_sources, a.distances_histogram, a.distances_info):
            assert _code(K, fn) == STATE                                       # before a run
        out = np.full(nv, -7.0)
        assert lib.komb_distances_fetch(a._ctx, None, None, None, ptr(out)) == STATE and (out == -7.0).all()
        hist = np.full(64, -7, np.int64)
        assert lib.komb_distances_histogram(a._ctx, ptr(hist), 64) == STATE and (hist == -7).all()
        first, _ = _check(a, [3, 1, 4, 1, 5])
        depth = first[3]["depth_max"]
        assert depth >= 2
        assert lib.komb_distances_histogram(a._ctx, ptr(hist), depth) == ARG and (hist == -7).all()   # one entry too few: nothing written
        assert lib.komb_distances_histogram(a._ctx, ptr(hist), 0) == ARG and lib.komb_distances_histogram(a._ctx, ptr(hist), -1) == ARG
        assert b"komb_distances_histogram" in lib.komb_last_error(a._ctx)
        assert lib.komb_distances_histogram(a._ctx, ptr(hist), depth + 1) == 0
        assert hist[:depth + 1].tolist() == first[2].tolist() and (hist[depth + 1:] == -7).all()
        src = np.asarray([0, nv, 1], np.int32)
        assert lib.komb_distances_run(a._ctx, 3, ptr(src)) == ARG              # an id out of range
        src = np.asarray([0, -1], np.int32)
        assert lib.komb_distances_run(a._ctx, 2, ptr(src)) == ARG
        assert lib.komb_distances_run(a._ctx, -1, ptr(src)) == ARG             # a negative count
        again = (a.distances_fetch(), a.distances_fetch_sources(), a.distances_histogram(), a.distances_info())
        assert _equal(again, first) and again[3] == first[3]                   # a refused run keeps the previous result
        assert lib.komb_distances_run(a._ctx, -5, None) == 0                   # NULL: every vertex, the count is ignored
        assert a.distances_info()["flags"] == K._lib.KOMB_DISTANCES_ALL and a.distances_info()["n_sources"] == nv
        assert lib.komb_distances_fetch(a._ctx, None, None, None, None) == 0   # NULL outputs are allowed
        assert lib.komb_distances_fetch_sources(a._ctx, None, None, None, None) == 0
        assert lib.komb_distances_info(a._ctx, *([None] * 9)) == 0
        assert lib.komb_distances_histogram(a._ctx, None, 1 << 40) == 0
        ecc = np.full(nv, -7, np.int32)
        assert lib.komb_distances_fetch(a._ctx, None, None, ptr(ecc), None) == 0 and (ecc >= 0).all()
        a.from_edges(3, [[0, 1], [1, 2]])                                      # a graph load drops it
        assert _code(K, a.distances_info) == STATE and _code(K, a.distances_fetch) == STATE and _code(K, a.distances_histogram) == STATE
        vert = a.run_distances()[0]
        assert vert["ecc"].tolist() == [2, 1, 2] and vert["harmonic"].tolist() == [1.5, 2.0, 1.5]


def test_the_other_analyses_and_this_one_leave_each_other_alone(K, hug):
    with _load(K, hug["nv"], hug["uv"]) as a:
        want = _hug_want(hug, 65, DEFAULT_WORDS)
        a.distances_run(hug["master"][:65])
        deg, core = a.run_core()
        eu, ev, tr, sup = a.run_truss(with_support=True)
        bc = a.run_betweenness(hug["master"][:3])
        stats = a.stats()
        held = (a.distances_fetch(), a.distances_fetch_sources(), a.distances_histogram(), a.distances_info())
        _same(held, want)                                                      # none of them changed it
        a.distances_run(hug["master"][:1])
        assert a.stats() == stats                                              # no komb_stats field moves
        deg2, core2 = a.core_fetch()
        eu2, ev2, tr2, sup2 = a.truss_fetch(with_support=True)
        for x, y in ((deg, deg2), (core, core2), (eu, eu2), (ev, ev2), (tr, tr2), (sup, sup2)):
            assert np.array_equal(x, y)
        assert np.array_equal(R.bits(a.betweenness_fetch()), R.bits(bc[0])) and a.betweenness_info() == bc[2]
        for name in bc[1]:
            assert np.array_equal(a.betweenness_fetch_sources()[name], bc[1][name])
        eu3, ev3, tr3, sup3 = a.run_truss(with_support=True)                   # the resident k-truss preparation still serves
        assert np.array_equal(tr, tr3) and np.array_equal(sup, sup3)
        _same((a.distances_fetch(), a.distances_fetch_sources(), a.distances_histogram(), a.distances_info()),
              _hug_want(hug, 1, DEFAULT_WORDS))


@pytest.mark.parametrize("word", ["0xFFFFFFFF", "0x00000001", "0x7FF00000"])
def test_poisoned_memory_on_a_reused_context(K, monkeypatch, word, hug):
    """Every word of the masks, the partial sums and the accumulators must be written before it is read.  0x7FF00000 repeated is
    a NaN as a double; 0xFFFFFFFF is a mask that has seen everything."""
    nv, pairs, sources, stored = R.load_fixture()
    monkeypatch.setenv("KOMB_POISON", word)
    with K.KombAccel() as a:
        for turn in range(2):
            a.from_edges(nv, pairs)
            assert np.array_equal(R.bits(a.run_distances(sources)[0]["harmonic"]), stored)
            _check(a, [48, 0, 17, 17, 3])
            a.from_edges(hug["nv"], np.asarray(hug["uv"], dtype=np.int64).reshape(-1, 2))
            for n in (65, 257):
                _same(a.run_distances(hug["master"][:n]), _hug_want(hug, n, DEFAULT_WORDS))


def test_every_allocation_request_fails_once(K):
    NOMEM = K._lib.KOMB_ERR_NOMEM
    nv, pairs, sources, stored = R.load_fixture()
    with _load(K, nv, pairs) as a:
        first, _ = _check(a, [9, 2, 30])
        in_use = a.alloc_info()["pool_blocks_in_use"]
        a.set_option("ALLOC_FAIL_AT", "0")                                     # only count
        a.distances_run(sources)
        n = a.alloc_info()["requests"]
        assert n >= 13                                                         # four result arrays, the three masks, the partial sums, ...
        assert np.array_equal(R.bits(a.distances_fetch()["harmonic"]), stored)
        a.distances_run([9, 2, 30])
        held = a.distances_info()
        assert {k: held[k] for k in INFO} == {k: first[3][k] for k in INFO}
        for i in range(1, n + 1):
            a.set_option("ALLOC_FAIL_AT", str(i))
            assert _code(K, lambda: a.distances_run(sources)) == NOMEM, i
            info = a.alloc_info()
            assert info["fired"] == 1 and info["pool_blocks_in_use"] == in_use, i
            assert a.distances_info() == held
            assert _equal((a.distances_fetch(), a.distances_fetch_sources(), a.distances_histogram(), held), first)
        a.set_option("ALLOC_FAIL_AT", str(n + 1))                              # one past the last: the run succeeds
        a.distances_run(sources)
        assert a.alloc_info()["fired"] == 0
        a.set_option("ALLOC_FAIL_AT", None)
        assert np.array_equal(R.bits(a.run_distances(sources)[0]["harmonic"]), stored)
        assert a.alloc_info()["pool_blocks_in_use"] == in_use
