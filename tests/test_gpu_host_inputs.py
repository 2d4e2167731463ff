"""GPU tests of the entry points that take arbitrary host arrays from the caller -- komb_corea_ranks / komb_corea_scores,
komb_graph_from_csr / komb_graph_from_edges, komb_densest_block (the suspiciousness array) -- on inputs that no graph
of the suite produces: CoreA keys of 2^31 and more, tie patterns that are not power laws, an n past one turn of the
grid-stride loops, every defect the CSR validator is there to refuse, vertex ids outside [0, nv) anywhere in a long pair
list, and priorities that all tie.  Results are compared bit for bit with the oracle (and, for CoreA, with the numpy
restatement of tests/corea_inputs.py)."""
import numpy as np
import pytest

import corea_inputs as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


# ---------------------------------------------------------------- CoreA
@pytest.fixture(scope="module")
def corea_ctx(K):
    """One context for every CoreA case, no graph loaded: CoreA needs none."""
    with K.KombAccel() as a:
        yield a


_WANT = {}


def _corea_want(O, name):
    """(rank_deg, rank_key, score) of the oracle, checked against the numpy restatement; computed once per case."""
    if name not in _WANT:
        _, deg, core = C.case(name)
        key = C.keys_of(deg, core)
        rd, rk = O.fractional_rank_fast(deg.astype(np.int64)), O.fractional_rank_fast(key)
        assert np.array_equal(rd, C.np_fractional_rank(deg)) and np.array_equal(rk, C.np_fractional_rank(key))
        score = O.corea_scores(deg, core)
        for x in (rd, rk, score):
            x.setflags(write=False)
        _WANT[name] = (rd, rk, score)
    return _WANT[name]


def _check_corea(a, O, name):
    _, deg, core = C.case(name)
    want_rd, want_rk, want_score = _corea_want(O, name)
    for turn in range(2):                                # the second call on the same case gives the same result
        rd, rk = a.fractional_ranks(deg, core)
        assert not np.isnan(rd).any() and not np.isnan(rk).any(), (name, turn)
        assert np.array_equal(rd, want_rd), (name, turn)
        assert np.array_equal(rk, want_rk), (name, turn)
        assert a.stats()["ms_corea"] > 0, (name, turn)
        score = a.get_anomaly_score(deg, core)
        assert not np.isnan(score).any(), (name, turn)
        assert np.array_equal(score, want_score), (name, turn)
        assert a.stats()["ms_corea"] > 0, (name, turn)


@pytest.mark.parametrize("name", C.case_names())
def test_corea_host_inputs(corea_ctx, O, name):
    _check_corea(corea_ctx, O, name)


def test_corea_beside_a_resident_graph(K, O):
    """CoreA borrows its scratch from the context's pool: with an n below and an n above the resident graph's nv it must
    neither be disturbed by the graph's buffers nor disturb them."""
    nv = 20000
    uv = K.gen_hug_edges(nv, 50000, 2.6, 4)
    small = next(n for n in C.case_names() if n.startswith("zeros-n4097-"))
    large = next(n for n in C.case_names() if n.startswith("wide-n%d-" % C.BIG))
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        csr = a.get_csr()
        deg, core = a.run_core()
        truss = a.run_truss()
        o_rowptr, o_col = O.simplify(nv, uv)
        assert np.array_equal(core, O.coreness(o_rowptr, o_col)) and np.array_equal(truss[2], O.trussness(o_rowptr, o_col))
        assert len(C.case(small)[1]) < nv < len(C.case(large)[1])
        for name in (large, small, large):
            _check_corea(a, O, name)
            got = a.core_fetch()
            assert np.array_equal(got[0], deg) and np.array_equal(got[1], core), name
            assert all(np.array_equal(x, y) for x, y in zip(a.truss_fetch(), truss)), name
            assert all(np.array_equal(x, y) for x, y in zip(a.get_csr(), csr)), name


def test_corea_refusals(corea_ctx, K, O):
    a = corea_ctx
    n = 1000
    rng = np.random.default_rng(5)
    deg = rng.integers(0, 50, n).astype(np.int32)
    core = rng.integers(0, 2**31, n).astype(np.int32)
    want = O.corea_scores(deg, core)
    for which in ("degree", "coreness"):
        for at in (0, n // 2, n - 1):
            d, c = deg.copy(), core.copy()
            (d if which == "degree" else c)[at] = -1
            for call in (a.fractional_ranks, a.get_anomaly_score):
                with pytest.raises(K.KombError) as e:
                    call(d, c)
                assert e.value.code == K._lib.KOMB_ERR_ARG, (which, at)
                assert str(e.value).endswith(" at %d" % at), (which, at, str(e.value))
                assert np.array_equal(a.get_anomaly_score(deg, core), want), (which, at)   # the next valid call
    rd, rk = a.fractional_ranks([], [])
    assert rd.shape == (0,) and rk.shape == (0,) and a.get_anomaly_score([], []).shape == (0,)
    assert a.stats()["ms_corea"] == 0


# ---------------------------------------------------------------- komb_graph_from_csr: the rejection matrix
_CSR_NV = 300
_CSR_ROWS = (0, _CSR_NV // 2, _CSR_NV - 1)               # first (the one longer than 256), middle and last row


@pytest.fixture(scope="module")
def csr_base(O):
    """A valid CSR: a random graph of 300 vertices, vertex 0 adjacent to 270 of them, every row of _CSR_ROWS with at
    least three neighbours."""
    nv = _CSR_NV
    rng = np.random.default_rng(23)
    uv = [rng.integers(0, nv, (1200, 2)), np.stack([np.zeros(270, np.int64), np.arange(1, 271)], axis=1)]
    for u in _CSR_ROWS[1:]:
        uv.append(np.array([[u, u - 3], [u, u - 2], [u, u - 1]]))
    rowptr, col = O.simplify(nv, np.concatenate(uv).astype(np.int64))
    assert rowptr[1] - rowptr[0] > 256 and all(rowptr[u + 1] - rowptr[u] >= 3 for u in _CSR_ROWS)
    core = O.coreness(rowptr, col)
    for x in (rowptr, col, core):
        x.setflags(write=False)
    return rowptr, col, core


def _swap(u):
    def f(rowptr, col):
        j = int(rowptr[u]) + (int(rowptr[u + 1]) - int(rowptr[u])) // 2
        col[j - 1], col[j] = col[j], col[j - 1]
    return f


def _duplicate(rowptr, col):
    j = int(rowptr[_CSR_NV // 2])
    col[j + 1] = col[j]


def _self_loop(rowptr, col):
    # where u itself would stand in its row, so that the row stays sorted: only the loop is wrong (and the lost reverse slot)
    u = _CSR_NV // 2
    b, e = int(rowptr[u]), int(rowptr[u + 1])
    col[min(b + int(np.searchsorted(col[b:e], u)), e - 1)] = u


def _set_col(row, last, value):
    def f(rowptr, col):
        col[int(rowptr[row + 1]) - 1 if last else int(rowptr[row])] = value      # the row stays sorted
    return f


def _missing_reverse(rowptr, col):
    # a neighbour replaced by a non-neighbour between its two row mates: simple and sorted, but not symmetric
    for u in range(1, _CSR_NV):
        b, e = int(rowptr[u]), int(rowptr[u + 1])
        for j in range(b + 1, e - 1):
            for w in range(int(col[j - 1]) + 1, int(col[j + 1])):
                if w != u and w != col[j]:
                    col[j] = w
                    return
    raise AssertionError("no slot to break")


def _rowptr(f):
    def g(rowptr, col):
        f(rowptr)
    return g


def _non_monotone(rowptr):
    i = _CSR_NV // 2
    assert rowptr[i + 1] > rowptr[i]
    rowptr[i], rowptr[i + 1] = rowptr[i + 1], rowptr[i]


def _first_is_one(rowptr):
    rowptr[0] = 1


def _odd_total(rowptr):
    rowptr[_CSR_NV] -= 1


def _above_total(value):
    def f(rowptr):
        rowptr[_CSR_NV // 2] = rowptr[_CSR_NV] + value
    return f


_CSR_DEFECTS = {
    "swap_first_row": _swap(_CSR_ROWS[0]), "swap_middle_row": _swap(_CSR_ROWS[1]), "swap_last_row": _swap(_CSR_ROWS[2]),
    "duplicate": _duplicate, "self_loop": _self_loop,
    "col_minus_one": _set_col(_CSR_NV // 2, False, -1), "col_nv": _set_col(_CSR_NV // 2, True, _CSR_NV),
    "col_int32_max": _set_col(_CSR_NV // 2, True, 2**31 - 1),
    "col_minus_one_first_slot": _set_col(0, False, -1), "col_nv_last_slot": _set_col(_CSR_NV - 1, True, _CSR_NV),
    "missing_reverse": _missing_reverse,
    "rowptr_non_monotone": _rowptr(_non_monotone), "rowptr_first_is_one": _rowptr(_first_is_one),
    "rowptr_odd_total": _rowptr(_odd_total),
    "rowptr_middle_above_total": _rowptr(_above_total(1)), "rowptr_middle_above_2_32": _rowptr(_above_total(2**32)),
}


def _refused_then_good(K, a, load_bad, load_good, want_core):
    """The bad load is refused with KOMB_ERR_ARG and leaves no graph; the good one on the same context then works.  A bad
    load that is accepted fails the test inside the `with`: nothing is computed on a graph that should not exist."""
    with pytest.raises(K.KombError) as e:
        load_bad()
    assert e.value.code == K._lib.KOMB_ERR_ARG, str(e.value)
    with pytest.raises(K.KombError) as e:
        a.core_run()
    assert e.value.code == K._lib.KOMB_ERR_STATE and "no graph loaded" in str(e.value)
    load_good()
    assert np.array_equal(a.run_core()[1], want_core)


@pytest.mark.parametrize("defect", list(_CSR_DEFECTS))
def test_from_csr_rejects(K, csr_base, defect):
    rowptr, col, core = csr_base
    bad_rowptr, bad_col = rowptr.copy(), col.copy()
    _CSR_DEFECTS[defect](bad_rowptr, bad_col)
    assert not (np.array_equal(bad_rowptr, rowptr) and np.array_equal(bad_col, col))
    with K.KombAccel() as a:                             # a fresh context per defect
        _refused_then_good(K, a, lambda: a.from_csr(bad_rowptr, bad_col), lambda: a.from_csr(rowptr, col), core)
        got = a.get_csr()
        assert np.array_equal(got[0], rowptr) and np.array_equal(got[1], col)


# ---------------------------------------------------------------- komb_graph_from_edges
_EDGES_NV, _EDGES_N = 1000, 1200000                      # more pairs than one turn of 4096 blocks x 256 threads


@pytest.fixture(scope="module")
def edges_base(O):
    rng = np.random.default_rng(29)
    uv = rng.integers(0, _EDGES_NV, (_EDGES_N, 2)).astype(np.int64)
    rowptr, col = O.simplify(_EDGES_NV, uv)
    core = O.coreness(rowptr, col)
    for x in (uv, core):
        x.setflags(write=False)
    return uv, core


@pytest.mark.parametrize("at", [0, _EDGES_N // 2 + 1, _EDGES_N - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("bad", [(-1, 5), (5, _EDGES_NV), (2**40, 5)], ids=["u_minus_one", "v_is_nv", "u_2_40"])
def test_from_edges_rejects(K, edges_base, bad, at):
    uv, core = edges_base
    bad_uv = uv.copy()
    bad_uv[at] = bad
    with K.KombAccel() as a:
        _refused_then_good(K, a, lambda: a.from_edges(_EDGES_NV, bad_uv), lambda: a.from_edges(_EDGES_NV, uv), core)


def _accepted_edge_inputs():
    loops = np.repeat(np.arange(_EDGES_NV, dtype=np.int64), 2).reshape(-1, 2)
    one = np.tile(np.array([[3, 7], [7, 3]], np.int64), (_EDGES_N // 2, 1))
    nv = 1024
    return {"all_loops": (_EDGES_NV, np.tile(loops, (3, 1))), "one_edge_repeated": (_EDGES_NV, one),
            "power_of_two_last_vertex": (nv, np.array([[nv - 2, nv - 1], [nv - 1, nv - 1]], np.int64))}


@pytest.mark.parametrize("which", ["all_loops", "one_edge_repeated", "power_of_two_last_vertex"])
def test_from_edges_accepts(K, O, which):
    nv, uv = _accepted_edge_inputs()[which]
    o_rowptr, o_col = O.simplify(nv, uv)
    assert len(o_col) == {"all_loops": 0, "one_edge_repeated": 2, "power_of_two_last_vertex": 2}[which]
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        assert (a.nv, a.ne) == (nv, len(o_col) // 2)
        rowptr, col = a.get_csr()
        assert np.array_equal(rowptr, o_rowptr) and np.array_equal(col, o_col)
        deg, core = a.run_core()
        assert np.array_equal(deg, O.degree(o_rowptr)) and np.array_equal(core, O.coreness(o_rowptr, o_col))


# ---------------------------------------------------------------- komb_densest_block
def _star(leaves):
    return leaves + 1, np.stack([np.zeros(leaves, np.int64), np.arange(1, leaves + 1)], axis=1)


def _densest_graphs():
    rng = np.random.default_rng(31)
    empty = np.zeros((0, 2), np.int64)
    return {"one_vertex": (1, empty), "five_isolated": (5, empty), "one_edge": (2, np.array([[0, 1]], np.int64)),
            "path_50": (50, np.stack([np.arange(49), np.arange(1, 50)], axis=1).astype(np.int64)),
            "star_lds_4096": _star(4095), "star_global_4097": _star(4096),
            "random_300": (300, rng.integers(0, 300, (1500, 2)).astype(np.int64))}


@pytest.mark.parametrize("which", ["one_vertex", "five_isolated", "one_edge", "path_50", "star_lds_4096", "star_global_4097",
                                   "random_300"])
def test_densest_block_tied_priorities(K, O, which):
    """Equal priorities are what make the removal order depend on the heaps' layout: suspiciousness arrays that tie every
    node (absent, 0.0, 0.5), tie many (small integers) or never change a comparison of their own (i * 1e-300)."""
    nv, uv = _densest_graphs()[which]
    assert (which == "star_lds_4096") == (nv == 4096) and (which == "star_global_4097") == (nv == 4097)
    rng = np.random.default_rng(37)
    susps = {"none": None, "zeros": np.zeros(nv), "halves": np.full(nv, 0.5),
             "small_integers": rng.integers(0, 4, nv).astype(np.float64), "tiny": np.arange(nv) * 1e-300}
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        rowptr, col = a.get_csr()
        for tag, susp in susps.items():
            got, want = a.densest_block(susp), O.run_merge(rowptr, col, susp)
            assert len(got[0]) == 2 * nv and sorted(got[0].tolist()) == sorted(list(range(nv)) * 2), (which, tag)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (which, tag)
            assert got[2:] == want[2:], (which, tag)


def test_densest_block_limits(K):
    nv = 2**17 + 1                                       # one above the limit (the limit itself is seconds of one lane's time)
    with K.KombAccel() as a:
        with pytest.raises(K.KombError) as e:            # no graph loaded
            a.densest_block()
        assert e.value.code == K._lib.KOMB_ERR_STATE
        a.from_edges(nv, np.zeros((0, 2), np.int64))
        for susp in (None, np.zeros(nv)):
            with pytest.raises(K.KombError) as e:
                a.densest_block(susp)
            assert e.value.code == K._lib.KOMB_ERR_LIMIT
        assert (a.nv, a.ne) == (nv, 0)                   # the graph stays loaded
        deg, core = a.run_core()
        assert len(deg) == nv and not deg.any() and not core.any()
