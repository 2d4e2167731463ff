"""The GPU path on memory nobody cleared: every device allocation filled with a poison word (option POISON), and one
context driven through a long mixed sequence so that its pooled blocks hold another graph's or another run's leftovers.

Every other GPU test starts from a fresh hipMalloc (zero pages in practice, not by contract) or from a pool block the same
graph's previous run left behind, so a counter, cursor, mark or slice of results that someone forgets to clear passes as
long as 0 or the previous value is the right answer.  Here it cannot: with POISON the library fills every block it hands
out -- new or reused, pooled or not -- with the word before it is returned (DESIGN.md section 8.1 lists what initialises
each buffer), and the Python plumbing fills every output array with a sentinel (komb_amd/api.py: SENTINEL_I32, NaN), so an
entry nobody writes fails at once.  Patterns: 0xFFFFFFFF (-1 / UINT_MAX: counters assumed zero, sign tests), 0x7FFFFFFF
(huge: a min-reduction started from garbage), 0x00000001 (equal to sweep / round number 1), 0x80000000 (INT_MIN).

Every comparison is bit for bit against the oracle (oracle/), computed once per graph.  The whole existing GPU suite runs
on poisoned memory too: `KOMB_POISON=0xFFFFFFFF python -m pytest tests -m gpu` (the plumbing forwards KOMB_POISON like any
option, before the graph load as well).  tests/manual/slice_zero_negative_control.sh shows that the slice test below fails
on a build that skips the clear of the results outside a rank's slice."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PATTERNS = ["0xFFFFFFFF", "0x7FFFFFFF", "0x00000001", "0x80000000"]

# engine configurations (KOMB_* switches, forwarded as per-context options); "sharded_w1" calls komb_core_run_sharded /
# komb_truss_run_sharded with world = 1 instead of the plain entry points
ENGINES = {
    "default": {},
    "finish_none": {"FINISH": "none"},
    "local_whole": {"FINISH": "local", "LOCAL_LIMIT": "4000000000"},
    "local_1500": {"FINISH": "local", "LOCAL_LIMIT": "1500"},
    "lds": {"FINISH": "lds", "TAIL": "2000", "CORE_TAIL": "300"},
    "two_pass": {"INDEX": "two_pass"},
    "rec_cap": {"REC_CAP": "2000"},             # the record stream runs out: the build falls back to two-pass
    "no_first_queue": {"NO_FIRST_QUEUE": "1"},
    "shard_engine": {"SHARD_ENGINE": "1"},
    "sharded_w1": {},
}
_SWITCHES = ("FINISH", "LOCAL_LIMIT", "LOCAL_ITEMS", "LOCAL_DENSITY", "TAIL", "CORE_TAIL", "INDEX", "TWO_PASS", "REC_CAP",
             "OWN_DENSE_CAP", "NO_OWN_DENSE", "NO_FIRST_QUEUE", "SHARD_ENGINE", "SHARD_PEEL", "RETIRE_EVERY", "POISON")
MERGE_MAX_NV = 6000                             # densest block (a sequential peel on one lane): the small graphs only


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _set_env(monkeypatch, poison, engine):
    for k in _SWITCHES:
        monkeypatch.delenv("KOMB_" + k, raising=False)
    if poison is not None:
        monkeypatch.setenv("KOMB_POISON", poison)
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv("KOMB_" + k, v)


def _book(k):
    pages = np.arange(2, k + 2)
    return np.concatenate([[[0, 1]], np.stack([np.zeros(k, int), pages], 1), np.stack([np.ones(k, int), pages], 1),
                           np.stack(np.triu_indices(12, 1), axis=1) + 2]).astype(np.int64)


def _graphs(K):
    """(name, nv, raw pairs): the families of the local-finish and threshold tests, at sizes that keep the module short."""
    rng = np.random.default_rng(77)
    g = [("gnm3000", 3000, rng.integers(0, 3000, (90000, 2)).astype(np.int64)),
         ("hug30k_a22", 30000, np.asarray(K.gen_hug_edges(30000, 90000, 2.2, 9)).reshape(-1, 2)),
         ("hug300k_a26", 300000, np.asarray(K.gen_hug_edges(300000, 740000, 2.6, 13)).reshape(-1, 2)),
         ("K300", 300, np.stack(np.triu_indices(300, 1), axis=1).astype(np.int64))]
    n = 4000
    path = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    g.append(("strip", n, np.concatenate([path, np.stack([np.arange(n - 2), np.arange(2, n)], axis=1)]).astype(np.int64)))
    star = np.stack([np.zeros(150000, np.int64), np.arange(1, 150001)], axis=1)
    ring = np.stack([np.arange(1, 2000), np.arange(2, 2001)], axis=1)
    g.append(("hub", 150001, np.concatenate([star, ring, [[1, 2000]]]).astype(np.int64)))
    g.append(("book257", 259, _book(257)))
    g.append(("book5000", 5002, _book(5000)))
    g.append(("empty", 0, np.zeros((0, 2), np.int64)))
    g.append(("loops", 10, np.stack([np.arange(10), np.arange(10)], axis=1).astype(np.int64)))
    g.append(("edge", 2, np.array([[0, 1]], np.int64)))
    return g


class _Want:
    """Everything the oracle says about one graph (computed once, kept for the module)."""

    def __init__(self, O, name, nv, uv):
        self.name, self.nv, self.uv = name, nv, uv
        self.rowptr, self.col = O.simplify(nv, uv)
        self.deg = O.degree(self.rowptr)
        self.core = O.coreness(self.rowptr, self.col)
        self.eu, self.ev = O.edge_list(self.rowptr, self.col)
        self.sup, self.tri = O.support(self.rowptr, self.col)
        self.tr = O.trussness(self.rowptr, self.col)
        self.rd = O.fractional_rank_fast(self.deg.astype(np.int64))
        self.rk = O.fractional_rank_fast(self.core.astype(np.int64) * nv + self.deg)
        self.score = O.corea_scores(self.deg, self.core)
        kmax = int(self.core.max()) if nv else 0
        self.masks = [("maxcore", (self.core == kmax).astype(np.uint8)),
                      ("random", (np.random.default_rng(nv + 5).random(nv) < 0.6).astype(np.uint8))]
        self.induced = {}
        for tag, m in self.masks:
            srp, scol, _ = O.induced_subgraph(self.rowptr, self.col, m)
            self.induced[tag] = O.trussness_induced(self.rowptr, self.col, m) + (O.support(srp, scol)[0],)
        self.merge = O.run_merge(self.rowptr, self.col) if 0 < nv <= MERGE_MAX_NV else None


@pytest.fixture(scope="module")
def wants(K, O):
    return [_Want(O, name, nv, uv) for name, nv, uv in _graphs(K)]


def _core(a, engine):
    if engine == "sharded_w1":
        a._sync_env_options()
        a._check(a._lib.komb_core_run_sharded(a._ctx, 0, 1, None, None))
        return a.core_fetch()
    return a.run_core()


def _truss(a, engine, vmask=None):
    if engine == "sharded_w1":
        from komb_amd._lib import ptr
        vm = None if vmask is None else np.ascontiguousarray(vmask, dtype=np.uint8)
        a._sync_env_options()
        a._check(a._lib.komb_truss_run_sharded(a._ctx, ptr(vm), 0, 1, None, None))
        return a.truss_fetch(with_support=True)
    return a.run_truss(vmask, with_support=True)


def _eq(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y))


def _check_whole(a, w, engine, tag):
    eu, ev, tr, sup = _truss(a, engine)
    assert _eq(eu, w.eu) and _eq(ev, w.ev), (tag, "edge list")
    assert _eq(sup, w.sup), (tag, "support")
    assert _eq(tr, w.tr), (tag, "trussness")
    assert a.stats()["triangles"] == w.tri, (tag, "triangles")


def _check_slices(a, w, world, tag):
    """komb_truss_run_slice: the rank's slice of the canonical edges equals the oracle, everything else is 0 (written by the
    library: the output arrays start as sentinels), and the slices add up to the whole result."""
    ne = len(w.tr)
    tot_tr = np.zeros(ne, np.int64); tot_sup = np.zeros(ne, np.int64)
    for rank in range(world):
        a.truss_run_slice(rank, world)
        eu, ev, tr, sup = a.truss_fetch(with_support=True)
        lo, hi = ne * rank // world, ne * (rank + 1) // world
        assert _eq(eu, w.eu) and _eq(ev, w.ev), (tag, rank, "edge list")
        assert _eq(tr[lo:hi], w.tr[lo:hi]) and _eq(sup[lo:hi], w.sup[lo:hi]), (tag, rank, "inside the slice")
        assert not tr[:lo].any() and not tr[hi:].any(), (tag, rank, "trussness outside the slice")
        assert not sup[:lo].any() and not sup[hi:].any(), (tag, rank, "support outside the slice")
        tot_tr += tr; tot_sup += sup
    assert _eq(tot_tr, w.tr) and _eq(tot_sup, w.sup), (tag, "sum of the slices")


def _assert_engine_reached(engine, runs):
    """The path a configuration names was taken (komb_stats of the whole-graph runs of every graph with edges: (nv, ne,
    k-core stats, k-truss stats)), so that its poisoned runs test that path and not the default one.  NO_FIRST_QUEUE has no
    statistic of its own."""
    flags = lambda st: st["engine_flags"]
    if engine in ("default", "local_whole"):
        assert any(c["core_local_units"] > 0 for _, _, c, _ in runs), (engine, "k-core local finish")
        assert any(t["truss_local_units"] > 0 for _, _, _, t in runs), (engine, "k-truss local finish")
    elif engine == "local_1500":
        # a hand-over in mid-peel: a graph larger than the limit gave the local finish at most 1500 units
        assert any(nv > 1500 and 0 < c["core_local_units"] <= 1500 for nv, _, c, _ in runs), (engine, "k-core hand-over")
        assert any(ne > 1500 and 0 < t["truss_local_units"] <= 1500 for _, ne, _, t in runs), (engine, "k-truss hand-over")
    elif engine == "finish_none":
        for _, _, c, t in runs:
            assert c["core_local_units"] == 0 and t["truss_local_units"] == 0 and t["truss_tail_runs"] == 0, engine
            assert flags(c) & 3 == 0 and flags(t) & 3 == 0, engine
    elif engine == "lds":
        assert any(t["truss_tail_runs"] > 0 for _, _, _, t in runs), (engine, "k-truss LDS tail")
        for _, _, c, t in runs:
            assert c["core_local_units"] == 0 and t["truss_local_units"] == 0 and flags(c) & 2, engine
    elif engine == "two_pass":
        for _, _, _, t in runs:
            assert t["index_layout"] == 2 and flags(t) & 8, engine
    elif engine == "rec_cap":
        assert any(t["index_layout"] == 2 and flags(t) & 8 for _, _, _, t in runs), (engine, "stream ran out: two-pass")
    elif engine == "shard_engine":
        for _, _, c, t in runs:
            assert flags(c) & 4 and flags(t) & 4, engine
    elif engine == "sharded_w1":
        for _, _, c, _ in runs:
            assert flags(c) & 4, engine                  # (komb_core_run_sharded: the sharded k-core engine with one rank)


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_paths_on_poisoned_memory(K, O, wants, monkeypatch, pattern, engine):
    """A fresh context with POISON set before the graph load, per graph: CSR, degree, coreness, supports, trussness and the
    triangle count, the subgraphs of a max-core and a random vertex mask, the CoreA ranks and scores, the densest block;
    and the statistics show that the configuration's engine ran."""
    _set_env(monkeypatch, pattern, engine)
    runs = []
    for w in wants:
        tag = (w.name, pattern, engine)
        with K.KombAccel() as a:
            a.from_edges(w.nv, w.uv)
            rowptr, col = a.get_csr()
            assert _eq(rowptr, w.rowptr) and _eq(col, w.col), (tag, "CSR")
            deg, core = _core(a, engine)
            assert _eq(deg, w.deg) and _eq(core, w.core), (tag, "degree / coreness")
            core_st = a.stats()
            _check_whole(a, w, engine, tag)
            if len(w.tr):
                runs.append((w.nv, len(w.tr), core_st, a.stats()))
            for mtag, m in w.masks:
                eu, ev, tr, sup = _truss(a, engine, m)
                weu, wev, wtr, wsup = w.induced[mtag]
                assert _eq(eu, weu) and _eq(ev, wev) and _eq(tr, wtr) and _eq(sup, wsup), (tag, mtag)
            rd, rk = a.fractional_ranks(deg, core)
            assert _eq(rd, w.rd) and _eq(rk, w.rk), (tag, "CoreA ranks")
            assert _eq(a.get_anomaly_score(deg, core), w.score), (tag, "CoreA scores")
            if w.merge is not None:
                order, side, nb, dens = a.densest_block()
                assert _eq(order, w.merge[0]) and _eq(side, w.merge[1]) and (nb, dens) == w.merge[2:], (tag, "densest block")
    _assert_engine_reached(engine, runs)


@pytest.mark.parametrize("engine", [e for e in ENGINES if e != "sharded_w1"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_result_slices_on_poisoned_memory(K, O, wants, monkeypatch, pattern, engine):
    """world = 3 slices of every graph on poisoned memory: the zeros outside a rank's slice are the library's, not the
    pool's (tests/manual/slice_zero_negative_control.sh: a build without that clear fails here)."""
    _set_env(monkeypatch, pattern, engine)
    for w in wants:
        if not len(w.tr):
            continue
        with K.KombAccel() as a:
            a.from_edges(w.nv, w.uv)
            _check_slices(a, w, 3, (w.name, pattern, engine))


def _fetch_varied(a, rng):
    """The result of the last k-truss run through komb_truss_fetch / _fetch_support in a varied order, some outputs NULL."""
    from komb_amd.api import _out_i32
    from komb_amd._lib import ptr
    n = ctypes.c_int64()
    a._check(a._lib.komb_truss_count(a._ctx, ctypes.byref(n)))
    eu, ev, tr, sup = (_out_i32(n.value) for _ in range(4))
    order = int(rng.integers(0, 3))
    if order == 0:                                  # supports first, endpoints later, trussness last
        a._check(a._lib.komb_truss_fetch_support(a._ctx, ptr(sup)))
        a.truss_fetch_into(eu, ev, None)
        a.truss_fetch_into(None, None, tr)
    elif order == 1:                                # trussness alone, then one endpoint at a time, supports last
        a.truss_fetch_into(None, None, tr)
        a.truss_fetch_into(None, ev, None)
        a.truss_fetch_into(eu, None, None)
        a._check(a._lib.komb_truss_fetch_support(a._ctx, ptr(sup)))
    else:
        a.truss_fetch_into(eu, ev, tr)
        a._check(a._lib.komb_truss_fetch_support(a._ctx, ptr(sup)))
    return eu, ev, tr, sup


@pytest.mark.parametrize("poisoned", [False, True], ids=["stale", "poisoned"])
def test_context_reuse_sequence(K, O, wants, monkeypatch, poisoned):
    """One context, a seeded random sequence of about 60 operations over graphs of very different sizes (tiny, 1k, 300k,
    tiny, 50k): graph loads, k-core and k-truss runs with and without a vertex mask, slices, prepare / unprepare, fetches in
    varied orders with some outputs NULL, CoreA, engine switches and -- poisoned -- a new poison word between steps.  A
    reused pool block is then another graph's or another run's leftover.  Every result against the oracle."""
    _set_env(monkeypatch, PATTERNS[0] if poisoned else None, "default")
    by_name = {w.name: w for w in wants}
    rng0 = np.random.default_rng(3)
    extra = {
        "g1k": _Want(O, "g1k", 1000, rng0.integers(0, 1000, (8000, 2)).astype(np.int64)),
        "hug50k": _Want(O, "hug50k", 50000, np.asarray(K.gen_hug_edges(50000, 150000, 2.4, 6)).reshape(-1, 2)),
    }
    plan = [by_name["book257"], extra["g1k"], by_name["hug300k_a26"], by_name["edge"], by_name["K300"], extra["hug50k"]]
    switches = [("FINISH", ["none", "lds", "local", None]), ("INDEX", ["two_pass", None]), ("LOCAL_LIMIT", ["1500", None]),
                ("NO_FIRST_QUEUE", ["1", None])]
    rng = np.random.default_rng(2024)
    n_ops = 0
    with K.KombAccel() as a:
        for w in plan:
            a.from_edges(w.nv, w.uv)
            n_ops += 1
            have_truss = None                       # what the last k-truss run should have left: (eu, ev, tr, sup, lo, hi)
            for step in range(10):
                op = rng.choice(["core", "truss", "vmask", "slice", "prepare", "unprepare", "fetch", "corea", "switch", "poison"])
                tag = (w.name, step, op)
                n_ops += 1
                if op == "core":
                    deg, core = a.run_core()
                    assert _eq(deg, w.deg) and _eq(core, w.core), tag
                elif op == "truss":
                    a.truss_run()
                    have_truss = (w.eu, w.ev, w.tr, w.sup, 0, len(w.tr))
                elif op == "vmask":
                    mtag, m = w.masks[int(rng.integers(0, 2))]
                    a.truss_run(m)
                    weu, wev, wtr, wsup = w.induced[mtag]
                    have_truss = (weu, wev, wtr, wsup, 0, len(wtr))
                elif op == "slice" and len(w.tr):
                    world = int(rng.integers(2, 5)); rank = int(rng.integers(0, world))
                    a.truss_run_slice(rank, world)
                    ne = len(w.tr)
                    have_truss = (w.eu, w.ev, w.tr, w.sup, ne * rank // world, ne * (rank + 1) // world)
                elif op == "prepare":
                    a.truss_prepare()
                elif op == "unprepare":
                    a.truss_unprepare()
                    have_truss = None               # (the last result goes with the preparation)
                elif op == "fetch" and have_truss is not None:
                    eu, ev, tr, sup = _fetch_varied(a, rng)
                    weu, wev, wtr, wsup, lo, hi = have_truss
                    assert _eq(eu, weu) and _eq(ev, wev), tag
                    assert _eq(tr[lo:hi], wtr[lo:hi]) and _eq(sup[lo:hi], wsup[lo:hi]), tag
                    assert not tr[:lo].any() and not tr[hi:].any() and not sup[:lo].any() and not sup[hi:].any(), tag
                elif op == "corea":
                    rd, rk = a.fractional_ranks(w.deg, w.core)
                    assert _eq(rd, w.rd) and _eq(rk, w.rk), tag
                    assert _eq(a.get_anomaly_score(w.deg, w.core), w.score), tag
                elif op == "switch":
                    name, values = switches[int(rng.integers(0, len(switches)))]
                    v = values[int(rng.integers(0, len(values)))]
                    if v is None: monkeypatch.delenv("KOMB_" + name, raising=False)
                    else: monkeypatch.setenv("KOMB_" + name, v)
                elif op == "poison" and poisoned:
                    monkeypatch.setenv("KOMB_POISON", PATTERNS[int(rng.integers(0, len(PATTERNS)))])
            # every graph ends with a whole run and a complete fetch in a varied order
            a.truss_run()
            eu, ev, tr, sup = _fetch_varied(a, rng)
            assert _eq(eu, w.eu) and _eq(ev, w.ev) and _eq(tr, w.tr) and _eq(sup, w.sup), (w.name, "final")
            deg, core = a.run_core()
            assert _eq(core, w.core), (w.name, "final core")
            n_ops += 2
    assert n_ops >= 60


def _oracle_trussness_fast(O, rowptr, col):
    if O.native_lib() is not None:
        return O.trussness_native(rowptr, col, min(16, len(os.sched_getaffinity(0))))
    return O.trussness(rowptr, col)


def test_full_size_c2_poisoned(K, O, monkeypatch):
    """BASELINE config C2 (|V| = 1M, |E| ~ 10M) under 0xFFFFFFFF: every coreness and trussness value against the oracle, with
    both peels handing a remainder of this size over to the local finish (asserted from the statistics)."""
    _set_env(monkeypatch, "0xFFFFFFFF", "default")
    nv = 1_000_000
    uv = K.gen_hug_edges(nv, 2_450_000, 2.6, 42)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        rowptr, col = a.get_csr()
        o_rowptr, o_col = O.simplify(nv, uv)
        assert _eq(rowptr, o_rowptr) and _eq(col, o_col)
        deg, core = a.run_core()
        assert _eq(deg, O.degree(o_rowptr)) and _eq(core, O.coreness(o_rowptr, o_col))
        assert a.stats()["core_local_units"] > 0, "k-core: no hand-over to the local finish"
        eu, ev, tr, sup = a.run_truss(with_support=True)
        oeu, oev = O.edge_list(o_rowptr, o_col)
        assert _eq(eu, oeu) and _eq(ev, oev)
        assert _eq(sup, O.support(o_rowptr, o_col)[0])
        assert _eq(tr, _oracle_trussness_fast(O, o_rowptr, o_col))
        assert a.stats()["truss_local_units"] > 0, "k-truss: no hand-over to the local finish"
