"""GPU tests of komb_densest_subgraph_run / _fetch / _profile / _info: member, load, the core density profile and every
integer of info compared exactly with the restatement of tests/densest_ref.py (coreness taken from the library's own
komb_core_run, whose parity other tests own), on both paths of the rounds (option DENSEST_LOCAL 0 and 1), under POISON and
on a reused context; the error paths; and that a run leaves every other result and komb_stats bit-equal."""
import numpy as np
import pytest

import densest_ref as D

pytestmark = pytest.mark.gpu

ITERS = (0, 1, 2, 7, 64)
LDS_WORDS = 160 * 1024 // 4              # loads + deltas of the local path: |P| above half of this cannot fit


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("KOMB_DENSEST_LOCAL", raising=False)


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


def _clique(n, off=0):
    return np.stack(np.triu_indices(n, 1), 1).astype(np.int64) + off


def _clique_plus(n, attached):
    """K_n and one more vertex joined to `attached` of its vertices."""
    return n + 1, np.concatenate([_clique(n), np.stack([np.full(attached, n), np.arange(attached)], 1)])


def _fetch_all(a):
    member, load = a.densest_subgraph_fetch()
    n_k, m_k = a.densest_subgraph_profile()
    return {"member": member, "load": load, "n_k": n_k, "m_k": m_k, **a.densest_subgraph_info()}


def _same(got, want, what):
    for f in ("member", "load"):
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), (what, f)
    for f in ("n_k", "m_k"):
        assert got[f].dtype == np.int64 and np.array_equal(got[f], want[f]), (what, f)
    for f in D.INFO_FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert got["ms"] >= 0.0


class _Case:
    """One loaded graph: its CSR and coreness read back once, the restatement computed once per iters."""

    def __init__(self, a):
        self.a = a
        self.rowptr, self.col = a.get_csr()
        _, self.core = a.run_core()
        self.want = {}

    def ref(self, iters):
        if iters not in self.want:
            self.want[iters] = D.densest(self.rowptr, self.col, self.core, iters)
        return self.want[iters]

    def check(self, monkeypatch, iters_list=ITERS, both_paths=True, what=""):
        for local in (("0", "1") if both_paths else (None,)):
            if local is None:
                monkeypatch.delenv("KOMB_DENSEST_LOCAL", raising=False)
            else:
                monkeypatch.setenv("KOMB_DENSEST_LOCAL", local)
            for iters in iters_list:
                self.a.densest_subgraph_run(iters)
                _same(_fetch_all(self.a), self.ref(iters), (what, local, iters))
        monkeypatch.delenv("KOMB_DENSEST_LOCAL", raising=False)
        for iters in iters_list[-1:]:                        # the automatic choice
            self.a.densest_subgraph_run(iters)
            _same(_fetch_all(self.a), self.ref(iters), (what, "auto", iters))
        return self


def _check_graph(K, monkeypatch, nv, uv, what, **kw):
    with K.KombAccel() as a:
        a.from_edges(nv, _i64(uv))
        return _Case(a).check(monkeypatch, what=what, **kw).want


def test_degenerate_graphs(K, monkeypatch):
    with K.KombAccel() as a:
        a.from_edges(0, np.zeros((0, 2)))
        a.run_core()
        for iters in (0, 3):
            member, load, info = a.run_densest_subgraph(iters)
            n_k, m_k = a.densest_subgraph_profile()
            assert len(member) == 0 and len(load) == 0 and n_k.tolist() == [0] and m_k.tolist() == [0]
            assert [info[f] for f in D.INFO_FIELDS] == [0, 0, 0, 0, 0, 0, 0, 0, iters, 0]
    want = _check_graph(K, monkeypatch, 7, np.zeros((0, 2)), "isolated")
    assert want[7]["member"].tolist() == [1] * 7 and (want[7]["m_sub"], want[7]["n_sub"], want[7]["source"]) == (0, 7, 0)
    want = _check_graph(K, monkeypatch, 4, [[3, 1]], "one edge")
    assert want[64]["member"].tolist() == [0, 1, 0, 1] and (want[64]["m_sub"], want[64]["n_sub"]) == (1, 2)
    n = 300
    _check_graph(K, monkeypatch, n, np.stack([np.arange(n - 1), np.arange(1, n)], 1), "path")


def test_star_k40_and_constructed(K, monkeypatch):
    n = 5001                                                 # one heavy row
    want = _check_graph(K, monkeypatch, n, np.stack([np.zeros(n - 1, int), np.arange(1, n)], 1), "star")
    assert want[64]["n_pruned"] == n and want[64]["m_pruned"] == n - 1
    want = _check_graph(K, monkeypatch, 40, _clique(40), "K40")
    assert (want[64]["m_sub"], want[64]["n_sub"], want[64]["k_best"]) == (780, 40, 39)
    nv, uv = D.constructed_graph()
    want = _check_graph(K, monkeypatch, nv, uv, "constructed")
    assert (want[0]["source"], want[0]["m_sub"], want[0]["n_sub"]) == (D.SOURCE_CORE, 15, 6)
    for iters in (2, 7, 64):
        assert (want[iters]["source"], want[iters]["m_sub"], want[iters]["n_sub"]) == (D.SOURCE_PREFIX, 21, 8)
    assert want[64]["load_max"] == 168
    rng = np.random.default_rng(5)
    _check_graph(K, monkeypatch, nv, rng.permutation(nv)[uv], "constructed, permuted")


@pytest.mark.parametrize("clique,attached,pairs", [(11, 8, 63), (11, 9, 64), (11, 10, 65), (45, 33, 1023), (45, 34, 1024), (45, 35, 1025)])
def test_pruned_edge_counts_around_a_wave_and_a_workgroup(K, monkeypatch, clique, attached, pairs):
    nv, uv = _clique_plus(clique, attached)
    want = _check_graph(K, monkeypatch, nv, uv, f"K{clique}+{attached}")
    assert want[64]["m_pruned"] == pairs and want[64]["n_pruned"] == nv


def test_golden_graphs(K, golden, monkeypatch):
    for g in golden:
        with K.KombAccel() as a:
            a.from_edges(g["nv"], _i64(g["raw"]))
            case = _Case(a)
            assert case.core.tolist() == list(g["coreness"])
            case.check(monkeypatch, what="golden")


@pytest.mark.parametrize("alpha", [2.6, 2.2])
def test_power_law_graphs(K, monkeypatch, alpha):
    uv = np.asarray(K.gen_hug_edges(20000, 40000, alpha, 11)).reshape(-1, 2)
    want = _check_graph(K, monkeypatch, 20000, uv, f"hug {alpha}", iters_list=(0, 1, 7, 64))
    assert want[64]["m_pruned"] > 0 and want[64]["load_max"] * want[64]["n_sub"] >= want[64]["m_sub"] * 64


def test_pruned_set_larger_than_lds_runs_on_the_grid(K, monkeypatch):
    n = 30000                                                # a cycle and a K_5: c = 2, P = everything
    uv = np.concatenate([np.stack([np.arange(n), (np.arange(n) + 1) % n], 1), _clique(5, n)])
    want = _check_graph(K, monkeypatch, n + 5, uv, "cycle", iters_list=(1, 2, 7, 64))
    assert want[64]["n_pruned"] == n + 5 and 2 * want[64]["n_pruned"] > LDS_WORDS
    assert (want[64]["m_sub"], want[64]["n_sub"]) == (10, 5)


def test_error_paths(K):
    E = K._lib
    n = 5001
    star = np.stack([np.zeros(n - 1, int), np.arange(1, n)], 1)
    with K.KombAccel() as a:
        a.from_edges(n, star)

        def code(call):
            with pytest.raises(K.KombError) as e:
                call()
            return e.value.code
        assert code(lambda: a.densest_subgraph_run(4)) == E.KOMB_ERR_STATE          # no komb_core_run yet
        a.run_core()
        assert code(a.densest_subgraph_fetch) == E.KOMB_ERR_STATE                   # no run yet
        assert code(a.densest_subgraph_profile) == E.KOMB_ERR_STATE
        assert code(a.densest_subgraph_info) == E.KOMB_ERR_STATE
        assert code(lambda: a.densest_subgraph_run(-1)) == E.KOMB_ERR_ARG
        case = _Case(a)
        a.densest_subgraph_run(7)
        before = _fetch_all(a)
        _same(before, case.ref(7), "star")
        too_many = 2 ** 31 // (n - 1) + 1                                           # iters * 5000 > 2^31 - 1
        with pytest.raises(D.LimitError):
            case.ref(too_many)
        assert code(lambda: a.densest_subgraph_run(too_many)) == E.KOMB_ERR_LIMIT
        assert code(lambda: a.densest_subgraph_run(-1)) == E.KOMB_ERR_ARG
        after = _fetch_all(a)                                                       # the previous result is still readable
        _same(after, case.ref(7), "star after the refusals")
        a.from_edges(4, [[0, 1]])                                                   # a new graph drops the result
        assert code(a.densest_subgraph_fetch) == E.KOMB_ERR_STATE
        assert code(a.densest_subgraph_info) == E.KOMB_ERR_STATE
        assert code(lambda: a.densest_subgraph_run(1)) == E.KOMB_ERR_STATE


def test_a_run_changes_no_other_result(K):
    uv = np.asarray(K.gen_hug_edges(6000, 14000, 2.4, 3)).reshape(-1, 2)
    with K.KombAccel() as a:
        a.from_edges(6000, uv)
        a.run_core(); a.run_onion(); a.run_truss()
        a.run_components("core", 2)
        a.run_hierarchy("core")

        def snapshot():
            nodes = a.hierarchy_fetch_nodes()
            return ([*a.core_fetch(), *a.onion_fetch(), *a.truss_fetch(), *a.components_fetch(), a.hierarchy_fetch_vertices()]
                    + [nodes[f] for f in a.HIER_FIELDS], a.stats(), a.components_info(), a.hierarchy_info(), a.onion_info())
        before = snapshot()
        for iters in (0, 9):
            a.run_densest_subgraph(iters)
        after = snapshot()
        for x, y in zip(before[0], after[0]):
            assert np.array_equal(x, y)
        assert before[1:] == after[1:]
        # and the other way round: later calls leave the densest result as it is
        kept = _fetch_all(a)
        a.run_core(); a.run_onion(); a.run_truss(); a.run_components("truss", 3); a.run_hierarchy("truss")
        again = _fetch_all(a)
        _same(again, kept, "after other calls")
        assert again["ms"] == kept["ms"]


@pytest.mark.parametrize("poison", ["0xFFFFFFFF", "0x7FFFFFFF", "0x00000001"])
def test_poisoned_memory_and_a_reused_context(K, monkeypatch, poison):
    monkeypatch.setenv("KOMB_POISON", poison)
    nv, uv = D.constructed_graph()
    n = 5001
    graphs = [(nv, uv), (n, np.stack([np.zeros(n - 1, int), np.arange(1, n)], 1)), _clique_plus(45, 34),
              (3000, np.asarray(K.gen_hug_edges(3000, 7000, 2.3, 21)).reshape(-1, 2)), (9, np.zeros((0, 2))), (nv, uv)]
    with K.KombAccel() as a:                                 # one context, one graph after the other
        for i, (gnv, guv) in enumerate(graphs):
            a.from_edges(gnv, _i64(guv))
            _Case(a).check(monkeypatch, iters_list=(0, 2, 33), what=("reused", i))
