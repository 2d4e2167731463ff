"""GPU tests of the onion decomposition (komb_onion_run / _fetch / _info) against networkx.onion_layers, the CPU
restatement of tests/onion_ref.py and its O(E) checker, with the consistency the ABI promises: the onion's coreness is
komb_core_run's, no engine option changes a layer, and onion calls leave every other result and komb_stats alone."""
import hashlib

import numpy as np
import pytest

import onion_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _onion(K, nv, uv=None, csr=None):
    with K.KombAccel() as a:
        if csr is not None:
            a.from_csr(np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32))
        else:
            a.from_edges(nv, np.asarray(uv, np.int64).reshape(-1, 2))
        layer, core = a.run_onion()
        info = a.onion_info()
        _, kcore = a.run_core()
    return layer, core, info, kcore


def _check_against_restatement(K, nv, uv):
    rowptr, col = R.simple_csr(nv, uv)
    want, want_core, n = R.onion_layers(rowptr, col)
    layer, core, info, kcore = _onion(K, nv, uv)
    assert np.array_equal(layer, want)
    assert np.array_equal(core, want_core) and np.array_equal(core, kcore)
    assert info["n_layers"] == n and info["max_coreness"] == (int(core.max()) if nv else 0)
    return layer


def test_golden_graphs_vs_networkx(K, golden):
    for g in golden:
        nv = g["nv"]
        want, n = R.networkx_layers(nv, np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int64))
        layer, core, info, kcore = _onion(K, nv, _i64(g["raw"]))
        assert layer.tolist() == want.tolist(), g["name"]
        assert core.tolist() == g["coreness"] and np.array_equal(core, kcore), g["name"]
        assert info["n_layers"] == n, g["name"]
        layer2, _, _, _ = _onion(K, nv, csr=(g["rowptr"], g["col"]))
        assert np.array_equal(layer2, layer), g["name"]


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1, 2)


@pytest.mark.parametrize("nv", [1000, 20000, 200000])
@pytest.mark.parametrize("alpha", [2.1, 2.2, 2.6])
def test_generated_graphs_vs_restatement(K, nv, alpha):
    uv = K.gen_hug_edges(nv, int(2.45 * nv), alpha, 11)
    _check_against_restatement(K, nv, uv)


def test_small_generated_graphs_vs_networkx(K):
    for seed, (nv, alpha) in enumerate([(300, 2.1), (2000, 2.2), (5000, 2.6)]):
        uv = K.gen_hug_edges(nv, int(2.45 * nv), alpha, seed + 1)
        rowptr, col = R.simple_csr(nv, uv)
        want, n = R.networkx_layers(nv, rowptr, col)
        layer, _, info, _ = _onion(K, nv, uv)
        assert np.array_equal(layer, want) and info["n_layers"] == n


def test_edge_cases(K):
    # only isolated vertices: one layer
    layer, core, info, _ = _onion(K, 5, np.zeros((0, 2)))
    assert layer.tolist() == [1] * 5 and core.tolist() == [0] * 5 and info["n_layers"] == 1 and info["max_coreness"] == 0
    # a single edge, plus an isolated vertex
    layer, core, info, _ = _onion(K, 2, [[0, 1]])
    assert layer.tolist() == [1, 1] and core.tolist() == [1, 1] and info["n_layers"] == 1
    layer, core, info, _ = _onion(K, 3, [[2, 0]])
    assert layer.tolist() == [2, 1, 2] and core.tolist() == [1, 0, 1] and info["n_layers"] == 2
    # a path peels from both ends
    n = 9
    layer, core, info, _ = _onion(K, n, [[i, i + 1] for i in range(n - 1)])
    assert layer.tolist() == [1, 2, 3, 4, 5, 4, 3, 2, 1] and set(core.tolist()) == {1}
    # a star: the leaves, then the centre
    layer, core, _, _ = _onion(K, 6, [[0, i] for i in range(1, 6)])
    assert layer.tolist() == [2, 1, 1, 1, 1, 1] and core.tolist() == [1] * 6
    # K_n: one layer at k = n - 1
    n = 40
    iu = np.stack(np.triu_indices(n, 1), 1)
    layer, core, info, _ = _onion(K, n, iu)
    assert layer.tolist() == [1] * n and core.tolist() == [n - 1] * n and info["max_coreness"] == n - 1
    # raw input with loops and duplicates: the simple graph's layers
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 300, (2000, 2))
    raw = np.concatenate([raw, raw[:500], raw[:500, ::-1], np.stack([np.arange(50)] * 2, 1)])
    _check_against_restatement(K, 310, raw)
    # the empty graph
    layer, core, info, _ = _onion(K, 0, np.zeros((0, 2)))
    assert len(layer) == 0 and info["n_layers"] == 0 and info["max_coreness"] == 0


def test_disconnected_and_structured(K):
    parts, off = [], 0
    for n in (3, 7, 25, 64, 65, 130):
        iu = np.stack(np.triu_indices(n, 1), 1) + off          # a clique
        parts.append(iu)
        off += n
        parts.append(np.stack([np.arange(off, off + n - 1), np.arange(off + 1, off + n)], 1))   # a path
        off += n
    parts.append(np.stack([np.full(3000, off), np.arange(off + 1, off + 3001)], 1))             # a hub of 3000 leaves
    off += 3001
    _check_against_restatement(K, off + 17, np.concatenate(parts))


@pytest.mark.parametrize("opts", [
    {"FINISH": "local"}, {"FINISH": "lds"}, {"FINISH": "none"},
    {"CORE_TAIL": "0"}, {"CORE_TAIL": "1024"}, {"CORE_TAIL": "37"},
    {"POISON": "0xFFFFFFFF"}, {"POISON": "0x00000001", "FINISH": "none"},
])
def test_engine_options_do_not_change_layers(K, monkeypatch, opts):
    graphs = [(30000, K.gen_hug_edges(30000, 73500, 2.2, 5)), (900, K.gen_hug_edges(900, 2200, 2.6, 6)),
              (50000, K.gen_hug_edges(50000, 122500, 2.6, 7))]
    want = []
    for nv, uv in graphs:
        want.append(_onion(K, nv, uv))
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)
    for (nv, uv), w in zip(graphs, want):
        got = _onion(K, nv, uv)
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])
        assert got[2]["n_layers"] == w[2]["n_layers"]


def test_interleaved_calls_change_nothing_else(K, monkeypatch):
    """Core, truss and CoreA results and every komb_stats field are the same with onion calls between them."""
    monkeypatch.setenv("KOMB_POISON", "0xA5A5A5A5")
    nv = 60000
    uv = K.gen_hug_edges(nv, int(2.45 * nv), 2.4, 21)

    def session(with_onion):
        out = []
        with K.KombAccel() as a:
            a.from_edges(nv, uv)
            if with_onion:
                a.run_onion()
            deg, core = a.run_core()
            st_core = a.stats()
            if with_onion:
                layer, ocore = a.run_onion()
                assert np.array_equal(ocore, core)
                out.append(layer)
                assert a.stats() == st_core
                assert np.array_equal(a.core_fetch()[1], core)
            eu, ev, tr = a.run_truss()
            st_truss = a.stats()
            if with_onion:
                a.run_onion()
                assert a.stats() == st_truss
                assert np.array_equal(a.truss_fetch()[2], tr)
            score = a.get_anomaly_score(deg, core)
            if with_onion:
                a.onion_run()
                assert np.array_equal(a.onion_fetch()[0], out[0])
            st = a.stats()
        times = [k for k in st if k.startswith("ms_")]
        return deg, core, eu, ev, tr, score, {k: v for k, v in st.items() if k not in times}

    plain, mixed = session(False), session(True)
    for x, y in zip(plain[:6], mixed[:6]):
        assert np.array_equal(x, y)
    assert plain[6] == mixed[6]


def test_repeated_calls_identical(K):
    nv = 100000
    uv = K.gen_hug_edges(nv, int(2.45 * nv), 2.2, 8)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        first = a.run_onion()
        info = a.onion_info()
        for _ in range(3):
            again = a.run_onion()
            assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
            assert a.onion_info()["n_layers"] == info["n_layers"]


def test_state_errors(K):
    with K.KombAccel() as a:
        for call in (a.onion_run, a.onion_info):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == K._lib.KOMB_ERR_ARG
        a.from_edges(4, [[0, 1], [1, 2]])
        for call in (a.onion_fetch, a.onion_info):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == K._lib.KOMB_ERR_STATE
        a.run_onion()
        assert a.onion_info()["n_layers"] == 3
        # a new graph invalidates the last run
        a.from_edges(3, [[0, 1]])
        with pytest.raises(K.KombError) as e:
            a.onion_fetch()
        assert e.value.code == K._lib.KOMB_ERR_STATE
        layer, _ = a.run_onion()
        assert layer.tolist() == [2, 2, 1]
        # a failed graph load leaves no graph
        with pytest.raises(K.KombError):
            a.from_edges(3, [[0, 5]])
        with pytest.raises(K.KombError) as e:
            a.onion_fetch()
        assert e.value.code == K._lib.KOMB_ERR_ARG


def test_full_size_c2(K):
    nv = 1_000_000
    uv = K.gen_hug_edges(nv, 2_450_000, 2.6, 42)
    rowptr, col = R.simple_csr(nv, uv)
    want, want_core, n = R.onion_layers(rowptr, col)
    layer, core, info, kcore = _onion(K, nv, uv)
    assert np.array_equal(layer, want) and np.array_equal(core, want_core) and np.array_equal(core, kcore)
    assert info["n_layers"] == n == 633 and info["max_coreness"] == 46
    assert hashlib.sha256(layer.astype(np.int32).tobytes()).hexdigest()[:16] == "bc117a630bde9f42"


def test_full_size_c3(K):
    """The pinned layer hash (computed on the CPU with onion_ref.onion_layers, whose coreness hash is the one the parity suite
    pins for C3) plus the O(E) checker -- no sequential restatement inside the test."""
    nv = 10_000_000
    uv = K.gen_hug_edges(nv, 24_250_000, 2.6, 42)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        del uv
        assert a.ne == 100_120_558
        layer, core = a.run_onion()
        info = a.onion_info()
        _, kcore = a.run_core()
        rowptr, col = a.get_csr()
    assert hashlib.sha256(core.tobytes()).hexdigest()[:16] == "120d47bf172d8b8f"
    assert hashlib.sha256(layer.tobytes()).hexdigest()[:16] == "48ed0ee753969c87"
    assert info["n_layers"] == 1005 and info["max_coreness"] == 72
    assert R.check_layering(rowptr, col, layer, core, kcore) == []
