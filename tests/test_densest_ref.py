"""CPU tests of tests/densest_ref.py, the restatement the GPU tests compare komb_densest_subgraph_* with: its result and
its certificate sandwich the exact optimum on small random graphs, and the constructed graph gives the stated values."""
import numpy as np
import pytest

import densest_ref as D


def _random_graphs():
    rng = np.random.default_rng(20260)
    for i in range(60):
        nv = int(rng.integers(4, 13))
        p = float(rng.uniform(0.15, 0.8))
        iu = np.stack(np.triu_indices(nv, 1), 1)
        yield nv, iu[rng.random(len(iu)) < p]


@pytest.fixture(scope="module")
def small_graphs():
    out = []
    for nv, uv in _random_graphs():
        rowptr, col = D.csr_of_edges(nv, uv)
        out.append((rowptr, col, D.coreness(rowptr, col), D.brute_force_optimum(rowptr, col)))
    return out


@pytest.mark.parametrize("iters", [0, 1, 8, 64])
def test_sandwich_against_brute_force(small_graphs, iters):
    for rowptr, col, core, (om, on) in small_graphs:
        r = D.densest(rowptr, col, core, iters)
        assert r["n_sub"] == int(r["member"].sum()) and r["m_sub"] == D.edges_inside(rowptr, col, r["member"])
        if r["n_sub"]:
            assert r["m_sub"] * on <= om * r["n_sub"]                     # found <= optimum
        assert om <= r["k_max"] * on                                      # optimum <= k_max
        if iters >= 1:
            assert om * iters <= r["load_max"] * on                       # optimum <= load_max / iters
        assert int(r["load"].sum()) == (r["m_pruned"] * iters if r["m_pruned"] else 0)
        assert r["n_k"][0] == len(core) and r["m_k"][0] == len(col) // 2


def test_constructed_graph():
    nv, uv = D.constructed_graph()
    rowptr, col = D.csr_of_edges(nv, uv)
    core = D.coreness(rowptr, col)
    r0 = D.densest(rowptr, col, core, 0)
    assert (r0["source"], r0["k_best"], r0["m_sub"], r0["n_sub"]) == (D.SOURCE_CORE, 5, 15, 6)
    assert np.flatnonzero(r0["member"]).tolist() == list(range(6))
    # no k-core is optimal: the 8-vertex set has 21 edges, 21 / 8 > 15 / 6
    for k in range(r0["k_max"] + 1):
        assert int(r0["m_k"][k]) * 8 < 21 * int(r0["n_k"][k])
    for iters in (2, 3, 7, 16, 64):
        r = D.densest(rowptr, col, core, iters)
        assert (r["source"], r["m_sub"], r["n_sub"]) == (D.SOURCE_PREFIX, 21, 8), iters
        assert np.flatnonzero(r["member"]).tolist() == list(range(8)), iters
    r = D.densest(rowptr, col, core, 64)
    assert r["load_max"] == 168                                           # 168 / 64 == 21 / 8: the certificate is tight
    assert r["load_max"] * 8 == 21 * 64


def test_degenerate_inputs():
    r = D.densest(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), 5)
    assert (r["n_sub"], r["m_sub"], r["k_max"], r["load_max"], len(r["member"])) == (0, 0, 0, 0, 0)
    rowptr, col = D.csr_of_edges(5, np.zeros((0, 2)))
    r = D.densest(rowptr, col, np.zeros(5, np.int32), 3)
    assert r["member"].tolist() == [1] * 5 and (r["source"], r["m_sub"], r["n_sub"], r["k_best"]) == (D.SOURCE_CORE, 0, 5, 0)
    with pytest.raises(ValueError):
        D.densest(rowptr, col, np.zeros(5, np.int32), -1)
    # the load word: a star with 5 000 leaves takes iters * 5 000 units on its centre at most
    nv = 5001
    rowptr, col = D.csr_of_edges(nv, [[0, i] for i in range(1, nv)])
    with pytest.raises(D.LimitError):
        D.densest(rowptr, col, np.ones(nv, np.int32), 2 ** 31 // 5000 + 1)
