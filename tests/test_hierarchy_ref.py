"""CPU tests of the hierarchy reference (tests/hierarchy_ref.py): the two worked examples of the definition, and on the golden
graphs and a composite graph the walk-up consequence against components_ref for every k, the size invariant and
parent[i] < i."""
import numpy as np
import pytest

import components_ref as R
import hierarchy_ref as H


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def k4(off):
    return [[off + a, off + b] for a in range(4) for b in range(a + 1, 4)]


CORE_EXAMPLE = (11, k4(0) + k4(4) + [[8, 0], [8, 4], [9, 8]], [3] * 8 + [2, 1, 0],
                {"k": [0, 1, 2, 3, 3], "rep": [10, 0, 0, 0, 4], "parent": [-1, -1, 1, 2, 2], "size": [1, 10, 9, 4, 4],
                 "shell": [1, 1, 1, 4, 4], "node": [3, 3, 3, 3, 4, 4, 4, 4, 2, 1, 0]})
TRUSS_EXAMPLE = (8, k4(0) + k4(4) + [[0, 4]],
                 {"k": [2, 4, 4], "rep": [0, 0, 4], "parent": [-1, 0, 0], "size": [8, 4, 4], "shell": [0, 4, 4],
                  "node": [1, 1, 1, 1, 2, 2, 2, 2]})


def _same(h, want):
    for f in H.FIELDS + ("node",):
        assert h[f].tolist() == list(want[f]), f


def test_worked_examples(O):
    nv, uv, core, want = CORE_EXAMPLE
    rowptr, col = R.simple_csr(nv, uv)
    assert O.coreness(rowptr, col).tolist() == core
    h = H.core_hierarchy(rowptr, col, core)
    _same(h, want)
    assert H.info(h, "core") == (5, 2, 3, 3)
    H.check_invariants(h, True)
    nv, uv, want = TRUSS_EXAMPLE
    rowptr, col = R.simple_csr(nv, uv)
    eu, ev = O.edge_list(rowptr, col)
    tr = O.trussness(rowptr, col)
    assert sorted(tr.tolist()) == [2] + [4] * 12
    h = H.truss_hierarchy(nv, eu, ev, tr)
    _same(h, want)
    assert H.info(h, "truss") == (3, 1, 4, 2)
    H.check_invariants(h, False)
    # no vertices, no edges
    e = np.zeros(0, np.int64)
    assert H.info(H.core_hierarchy(np.zeros(1, np.int64), e, e), "core") == (0, 0, 0, 0)
    assert H.info(H.truss_hierarchy(3, e, e, e), "truss") == (0, 0, 2, 0)
    assert H.truss_hierarchy(3, e, e, e)["node"].tolist() == [-1] * 3


def _check_core(rowptr, col, core):
    core = np.asarray(core, np.int64)
    h = H.core_hierarchy(rowptr, col, core)
    H.check_invariants(h, True)
    for k in range(0, (int(core.max()) if len(core) else 0) + 2):
        assert np.array_equal(H.walk_up_labels(h, core, k), R.core_components(rowptr, col, core, k)), k
    return h


def _check_truss(nv, eu, ev, tr):
    h = H.truss_hierarchy(nv, eu, ev, tr)
    H.check_invariants(h, False)
    lvl = H.truss_levels(nv, eu, ev, tr)
    for k in range(2, (int(max(tr)) if len(tr) else 2) + 2):
        assert np.array_equal(H.walk_up_labels(h, lvl, k), R.truss_components(nv, eu, ev, tr, k)), k
    return h


def test_golden_graphs(golden):
    for g in golden:
        _check_core(np.asarray(g["rowptr"], np.int64), np.asarray(g["col"], np.int64), g["coreness"])
        _check_truss(g["nv"], g["eu"], g["ev"], g["trussness"])
        _check_truss(g["nv"], g["sub_eu"], g["sub_ev"], g["sub_trussness"])


def test_composite(K, O):
    nv, uv = R.composite(K.gen_hug_edges, 1)
    rowptr, col = O.simplify(nv, uv)
    h = _check_core(rowptr, col, O.coreness(rowptr, col))
    assert H.info(h, "core")[1] == 3949                    # the components of the whole graph (test_components_ref.py)
    eu, ev = O.edge_list(rowptr, col)
    h = _check_truss(nv, eu, ev, O.trussness(rowptr, col))
    assert (h["shell"] == 0).any()                         # cliques joined by a bridge edge: a node that only merges


def _core_and_truss(O, nv, uv):
    rowptr, col = R.simple_csr(nv, uv)
    hc = _check_core(rowptr, col, O.coreness(rowptr, col))
    eu, ev = O.edge_list(rowptr, col)
    return hc, _check_truss(nv, eu, ev, O.trussness(rowptr, col))


@pytest.mark.parametrize("nv", [255, 256, 257, 513])
def test_isolated_vertices(O, nv):
    hc, ht = _core_and_truss(O, nv, np.zeros((0, 2), np.int64))
    assert hc["k"].tolist() == [0] * nv and hc["rep"].tolist() == list(range(nv)) and hc["parent"].tolist() == [-1] * nv
    assert hc["size"].tolist() == [1] * nv and hc["shell"].tolist() == [1] * nv and hc["node"].tolist() == list(range(nv))
    assert len(ht["k"]) == 0 and ht["node"].tolist() == [-1] * nv


def test_strided_claim_graph(O):
    nv, uv = H.strided_claim_graph()
    n = H.STRIDE_ISOLATED
    hc, ht = _core_and_truss(O, nv, uv)
    assert len(hc["k"]) == n + 1 and (hc["k"][:n] == 0).all() and (hc["size"][:n] == 1).all() and (hc["shell"][:n] == 1).all()
    assert (hc["k"][n], hc["rep"][n], hc["parent"][n], hc["size"][n], hc["shell"][n]) == (3, n, -1, 4, 4)
    assert np.array_equal(hc["node"], np.minimum(np.arange(nv), n))
    assert {f: ht[f].tolist() for f in H.FIELDS} == {"k": [4], "rep": [n], "parent": [-1], "size": [4], "shell": [4]}


def test_shell_first_graph(O):
    nv, uv = H.shell_first_graph()
    for ids in (np.arange(nv), np.random.default_rng(12).permutation(nv)):
        hc, ht = _core_and_truss(O, nv, ids[uv])
        k, size = hc["k"].tolist(), hc["size"].tolist()
        assert k == [1] * 302 + [5, 30] and sorted(size[:302]) == [2] * 300 + [2106, 2131] and sorted(size[302:]) == [6, 31]
        assert sorted(ht["k"].tolist()) == [2] * 302 + [6, 31]
