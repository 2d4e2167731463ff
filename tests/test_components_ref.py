"""CPU tests of the components reference (tests/components_ref.py), of the composite test graph and of the new entry
points without a device."""
import numpy as np
import pytest

import components_ref as R


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def _nx_labels(nv, eu, ev):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(nv))
    g.add_edges_from(zip(np.asarray(eu).tolist(), np.asarray(ev).tolist()))
    out = np.full(nv, -1, np.int64)
    for comp in nx.connected_components(g):
        comp = list(comp)
        out[comp] = min(comp)
    return out


def _check_min_labels(nv, uv, name):
    uv = np.asarray(uv, np.int64).reshape(-1, 2)
    got = R.min_labels(nv, uv[:, 0], uv[:, 1], np.ones(nv, bool))
    want = _nx_labels(nv, uv[:, 0], uv[:, 1])
    assert np.array_equal(got, want), name
    # the smallest-id rule, stated directly: a label is a vertex that labels itself, and no vertex is below its label
    assert np.array_equal(got[got], got) and np.all(got <= np.arange(nv)), name
    sz = R.sizes(got)
    assert sz.sum() == sum(int(s) * int(s) for s in np.bincount(got)), name
    return got


def test_min_labels_equals_networkx(K, golden):
    for g in golden:
        _check_min_labels(g["nv"], np.stack([np.asarray(g["eu"], np.int64), np.asarray(g["ev"], np.int64)], 1), g["name"])
        _check_min_labels(g["nv"], g["raw"], g["name"] + " raw")
    for i, (nv, e) in enumerate(R.composite_parts(K.gen_hug_edges, 1)):
        _check_min_labels(nv, e, f"part {i}")
    # members only: everyone else is -1 and counts for nothing
    lab = R.min_labels(6, [0, 4], [1, 5], np.array([1, 1, 0, 0, 1, 1], bool))
    assert lab.tolist() == [0, 0, -1, -1, 4, 4] and R.sizes(lab).tolist() == [2, 2, 0, 0, 2, 2]
    assert R.summary(lab) == (4, 2, 2)
    assert len(R.min_labels(0, [], [], np.zeros(0, bool))) == 0


@pytest.mark.parametrize("seed", [1, 2])
def test_composite_has_many_components(K, O, seed):
    nv, uv = R.composite(K.gen_hug_edges, seed)
    rowptr, col = O.simplify(nv, uv)
    core = O.coreness(rowptr, col)
    eu, ev = O.edge_list(rowptr, col)
    tr = O.trussness(rowptr, col)
    assert nv == 196066
    if seed == 1:
        assert len(eu) == 959288 and core.max() == 63 and tr.max() == 64
    for k in (1, 2, 3, 5):
        lab = R.core_components(rowptr, col, core, k)
        sz = R.sizes(lab)
        n_big = int(((lab == np.arange(nv)) & (sz > 1)).sum())
        assert n_big >= 12, (k, n_big)
        assert np.array_equal(lab >= 0, core >= k)
    for k in (3, 4, 6):
        lab = R.truss_components(nv, eu, ev, tr, k)
        sz = R.sizes(lab)
        n_big = int(((lab == np.arange(nv)) & (sz > 1)).sum())
        assert n_big >= 12, (k, n_big)
    if seed == 1:
        assert R.summary(R.core_components(rowptr, col, core, 0)) == (196066, 3949, 100000)
        assert R.summary(R.core_components(rowptr, col, core, 2)) == (84671, 15, 48304)
        assert R.summary(R.truss_components(nv, eu, ev, tr, 3)) == (82480, 20, 47655)
        assert R.summary(R.truss_components(nv, eu, ev, tr, 6)) == (50623, 23, 29926)
        assert R.summary(R.core_components(rowptr, col, core, 63)) == (64, 1, 64)


def test_binding_declares_components_and_fails_without_device(K):
    """The binding covers the three new entry points; without a GPU they answer KOMB_ERR_DEVICE (no CPU fallback)."""
    from komb_amd import _lib
    for name in ("komb_components_run", "komb_components_fetch", "komb_components_info"):
        assert name in _lib.SIGNATURES
    for name in ("components_run", "components_fetch", "components_info", "run_components"):
        assert callable(getattr(K.KombAccel, name))
    assert (_lib.KOMB_COMP_CORE, _lib.KOMB_COMP_TRUSS, _lib.KOMB_COMP_K_MAX) == (0, 1, -1)
    assert "COMP_SAMPLE" in K.api.OPTION_NAMES
    g = K.KombAccel()
    try:
        g.from_edges(3, [[0, 1]])
    except K.KombError as e:
        assert e.code == _lib.KOMB_ERR_DEVICE
    else:
        g.close()
        return                                   # a usable GPU is present: the GPU tests cover the calls
    with pytest.raises(K.KombError) as e:
        g.components_run("core", 0)
    assert e.value.code == _lib.KOMB_ERR_DEVICE
    for call in (g.components_fetch, g.components_info, lambda: g.run_components("truss", -1)):
        with pytest.raises(K.KombError) as e:
            call()
        assert e.value.code == _lib.KOMB_ERR_DEVICE
    g.close()
