"""CPU tests of the onion decomposition's test helpers (tests/onion_ref.py) and of the new entry points without a device."""
import numpy as np
import pytest

import onion_ref as R


def _graphs():
    rng = np.random.default_rng(1)
    out = []
    for nv, m in ((1, 0), (2, 1), (5, 3), (30, 40), (60, 400), (200, 300), (200, 2000), (500, 250), (1000, 1500), (1000, 8000)):
        out.append((f"random{nv}x{m}", nv, rng.integers(0, nv, (m, 2))))
    out.append(("path", 12, np.stack([np.arange(11), np.arange(1, 12)], 1)))
    out.append(("star", 9, np.stack([np.zeros(8, int), np.arange(1, 9)], 1)))
    out.append(("two stars", 20, np.concatenate([np.stack([np.zeros(8, int), np.arange(1, 9)], 1),
                                                 np.stack([np.full(10, 9), np.arange(10, 20)], 1), [[0, 9]]])))
    for n in (2, 3, 7, 20, 33):
        out.append((f"clique{n}", n, np.stack(np.triu_indices(n, 1), 1)))
    iu = np.stack(np.triu_indices(6, 1), 1)
    out.append(("disconnected", 40, np.concatenate([iu, iu + 10, np.stack([np.arange(20, 29), np.arange(21, 30)], 1)])))
    out.append(("isolated", 50, rng.integers(0, 25, (60, 2))))
    out.append(("loops+duplicates", 60, np.concatenate([rng.integers(0, 60, (150, 2)), np.stack([np.arange(10)] * 2, 1),
                                                        np.array([[3, 4]] * 5), np.array([[4, 3]] * 5)])))
    out.append(("empty", 0, np.zeros((0, 2), int)))
    return out


def _hugs():
    try:
        import komb_amd
        komb_amd._lib.load()
    except ImportError:
        return []
    out = []
    for nv, alpha, seed in ((2000, 2.1, 1), (2000, 2.2, 2), (2000, 2.6, 3), (20000, 2.1, 4), (20000, 2.2, 5), (20000, 2.6, 6),
                            (5000, 2.4, 7), (8000, 2.2, 8), (12000, 2.1, 9)):
        out.append((f"hug{nv}a{alpha}", nv, komb_amd.gen_hug_edges(nv, int(2.45 * nv), alpha, seed)))
    return out


def test_restatement_equals_networkx(built):
    cases = _graphs() + _hugs()
    assert len(cases) >= 30
    for name, nv, uv in cases:
        rowptr, col = R.simple_csr(nv, uv)
        layer, core, n = R.onion_layers(rowptr, col)
        want, wn = R.networkx_layers(nv, rowptr, col)
        assert np.array_equal(layer, want), name
        assert n == wn, name
        if nv:
            import networkx as nx
            g = nx.Graph()
            g.add_nodes_from(range(nv))
            src = np.repeat(np.arange(nv), np.diff(rowptr))
            g.add_edges_from(zip(src.tolist(), col.tolist()))
            cn = nx.core_number(g)
            assert core.tolist() == [cn[v] for v in range(nv)], name


def test_checker_accepts_true_and_rejects_perturbed_layerings(built):
    rng = np.random.default_rng(7)
    tried = 0
    for name, nv, uv in _graphs() + _hugs():
        if nv < 2:
            continue
        rowptr, col = R.simple_csr(nv, uv)
        layer, core, _ = R.onion_layers(rowptr, col)
        assert R.check_layering(rowptr, col, layer, core, core) == [], name
        for v in rng.integers(0, nv, 12):
            for d in (-1, 1):
                bad = layer.copy()
                bad[v] += d
                assert R.check_layering(rowptr, col, bad, core, core) != [], (name, int(v), d)
                tried += 1
        wrong = core.copy()
        wrong[rng.integers(0, nv)] += 1
        assert R.check_layering(rowptr, col, layer, wrong, core) != [], name
    assert tried >= 400


def test_no_device_onion_entry_points_fail(built):
    """Without a GPU the three onion entry points answer KOMB_ERR_DEVICE (no CPU fallback)."""
    import ctypes
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import komb_amd
    from komb_amd import _lib
    lib = _lib.load()
    g = komb_amd.KombAccel()
    n, k, ms = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()
    buf = np.zeros(4, np.int32)
    assert lib.komb_onion_run(g._ctx) == _lib.KOMB_ERR_DEVICE
    assert lib.komb_onion_fetch(g._ctx, _lib.ptr(buf), _lib.ptr(buf)) == _lib.KOMB_ERR_DEVICE
    assert lib.komb_onion_info(g._ctx, ctypes.byref(n), ctypes.byref(k), ctypes.byref(ms)) == _lib.KOMB_ERR_DEVICE
    with pytest.raises(komb_amd.KombError) as e:
        g.run_onion()
    assert e.value.code == _lib.KOMB_ERR_DEVICE
    g.close()
