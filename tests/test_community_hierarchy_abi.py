"""CPU tests of the komb_community_hierarchy_* boundary: the six symbols are declared, exported and bound, and a context
without a graph answers KOMB_ERR_ARG to every one of them, with and without output pointers (a run on a loaded graph needs
the GPU: tests/test_gpu_community_hierarchy.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_community_hierarchy_run", "komb_community_hierarchy_count", "komb_community_hierarchy_fetch_nodes",
         "komb_community_hierarchy_fetch_edges", "komb_community_hierarchy_labels", "komb_community_hierarchy_info")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def test_symbols_declared_exported_and_bound(K):
    text = open(os.path.join(ROOT, "include", "komb_accel.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(K._lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in K._lib.SIGNATURES, name
    assert K._lib.load().komb_abi_version() == 7
    for name in ("community_hierarchy_run", "community_hierarchy_fetch_nodes", "community_hierarchy_fetch_edges",
                 "community_hierarchy_labels", "community_hierarchy_info", "run_community_hierarchy"):
        assert callable(getattr(K.KombAccel, name))


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        n, roots, mem = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
        kmax, depth, ms = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_double(-7.0)
        out = [np.full(4, -7, np.int32) for _ in range(5)]
        assert lib.komb_community_hierarchy_run(g._ctx) == ARG
        assert lib.komb_community_hierarchy_count(g._ctx, ctypes.byref(n)) == ARG
        assert lib.komb_community_hierarchy_count(g._ctx, None) == ARG
        assert lib.komb_community_hierarchy_fetch_nodes(g._ctx, None, None, None, None, None) == ARG
        assert lib.komb_community_hierarchy_fetch_nodes(g._ctx, *(K._lib.ptr(x) for x in out)) == ARG
        assert lib.komb_community_hierarchy_fetch_edges(g._ctx, None) == ARG
        assert lib.komb_community_hierarchy_fetch_edges(g._ctx, K._lib.ptr(out[0])) == ARG
        for k in (-2, -1, 0, 3, 1000):
            assert lib.komb_community_hierarchy_labels(g._ctx, k, None, None) == ARG
            assert lib.komb_community_hierarchy_labels(g._ctx, k, K._lib.ptr(out[0]), K._lib.ptr(out[1])) == ARG
        assert lib.komb_community_hierarchy_info(g._ctx, None, None, None, None, None, None) == ARG
        assert lib.komb_community_hierarchy_info(g._ctx, ctypes.byref(n), ctypes.byref(roots), ctypes.byref(kmax), ctypes.byref(depth),
                                                 ctypes.byref(mem), ctypes.byref(ms)) == ARG
        assert (n.value, roots.value, mem.value, kmax.value, depth.value, ms.value) == (-7, -7, -7, -7, -7, -7.0)   # nothing written
        assert all((x == -7).all() for x in out)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.community_hierarchy_run, g.community_hierarchy_fetch_nodes, g.community_hierarchy_fetch_edges,
                     lambda: g.community_hierarchy_labels(3), g.community_hierarchy_info, g.run_community_hierarchy):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    for name in NAMES:                                       # no context at all
        args = {"komb_community_hierarchy_run": (), "komb_community_hierarchy_count": (None,),
                "komb_community_hierarchy_fetch_nodes": (None,) * 5, "komb_community_hierarchy_fetch_edges": (None,),
                "komb_community_hierarchy_labels": (3, None, None), "komb_community_hierarchy_info": (None,) * 6}[name]
        assert getattr(lib, name)(None, *args) == ARG
