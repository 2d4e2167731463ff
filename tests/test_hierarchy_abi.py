"""CPU tests of the komb_hierarchy_* boundary: the five symbols are declared, exported and bound, and a context without a
graph answers KOMB_ERR_ARG to every one of them, with and without output pointers (a run on a loaded graph needs the GPU:
tests/test_gpu_hierarchy.py)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_hierarchy_run", "komb_hierarchy_count", "komb_hierarchy_fetch_nodes", "komb_hierarchy_fetch_vertices",
         "komb_hierarchy_info")


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
    for name in ("hierarchy_run", "hierarchy_fetch_nodes", "hierarchy_fetch_vertices", "hierarchy_info", "run_hierarchy"):
        assert callable(getattr(K.KombAccel, name))


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        n, roots = ctypes.c_int64(-7), ctypes.c_int64(-7)
        kind, kmax, depth, ms = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_double(-7.0)
        for kind_arg in (0, 1, 2, -1):
            assert lib.komb_hierarchy_run(g._ctx, kind_arg) == ARG
        assert lib.komb_hierarchy_count(g._ctx, ctypes.byref(n)) == ARG
        assert lib.komb_hierarchy_count(g._ctx, None) == ARG
        assert lib.komb_hierarchy_fetch_nodes(g._ctx, None, None, None, None, None) == ARG
        assert lib.komb_hierarchy_fetch_vertices(g._ctx, None) == ARG
        assert lib.komb_hierarchy_info(g._ctx, None, None, None, None, None, None) == ARG
        assert lib.komb_hierarchy_info(g._ctx, ctypes.byref(kind), ctypes.byref(n), ctypes.byref(roots), ctypes.byref(kmax),
                                       ctypes.byref(depth), ctypes.byref(ms)) == ARG
        assert (n.value, roots.value, kind.value, kmax.value, depth.value, ms.value) == (-7, -7, -7, -7, -7, -7.0)   # nothing written
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (lambda: g.hierarchy_run("core"), lambda: g.hierarchy_run("truss"), g.hierarchy_fetch_nodes,
                     g.hierarchy_fetch_vertices, g.hierarchy_info, g.run_hierarchy):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_hierarchy_run(None, 0) == ARG          # no context at all
