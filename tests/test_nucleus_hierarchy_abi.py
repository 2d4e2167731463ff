"""CPU tests of the komb_nucleus_hierarchy_* boundary: the seven symbols are declared, exported and bound with the header's
argument lists, the ABI version is unchanged, and a missing context or a context without a graph answers KOMB_ERR_ARG to every
one of them and writes nothing (a run on a loaded graph needs the GPU: tests/test_gpu_nucleus_hierarchy.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_nucleus_hierarchy_run", "komb_nucleus_hierarchy_count", "komb_nucleus_hierarchy_fetch_nodes",
         "komb_nucleus_hierarchy_fetch_triangles", "komb_nucleus_hierarchy_labels", "komb_nucleus_hierarchy_nuclei",
         "komb_nucleus_hierarchy_info")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def test_symbols_declared_exported_and_bound(K):
    raw = open(os.path.join(ROOT, "include", "komb_accel.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(K._lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert hasattr(lib, name), name
        assert name in K._lib.SIGNATURES, name
        restype, argtypes = K._lib.SIGNATURES[name]
        assert restype is ctypes.c_int32 or restype is ctypes.c_int
        assert len(argtypes) == len(m.group(1).split(",")), name          # as many arguments as the header declares
    assert K._lib.load().komb_abi_version() == 7
    assert re.search(r"#define\s+KOMB_ACCEL_ABI_VERSION\s+7\b", text)
    assert re.search(r"#define\s+KOMB_NUCLEUS_K_MAX\s+\(-1\)", text)
    for name in ("nucleus_hierarchy_run", "nucleus_hierarchy_fetch_nodes", "nucleus_hierarchy_fetch_triangles", "nucleus_hierarchy_labels",
                 "nucleus_hierarchy_nuclei", "nucleus_hierarchy_info", "run_nucleus_hierarchy"):
        assert callable(getattr(K.KombAccel, name))
    assert "NUC_SHORT" in K.api.OPTION_NAMES                              # the one option the run reads


def test_no_context_and_no_graph_are_argument_errors(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i64 = [ctypes.c_int64(-7) for _ in range(5)]
        i32 = [ctypes.c_int32(-7) for _ in range(2)]
        ms = ctypes.c_double(-7.0)
        bufs = [np.full(4, -7, np.int32) for _ in range(12)]
        p = [K._lib.ptr(b) for b in bufs]
        info = (ctypes.byref(i64[0]), ctypes.byref(i64[1]), ctypes.byref(i32[0]), ctypes.byref(i32[1]), ctypes.byref(i64[2]), ctypes.byref(ms))
        assert lib.komb_nucleus_hierarchy_run(g._ctx) == ARG
        assert lib.komb_nucleus_hierarchy_count(g._ctx, None) == ARG
        assert lib.komb_nucleus_hierarchy_count(g._ctx, ctypes.byref(i64[3])) == ARG
        assert lib.komb_nucleus_hierarchy_fetch_nodes(g._ctx, None, None, None, None, None) == ARG
        assert lib.komb_nucleus_hierarchy_fetch_nodes(g._ctx, *p[:5]) == ARG
        assert lib.komb_nucleus_hierarchy_fetch_triangles(g._ctx, None) == ARG
        assert lib.komb_nucleus_hierarchy_fetch_triangles(g._ctx, p[5]) == ARG
        for k in (-2, -1, 0, 1, 5):
            assert lib.komb_nucleus_hierarchy_labels(g._ctx, k, None, None) == ARG
            assert lib.komb_nucleus_hierarchy_labels(g._ctx, k, p[6], p[7]) == ARG
            assert lib.komb_nucleus_hierarchy_nuclei(g._ctx, k, 0, None, None, None, None, None) == ARG
            assert lib.komb_nucleus_hierarchy_nuclei(g._ctx, k, 4, ctypes.byref(i64[4]), *p[8:12]) == ARG
        assert lib.komb_nucleus_hierarchy_info(g._ctx, *([None] * 6)) == ARG
        assert lib.komb_nucleus_hierarchy_info(g._ctx, *info) == ARG
        assert [x.value for x in i64 + i32] == [-7] * 7 and ms.value == -7.0             # nothing written
        assert all(b.tolist() == [-7] * 4 for b in bufs)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.nucleus_hierarchy_run, g.nucleus_hierarchy_fetch_nodes, g.nucleus_hierarchy_fetch_triangles, g.nucleus_hierarchy_labels,
                     g.nucleus_hierarchy_nuclei, g.nucleus_hierarchy_info, g.run_nucleus_hierarchy):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_nucleus_hierarchy_run(None) == ARG                                   # no context at all
    assert lib.komb_nucleus_hierarchy_count(None, None) == ARG
    assert lib.komb_nucleus_hierarchy_fetch_nodes(None, None, None, None, None, None) == ARG
    assert lib.komb_nucleus_hierarchy_fetch_triangles(None, None) == ARG
    assert lib.komb_nucleus_hierarchy_labels(None, 1, None, None) == ARG
    assert lib.komb_nucleus_hierarchy_nuclei(None, 1, 0, None, None, None, None, None) == ARG
    assert lib.komb_nucleus_hierarchy_info(None, *([None] * 6)) == ARG
