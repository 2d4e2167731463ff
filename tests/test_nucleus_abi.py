"""CPU tests of the komb_nucleus_* boundary: the six symbols are declared, exported and bound with the header's argument
lists, the ABI version is unchanged, the options are forwarded, and a missing context or a context without a graph answers
KOMB_ERR_ARG to every one of them and writes nothing (a run on a loaded graph needs the GPU: tests/test_gpu_nucleus.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_nucleus_run", "komb_nucleus_count", "komb_nucleus_fetch", "komb_nucleus_fetch_edges", "komb_nucleus_fetch_vertices",
         "komb_nucleus_info")


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
    for name in ("nucleus_run", "nucleus_fetch", "nucleus_fetch_edges", "nucleus_fetch_vertices", "nucleus_info", "run_nucleus"):
        assert callable(getattr(K.KombAccel, name))
    for opt in ("NUC_SHORT", "NUC_HEAVY", "NUC_CAP", "NUC_DEBUG"):
        assert opt in K.api.OPTION_NAMES
        assert opt in raw                                                 # the header's option list names them


def test_no_context_and_no_graph_are_argument_errors(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        n = ctypes.c_int64(-7)
        i64 = [ctypes.c_int64(-7) for _ in range(3)]
        i32 = [ctypes.c_int32(-7) for _ in range(2)]
        ms = ctypes.c_double(-7.0)
        bufs = [np.full(4, -7, np.int32) for _ in range(7)]
        info = (ctypes.byref(i64[0]), ctypes.byref(i64[1]), ctypes.byref(i32[0]), ctypes.byref(i32[1]), ctypes.byref(i64[2]), ctypes.byref(ms))
        assert lib.komb_nucleus_run(g._ctx) == ARG
        assert lib.komb_nucleus_count(g._ctx, None) == ARG
        assert lib.komb_nucleus_count(g._ctx, ctypes.byref(n)) == ARG
        assert lib.komb_nucleus_fetch(g._ctx, None, None, None, None, None) == ARG
        assert lib.komb_nucleus_fetch(g._ctx, *(K._lib.ptr(b) for b in bufs[:5])) == ARG
        assert lib.komb_nucleus_fetch_edges(g._ctx, None) == ARG
        assert lib.komb_nucleus_fetch_edges(g._ctx, K._lib.ptr(bufs[5])) == ARG
        assert lib.komb_nucleus_fetch_vertices(g._ctx, None) == ARG
        assert lib.komb_nucleus_fetch_vertices(g._ctx, K._lib.ptr(bufs[6])) == ARG
        assert lib.komb_nucleus_info(g._ctx, *([None] * 6)) == ARG
        assert lib.komb_nucleus_info(g._ctx, *info) == ARG
        assert [x.value for x in [n] + i64 + i32] == [-7] * 6 and ms.value == -7.0       # nothing written
        assert all(b.tolist() == [-7] * 4 for b in bufs)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.nucleus_run, g.nucleus_fetch, g.nucleus_fetch_edges, g.nucleus_fetch_vertices, g.nucleus_info, g.run_nucleus):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_nucleus_run(None) == ARG                                             # no context at all
    assert lib.komb_nucleus_count(None, None) == ARG
    assert lib.komb_nucleus_fetch(None, None, None, None, None, None) == ARG
    assert lib.komb_nucleus_fetch_edges(None, None) == ARG
    assert lib.komb_nucleus_fetch_vertices(None, None) == ARG
    assert lib.komb_nucleus_info(None, *([None] * 6)) == ARG
