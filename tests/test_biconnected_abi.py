"""CPU tests of the komb_biconnected_* boundary: the six symbols are declared, exported and bound with the header's argument
lists, the ABI version is unchanged, the option is in the header and in OPTION_NAMES, and a missing context or a context
without a graph answers KOMB_ERR_ARG to every one of them and writes nothing (a run on a loaded graph needs the GPU:
tests/test_gpu_biconnected.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_biconnected_run", "komb_biconnected_count", "komb_biconnected_fetch_edges", "komb_biconnected_fetch_vertices",
         "komb_biconnected_fetch_blocks", "komb_biconnected_info")
N_ARGS = (2, 2, 3, 4, 4, 12)
OPTIONS = ("BICONN_HEAVY",)
METHODS = ("biconnected_run", "biconnected_count", "biconnected_fetch_edges", "biconnected_fetch_vertices", "biconnected_fetch_blocks",
           "biconnected_info", "run_biconnected")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def test_symbols_declared_exported_and_bound(K):
    raw = open(os.path.join(ROOT, "include", "komb_accel.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(K._lib.LIB_PATH)
    for name, n_args in zip(NAMES, N_ARGS):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert hasattr(lib, name), name
        assert name in K._lib.SIGNATURES, name
        restype, argtypes = K._lib.SIGNATURES[name]
        assert restype is ctypes.c_int32 or restype is ctypes.c_int
        assert len(argtypes) == len(m.group(1).split(",")) == n_args, name     # as many arguments as the header declares
    assert K._lib.load().komb_abi_version() == 7
    assert re.search(r"#define\s+KOMB_ACCEL_ABI_VERSION\s+7\b", text)
    assert re.search(r"#define\s+KOMB_BICONN_K_MAX\s+\(-1\)", text) and K._lib.KOMB_BICONN_K_MAX == -1
    for name in METHODS:
        assert callable(getattr(K.KombAccel, name))
    for opt in OPTIONS:
        assert opt in K.api.OPTION_NAMES
        assert opt in raw                                                 # the header's option list names it


def test_no_context_and_no_graph_are_argument_errors(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i32 = [ctypes.c_int32(-7) for _ in range(2)]
        i64 = [ctypes.c_int64(-7) for _ in range(9)]
        ms = ctypes.c_double(-7.0)
        bufs = [np.full(4, 7, np.int32) for _ in range(8)]
        p = K._lib.ptr
        info = (ctypes.byref(i32[0]),) + tuple(ctypes.byref(x) for x in i64[:8]) + (ctypes.byref(i32[1]), ctypes.byref(ms))
        for k in (2, 3, -1, -2):
            assert lib.komb_biconnected_run(g._ctx, k) == ARG
        assert lib.komb_biconnected_count(g._ctx, None) == ARG
        assert lib.komb_biconnected_count(g._ctx, ctypes.byref(i64[8])) == ARG
        assert lib.komb_biconnected_fetch_edges(g._ctx, None, None) == ARG
        assert lib.komb_biconnected_fetch_edges(g._ctx, p(bufs[0]), p(bufs[1])) == ARG
        assert lib.komb_biconnected_fetch_vertices(g._ctx, None, None, None) == ARG
        assert lib.komb_biconnected_fetch_vertices(g._ctx, p(bufs[2]), p(bufs[3]), p(bufs[4])) == ARG
        assert lib.komb_biconnected_fetch_blocks(g._ctx, None, None, None) == ARG
        assert lib.komb_biconnected_fetch_blocks(g._ctx, p(bufs[5]), p(bufs[6]), p(bufs[7])) == ARG
        assert lib.komb_biconnected_info(g._ctx, *([None] * 11)) == ARG
        assert lib.komb_biconnected_info(g._ctx, *info) == ARG
        assert [x.value for x in i32 + i64] == [-7] * 11 and ms.value == -7.0            # nothing written
        assert all(b.tolist() == [7] * 4 for b in bufs)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for name in METHODS:
            with pytest.raises(K.KombError) as e:
                getattr(g, name)()
            assert e.value.code == ARG, name
    assert lib.komb_biconnected_run(None, 2) == ARG                                       # no context at all
    assert lib.komb_biconnected_count(None, None) == ARG
    assert lib.komb_biconnected_fetch_edges(None, None, None) == ARG
    assert lib.komb_biconnected_fetch_vertices(None, None, None, None) == ARG
    assert lib.komb_biconnected_fetch_blocks(None, None, None, None) == ARG
    assert lib.komb_biconnected_info(None, *([None] * 11)) == ARG
