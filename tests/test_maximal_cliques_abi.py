"""CPU tests of the komb_maximal_cliques_* boundary: the four symbols are declared, exported and bound with the header's argument
lists, the ABI version is unchanged, the flag macros and the options are in the header, and a missing context or a context
without a graph answers KOMB_ERR_ARG to every one of them and writes nothing (a run on a loaded graph needs the GPU:
tests/test_gpu_maximal_cliques.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_maximal_cliques_run", "komb_maximal_cliques_fetch", "komb_maximal_cliques_list", "komb_maximal_cliques_info")
OPTIONS = ("MAXIMAL_LDS", "MAXIMAL_PIVOT", "MAXIMAL_LIST", "MAXIMAL_DEBUG")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def test_symbols_declared_exported_and_bound(K):
    raw = open(os.path.join(ROOT, "include", "komb_accel.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(K._lib.LIB_PATH)
    for name, n_args in zip(NAMES, (3, 4, 7, 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert hasattr(lib, name), name
        assert name in K._lib.SIGNATURES, name
        restype, argtypes = K._lib.SIGNATURES[name]
        assert restype is ctypes.c_int32 or restype is ctypes.c_int
        assert len(argtypes) == len(m.group(1).split(",")) == n_args, name     # as many arguments as the header declares
    assert K._lib.load().komb_abi_version() == 7
    assert re.search(r"#define\s+KOMB_ACCEL_ABI_VERSION\s+7\b", text)
    for macro, value in (("KOMB_MAXIMAL_COMPLETE", 1), ("KOMB_MAXIMAL_LISTED", 2)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", text), macro
        assert getattr(K._lib, macro) == value
    for name in ("maximal_cliques_run", "maximal_cliques_fetch", "maximal_cliques_list", "maximal_cliques_info", "run_maximal_cliques"):
        assert callable(getattr(K.KombAccel, name))
    for opt in OPTIONS:
        assert opt in K.api.OPTION_NAMES
        assert opt in raw                                                 # the header's option list names them


def test_no_context_and_no_graph_are_argument_errors(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i32 = [ctypes.c_int32(-7) for _ in range(6)]
        i64 = [ctypes.c_int64(-7) for _ in range(5)]
        ms = ctypes.c_double(-7.0)
        hist, offset = np.full(4, 7, np.int64), np.full(4, 7, np.int64)
        bufs = [np.full(4, 7, np.int32) for _ in range(3)]
        info = tuple(ctypes.byref(x) for x in i32[:5] + [i64[0], i32[5]] + i64[1:3]) + (ctypes.byref(ms),)
        assert lib.komb_maximal_cliques_run(g._ctx, 2, 0) == ARG
        assert lib.komb_maximal_cliques_run(g._ctx, 2, -1) == ARG
        assert lib.komb_maximal_cliques_run(g._ctx, 1, 0) == ARG
        assert lib.komb_maximal_cliques_fetch(g._ctx, None, None, None) == ARG
        assert lib.komb_maximal_cliques_fetch(g._ctx, K._lib.ptr(hist), K._lib.ptr(bufs[0]), K._lib.ptr(bufs[1])) == ARG
        assert lib.komb_maximal_cliques_list(g._ctx, 0, 0, None, None, None, None) == ARG
        assert lib.komb_maximal_cliques_list(g._ctx, 3, 4, ctypes.byref(i64[3]), ctypes.byref(i64[4]), K._lib.ptr(offset), K._lib.ptr(bufs[2])) == ARG
        assert lib.komb_maximal_cliques_info(g._ctx, *([None] * 10)) == ARG
        assert lib.komb_maximal_cliques_info(g._ctx, *info) == ARG
        assert [x.value for x in i32 + i64] == [-7] * 11 and ms.value == -7.0            # nothing written
        assert all(b.tolist() == [7] * 4 for b in bufs + [hist, offset])
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.maximal_cliques_run, g.maximal_cliques_fetch, g.maximal_cliques_list, g.maximal_cliques_info, g.run_maximal_cliques):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_maximal_cliques_run(None, 2, 0) == ARG                                # no context at all
    assert lib.komb_maximal_cliques_fetch(None, None, None, None) == ARG
    assert lib.komb_maximal_cliques_list(None, 0, 0, None, None, None, None) == ARG
    assert lib.komb_maximal_cliques_info(None, *([None] * 10)) == ARG
