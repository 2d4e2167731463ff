"""CPU tests of the komb_clique_communities_* boundary: the six symbols are declared, exported and bound with the header's
argument lists, the ABI version is unchanged, the two options are in the header and in OPTION_NAMES, and a missing context or a
context without a graph answers KOMB_ERR_ARG to every one of them and writes nothing (a run on a loaded graph needs the GPU:
tests/test_gpu_clique_communities.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_clique_communities_run", "komb_clique_communities_count", "komb_clique_communities_fetch",
         "komb_clique_communities_fetch_communities", "komb_clique_communities_fetch_vertices", "komb_clique_communities_info")
N_ARGS = (3, 3, 3, 5, 3, 10)
OPTIONS = ("PERC_GROUP", "PERC_DEBUG")
METHODS = ("clique_communities_run", "clique_communities_count", "clique_communities_fetch", "clique_communities_fetch_communities",
           "clique_communities_fetch_vertices", "clique_communities_info", "run_clique_communities")


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
    for name in METHODS:
        assert callable(getattr(K.KombAccel, name))
    for opt in OPTIONS:
        assert opt in K.api.OPTION_NAMES
        assert opt in raw                                                 # the header's option list names them


def test_no_context_and_no_graph_are_argument_errors(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i32 = [ctypes.c_int32(-7) for _ in range(2)]
        i64 = [ctypes.c_int64(-7) for _ in range(8)]
        ms = ctypes.c_double(-7.0)
        offset = np.full(4, 7, np.int64)
        bufs = [np.full(4, 7, np.int32) for _ in range(7)]
        p = K._lib.ptr
        info = tuple(ctypes.byref(x) for x in i32 + i64[:6]) + (ctypes.byref(ms),)
        assert lib.komb_clique_communities_run(g._ctx, 3, 0) == ARG
        assert lib.komb_clique_communities_run(g._ctx, 3, -1) == ARG
        assert lib.komb_clique_communities_run(g._ctx, 1, 0) == ARG
        assert lib.komb_clique_communities_count(g._ctx, None, None) == ARG
        assert lib.komb_clique_communities_count(g._ctx, ctypes.byref(i64[6]), ctypes.byref(i64[7])) == ARG
        assert lib.komb_clique_communities_fetch(g._ctx, None, None) == ARG
        assert lib.komb_clique_communities_fetch(g._ctx, p(bufs[0]), p(bufs[1])) == ARG
        assert lib.komb_clique_communities_fetch_communities(g._ctx, None, None, None, None) == ARG
        assert lib.komb_clique_communities_fetch_communities(g._ctx, p(bufs[2]), p(bufs[3]), p(offset), p(bufs[4])) == ARG
        assert lib.komb_clique_communities_fetch_vertices(g._ctx, None, None) == ARG
        assert lib.komb_clique_communities_fetch_vertices(g._ctx, p(bufs[5]), p(bufs[6])) == ARG
        assert lib.komb_clique_communities_info(g._ctx, *([None] * 9)) == ARG
        assert lib.komb_clique_communities_info(g._ctx, *info) == ARG
        assert [x.value for x in i32 + i64] == [-7] * 10 and ms.value == -7.0            # nothing written
        assert all(b.tolist() == [7] * 4 for b in bufs + [offset])
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for name in METHODS:
            with pytest.raises(K.KombError) as e:
                getattr(g, name)()
            assert e.value.code == ARG, name
    assert lib.komb_clique_communities_run(None, 3, 0) == ARG                             # no context at all
    assert lib.komb_clique_communities_count(None, None, None) == ARG
    assert lib.komb_clique_communities_fetch(None, None, None) == ARG
    assert lib.komb_clique_communities_fetch_communities(None, None, None, None, None) == ARG
    assert lib.komb_clique_communities_fetch_vertices(None, None, None) == ARG
    assert lib.komb_clique_communities_info(None, *([None] * 9)) == ARG
