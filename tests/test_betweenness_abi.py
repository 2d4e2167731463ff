"""CPU tests of the komb_betweenness_* boundary: the four symbols are declared, exported and bound, the constant has its value,
the ABI version is unchanged, the options are forwarded, and a context without a graph answers KOMB_ERR_ARG to every one of
them and writes nothing (a run on a loaded graph needs the GPU: tests/test_gpu_betweenness.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_betweenness_run", "komb_betweenness_fetch", "komb_betweenness_fetch_sources", "komb_betweenness_info")


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def test_symbols_declared_exported_and_bound(K):
    raw = open(os.path.join(ROOT, "include", "komb_accel.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(K._lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in K._lib.SIGNATURES, name
    assert K._lib.load().komb_abi_version() == 7
    assert re.search(r"#define\s+KOMB_ACCEL_ABI_VERSION\s+7\b", text)
    for name in ("betweenness_run", "betweenness_fetch", "betweenness_fetch_sources", "betweenness_info", "run_betweenness"):
        assert callable(getattr(K.KombAccel, name))
    assert K._lib.KOMB_BETWEENNESS_ROUNDED == 1
    assert re.search(r"#define\s+KOMB_BETWEENNESS_ROUNDED\s+1\b", text)
    for name in ("BTW_GRID", "BTW_DEBUG"):
        assert name in K.api.OPTION_NAMES
        assert name in raw                                                   # the header's list of options names it


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i64 = [ctypes.c_int64(-7) for _ in range(3)]
        i32 = [ctypes.c_int32(-7) for _ in range(2)]
        ms = ctypes.c_double(-7.0)
        bc = np.full(4, -7.0)
        src, ecc = np.full(4, -7, np.int32), np.full(4, -7, np.int32)
        reached, sumd = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
        sources = np.zeros(2, np.int32)
        ptr = K._lib.ptr
        assert lib.komb_betweenness_run(g._ctx, 0, None) == ARG
        assert lib.komb_betweenness_run(g._ctx, 2, ptr(sources)) == ARG
        assert lib.komb_betweenness_fetch(g._ctx, None) == ARG
        assert lib.komb_betweenness_fetch(g._ctx, ptr(bc)) == ARG
        assert lib.komb_betweenness_fetch_sources(g._ctx, None, None, None, None) == ARG
        assert lib.komb_betweenness_fetch_sources(g._ctx, ptr(src), ptr(reached), ptr(sumd), ptr(ecc)) == ARG
        assert lib.komb_betweenness_info(g._ctx, *([None] * 6)) == ARG
        assert lib.komb_betweenness_info(g._ctx, ctypes.byref(i64[0]), ctypes.byref(i32[0]), ctypes.byref(i32[1]), ctypes.byref(i64[1]),
                                         ctypes.byref(i64[2]), ctypes.byref(ms)) == ARG
        assert [x.value for x in i64 + i32] == [-7] * 5 and ms.value == -7.0     # nothing written
        assert bc.tolist() == [-7.0] * 4 and all(a.tolist() == [-7] * 4 for a in (src, ecc, reached, sumd))
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.betweenness_run, g.betweenness_fetch, g.betweenness_fetch_sources, g.betweenness_info, g.run_betweenness):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_betweenness_run(None, 0, None) == ARG                    # no context at all
    assert lib.komb_betweenness_fetch(None, None) == ARG
    assert lib.komb_betweenness_fetch_sources(None, None, None, None, None) == ARG
    assert lib.komb_betweenness_info(None, *([None] * 6)) == ARG
