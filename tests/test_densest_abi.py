"""CPU tests of the komb_densest_subgraph_* boundary: the four symbols are declared, exported and bound, and a context
without a graph answers KOMB_ERR_ARG to every one of them and writes nothing (a run on a loaded graph needs the GPU:
tests/test_gpu_densest.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_densest_subgraph_run", "komb_densest_subgraph_fetch", "komb_densest_subgraph_profile", "komb_densest_subgraph_info")


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
    assert re.search(r"#define\s+KOMB_ACCEL_ABI_VERSION\s+7\b", text)
    for name in ("densest_subgraph_run", "densest_subgraph_fetch", "densest_subgraph_profile", "densest_subgraph_info",
                 "run_densest_subgraph"):
        assert callable(getattr(K.KombAccel, name))
    assert "DENSEST_LOCAL" in K.api.OPTION_NAMES
    assert (K._lib.KOMB_DENSEST_CORE, K._lib.KOMB_DENSEST_PREFIX) == (0, 1)


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i32 = [ctypes.c_int32(-7) for _ in range(5)]
        i64 = [ctypes.c_int64(-7) for _ in range(5)]
        ms = ctypes.c_double(-7.0)
        buf = np.full(4, -7, np.int32)
        wide = np.full(4, -7, np.int64)
        for iters in (0, 1, 64, -1):
            assert lib.komb_densest_subgraph_run(g._ctx, iters) == ARG
        assert lib.komb_densest_subgraph_fetch(g._ctx, None, None) == ARG
        assert lib.komb_densest_subgraph_fetch(g._ctx, K._lib.ptr(buf), K._lib.ptr(buf)) == ARG
        assert lib.komb_densest_subgraph_profile(g._ctx, None, None) == ARG
        assert lib.komb_densest_subgraph_profile(g._ctx, K._lib.ptr(wide), K._lib.ptr(wide)) == ARG
        assert lib.komb_densest_subgraph_info(g._ctx, *([None] * 11)) == ARG
        assert lib.komb_densest_subgraph_info(g._ctx, ctypes.byref(i32[0]), ctypes.byref(i32[1]), ctypes.byref(i32[2]),
                                              ctypes.byref(i64[0]), ctypes.byref(i64[1]), ctypes.byref(i64[2]), ctypes.byref(i64[3]),
                                              ctypes.byref(i64[4]), ctypes.byref(i32[3]), ctypes.byref(i32[4]), ctypes.byref(ms)) == ARG
        assert [x.value for x in i32 + i64] == [-7] * 10 and ms.value == -7.0      # nothing written
        assert buf.tolist() == [-7] * 4 and wide.tolist() == [-7] * 4
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.densest_subgraph_run, lambda: g.densest_subgraph_run(0), g.densest_subgraph_fetch, g.densest_subgraph_profile,
                     g.densest_subgraph_info, g.run_densest_subgraph):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_densest_subgraph_run(None, 1) == ARG          # no context at all
