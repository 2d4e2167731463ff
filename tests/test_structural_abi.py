"""CPU tests of the komb_structural_clusters_* boundary: the four symbols are declared, exported and bound, the role
constants have their values, the ABI version is unchanged, and a context without a graph answers KOMB_ERR_ARG to every one
of them and writes nothing (a run on a loaded graph needs the GPU: tests/test_gpu_structural.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_structural_clusters_run", "komb_structural_clusters_fetch", "komb_structural_clusters_fetch_edges",
         "komb_structural_clusters_info")


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
    for name in ("structural_clusters_run", "structural_clusters_fetch", "structural_clusters_fetch_edges", "structural_clusters_info",
                 "run_structural_clusters"):
        assert callable(getattr(K.KombAccel, name))
    want = {"KOMB_SC_OUTLIER": 0, "KOMB_SC_HUB": 1, "KOMB_SC_BORDER": 2, "KOMB_SC_CORE": 3}
    for name, value in want.items():
        assert getattr(K._lib, name) == value
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
    assert "STRUCT_DEBUG" in K.api.OPTION_NAMES


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        i32 = [ctypes.c_int32(-7) for _ in range(3)]
        i64 = [ctypes.c_int64(-7) for _ in range(7)]
        ms = ctypes.c_double(-7.0)
        bufs = [np.full(4, -7, np.int32) for _ in range(5)]
        for args in ((7, 10, 3), (1, 1, 2), (0, 10, 3), (7, 10, 1), (11, 10, 3)):
            assert lib.komb_structural_clusters_run(g._ctx, *args) == ARG
        assert lib.komb_structural_clusters_fetch(g._ctx, None, None, None, None) == ARG
        assert lib.komb_structural_clusters_fetch(g._ctx, *(K._lib.ptr(b) for b in bufs[:4])) == ARG
        assert lib.komb_structural_clusters_fetch_edges(g._ctx, None) == ARG
        assert lib.komb_structural_clusters_fetch_edges(g._ctx, K._lib.ptr(bufs[4])) == ARG
        assert lib.komb_structural_clusters_info(g._ctx, *([None] * 11)) == ARG
        assert lib.komb_structural_clusters_info(g._ctx, *(ctypes.byref(x) for x in i32 + i64), ctypes.byref(ms)) == ARG
        assert [x.value for x in i32 + i64] == [-7] * 10 and ms.value == -7.0      # nothing written
        assert all(b.tolist() == [-7] * 4 for b in bufs)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.structural_clusters_run, lambda: g.structural_clusters_run(1, 2, 2), g.structural_clusters_fetch,
                     g.structural_clusters_fetch_edges, g.structural_clusters_info, g.run_structural_clusters):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_structural_clusters_run(None, 7, 10, 3) == ARG          # no context at all
    assert lib.komb_structural_clusters_fetch(None, None, None, None, None) == ARG
    assert lib.komb_structural_clusters_fetch_edges(None, None) == ARG
    assert lib.komb_structural_clusters_info(None, *([None] * 11)) == ARG
