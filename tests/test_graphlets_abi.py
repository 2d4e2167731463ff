"""CPU tests of the komb_graphlets_* boundary: the four symbols are declared, exported and bound, the constants have their
values, the ABI version is unchanged, the options are forwarded, and a context without a graph answers KOMB_ERR_ARG to
every one of them and writes nothing (a run on a loaded graph needs the GPU: tests/test_gpu_graphlets.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_graphlets_run", "komb_graphlets_fetch_vertices", "komb_graphlets_fetch_edges", "komb_graphlets_info")


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
    for name in ("graphlets_run", "graphlets_fetch_vertices", "graphlets_fetch_edges", "graphlets_info", "run_graphlets"):
        assert callable(getattr(K.KombAccel, name))
    want = {"KOMB_GRAPHLET_ORBITS": 15, "KOMB_GRAPHLET_TYPES": 9, "KOMB_GRAPHLET_SATURATED": 1}
    for name, value in want.items():
        assert getattr(K._lib, name) == value
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
    for name in ("GRAPHLET_LDS", "GRAPHLET_SHORT", "GRAPHLET_DEBUG"):
        assert name in K.api.OPTION_NAMES
    assert len(K.KombAccel.GRAPHLET_TYPES) == 9


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    with K.KombAccel() as g:
        total = (ctypes.c_uint64 * 9)(*([7] * 9))
        i32 = [ctypes.c_int32(-7) for _ in range(2)]
        i64 = [ctypes.c_int64(-7) for _ in range(3)]
        ms = ctypes.c_double(-7.0)
        bufs = [np.full(15, 7, np.uint64) for _ in range(3)]
        assert lib.komb_graphlets_run(g._ctx) == ARG
        assert lib.komb_graphlets_fetch_vertices(g._ctx, None) == ARG
        assert lib.komb_graphlets_fetch_vertices(g._ctx, K._lib.ptr(bufs[0])) == ARG
        assert lib.komb_graphlets_fetch_edges(g._ctx, None, None) == ARG
        assert lib.komb_graphlets_fetch_edges(g._ctx, K._lib.ptr(bufs[1]), K._lib.ptr(bufs[2])) == ARG
        assert lib.komb_graphlets_info(g._ctx, *([None] * 7)) == ARG
        assert lib.komb_graphlets_info(g._ctx, total, *(ctypes.byref(x) for x in i32 + i64), ctypes.byref(ms)) == ARG
        assert list(total) == [7] * 9 and [x.value for x in i32 + i64] == [-7] * 5 and ms.value == -7.0      # nothing written
        assert all(b.tolist() == [7] * 15 for b in bufs)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for call in (g.graphlets_run, g.graphlets_fetch_vertices, g.graphlets_fetch_edges, g.graphlets_info, g.run_graphlets):
            with pytest.raises(K.KombError) as e:
                call()
            assert e.value.code == ARG
    assert lib.komb_graphlets_run(None) == ARG                              # no context at all
    assert lib.komb_graphlets_fetch_vertices(None, None) == ARG
    assert lib.komb_graphlets_fetch_edges(None, None, None) == ARG
    assert lib.komb_graphlets_info(None, *([None] * 7)) == ARG
