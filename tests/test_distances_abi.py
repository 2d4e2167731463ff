"""CPU tests of the komb_distances_* boundary: the five symbols are declared, exported and bound, the constant has its value, the
ABI version is unchanged, the options are forwarded, and a context without a graph answers KOMB_ERR_ARG to every one of them
and writes nothing (a run on a loaded graph needs the GPU: tests/test_gpu_distances.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("komb_distances_run", "komb_distances_fetch", "komb_distances_fetch_sources", "komb_distances_histogram", "komb_distances_info")
METHODS = ("distances_run", "distances_fetch", "distances_fetch_sources", "distances_histogram", "distances_info", "run_distances")


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
    for name in METHODS:
        assert callable(getattr(K.KombAccel, name))
    assert K._lib.KOMB_DISTANCES_ALL == 1
    assert re.search(r"#define\s+KOMB_DISTANCES_ALL\s+1\b", text)
    for name in ("DIST_WORDS", "DIST_GRID", "DIST_DEBUG"):
        assert name in K.api.OPTION_NAMES
        assert name in raw                                                   # the header's list of options names it


def test_no_graph_is_an_argument_error(K):
    ARG = K._lib.KOMB_ERR_ARG
    lib = K._lib.load()
    ptr = K._lib.ptr

    def info_args():
        i64 = [ctypes.c_int64(-7) for _ in range(5)]
        i32 = [ctypes.c_int32(-7) for _ in range(3)]
        ms = ctypes.c_double(-7.0)
        args = [ctypes.byref(i64[0])] + [ctypes.byref(x) for x in i32] + [ctypes.byref(x) for x in i64[1:]] + [ctypes.byref(ms)]
        return args, i64 + i32, ms

    def check(ctx):
        harmonic = np.full(4, -7.0)
        src, ecc = np.full(4, -7, np.int32), np.full(4, -7, np.int32)
        reached, sumd, pairs = np.full(4, -7, np.int64), np.full(4, -7, np.int64), np.full(4, -7, np.int64)
        sources = np.zeros(2, np.int32)
        assert lib.komb_distances_run(ctx, 0, None) == ARG
        assert lib.komb_distances_run(ctx, 2, ptr(sources)) == ARG
        assert lib.komb_distances_fetch(ctx, None, None, None, None) == ARG
        assert lib.komb_distances_fetch(ctx, ptr(reached), ptr(sumd), ptr(ecc), ptr(harmonic)) == ARG
        assert lib.komb_distances_fetch_sources(ctx, None, None, None, None) == ARG
        assert lib.komb_distances_fetch_sources(ctx, ptr(src), ptr(reached), ptr(sumd), ptr(ecc)) == ARG
        assert lib.komb_distances_histogram(ctx, None, 0) == ARG
        assert lib.komb_distances_histogram(ctx, ptr(pairs), 4) == ARG
        assert lib.komb_distances_info(ctx, *([None] * 9)) == ARG
        args, ints, ms = info_args()
        assert lib.komb_distances_info(ctx, *args) == ARG
        assert [x.value for x in ints] == [-7] * 8 and ms.value == -7.0        # nothing written
        assert harmonic.tolist() == [-7.0] * 4 and all(a.tolist() == [-7] * 4 for a in (src, ecc, reached, sumd, pairs))

    with K.KombAccel() as g:
        check(g._ctx)
        assert b"no graph" in lib.komb_last_error(g._ctx)
        for name in METHODS:
            with pytest.raises(K.KombError) as e:
                getattr(g, name)()
            assert e.value.code == ARG
    check(None)                                                              # no context at all
