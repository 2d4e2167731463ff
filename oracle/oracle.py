"""ctypes binding of oracle/liboracle.so -- the CPU checker.

TEST INFRASTRUCTURE ONLY: importable from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg; never from komb_amd/ (the product).  See
komb_oracle.h for the parity status of each half ("parity unpinned" for the
igraph half; CoreA half pinned by oracle/_ref/corea_ref).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_i64 = ctypes.c_int64


def build():
    """Compile liboracle.so (and oracle/_ref when /root/reference is present)."""
    subprocess.run(["make", "-s", "-C", _HERE, "all"], check=True)


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "liboracle.so")
        if not os.path.exists(path):
            build()
        L = ctypes.CDLL(path)
        L.orc_simplify.restype = _i64
        L.orc_simplify.argtypes = [_i64, _i64, _i64p, _i64p, _i32p]
        L.orc_degree.restype = None
        L.orc_degree.argtypes = [_i64, _i64p, _i32p]
        L.orc_coreness.restype = ctypes.c_int32
        L.orc_coreness.argtypes = [_i64, _i64p, _i32p, _i32p]
        L.orc_induced_subgraph.restype = _i64
        L.orc_induced_subgraph.argtypes = [_i64, _i64p, _i32p, _u8p, _i64p, _i32p, _i32p]
        L.orc_edge_list.restype = _i64
        L.orc_edge_list.argtypes = [_i64, _i64p, _i32p, _i32p, _i32p]
        L.orc_support.restype = _i64
        L.orc_support.argtypes = [_i64, _i64p, _i32p, _i32p]
        L.orc_trussness.restype = ctypes.c_int32
        L.orc_trussness.argtypes = [_i64, _i64p, _i32p, _i32p]
        L.orc_fractional_rank_faithful.restype = None
        L.orc_fractional_rank_faithful.argtypes = [_f64p, _i64, _f64p]
        L.orc_fractional_rank_fast.restype = None
        L.orc_fractional_rank_fast.argtypes = [_i64p, _i64, _f64p]
        L.orc_corea_scores.restype = None
        L.orc_corea_scores.argtypes = [_i32p, _i32p, _i64, ctypes.c_int, _f64p]
        L.orc_run_merge.restype = ctypes.c_int32
        L.orc_run_merge.argtypes = [_i64, _i64p, _i32p, ctypes.c_void_p, _i32p, _i32p, ctypes.POINTER(ctypes.c_double)]
        _vp = ctypes.c_void_p
        L.orc_clique_census.restype = ctypes.c_int32
        L.orc_clique_census.argtypes = [_i64, _i64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _vp,
                                        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
        L.orc_maximal_cliques.restype = _i64
        L.orc_maximal_cliques.argtypes = [_i64, _i64p, _i32p, ctypes.c_int32, ctypes.c_int32, _i64p, _i32p, _i32p,
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)]
        L.orc_free.restype = None
        L.orc_free.argtypes = [_vp]
        L.orc_nucleus_count.restype = _i64
        L.orc_nucleus_count.argtypes = [_i64, _i64p, _i32p, ctypes.POINTER(_i64)]
        L.orc_nucleus.restype = ctypes.c_int32
        L.orc_nucleus.argtypes = [_i64, _i64p, _i32p, _i64, _i64] + [_i32p] * 8
        L.orc_bfs_sources.restype = ctypes.c_int32
        L.orc_bfs_sources.argtypes = [_i64, _i64p, _i32p, _i64, _i32p, _i64p, _i64p, _i32p, _i64p, _i64p, _i32p, _f64p, _i64p]
        L.orc_betweenness.restype = ctypes.c_int32
        L.orc_betweenness.argtypes = [_i64, _i64p, _i32p, _i64, _i32p, _f64p, _i64p, _i64p, _i32p, ctypes.POINTER(ctypes.c_int32)]
        L.orc_graphlets.restype = ctypes.c_int32
        L.orc_graphlets.argtypes = [_i64, _i64p, _i32p, _u64p, _u64p, _u64p, _i64p]
        L.orc_orbits_by_definition.restype = _i64
        L.orc_orbits_by_definition.argtypes = [_i64, _i64p, _i32p, ctypes.c_int32, _i64, _u64p]
        _LIB = L
    return _LIB


_NATIVE = None


def native_lib():
    """liboracle built for THIS machine (-march=native, OpenMP): bench.py's CPU baseline.  None if it cannot be built."""
    global _NATIVE
    if _NATIVE is None:
        path = os.path.join(_HERE, "_native", "liboracle_native.so")
        try:
            subprocess.run(["make", "-s", "-C", _HERE, "native"], check=True, stdout=subprocess.DEVNULL)
            L = ctypes.CDLL(path)
            for name in ("orc_trussness", "orc_trussness_omp"):
                getattr(L, name).restype = ctypes.c_int32
            L.orc_trussness.argtypes = [_i64, _i64p, _i32p, _i32p]
            L.orc_trussness_omp.argtypes = [_i64, _i64p, _i32p, _i32p, ctypes.c_int]
            _NATIVE = L
        except (OSError, subprocess.CalledProcessError):
            _NATIVE = False
    return _NATIVE or None


def trussness_native(rowptr, col, threads=1):
    """orc_trussness (threads == 1) or orc_trussness_omp from the native build."""
    L = native_lib()
    if L is None:
        raise RuntimeError("native oracle build unavailable")
    nv = len(rowptr) - 1
    ne = int(rowptr[nv]) // 2
    t = np.zeros(max(ne, 1), dtype=np.int32)
    if threads == 1:
        L.orc_trussness(nv, rowptr, _colbuf(col), t)
    else:
        L.orc_trussness_omp(nv, rowptr, _colbuf(col), t, int(threads))
    return t[:ne]


def ref_corea_path():
    p = os.path.join(_HERE, "_ref", "corea_ref")
    return p if os.path.exists(p) else None


# ------------------------------------------------------------------ wrappers
def simplify(nv, uv):
    """a1: raw (u,v) pairs [n_raw,2] int64 -> (rowptr int64[nv+1], col int32[2*ne])."""
    uv = np.ascontiguousarray(np.asarray(uv, dtype=np.int64).reshape(-1, 2))
    n_raw = uv.shape[0]
    rowptr = np.zeros(nv + 1, dtype=np.int64)
    col = np.zeros(max(2 * n_raw, 1), dtype=np.int32)
    ne = lib().orc_simplify(nv, n_raw, uv.reshape(-1), rowptr, col)
    if ne < 0:
        raise ValueError("orc_simplify: bad input")
    return rowptr, np.ascontiguousarray(col[: 2 * ne])


def degree(rowptr):
    nv = len(rowptr) - 1
    d = np.zeros(max(nv, 1), dtype=np.int32)
    lib().orc_degree(nv, rowptr, d)
    return d[:nv]


def _colbuf(col):
    return col if len(col) else np.zeros(1, dtype=np.int32)


def coreness(rowptr, col):
    nv = len(rowptr) - 1
    c = np.zeros(max(nv, 1), dtype=np.int32)
    lib().orc_coreness(nv, rowptr, _colbuf(col), c)
    return c[:nv]


def edge_list(rowptr, col):
    nv = len(rowptr) - 1
    ne = int(rowptr[nv]) // 2
    eu = np.zeros(max(ne, 1), dtype=np.int32)
    ev = np.zeros(max(ne, 1), dtype=np.int32)
    lib().orc_edge_list(nv, rowptr, _colbuf(col), eu, ev)
    return eu[:ne], ev[:ne]


def support(rowptr, col):
    nv = len(rowptr) - 1
    ne = int(rowptr[nv]) // 2
    s = np.zeros(max(ne, 1), dtype=np.int32)
    t = lib().orc_support(nv, rowptr, _colbuf(col), s)
    return s[:ne], int(t)


def trussness(rowptr, col):
    nv = len(rowptr) - 1
    ne = int(rowptr[nv]) // 2
    t = np.zeros(max(ne, 1), dtype=np.int32)
    lib().orc_trussness(nv, rowptr, _colbuf(col), t)
    return t[:ne]


def induced_subgraph(rowptr, col, vmask):
    nv = len(rowptr) - 1
    vmask = np.ascontiguousarray(vmask, dtype=np.uint8)
    srp = np.zeros(nv + 1, dtype=np.int64)
    scol = np.zeros(max(len(col), 1), dtype=np.int32)
    inv = np.zeros(max(nv, 1), dtype=np.int32)
    ns = lib().orc_induced_subgraph(nv, rowptr, _colbuf(col), vmask, srp, scol, inv)
    srp = np.ascontiguousarray(srp[: ns + 1])
    return srp, np.ascontiguousarray(scol[: int(srp[ns])]), inv[:ns]


def trussness_induced(rowptr, col, vmask):
    """a5+a6 as KOMB's runTruss composes them (src/graph.cpp:502,508,529-532):
    returns (eu, ev, truss) with ORIGINAL vertex ids, canonical order."""
    srp, scol, inv = induced_subgraph(rowptr, col, vmask)
    t = trussness(srp, scol)
    su, sv = edge_list(srp, scol)
    return inv[su].astype(np.int32), inv[sv].astype(np.int32), t


def fractional_rank_faithful(scores):
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    out = np.zeros(max(len(scores), 1), dtype=np.float64)
    lib().orc_fractional_rank_faithful(scores if len(scores) else out, len(scores), out)
    return out[: len(scores)]


def fractional_rank_fast(keys):
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    out = np.zeros(max(len(keys), 1), dtype=np.float64)
    lib().orc_fractional_rank_fast(keys if len(keys) else np.zeros(1, np.int64), len(keys), out)
    return out[: len(keys)]


def corea_scores(deg, core, faithful=False):
    deg = np.ascontiguousarray(deg, dtype=np.int32)
    core = np.ascontiguousarray(core, dtype=np.int32)
    n = len(deg)
    out = np.zeros(max(n, 1), dtype=np.float64)
    if n:
        lib().orc_corea_scores(deg, core, n, 1 if faithful else 0, out)
    return out[:n]


def ref_corea_scores(deg, core):
    """Scores from the REFERENCE's own CoreA.h (oracle/_ref/corea_ref)."""
    exe = ref_corea_path()
    if exe is None:
        raise FileNotFoundError("oracle/_ref/corea_ref not built")
    text = "%d\n" % len(deg) + "".join("%d %d\n" % (int(d), int(c)) for d, c in zip(deg, core))
    out = subprocess.run([exe, "arrays"], input=text, capture_output=True, text=True, check=True).stdout
    return np.array([float(x) for x in out.split()], dtype=np.float64)


def run_merge(rowptr, col, susp=None):
    """a12 + a13: the greedy densest-block peel of CombineCoreA::runMerge over its indexed min-heaps.
    Returns (order int32[2*nv], side int32[2*nv], n_block, max_density)."""
    nv = len(rowptr) - 1
    order = np.zeros(max(2 * nv, 1), dtype=np.int32)
    side = np.zeros(max(2 * nv, 1), dtype=np.int32)
    dens = ctypes.c_double(0.0)
    sp = None
    if susp is not None:
        susp = np.ascontiguousarray(susp, dtype=np.float64)
        sp = susp.ctypes.data_as(ctypes.c_void_p)
    nb = lib().orc_run_merge(nv, rowptr, _colbuf(col), sp, order, side, ctypes.byref(dens))
    return order[: 2 * nv], side[: 2 * nv], int(nb), float(dens.value)


def ref_merge_path():
    p = os.path.join(_HERE, "_ref", "merge_ref")
    return p if os.path.exists(p) else None


def ref_run_merge(rowptr, col, susp=None):
    """The same from the REFERENCE's own HashIndexedMinHeap.h (oracle/_ref/merge_ref: its class under a restatement of the loop)."""
    import tempfile
    exe = ref_merge_path()
    if exe is None:
        raise FileNotFoundError("oracle/_ref/merge_ref not built")
    nv = len(rowptr) - 1
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        np.array([nv, len(col)], dtype=np.int64).tofile(f)
        np.asarray(rowptr, dtype=np.int64).tofile(f)
        np.asarray(col, dtype=np.int32).tofile(f)
        np.array([0 if susp is None else 1], dtype=np.int64).tofile(f)
        if susp is not None:
            np.asarray(susp, dtype=np.float64).tofile(f)
        f.flush()
        out = subprocess.run([exe, f.name], capture_output=True, text=True, check=True).stdout.split()
    nb, dens = int(out[0]), float(out[1])
    rest = np.array(out[2:], dtype=np.int64).reshape(-1, 2)
    return rest[:, 0].astype(np.int32), rest[:, 1].astype(np.int32), nb, dens


# ------------------------------------------------ cliques and nuclei (komb_oracle.h: vertex-rooted, sorted arrays, no trussness)
SAT = 2 ** 64 - 1


def _csr(rowptr, col):
    return np.ascontiguousarray(rowptr, dtype=np.int64), _colbuf(np.ascontiguousarray(col, dtype=np.int32))


def t_max(rowptr, col):
    """The largest trussness (0 without an edge): what sizes the windows of the clique analyses.  From orc_trussness."""
    t = trussness(*_csr(rowptr, col))
    return int(t.max()) if len(t) else 0


def _k_cap(rowptr):
    """No clique has more vertices than the largest degree + 1."""
    return int(np.diff(rowptr).max()) + 2 if len(rowptr) > 1 else 2


def clique_counts(rowptr, col, k_local=0):
    """orc_clique_census as it is: {"total": uint64[k_cap + 1] indexed by k, "local": uint64[nv] or None, "clique_number",
    "nodes", "seconds"}."""
    import time
    rowptr, col = _csr(rowptr, col)
    nv = len(rowptr) - 1
    k_cap = _k_cap(rowptr)
    total = np.zeros(k_cap + 1, dtype=np.uint64)
    local = np.zeros(max(nv, 1), dtype=np.uint64) if k_local else None
    sat, nodes = ctypes.c_int32(), ctypes.c_uint64()
    t0 = time.perf_counter()
    omega = lib().orc_clique_census(nv, rowptr, col, k_cap, k_local, total, None if local is None else local.ctypes.data,
                                    ctypes.byref(sat), ctypes.byref(nodes))
    if omega < 0:
        raise ValueError("orc_clique_census: bad arguments")
    return {"total": total, "local": None if local is None else local[:nv], "clique_number": int(omega), "nodes": int(nodes.value),
            "seconds": time.perf_counter() - t0}


def census_window(counts, tmax, k_lo=2, k_hi=-1, k_local=0):
    """What komb_clique_census_run reports for a window, from clique_counts(k_local) of the same graph and its t_max:
    {"k_lo", "k_hi" (as used), "k_local", "t_max", "omega", "flags", "total", "local"}.  ValueError where the library answers
    KOMB_ERR_ARG."""
    if k_lo < 2 or (k_hi != -1 and k_hi < k_lo) or k_local < 0:
        raise ValueError("bad window")
    if k_hi == -1 or k_hi > tmax:
        k_hi = max(tmax, k_lo)
    if k_local and not k_lo <= k_local <= k_hi:
        raise ValueError("k_local outside the window")
    assert (counts["local"] is not None) == bool(k_local)
    all_k = counts["total"]
    assert counts["clique_number"] <= tmax < len(all_k)
    total = np.zeros(k_hi - k_lo + 1, dtype=np.uint64)
    n = max(min(k_hi + 1, len(all_k)) - k_lo, 0)
    total[:n] = all_k[k_lo:k_lo + n]
    local = counts["local"].copy() if k_local else None
    sat = bool((total == SAT).any()) or (k_local and bool((local == SAT).any()))
    nz = np.flatnonzero(total)
    return {"k_lo": k_lo, "k_hi": k_hi, "k_local": k_local, "t_max": tmax, "omega": int(nz[-1]) + k_lo if len(nz) else 0,
            "flags": 1 | (2 if sat else 0), "total": total, "local": local}


def clique_census(rowptr, col, k_lo=2, k_hi=-1, k_local=0, tmax=None):
    """One census of a symmetric CSR as komb_clique_census_run defines it (see census_window)."""
    tmax = t_max(rowptr, col) if tmax is None else tmax
    kl = k_local if k_local >= 0 else 0
    return census_window(clique_counts(rowptr, col, kl), tmax, k_lo, k_hi, k_local)


def maximal_cliques_all(rowptr, col, k_min=2, want_list=True):
    """orc_maximal_cliques as it is: {"hist_all": int64[k_cap + 1] indexed by size (every size), "count", "largest": int32[nv],
    "omega", "n_cliques", "offset": int64[n + 1], "verts": int32 (None, None without the list), "nodes", "seconds"}; count,
    largest, omega and the list cover the cliques of >= k_min vertices."""
    import time
    rowptr, col = _csr(rowptr, col)
    nv = len(rowptr) - 1
    k_cap = _k_cap(rowptr)
    hist = np.zeros(k_cap + 1, dtype=np.int64)
    count = np.zeros(max(nv, 1), dtype=np.int32)
    largest = np.zeros(max(nv, 1), dtype=np.int32)
    omega, nodes, n_verts = ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int64()
    p_off, p_verts = ctypes.c_void_p(), ctypes.c_void_p()
    t0 = time.perf_counter()
    n = lib().orc_maximal_cliques(nv, rowptr, col, k_min, k_cap, hist, count, largest, ctypes.byref(omega), ctypes.byref(nodes),
                                  ctypes.byref(p_off) if want_list else None, ctypes.byref(p_verts) if want_list else None,
                                  ctypes.byref(n_verts))
    seconds = time.perf_counter() - t0
    offset = verts = None
    if want_list:
        try:
            if n >= 0:
                offset = np.ctypeslib.as_array(ctypes.cast(p_off, ctypes.POINTER(ctypes.c_int64)), (n + 1,)).copy()
                verts = (np.ctypeslib.as_array(ctypes.cast(p_verts, ctypes.POINTER(ctypes.c_int32)), (n_verts.value,)).copy()
                         if n_verts.value else np.zeros(0, np.int32))
        finally:
            lib().orc_free(p_off)
            lib().orc_free(p_verts)
    if n < 0:
        raise ValueError("orc_maximal_cliques: bad arguments")
    return {"k_min": k_min, "hist_all": hist, "count": count[:nv], "largest": largest[:nv], "omega": int(omega.value), "n_cliques": int(n),
            "offset": offset, "verts": verts, "nodes": int(nodes.value), "seconds": seconds}


def maximal_view(allc, tmax, k_min=2):
    """What komb_maximal_cliques_run(k_min) reports, in numpy from the k_min = 2 list of maximal_cliques_all and the graph's
    t_max: {"k_min", "k_hi", "t_max", "omega", "flags" (3), "n_cliques", "hist", "count", "largest", "offset", "verts"}."""
    if k_min < 2:
        raise ValueError("bad k_min")
    assert allc["k_min"] == 2 and allc["offset"] is not None
    nv = len(allc["count"])
    k_hi = max(k_min, tmax)
    size = np.diff(allc["offset"])
    assert (size <= max(tmax, 2)).all()
    keep = size >= k_min
    hist = np.bincount(size[keep] - k_min, minlength=k_hi - k_min + 1).astype(np.int64)
    member = np.repeat(keep, size)
    verts = allc["verts"][member]
    count = np.bincount(verts, minlength=nv).astype(np.int32)
    largest = np.zeros(nv, np.int32)
    np.maximum.at(largest, verts, np.repeat(size[keep], size[keep]).astype(np.int32))
    offset = np.concatenate([[0], np.cumsum(size[keep])]).astype(np.int64)
    return {"k_min": k_min, "k_hi": k_hi, "t_max": tmax, "omega": int(size[keep].max()) if keep.any() else 0, "flags": 3,
            "n_cliques": int(keep.sum()), "hist": hist, "count": count, "largest": largest, "offset": offset, "verts": verts}


def maximal_cliques(rowptr, col, k_min=2, tmax=None):
    """The maximal cliques of >= k_min vertices of a symmetric CSR as komb_maximal_cliques_run defines them (see maximal_view)."""
    tmax = t_max(rowptr, col) if tmax is None else tmax
    return maximal_view(maximal_cliques_all(rowptr, col, 2), tmax, k_min)


def maximum_cliques(view, tmax=None):
    """What komb_max_clique_run reports with all three flags, in numpy from a maximal_view whose k_min does not exceed the clique
    number: {"omega", "upper", "flags" (7), "t_max", "n_max_cliques", "count": int32[nv], "list": int32[n, omega]}."""
    nv = len(view["count"])
    size = np.diff(view["offset"])
    omega = int(size.max()) if len(size) else 0
    rows = np.flatnonzero(size == omega) if omega else np.zeros(0, np.int64)
    cl = (view["verts"][(view["offset"][rows][:, None] + np.arange(omega)[None, :]).reshape(-1)].reshape(len(rows), omega)
          if omega else np.zeros((0, 0), np.int32))
    return {"omega": omega, "upper": omega, "flags": 7, "t_max": view["t_max"] if tmax is None else tmax, "n_max_cliques": len(rows),
            "count": np.bincount(cl.reshape(-1), minlength=nv).astype(np.int32), "list": cl.astype(np.int32)}


def nucleus(rowptr, col):
    """orc_nucleus: {"a", "b", "c", "key0", "theta": int32[n_triangles], "edge_theta": int32[ne], "vertex_theta": int32[nv],
    "quads": int32[n_cliques4, 4] (triangle ids), "info": {"n_triangles", "n_cliques4", "theta_max", "n_levels"}, "seconds"}."""
    import time
    rowptr, col = _csr(rowptr, col)
    nv = len(rowptr) - 1
    ne = int(rowptr[nv]) // 2
    t0 = time.perf_counter()
    nq = ctypes.c_int64()
    nt = lib().orc_nucleus_count(nv, rowptr, col, ctypes.byref(nq))
    tri = [np.zeros(max(nt, 1), dtype=np.int32) for _ in range(5)]
    edge_theta = np.zeros(max(ne, 1), dtype=np.int32)
    vertex_theta = np.zeros(max(nv, 1), dtype=np.int32)
    quads = np.zeros(max(4 * nq.value, 1), dtype=np.int32)
    tmax = lib().orc_nucleus(nv, rowptr, col, nt, nq.value, *tri, edge_theta, vertex_theta, quads)
    if tmax < -1:
        raise RuntimeError("orc_nucleus: inconsistent counts")
    out = {name: x[:nt] for name, x in zip(("a", "b", "c", "key0", "theta"), tri)}
    out.update(edge_theta=edge_theta[:ne], vertex_theta=vertex_theta[:nv], quads=quads[:4 * nq.value].reshape(-1, 4),
               info={"n_triangles": int(nt), "n_cliques4": int(nq.value), "theta_max": int(tmax),
                     "n_levels": len(np.unique(out["theta"]))}, seconds=time.perf_counter() - t0)
    return out


def nuclei_labels(theta, quads, k):
    """(label, size) int32[n_triangles] of the k-nuclei, k >= 1, from the definition: the 4-cliques whose four triangles all have
    theta >= k link their triangles; a class's label is its smallest triangle id; -1 / 0 where theta < k."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    theta = np.asarray(theta, np.int64)
    nt = len(theta)
    label, size = np.full(nt, -1, np.int32), np.zeros(nt, np.int32)
    mem = np.flatnonzero(theta >= k)
    if not len(mem):
        return label, size
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    q = q[(theta[q] >= k).all(axis=1)] if len(q) else q
    u, v = np.repeat(q[:, 0], 3), q[:, 1:].reshape(-1)
    _, comp = connected_components(coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(nt, nt)), directed=False)
    comp = comp[mem]
    first = np.full(int(comp.max()) + 1, nt, np.int64)
    np.minimum.at(first, comp, mem)
    label[mem] = first[comp]
    size[mem] = np.bincount(comp)[comp]
    return label, size


# ------------------------------------------------ clique percolation (komb_clique_communities_run), from a list of maximal cliques
def _member_rows(offset, verts, k):
    """The member cliques (>= k vertices) of a list: (mem: their indices, ms: their sizes, mv: their vertices, flat, start: the
    first entry of each in mv)."""
    offset = np.asarray(offset, np.int64)
    verts = np.asarray(verts, np.int64)
    size = np.diff(offset)
    keep = size >= k
    mem, ms = np.flatnonzero(keep), size[keep]
    mv = verts[np.repeat(keep, size)]
    return mem, ms, mv, np.concatenate([[0], np.cumsum(ms)])[:-1]


def clique_communities(nv, offset, verts, k):
    """Every output of komb_clique_communities_run(k) for the list (offset, verts) of maximal cliques -- ascending tuples in
    lexicographic order --, from the definition by shared subsets: two cliques of >= k vertices are adjacent when a set of k - 1
    vertices lies in both, so every (k - 1)-subset of every member clique is written out (per clique size, one column choice at
    a time), equal subsets get one number (np.unique over the rows), and the communities are the connected components of the
    bipartite clique -- subset graph.  No pivots, no pair of cliques is ever looked at.
    {"k", "label", "size": int32[n_cliques of the list], "rep", "n_cliques": int32[n], "offset": int64[n + 1], "verts": int32,
    "n_comm", "first": int32[nv], "n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap"}."""
    from itertools import combinations
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if k < 2:
        raise ValueError("bad k")
    n_list = len(offset) - 1
    mem, ms, mv, start = _member_rows(offset, verts, k)
    nm = len(mem)
    label, size = np.full(n_list, -1, np.int32), np.zeros(n_list, np.int32)
    out = {"k": k, "label": label, "size": size, "rep": np.zeros(0, np.int32), "n_cliques": np.zeros(0, np.int32),
           "offset": np.zeros(1, np.int64), "verts": np.zeros(0, np.int32), "n_comm": np.zeros(nv, np.int32),
           "first": np.full(nv, -1, np.int32), "n_member_cliques": nm, "n_communities": 0, "largest": 0, "n_covered": 0, "n_overlap": 0}
    if nm == 0:
        return out
    rows, owner = [], []
    for s in np.unique(ms).tolist():
        which = np.flatnonzero(ms == s)                                             # positions among the members
        mat = mv[start[which][:, None] + np.arange(s)[None, :]]
        for cols in combinations(range(s), k - 1):
            rows.append(mat[:, cols])
            owner.append(which)
    rows, owner = np.concatenate(rows), np.concatenate(owner)
    _, sub = np.unique(rows, axis=0, return_inverse=True)
    sub = sub.reshape(-1)
    n_sub = int(sub.max()) + 1
    graph = coo_matrix((np.ones(len(owner), np.int8), (owner, nm + sub)), shape=(nm + n_sub, nm + n_sub))
    _, comp = connected_components(graph, directed=False)
    comp = comp[:nm]
    first_of = np.full(int(comp.max()) + 1, n_list, np.int64)
    np.minimum.at(first_of, comp, mem)                                              # a community's rep: its smallest clique index
    rep_of = first_of[comp]
    reps, number, n_cl = np.unique(rep_of, return_inverse=True, return_counts=True)
    number = number.reshape(-1)
    label[mem], size[mem] = rep_of, n_cl[number]
    key = np.unique(np.repeat(number, ms) * max(nv, 1) + mv)                         # the distinct (community, vertex) pairs, in order
    c_of, v_of = key // max(nv, 1), key % max(nv, 1)
    per_comm = np.bincount(c_of, minlength=len(reps))
    n_comm = np.bincount(v_of, minlength=nv)
    first = np.full(nv, len(reps), np.int64)
    np.minimum.at(first, v_of, c_of)
    first[n_comm == 0] = -1
    out.update(rep=reps.astype(np.int32), n_cliques=n_cl.astype(np.int32), offset=np.concatenate([[0], np.cumsum(per_comm)]).astype(np.int64),
               verts=v_of.astype(np.int32), n_comm=n_comm.astype(np.int32), first=first.astype(np.int32), n_communities=len(reps),
               largest=int(per_comm.max()), n_covered=int((n_comm >= 1).sum()), n_overlap=int((n_comm >= 2).sum()))
    return out


def percolation_pair_tests(nv, offset, verts, k):
    """info["pair_tests"] of komb_clique_communities_run(k): the pivot rule of the contract restated over whole arrays.  load(v) =
    the member cliques through v; the pivots of a member clique of s vertices are its s - k + 2 vertices of smallest
    (load(v), v); the result is the sum, over the member cliques i and their pivots v, of the member cliques j > i through v
    (the entries of v's row above i: the rows ascend by clique index)."""
    if k < 2:
        raise ValueError("bad k")
    mem, ms, mv, start = _member_rows(offset, verts, k)
    if not len(mem):
        return 0
    load = np.bincount(mv, minlength=max(nv, 1))
    by_row = np.argsort(mv, kind="stable")                                          # row by row, clique indices ascending inside
    row_start = np.concatenate([[0], np.cumsum(load)])
    pos = np.empty(len(mv), np.int64)
    pos[by_row] = np.arange(len(mv)) - row_start[mv[by_row]]
    above = load[mv] - 1 - pos
    total = 0
    for s in np.unique(ms).tolist():
        idx = start[ms == s][:, None] + np.arange(s)[None, :]
        v = mv[idx]
        pivots = np.argsort(load[v] * max(nv, 1) + v, axis=1, kind="stable")[:, :s - k + 2]
        total += int(np.take_along_axis(above[idx], pivots, axis=1).sum())
    return total


# ------------------------------------------------ traversals and graphlets (komb_oracle.h: one queue BFS per source, dense arrays)
class Limit(Exception):
    """orc_betweenness: a sigma reached +inf, where the library answers KOMB_ERR_LIMIT"""


def _sources(nv, sources):
    return np.ascontiguousarray(np.arange(nv) if sources is None else np.asarray(sources).reshape(-1), dtype=np.int32)


def distances(rowptr, col, sources=None, words=4):
    """What komb_distances_run / _fetch / _fetch_sources / _histogram / _info give, in the layout of tests/distances_ref.py
    distances(): the arrays are orc_bfs_sources', the info fields are derived here from the per-source arrays and `words`
    (DIST_WORDS) exactly as that function derives them.  "seconds" is the time of the C call."""
    import time
    rowptr, col = _csr(rowptr, col)
    nv = len(rowptr) - 1
    src = _sources(nv, sources)
    n = len(src)
    if words not in (1, 2, 4) or (n and (src.min() < 0 or src.max() >= nv)):
        raise ValueError("bad sources or words")
    per = {"source": src.copy(), "n_reached": np.zeros(n, np.int64), "sum_dist": np.zeros(n, np.int64), "ecc": np.zeros(n, np.int32)}
    room = max(nv, 1)
    out = {"n_reached": np.zeros(room, np.int64), "sum_dist": np.zeros(room, np.int64), "ecc": np.full(room, -1, np.int32),
           "harmonic": np.zeros(room, np.float64)}
    pairs = np.zeros(room, np.int64)
    pad = lambda x: x if len(x) else np.zeros(1, x.dtype)
    t0 = time.perf_counter()
    deepest = lib().orc_bfs_sources(nv, rowptr, col, n, pad(src), pad(per["n_reached"]), pad(per["sum_dist"]), pad(per["ecc"]),
                                    out["n_reached"], out["sum_dist"], out["ecc"], out["harmonic"], pairs)
    seconds = time.perf_counter() - t0
    if deepest < 0:
        raise ValueError("orc_bfs_sources: bad arguments")
    out = {name: x[:nv] for name, x in out.items()}
    depth_max = int(per["ecc"].max()) if n else 0
    assert depth_max == deepest
    out.update(sources=per, pairs=pairs[:depth_max + 1].copy(), seconds=seconds, all=sources is None)
    out["info"] = distances_info(out, words)
    return out


def distances_info(out, words):
    """info of a distances() result at DIST_WORDS = words: only the batch and step counts depend on it."""
    ecc, pairs, nv = out["sources"]["ecc"], out["pairs"], len(out["ecc"])
    n = len(ecc)
    group = 64 * words
    batches = [ecc[i:i + group] for i in range(0, n, group)]
    return {"n_sources": n, "flags": 1 if out["all"] else 0, "depth_max": int(ecc.max()) if n else 0, "depth_min": int(ecc.min()) if n else 0,
            "n_pairs": int(pairs.sum()), "sum_all": int((pairs * np.arange(len(pairs))).sum()), "n_batches": len(batches),
            "n_level_steps": sum(int(b.max()) + 1 for b in batches) if nv else 0}


def betweenness(rowptr, col, sources=None):
    """What komb_betweenness_run / _fetch / _fetch_sources / _info give, in the layout of tests/betweenness_ref.py
    betweenness(), from orc_betweenness; the batch and step counts are derived here as that function derives them.  Raises
    Limit where the library answers KOMB_ERR_LIMIT."""
    import time
    rowptr, col = _csr(rowptr, col)
    nv = len(rowptr) - 1
    src = _sources(nv, sources)
    n = len(src)
    if n and (src.min() < 0 or src.max() >= nv):
        raise ValueError("bad sources")
    bc = np.zeros(max(nv, 1), np.float64)
    reached, sumd, ecc = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    flags = ctypes.c_int32()
    t0 = time.perf_counter()
    rc = lib().orc_betweenness(nv, rowptr, col, n, src if n else np.zeros(1, np.int32), bc, reached, sumd, ecc, ctypes.byref(flags))
    seconds = time.perf_counter() - t0
    if rc == -2:
        raise Limit()
    if rc != 0:
        raise ValueError("orc_betweenness: bad arguments")
    ecc = ecc[:n]
    batches = [ecc[i:i + 64] for i in range(0, n, 64)]
    steps = sum((int(b.max()) + 1) + max(int(b.max()) - 1, 0) for b in batches) if nv > 0 else 0
    return {"bc": bc[:nv], "source": src.copy(), "n_reached": reached[:n], "sum_dist": sumd[:n], "ecc": ecc, "flags": int(flags.value),
            "depth_max": int(ecc.max()) if n else 0, "n_sources": n, "n_batches": len(batches), "n_level_steps": steps, "seconds": seconds}


GRAPHLET_TOTAL_OF = {"edge": (0, 2), "wedge": (2, 1), "triangle": (3, 3), "path4": (5, 2), "claw": (7, 1), "cycle4": (8, 4),
                     "paw": (11, 1), "diamond": (13, 2), "clique4": (14, 4)}       # total = the sum of orbit o over the vertices / divisor


def graphlets(rowptr, col):
    """orc_graphlets in the layout of tests/graphlets_ref.py census(): {"orbit": uint64[15, nv], "cycles4", "cliques4": uint64[ne],
    "sup": int64[ne], "total": {name: int}, "seconds"}, the per-edge arrays in canonical order."""
    import time
    rowptr, col = _csr(rowptr, col)
    nv = len(rowptr) - 1
    ne = int(rowptr[nv]) // 2
    orbit = np.zeros(15 * max(nv, 1), np.uint64)
    cyc, clq, sup = np.zeros(max(ne, 1), np.uint64), np.zeros(max(ne, 1), np.uint64), np.zeros(max(ne, 1), np.int64)
    t0 = time.perf_counter()
    rc = lib().orc_graphlets(nv, rowptr, col, orbit, cyc, clq, sup)
    seconds = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError("orc_graphlets: %d" % rc)
    orbit = orbit[:15 * nv].reshape(15, nv)
    total = {}
    for name, (o, div) in GRAPHLET_TOTAL_OF.items():
        s = sum(int(x) for x in orbit[o])
        assert s % div == 0, (name, s, div)
        total[name] = s // div
    return {"orbit": orbit, "cycles4": cyc[:ne], "cliques4": clq[:ne], "sup": sup[:ne], "total": total, "seconds": seconds}


def orbits_by_definition(rowptr, col, v, ball_limit=0):
    """(orbit vector uint64[15] of vertex v from orc_orbits_by_definition, the vertices within three hops of v); (None, None)
    when ball_limit > 0 and the ball is larger."""
    rowptr, col = _csr(rowptr, col)
    out = np.zeros(15, np.uint64)
    ball = lib().orc_orbits_by_definition(len(rowptr) - 1, rowptr, col, int(v), int(ball_limit), out)
    if ball == -1:
        return None, None
    if ball < 0:
        raise ValueError("orc_orbits_by_definition: bad arguments")
    return out, int(ball)
