"""Host-side Python view of the komb_accel C ABI.

Thin plumbing for tests and bench.py: one `KombAccel` object = one komb_ctx on
one GPU.  Method names follow the reference's seam: `run_core` stands where
Kgraph::runCore calls igraph_degree + igraph_coreness (src/graph.cpp:462-463),
`run_truss` where Kgraph::runTruss calls igraph_induced_subgraph_map +
igraph_trussness (src/graph.cpp:502,508), `get_anomaly_score` where
CombineCoreA::run calls CoreA::getAnomalyScore (src/CombineCoreA.h:30).
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import KombOpts, KombStats, as_c, ptr


class KombError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"komb_accel error {code}: {msg}")
        self.code = code


def gen_hug_edges(nv, n_cliques, alpha=2.6, seed=42):
    """Synthetic power-law unitig graph: raw (u,v) pairs int64[n_raw,2] (host code)."""
    lib = _lib.load()
    n_raw = lib.komb_gen_hug_edges(nv, n_cliques, alpha, seed, None)
    if n_raw < 0:
        raise ValueError("komb_gen_hug_edges: bad arguments")
    uv = np.empty((n_raw, 2), dtype=np.int64)
    got = lib.komb_gen_hug_edges(nv, n_cliques, alpha, seed, ptr(uv))
    assert got == n_raw
    return uv


# The library reads no KOMB_* environment variable (ABI 7): its tuning / test switches are per-context options
# (komb_set_option).  The TESTS still say what they want through the environment (monkeypatch.setenv("KOMB_FINISH", "lds")):
# with FORWARD_ENV_OPTIONS on (tests/conftest.py turns it on; bench.py never does) this plumbing hands those variables to
# komb_set_option before every compute call -- the forwarding is test infrastructure, the option mechanism is the ABI's.
FORWARD_ENV_OPTIONS = False
OPTION_NAMES = ("FINISH", "LOCAL_LIMIT", "LOCAL_ITEMS", "LOCAL_DENSITY", "LOCAL_DEFER_CHUNKS", "TAIL", "CORE_TAIL", "INDEX",
                "REC_CAP", "OWN_DENSE_CAP", "NO_OWN_DENSE", "NO_REC_SCRATCH", "NO_FIRST_QUEUE", "FULL_CAPS", "PREP_ROW_STAGE", "RETIRE_EVERY", "SHARD_ENGINE",
                "TRI_DEBUG", "POOL_DEBUG", "BUILD_DEBUG", "LOCAL_DEBUG", "TAIL_DEBUG", "COMP_SAMPLE", "COMM_SHORT", "COMM_HEAVY", "DENSEST_LOCAL", "STRUCT_DEBUG",
                "NUC_SHORT", "NUC_HEAVY", "NUC_CAP", "NUC_DEBUG", "MAXCLQ_SEED", "MAXCLQ_LDS", "MAXCLQ_LIST", "MAXCLQ_DEBUG", "CENSUS_LDS", "CENSUS_PIVOT",
                "CENSUS_DEBUG", "MAXIMAL_LDS", "MAXIMAL_PIVOT", "MAXIMAL_LIST", "MAXIMAL_DEBUG", "PERC_GROUP", "PERC_DEBUG", "BICONN_HEAVY",
                "GRAPHLET_LDS", "GRAPHLET_SHORT", "GRAPHLET_DEBUG", "BTW_GRID", "BTW_DEBUG", "DIST_WORDS", "DIST_GRID",
                "DIST_DEBUG", "POISON")

# (ALLOC_FAIL_AT / ALLOC_TRIM_AT are one-shot triggers counted from the moment they are set: they are NOT forwarded -- forwarding
# would re-arm them before every call; a test sets them with set_option)

# Every output array starts as a sentinel, not as zeros: an entry the library leaves unwritten fails any comparison at once
# instead of passing wherever 0 is the expected value.
SENTINEL_I32 = -0x5A5A5A5B              # 0xA5A5A5A5


def _out_i32(n):
    return np.full(n, SENTINEL_I32, dtype=np.int32)


def _out_f64(n):
    return np.full(n, np.nan, dtype=np.float64)


SENTINEL_U64 = 0xA5A5A5A5A5A5A5A5


def _out_u64(n):
    return np.full(n, SENTINEL_U64, dtype=np.uint64)


class KombAccel:
    def __init__(self, device=0, verbosity=0, flags=0):
        self._lib = _lib.load()
        opts = KombOpts(device=device, verbosity=verbosity)
        opts.reserved[0] = flags
        self._ctx = self._lib.komb_create(ctypes.byref(opts))
        if not self._ctx:
            raise MemoryError("komb_create failed")
        self.device = device
        self.nv = -1
        self.ne = 0
        self._forwarded = {}

    def set_option(self, name, value):
        """komb_set_option: a tuning / test switch of this context (None unsets).  No option changes a result."""
        v = None if value is None else str(value).encode()
        self._check(self._lib.komb_set_option(self._ctx, name.encode(), v))

    def alloc_info(self):
        """komb_alloc_info: the allocation-request counter of options ALLOC_FAIL_AT / ALLOC_TRIM_AT and the pool's state (host
        state only; works without a device)."""
        req, used, nbytes, cached, trims = (ctypes.c_int64() for _ in range(5))
        fired = ctypes.c_int32()
        self._check(self._lib.komb_alloc_info(self._ctx, ctypes.byref(req), ctypes.byref(fired), ctypes.byref(used), ctypes.byref(nbytes),
                                              ctypes.byref(cached), ctypes.byref(trims)))
        return {"requests": req.value, "fired": fired.value, "pool_blocks_in_use": used.value, "pool_bytes_in_use": nbytes.value,
                "pool_blocks_cached": cached.value, "trims": trims.value}

    def _sync_env_options(self):
        if not FORWARD_ENV_OPTIONS:
            return
        for name in OPTION_NAMES:
            v = os.environ.get("KOMB_" + name)
            if name == "INDEX" and os.environ.get("KOMB_TWO_PASS"):
                v = "two_pass"
            if name == "SHARD_ENGINE" and v is None:
                v = os.environ.get("KOMB_SHARD_PEEL")
            if self._forwarded.get(name) != v:
                self.set_option(name, v)
                self._forwarded[name] = v

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.komb_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise KombError(rc, self._lib.komb_last_error(self._ctx).decode())

    # ---- graph (a1)
    def from_edges(self, nv, uv):
        uv = as_c(np.asarray(uv).reshape(-1, 2), np.int64)
        self._sync_env_options()                         # (the build's own buffers come from the context too: POISON)
        self._check(self._lib.komb_graph_from_edges(self._ctx, nv, uv.shape[0], ptr(uv)))
        self._info()
        return self

    def from_csr(self, rowptr, col):
        rowptr = as_c(rowptr, np.int64)
        col = as_c(col, np.int32)
        self._sync_env_options()
        self._check(self._lib.komb_graph_from_csr(self._ctx, len(rowptr) - 1, ptr(rowptr), ptr(col)))
        self._info()
        return self

    def _info(self):
        nv, ne = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.komb_graph_info(self._ctx, ctypes.byref(nv), ctypes.byref(ne)))
        self.nv, self.ne = nv.value, ne.value

    def get_csr(self):
        rowptr = np.full(self.nv + 1, SENTINEL_I32, dtype=np.int64)
        col = _out_i32(2 * self.ne)
        self._check(self._lib.komb_graph_get_csr(self._ctx, ptr(rowptr), ptr(col)))
        return rowptr, col

    # ---- k-core (a2 + a3)
    def core_run(self):
        self._sync_env_options()
        self._check(self._lib.komb_core_run(self._ctx))

    def set_shard_peel(self, on=True):
        """komb_set_shard_peel: sharded k-truss runs split the peel by edge range as well (opt-in; shard_dev.h)."""
        self._check(self._lib.komb_set_shard_peel(self._ctx, 1 if on else 0))

    def core_fetch(self):
        deg = _out_i32(self.nv)
        core = _out_i32(self.nv)
        self._check(self._lib.komb_core_fetch(self._ctx, ptr(deg), ptr(core)))
        return deg, core

    def run_core(self):
        """degree, coreness -- what Kgraph::runCore gets from igraph."""
        self.core_run()
        return self.core_fetch()

    # ---- onion decomposition (per-vertex peel layer inside each k-shell; include/komb_accel.h)
    def onion_run(self):
        self._sync_env_options()
        self._check(self._lib.komb_onion_run(self._ctx))

    def onion_fetch(self):
        """(layer, coreness) int32[nv] of the last komb_onion_run on this graph."""
        layer = _out_i32(self.nv)
        core = _out_i32(self.nv)
        self._check(self._lib.komb_onion_fetch(self._ctx, ptr(layer), ptr(core)))
        return layer, core

    def run_onion(self):
        """layer, coreness -- what networkx.onion_layers gives (layers from 1; isolated vertices are layer 1)."""
        self.onion_run()
        return self.onion_fetch()

    def onion_info(self):
        """{"n_layers", "max_coreness", "ms"} of the last komb_onion_run (ms: its device time)."""
        n, k, ms = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()
        self._check(self._lib.komb_onion_info(self._ctx, ctypes.byref(n), ctypes.byref(k), ctypes.byref(ms)))
        return {"n_layers": n.value, "max_coreness": k.value, "ms": ms.value}

    # ---- connected components of a k-core / k-truss subgraph (include/komb_accel.h)
    COMP_KINDS = {"core": _lib.KOMB_COMP_CORE, "truss": _lib.KOMB_COMP_TRUSS}

    def components_run(self, kind, k):
        """kind: "core" | "truss" (or the KOMB_COMP_* number); k: the threshold, -1 (KOMB_COMP_K_MAX) for the largest."""
        self._sync_env_options()
        self._check(self._lib.komb_components_run(self._ctx, self.COMP_KINDS.get(kind, kind), k))

    def components_fetch(self):
        """(label, size) int32[nv] of the last komb_components_run on this graph: the smallest vertex id of the vertex'
        component (-1: not a member) and the component's number of vertices (0: not a member)."""
        label = _out_i32(max(self.nv, 0))
        size = _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_components_fetch(self._ctx, ptr(label), ptr(size)))
        return label, size

    def components_info(self):
        """{"kind", "k_used", "n_members", "n_components", "largest", "ms"} of the last komb_components_run."""
        kind, k = ctypes.c_int32(), ctypes.c_int32()
        mem, comp, big, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._check(self._lib.komb_components_info(self._ctx, ctypes.byref(kind), ctypes.byref(k), ctypes.byref(mem),
                                                   ctypes.byref(comp), ctypes.byref(big), ctypes.byref(ms)))
        return {"kind": kind.value, "k_used": k.value, "n_members": mem.value, "n_components": comp.value,
                "largest": big.value, "ms": ms.value}

    def run_components(self, kind="core", k=0):
        """label, size of the connected components of the k-core (kind="core") or of the last k-truss result's k-truss."""
        self.components_run(kind, k)
        return self.components_fetch()

    # ---- component hierarchy: the nesting forest of the k-core / k-truss components over all k (include/komb_accel.h)
    HIER_FIELDS = ("k", "rep", "parent", "size", "shell")

    def hierarchy_run(self, kind="core"):
        """kind: "core" | "truss" (or the KOMB_COMP_* number); needs the coreness / a complete k-truss result on this graph."""
        self._sync_env_options()
        self._check(self._lib.komb_hierarchy_run(self._ctx, self.COMP_KINDS.get(kind, kind)))

    def hierarchy_fetch_nodes(self):
        """{"k", "rep", "parent", "size", "shell"}: int32[n_nodes] each, nodes in ascending (k, rep) order."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_hierarchy_count(self._ctx, ctypes.byref(n)))
        out = {name: _out_i32(max(n.value, 0)) for name in self.HIER_FIELDS}
        self._check(self._lib.komb_hierarchy_fetch_nodes(self._ctx, *(ptr(out[name]) for name in self.HIER_FIELDS)))
        return out

    def hierarchy_fetch_vertices(self):
        """node int32[nv]: the node of every vertex (its level's component), -1 for a non-member (truss kind only)."""
        node = _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_hierarchy_fetch_vertices(self._ctx, ptr(node)))
        return node

    def hierarchy_info(self):
        """{"kind", "n_nodes", "n_roots", "k_max", "depth", "ms"} of the last komb_hierarchy_run."""
        kind, kmax, depth = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        n, roots, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._check(self._lib.komb_hierarchy_info(self._ctx, ctypes.byref(kind), ctypes.byref(n), ctypes.byref(roots),
                                                  ctypes.byref(kmax), ctypes.byref(depth), ctypes.byref(ms)))
        return {"kind": kind.value, "n_nodes": n.value, "n_roots": roots.value, "k_max": kmax.value, "depth": depth.value,
                "ms": ms.value}

    def run_hierarchy(self, kind="core"):
        """(nodes, node): the dict of hierarchy_fetch_nodes and the per-vertex node array of the hierarchy of `kind`."""
        self.hierarchy_run(kind)
        return self.hierarchy_fetch_nodes(), self.hierarchy_fetch_vertices()

    # ---- densest-subgraph search with a certified bound (include/komb_accel.h)
    DENSEST_INFO = ("source", "k_best", "k_prune", "n_pruned", "m_pruned", "n_sub", "m_sub", "load_max", "iters", "k_max", "ms")

    def densest_subgraph_run(self, iters=64):
        """iters Frank-Wolfe rounds (0: the best core only); needs the coreness komb_core_run left on this graph."""
        self._sync_env_options()
        self._check(self._lib.komb_densest_subgraph_run(self._ctx, iters))

    def densest_subgraph_fetch(self):
        """(member, load) int32[nv] of the last komb_densest_subgraph_run: 1 | 0, and the vertex' load (0 outside the pruned set)."""
        member = _out_i32(max(self.nv, 0))
        load = _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_densest_subgraph_fetch(self._ctx, ptr(member), ptr(load)))
        return member, load

    def densest_subgraph_info(self):
        """{"source", "k_best", "k_prune", "n_pruned", "m_pruned", "n_sub", "m_sub", "load_max", "iters", "k_max", "ms"}."""
        i32 = {n: ctypes.c_int32() for n in ("source", "k_best", "k_prune", "iters", "k_max")}
        i64 = {n: ctypes.c_int64() for n in ("n_pruned", "m_pruned", "n_sub", "m_sub", "load_max")}
        ms = ctypes.c_double()
        self._check(self._lib.komb_densest_subgraph_info(
            self._ctx, ctypes.byref(i32["source"]), ctypes.byref(i32["k_best"]), ctypes.byref(i32["k_prune"]),
            ctypes.byref(i64["n_pruned"]), ctypes.byref(i64["m_pruned"]), ctypes.byref(i64["n_sub"]), ctypes.byref(i64["m_sub"]),
            ctypes.byref(i64["load_max"]), ctypes.byref(i32["iters"]), ctypes.byref(i32["k_max"]), ctypes.byref(ms)))
        out = {n: v.value for n, v in {**i32, **i64}.items()}
        out["ms"] = ms.value
        return out

    def densest_subgraph_profile(self):
        """(n_k, m_k) int64[k_max + 1]: vertices of coreness >= k, edges between two of them."""
        k = self.densest_subgraph_info()["k_max"] + 1
        n_k = np.full(k, SENTINEL_I32, dtype=np.int64)
        m_k = np.full(k, SENTINEL_I32, dtype=np.int64)
        self._check(self._lib.komb_densest_subgraph_profile(self._ctx, ptr(n_k), ptr(m_k)))
        return n_k, m_k

    def run_densest_subgraph(self, iters=64):
        """(member, load, info): the densest subgraph found on the resident graph and the integers of its certificate."""
        self.densest_subgraph_run(iters)
        member, load = self.densest_subgraph_fetch()
        return member, load, self.densest_subgraph_info()

    # ---- k-truss (a5 + a6)
    def truss_run(self, vmask=None):
        if vmask is not None:
            vmask = as_c(vmask, np.uint8)
            if len(vmask) != self.nv:
                raise ValueError("vmask must have nv entries")
        self._sync_env_options()
        self._check(self._lib.komb_truss_run(self._ctx, ptr(vmask)))

    def truss_run_slice(self, rank, world, vmask=None):
        """komb_truss_run_slice: the whole k-truss path on this rank's copy of the graph, the results of canonical edges
        [ne*rank/world, ne*(rank+1)/world) only (zeros elsewhere); no exchange between the ranks."""
        if vmask is not None:
            vmask = as_c(vmask, np.uint8)
            if len(vmask) != self.nv:
                raise ValueError("vmask must have nv entries")
        self._sync_env_options()
        self._check(self._lib.komb_truss_run_slice(self._ctx, ptr(vmask), int(rank), int(world)))

    def truss_prepare(self):
        """komb_truss_prepare: the k-truss side of the resident graph, made now (a no-op when it exists)."""
        self._check(self._lib.komb_truss_prepare(self._ctx))

    def truss_unprepare(self):
        """komb_truss_unprepare: drop the preparation and the last k-truss result (the next k-truss call rebuilds it)."""
        self._check(self._lib.komb_truss_unprepare(self._ctx))

    def graph_moments(self):
        """komb_graph_moments (measurement only): fills stats sum_deg_sq / wedge_items / max_degree / oriented_items."""
        self._check(self._lib.komb_graph_moments(self._ctx))

    def truss_fetch_into(self, eu=None, ev=None, tr=None):
        """komb_truss_fetch into caller-owned int32 arrays of komb_truss_count entries; None = not wanted."""
        self._check(self._lib.komb_truss_fetch(self._ctx, ptr(eu) if eu is not None else None, ptr(ev) if ev is not None else None,
                                               ptr(tr) if tr is not None else None))

    def truss_fetch(self, with_support=False):
        n = ctypes.c_int64()
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        eu = _out_i32(n.value)
        ev = _out_i32(n.value)
        tr = _out_i32(n.value)
        self._check(self._lib.komb_truss_fetch(self._ctx, ptr(eu), ptr(ev), ptr(tr)))
        if not with_support:
            return eu, ev, tr
        sup = _out_i32(n.value)
        self._check(self._lib.komb_truss_fetch_support(self._ctx, ptr(sup)))
        return eu, ev, tr, sup

    def run_truss(self, vmask=None, with_support=False):
        """(eu, ev, trussness) in canonical edge order, original vertex ids."""
        self.truss_run(vmask)
        return self.truss_fetch(with_support)

    # ---- k-truss communities: triangle-connected classes of the k-truss' edges (include/komb_accel.h)
    def truss_communities_run(self, k=3):
        """k: the trussness threshold (0..2 run as 2), -1 (KOMB_COMM_K_MAX) for the largest trussness of the result."""
        self._sync_env_options()
        self._check(self._lib.komb_truss_communities_run(self._ctx, k))

    def truss_communities_fetch(self):
        """(label, size) int32[ne_sub] of the last komb_truss_communities_run, in the canonical edge order of the k-truss
        result: the smallest canonical edge index of the edge's community (-1: not a member) and its number of edges."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        label = _out_i32(max(n.value, 0))
        size = _out_i32(max(n.value, 0))
        self._check(self._lib.komb_truss_communities_fetch(self._ctx, ptr(label), ptr(size)))
        return label, size

    def truss_communities_fetch_vertices(self):
        """n_comm int32[nv]: the number of distinct communities among the member edges at every vertex."""
        n_comm = _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_truss_communities_fetch_vertices(self._ctx, ptr(n_comm)))
        return n_comm

    def truss_communities_info(self):
        """{"k_used", "n_member_edges", "n_communities", "largest", "n_multi_vertices", "ms"} of the last run."""
        k = ctypes.c_int32()
        mem, comm, big, multi, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._check(self._lib.komb_truss_communities_info(self._ctx, ctypes.byref(k), ctypes.byref(mem), ctypes.byref(comm),
                                                          ctypes.byref(big), ctypes.byref(multi), ctypes.byref(ms)))
        return {"k_used": k.value, "n_member_edges": mem.value, "n_communities": comm.value, "largest": big.value,
                "n_multi_vertices": multi.value, "ms": ms.value}

    def run_truss_communities(self, k=3):
        """label, size of the k-truss communities of the last k-truss result."""
        self.truss_communities_run(k)
        return self.truss_communities_fetch()

    # ---- biconnected components, articulation points, bridges of the k-truss (include/komb_accel.h)
    BICONN_INFO = (("k_used", ctypes.c_int32), ("n_member_edges", ctypes.c_int64), ("n_member_vertices", ctypes.c_int64),
                   ("n_blocks", ctypes.c_int64), ("n_bridges", ctypes.c_int64), ("n_articulation", ctypes.c_int64),
                   ("largest_block", ctypes.c_int64), ("n_ecc", ctypes.c_int64), ("largest_ecc", ctypes.c_int64),
                   ("depth", ctypes.c_int32), ("ms", ctypes.c_double))

    def biconnected_run(self, k=2):
        """k: the trussness threshold (0..2 run as 2), -1 (KOMB_BICONN_K_MAX) for the largest trussness of the result."""
        self._sync_env_options()
        self._check(self._lib.komb_biconnected_run(self._ctx, k))

    def biconnected_count(self):
        """The number of blocks of the last komb_biconnected_run."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_biconnected_count(self._ctx, ctypes.byref(n)))
        return n.value

    def biconnected_fetch_edges(self):
        """(block, size) int32[ne_sub] in the canonical edge order of the k-truss result: the smallest canonical edge index
        of the edge's block (-1: not a member) and its number of edges (1: a bridge)."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_biconnected_count(self._ctx, None))     # (the blocks' own errors first: no graph, no run)
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        block = _out_i32(max(n.value, 0))
        size = _out_i32(max(n.value, 0))
        self._check(self._lib.komb_biconnected_fetch_edges(self._ctx, ptr(block), ptr(size)))
        return block, size

    def biconnected_fetch_vertices(self):
        """(n_blocks, ecc_label, ecc_size) int32[nv]: the blocks that contain the vertex (>= 2: an articulation point), the
        smallest id of its 2-edge-connected component (-1: not a member) and that component's vertices."""
        out = [_out_i32(max(self.nv, 0)) for _ in range(3)]
        self._check(self._lib.komb_biconnected_fetch_vertices(self._ctx, *(ptr(x) for x in out)))
        return tuple(out)

    def biconnected_fetch_blocks(self):
        """{"rep", "n_edges", "n_verts"}: int32[n_blocks] each, blocks in ascending rep order."""
        n = self.biconnected_count()
        out = {name: _out_i32(max(n, 0)) for name in ("rep", "n_edges", "n_verts")}
        self._check(self._lib.komb_biconnected_fetch_blocks(self._ctx, *(ptr(x) for x in out.values())))
        return out

    def biconnected_info(self):
        """A dict keyed by the C names of komb_biconnected_info's outputs."""
        vals = [t() for _, t in self.BICONN_INFO]
        self._check(self._lib.komb_biconnected_info(self._ctx, *(ctypes.byref(x) for x in vals)))
        return {name: x.value for (name, _), x in zip(self.BICONN_INFO, vals)}

    def run_biconnected(self, k=2):
        """block, size of the biconnected components of the last k-truss result."""
        self.biconnected_run(k)
        return self.biconnected_fetch_edges()

    # ---- k-truss community hierarchy: the nesting forest of the communities over all k (include/komb_accel.h)
    def community_hierarchy_run(self):
        """Needs a complete k-truss result on this graph."""
        self._sync_env_options()
        self._check(self._lib.komb_community_hierarchy_run(self._ctx))

    def community_hierarchy_fetch_nodes(self):
        """{"k", "rep", "parent", "size", "shell"}: int32[n_nodes] each, nodes in ascending (k, rep) order; rep is a
        canonical edge index, size and shell count edges."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_community_hierarchy_count(self._ctx, ctypes.byref(n)))
        out = {name: _out_i32(max(n.value, 0)) for name in self.HIER_FIELDS}
        self._check(self._lib.komb_community_hierarchy_fetch_nodes(self._ctx, *(ptr(out[name]) for name in self.HIER_FIELDS)))
        return out

    def _community_hierarchy_edges(self):
        """ne_sub of the k-truss result the stored forest indexes (the forest's own errors first: no graph, no run)."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_community_hierarchy_count(self._ctx, None))
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        return max(n.value, 0)

    def community_hierarchy_fetch_edges(self):
        """node int32[ne_sub]: the node of every canonical edge of the k-truss result, -1 for an edge of trussness 2."""
        n = self._community_hierarchy_edges()
        node = _out_i32(n)
        self._check(self._lib.komb_community_hierarchy_fetch_edges(self._ctx, ptr(node)))
        return node

    def community_hierarchy_labels(self, k=3):
        """(label, size) int32[ne_sub]: what run_truss_communities(k) returns, read off the stored forest."""
        n = self._community_hierarchy_edges()
        label = _out_i32(n)
        size = _out_i32(n)
        self._check(self._lib.komb_community_hierarchy_labels(self._ctx, k, ptr(label), ptr(size)))
        return label, size

    def community_hierarchy_info(self):
        """{"n_nodes", "n_roots", "k_max", "depth", "n_member_edges", "ms"} of the last komb_community_hierarchy_run."""
        kmax, depth = ctypes.c_int32(), ctypes.c_int32()
        n, roots, mem, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._check(self._lib.komb_community_hierarchy_info(self._ctx, ctypes.byref(n), ctypes.byref(roots), ctypes.byref(kmax),
                                                            ctypes.byref(depth), ctypes.byref(mem), ctypes.byref(ms)))
        return {"n_nodes": n.value, "n_roots": roots.value, "k_max": kmax.value, "depth": depth.value,
                "n_member_edges": mem.value, "ms": ms.value}

    def run_community_hierarchy(self):
        """(nodes, node): the dict of community_hierarchy_fetch_nodes and the per-edge node array."""
        self.community_hierarchy_run()
        return self.community_hierarchy_fetch_nodes(), self.community_hierarchy_fetch_edges()

    # ---- structural clustering: clusters, hubs and outliers of the last k-truss result (include/komb_accel.h)
    SC_INFO_FIELDS = ("eps_num", "eps_den", "mu", "n_similar_edges", "n_cores", "n_borders", "n_hubs", "n_outliers", "n_clusters",
                      "largest", "ms")

    def structural_clusters_run(self, eps_num=7, eps_den=10, mu=3):
        """eps = eps_num / eps_den (1 <= eps_num <= eps_den <= 1 000 000), mu >= 2.  Needs a complete k-truss result."""
        self._sync_env_options()
        self._check(self._lib.komb_structural_clusters_run(self._ctx, eps_num, eps_den, mu))

    def structural_clusters_fetch(self):
        """(label, size, role, sim_deg) int32[nv] of the last komb_structural_clusters_run: the vertex' cluster (the smallest
        id of its cores' class; -1 for a hub / an outlier), the vertices that carry that label, KOMB_SC_* and the number of
        similar edges at the vertex."""
        out = [_out_i32(max(self.nv, 0)) for _ in range(4)]
        self._check(self._lib.komb_structural_clusters_fetch(self._ctx, *(ptr(x) for x in out)))
        return tuple(out)

    def structural_clusters_fetch_edges(self):
        """similar int32[ne_sub]: 1 for a similar edge, in the canonical edge order of the k-truss result."""
        self._check(self._lib.komb_structural_clusters_info(self._ctx, *([None] * 11)))    # (the clustering's own errors first)
        n = ctypes.c_int64()
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        similar = _out_i32(max(n.value, 0))
        self._check(self._lib.komb_structural_clusters_fetch_edges(self._ctx, ptr(similar)))
        return similar

    def structural_clusters_info(self):
        """{"eps_num", "eps_den", "mu", "n_similar_edges", "n_cores", "n_borders", "n_hubs", "n_outliers", "n_clusters",
        "largest", "ms"} of the last run."""
        i32 = [ctypes.c_int32() for _ in range(3)]
        i64 = [ctypes.c_int64() for _ in range(7)]
        ms = ctypes.c_double()
        self._check(self._lib.komb_structural_clusters_info(self._ctx, *(ctypes.byref(x) for x in i32 + i64), ctypes.byref(ms)))
        return dict(zip(self.SC_INFO_FIELDS, [x.value for x in i32 + i64] + [ms.value]))

    def run_structural_clusters(self, eps_num=7, eps_den=10, mu=3):
        """(label, size, role, sim_deg) of the structural clustering of the last k-truss result."""
        self.structural_clusters_run(eps_num, eps_den, mu)
        return self.structural_clusters_fetch()

    # ---- graphlet census: 3- and 4-vertex orbit counts of the last k-truss result (include/komb_accel.h)
    GRAPHLET_TYPES = ("edge", "wedge", "triangle", "path4", "claw", "cycle4", "paw", "diamond", "clique4")

    def graphlets_run(self):
        """Needs a complete k-truss result on this graph."""
        self._sync_env_options()
        self._check(self._lib.komb_graphlets_run(self._ctx))

    def graphlets_fetch_vertices(self):
        """orbit uint64[15, nv]: orbit[o, v] = the induced 3- and 4-vertex subgraphs v lies in at orbit o (Przulj's 0-14)."""
        orbit = _out_u64(_lib.KOMB_GRAPHLET_ORBITS * max(self.nv, 0))
        self._check(self._lib.komb_graphlets_fetch_vertices(self._ctx, ptr(orbit)))
        return orbit.reshape(_lib.KOMB_GRAPHLET_ORBITS, max(self.nv, 0))

    def graphlets_fetch_edges(self):
        """(cycles4, cliques4) uint64[ne_sub], in the canonical edge order of the k-truss result."""
        self._check(self._lib.komb_graphlets_info(self._ctx, *([None] * 7)))    # (the census' own errors first)
        n = ctypes.c_int64()
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        cycles4, cliques4 = _out_u64(max(n.value, 0)), _out_u64(max(n.value, 0))
        self._check(self._lib.komb_graphlets_fetch_edges(self._ctx, ptr(cycles4), ptr(cliques4)))
        return cycles4, cliques4

    def graphlets_info(self):
        """{"total": {graphlet: count}, "flags", "max_degree", "cycle_items", "n_triangles", "n_cliques4", "ms"} of the last run."""
        total = (ctypes.c_uint64 * _lib.KOMB_GRAPHLET_TYPES)()
        flags, maxd = ctypes.c_int32(), ctypes.c_int32()
        items, tri, clq, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._check(self._lib.komb_graphlets_info(self._ctx, total, ctypes.byref(flags), ctypes.byref(maxd), ctypes.byref(items),
                                                  ctypes.byref(tri), ctypes.byref(clq), ctypes.byref(ms)))
        return {"total": dict(zip(self.GRAPHLET_TYPES, (int(x) for x in total))), "flags": flags.value, "max_degree": maxd.value,
                "cycle_items": items.value, "n_triangles": tri.value, "n_cliques4": clq.value, "ms": ms.value}

    def run_graphlets(self):
        """(orbit, cycles4, cliques4, info) of the graphlet census of the last k-truss result."""
        self.graphlets_run()
        cycles4, cliques4 = self.graphlets_fetch_edges()
        return self.graphlets_fetch_vertices(), cycles4, cliques4, self.graphlets_info()

    # ---- betweenness centrality from chosen sources on the resident graph (include/komb_accel.h)
    def betweenness_run(self, sources=None):
        """sources: vertex ids in the order they count (duplicates allowed); None = every vertex in ascending order."""
        self._sync_env_options()
        if sources is None:
            self._check(self._lib.komb_betweenness_run(self._ctx, 0, None))
            return
        src = as_c(np.asarray(sources).reshape(-1), np.int32)
        self._check(self._lib.komb_betweenness_run(self._ctx, len(src), ptr(src) if len(src) else ptr(np.zeros(1, np.int32))))

    def betweenness_fetch(self):
        """bc float64[nv]: the raw betweenness, neither halved nor normalised."""
        bc = _out_f64(max(self.nv, 0))
        self._check(self._lib.komb_betweenness_fetch(self._ctx, ptr(bc)))
        return bc

    def betweenness_fetch_sources(self):
        """{"source", "n_reached", "sum_dist", "ecc"}: one entry per source of the last run, in the order given."""
        n = self.betweenness_info()["n_sources"]
        source, ecc = _out_i32(n), _out_i32(n)
        reached, sumd = np.full(n, SENTINEL_I32, dtype=np.int64), np.full(n, SENTINEL_I32, dtype=np.int64)
        self._check(self._lib.komb_betweenness_fetch_sources(self._ctx, ptr(source), ptr(reached), ptr(sumd), ptr(ecc)))
        return {"source": source, "n_reached": reached, "sum_dist": sumd, "ecc": ecc}

    def betweenness_info(self):
        """{"n_sources", "flags", "depth_max", "n_batches", "n_level_steps", "ms"} of the last run."""
        n, nb, steps = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        flags, depth, ms = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        self._check(self._lib.komb_betweenness_info(self._ctx, ctypes.byref(n), ctypes.byref(flags), ctypes.byref(depth), ctypes.byref(nb),
                                                    ctypes.byref(steps), ctypes.byref(ms)))
        return {"n_sources": n.value, "flags": flags.value, "depth_max": depth.value, "n_batches": nb.value,
                "n_level_steps": steps.value, "ms": ms.value}

    def run_betweenness(self, sources=None, halve=False):
        """(bc, per-source dict, info).  halve: bc / 2, which with every vertex as a source is igraph's / networkx's undirected
        unnormalised betweenness (exact: a division by two rounds nothing)."""
        self.betweenness_run(sources)
        bc = self.betweenness_fetch()
        return (bc / 2 if halve else bc), self.betweenness_fetch_sources(), self.betweenness_info()

    # ---- distance analysis from chosen sources on the resident graph (include/komb_accel.h)
    def distances_run(self, sources=None):
        """sources: vertex ids in the order they count (duplicates allowed); None = every vertex in ascending order."""
        self._sync_env_options()
        if sources is None:
            self._check(self._lib.komb_distances_run(self._ctx, 0, None))
            return
        src = as_c(np.asarray(sources).reshape(-1), np.int32)
        self._check(self._lib.komb_distances_run(self._ctx, len(src), ptr(src) if len(src) else ptr(np.zeros(1, np.int32))))

    def distances_fetch(self):
        """{"n_reached", "sum_dist", "ecc", "harmonic"}: one entry per vertex."""
        n = max(self.nv, 0)
        ecc, harmonic = _out_i32(n), _out_f64(n)
        reached, sumd = np.full(n, SENTINEL_I32, dtype=np.int64), np.full(n, SENTINEL_I32, dtype=np.int64)
        self._check(self._lib.komb_distances_fetch(self._ctx, ptr(reached), ptr(sumd), ptr(ecc), ptr(harmonic)))
        return {"n_reached": reached, "sum_dist": sumd, "ecc": ecc, "harmonic": harmonic}

    def distances_fetch_sources(self):
        """{"source", "n_reached", "sum_dist", "ecc"}: one entry per source of the last run, in the order given."""
        n = self.distances_info()["n_sources"]
        source, ecc = _out_i32(n), _out_i32(n)
        reached, sumd = np.full(n, SENTINEL_I32, dtype=np.int64), np.full(n, SENTINEL_I32, dtype=np.int64)
        self._check(self._lib.komb_distances_fetch_sources(self._ctx, ptr(source), ptr(reached), ptr(sumd), ptr(ecc)))
        return {"source": source, "n_reached": reached, "sum_dist": sumd, "ecc": ecc}

    def distances_histogram(self):
        """pairs int64[depth_max + 1]: the (source, vertex) pairs at every distance."""
        pairs = np.full(self.distances_info()["depth_max"] + 1, SENTINEL_I32, dtype=np.int64)
        self._check(self._lib.komb_distances_histogram(self._ctx, ptr(pairs), len(pairs)))
        return pairs

    def distances_info(self):
        """{"n_sources", "flags", "depth_max", "depth_min", "n_pairs", "sum_all", "n_batches", "n_level_steps", "ms"} of the last run."""
        n, npairs, total, nb, steps = (ctypes.c_int64() for _ in range(5))
        flags, dmax, dmin, ms = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        self._check(self._lib.komb_distances_info(self._ctx, ctypes.byref(n), ctypes.byref(flags), ctypes.byref(dmax), ctypes.byref(dmin),
                                                  ctypes.byref(npairs), ctypes.byref(total), ctypes.byref(nb), ctypes.byref(steps),
                                                  ctypes.byref(ms)))
        return {"n_sources": n.value, "flags": flags.value, "depth_max": dmax.value, "depth_min": dmin.value, "n_pairs": npairs.value,
                "sum_all": total.value, "n_batches": nb.value, "n_level_steps": steps.value, "ms": ms.value}

    def run_distances(self, sources=None):
        """(per-vertex dict, per-source dict, pairs, info)."""
        self.distances_run(sources)
        return self.distances_fetch(), self.distances_fetch_sources(), self.distances_histogram(), self.distances_info()

    # ---- (3,4)-nucleus decomposition: triangles of the last k-truss result peeled by their 4-cliques (include/komb_accel.h)
    NUCLEUS_FIELDS = ("a", "b", "c", "key0", "theta")

    def nucleus_run(self):
        """Needs a complete k-truss result on this graph."""
        self._sync_env_options()
        self._check(self._lib.komb_nucleus_run(self._ctx))

    def nucleus_fetch(self):
        """{"a", "b", "c", "key0", "theta"}: int32[n_triangles] each, the triangles a < b < c in ascending (a, b, c) order, the
        4-cliques each lies in and its nucleus number."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_nucleus_count(self._ctx, ctypes.byref(n)))
        out = {name: _out_i32(max(n.value, 0)) for name in self.NUCLEUS_FIELDS}
        self._check(self._lib.komb_nucleus_fetch(self._ctx, *(ptr(out[name]) for name in self.NUCLEUS_FIELDS)))
        return out

    def nucleus_fetch_edges(self):
        """edge_theta int32[ne_sub]: the largest theta over the triangles through every canonical edge, -1 without one."""
        self._check(self._lib.komb_nucleus_count(self._ctx, None))                 # (the decomposition's own errors first)
        n = ctypes.c_int64()
        self._check(self._lib.komb_truss_count(self._ctx, ctypes.byref(n)))
        edge_theta = _out_i32(max(n.value, 0))
        self._check(self._lib.komb_nucleus_fetch_edges(self._ctx, ptr(edge_theta)))
        return edge_theta

    def nucleus_fetch_vertices(self):
        """vertex_theta int32[nv]: the largest theta over the triangles at every vertex, -1 without one."""
        vertex_theta = _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_nucleus_fetch_vertices(self._ctx, ptr(vertex_theta)))
        return vertex_theta

    def nucleus_info(self):
        """{"n_triangles", "n_cliques4", "theta_max", "n_levels", "n_subrounds", "ms"} of the last komb_nucleus_run."""
        tri, clq, sub, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        tmax, lev = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._lib.komb_nucleus_info(self._ctx, ctypes.byref(tri), ctypes.byref(clq), ctypes.byref(tmax), ctypes.byref(lev),
                                                ctypes.byref(sub), ctypes.byref(ms)))
        return {"n_triangles": tri.value, "n_cliques4": clq.value, "theta_max": tmax.value, "n_levels": lev.value,
                "n_subrounds": sub.value, "ms": ms.value}

    def run_nucleus(self):
        """(triangles, edge_theta, vertex_theta): the dict of nucleus_fetch and the per-edge / per-vertex maxima."""
        self.nucleus_run()
        return self.nucleus_fetch(), self.nucleus_fetch_edges(), self.nucleus_fetch_vertices()

    # ---- (3,4)-nucleus hierarchy: the k-nuclei as connected classes and their nesting forest over all k (include/komb_accel.h)
    NUCLEI_FIELDS = ("rep", "n_triangles", "n_edges", "n_vertices")

    def nucleus_hierarchy_run(self):
        """Needs a nucleus decomposition (nucleus_run) of the current k-truss result."""
        self._sync_env_options()
        self._check(self._lib.komb_nucleus_hierarchy_run(self._ctx))

    def nucleus_hierarchy_fetch_nodes(self):
        """{"k", "rep", "parent", "size", "shell"}: int32[n_nodes] each, nodes in ascending (k, rep) order; rep is a
        triangle id, size and shell count triangles."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_nucleus_hierarchy_count(self._ctx, ctypes.byref(n)))
        out = {name: _out_i32(max(n.value, 0)) for name in self.HIER_FIELDS}
        self._check(self._lib.komb_nucleus_hierarchy_fetch_nodes(self._ctx, *(ptr(out[name]) for name in self.HIER_FIELDS)))
        return out

    def _nucleus_hierarchy_triangles(self):
        """n_triangles of the nucleus result the stored forest indexes (the forest's own errors first: no graph, no run)."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_nucleus_hierarchy_count(self._ctx, None))
        self._check(self._lib.komb_nucleus_count(self._ctx, ctypes.byref(n)))
        return max(n.value, 0)

    def nucleus_hierarchy_fetch_triangles(self):
        """node int32[n_triangles]: the node of every triangle of the nucleus result, -1 for a triangle with theta 0."""
        node = _out_i32(self._nucleus_hierarchy_triangles())
        self._check(self._lib.komb_nucleus_hierarchy_fetch_triangles(self._ctx, ptr(node)))
        return node

    def nucleus_hierarchy_labels(self, k=1):
        """(label, size) int32[n_triangles]: the rep and the triangle count of every triangle's k-nucleus, -1 / 0 where
        theta < k; k = -1: the largest theta."""
        n = self._nucleus_hierarchy_triangles()
        label = _out_i32(n)
        size = _out_i32(n)
        self._check(self._lib.komb_nucleus_hierarchy_labels(self._ctx, k, ptr(label), ptr(size)))
        return label, size

    def nucleus_hierarchy_nuclei(self, k=1):
        """{"rep", "n_triangles", "n_edges", "n_vertices"}: int32[n_nuclei] each, the k-nuclei as subgraphs in ascending
        rep order; k = -1: the largest theta."""
        n = ctypes.c_int64()
        self._check(self._lib.komb_nucleus_hierarchy_nuclei(self._ctx, k, 0, ctypes.byref(n), None, None, None, None))
        out = {name: _out_i32(max(n.value, 0)) for name in self.NUCLEI_FIELDS}
        self._check(self._lib.komb_nucleus_hierarchy_nuclei(self._ctx, k, n.value, ctypes.byref(n),
                                                            *(ptr(out[name]) for name in self.NUCLEI_FIELDS)))
        return out

    def nucleus_hierarchy_info(self):
        """{"n_nodes", "n_roots", "theta_max", "depth", "n_member_triangles", "ms"} of the last komb_nucleus_hierarchy_run."""
        tmax, depth = ctypes.c_int32(), ctypes.c_int32()
        n, roots, mem, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._check(self._lib.komb_nucleus_hierarchy_info(self._ctx, ctypes.byref(n), ctypes.byref(roots), ctypes.byref(tmax),
                                                          ctypes.byref(depth), ctypes.byref(mem), ctypes.byref(ms)))
        return {"n_nodes": n.value, "n_roots": roots.value, "theta_max": tmax.value, "depth": depth.value,
                "n_member_triangles": mem.value, "ms": ms.value}

    def run_nucleus_hierarchy(self):
        """(nodes, node): the dict of nucleus_hierarchy_fetch_nodes and the per-triangle node array."""
        self.nucleus_hierarchy_run()
        return self.nucleus_hierarchy_fetch_nodes(), self.nucleus_hierarchy_fetch_triangles()

    # ---- maximum-clique search with a certified bound on the last k-truss result (include/komb_accel.h)
    MAX_CLIQUE_INFO_FIELDS = ("omega", "upper", "flags", "t_max", "n_max_cliques", "n_roots", "nodes", "ms")

    def max_clique_run(self, budget=0):
        """Needs a complete k-truss result on this graph.  budget: the node cap of the whole run, 0 for the default."""
        self._sync_env_options()
        self._check(self._lib.komb_max_clique_run(self._ctx, budget))

    def max_clique_info(self):
        """{"omega", "upper", "flags", "t_max", "n_max_cliques", "n_roots", "nodes", "ms"} of the last komb_max_clique_run."""
        i32 = [ctypes.c_int32() for _ in range(4)]
        i64 = [ctypes.c_int64() for _ in range(3)]
        ms = ctypes.c_double()
        self._check(self._lib.komb_max_clique_info(self._ctx, *(ctypes.byref(x) for x in i32 + i64), ctypes.byref(ms)))
        return dict(zip(self.MAX_CLIQUE_INFO_FIELDS, [x.value for x in i32 + i64] + [ms.value]))

    def max_clique_fetch(self):
        """(count int32[nv], witness int32[omega]): the maximum cliques through every vertex (1 on the witness without the
        ENUMERATED flag) and one clique of omega vertices, ascending."""
        omega = self.max_clique_info()["omega"]
        count = _out_i32(max(self.nv, 0))
        witness = _out_i32(omega)
        self._check(self._lib.komb_max_clique_fetch(self._ctx, ptr(count), ptr(witness)))
        return count, witness

    def max_clique_list(self):
        """int32[n_max_cliques, omega]: every maximum clique as an ascending tuple, in lexicographic order (KOMB_ERR_LIMIT
        when the list was not kept)."""
        omega = self.max_clique_info()["omega"]
        n = ctypes.c_int64()
        self._check(self._lib.komb_max_clique_list(self._ctx, 0, ctypes.byref(n), None))
        verts = _out_i32(n.value * omega)
        self._check(self._lib.komb_max_clique_list(self._ctx, n.value, ctypes.byref(n), ptr(verts)))
        return verts.reshape(n.value, omega)

    def run_max_clique(self, budget=0):
        """(info, count, witness) of a maximum-clique search of the last k-truss result."""
        self.max_clique_run(budget)
        count, witness = self.max_clique_fetch()
        return self.max_clique_info(), count, witness

    # ---- clique census: exact k-clique counts of the last k-truss result for every k of a window (include/komb_accel.h)
    CLIQUE_CENSUS_INFO_FIELDS = ("k_lo", "k_hi", "k_local", "t_max", "omega", "flags", "max_candidates", "n_roots", "nodes", "ms")

    def clique_census_run(self, k_lo=2, k_hi=-1, k_local=0, budget=0):
        """Needs a complete k-truss result on this graph.  k_hi = -1: up to t_max; k_local: 0, or the size whose cliques are
        counted per vertex; budget: the node cap of the run, 0 for the default."""
        self._sync_env_options()
        self._check(self._lib.komb_clique_census_run(self._ctx, k_lo, k_hi, k_local, budget))

    def clique_census_info(self):
        """{"k_lo", "k_hi", "k_local", "t_max", "omega", "flags", "max_candidates", "n_roots", "nodes", "ms"} of the last
        komb_clique_census_run; k_hi is the one the run used."""
        i32 = [ctypes.c_int32() for _ in range(7)]
        i64 = [ctypes.c_int64() for _ in range(2)]
        ms = ctypes.c_double()
        self._check(self._lib.komb_clique_census_info(self._ctx, *(ctypes.byref(x) for x in i32 + i64), ctypes.byref(ms)))
        return dict(zip(self.CLIQUE_CENSUS_INFO_FIELDS, [x.value for x in i32 + i64] + [ms.value]))

    def clique_census_fetch(self):
        """(total uint64[k_hi - k_lo + 1], local uint64[nv] or None): the k-cliques for k = k_lo .. k_hi and, after a run with
        a k_local, the k_local-cliques through every vertex; every entry saturates at 2^64 - 1."""
        info = self.clique_census_info()
        total = _out_u64(info["k_hi"] - info["k_lo"] + 1)
        local = _out_u64(max(self.nv, 0)) if info["k_local"] else None
        self._check(self._lib.komb_clique_census_fetch(self._ctx, ptr(total), ptr(local)))
        return total, local

    def run_clique_census(self, k_lo=2, k_hi=-1, k_local=0, budget=0):
        """(total, local, info) of a clique census of the last k-truss result."""
        self.clique_census_run(k_lo, k_hi, k_local, budget)
        total, local = self.clique_census_fetch()
        return total, local, self.clique_census_info()

    # ---- maximal cliques of the last k-truss result: Bron-Kerbosch with pivoting (include/komb_accel.h)
    MAXIMAL_CLIQUES_INFO_FIELDS = ("k_min", "k_hi", "t_max", "omega", "flags", "n_cliques", "max_candidates", "n_roots", "nodes", "ms")

    def maximal_cliques_run(self, k_min=2, budget=0):
        """Needs a complete k-truss result on this graph.  k_min: the smallest clique reported; budget: the node cap of the
        run, 0 for the default."""
        self._sync_env_options()
        self._check(self._lib.komb_maximal_cliques_run(self._ctx, k_min, budget))

    def maximal_cliques_info(self):
        """{"k_min", "k_hi", "t_max", "omega", "flags", "n_cliques", "max_candidates", "n_roots", "nodes", "ms"} of the last
        komb_maximal_cliques_run."""
        i32 = [ctypes.c_int32() for _ in range(5)]
        n, mc = ctypes.c_int64(), ctypes.c_int32()
        i64 = [ctypes.c_int64() for _ in range(2)]
        ms = ctypes.c_double()
        self._check(self._lib.komb_maximal_cliques_info(self._ctx, *(ctypes.byref(x) for x in i32 + [n, mc] + i64), ctypes.byref(ms)))
        return dict(zip(self.MAXIMAL_CLIQUES_INFO_FIELDS, [x.value for x in i32 + [n, mc] + i64] + [ms.value]))

    def maximal_cliques_fetch(self):
        """(hist int64[k_hi - k_min + 1], count int32[nv], largest int32[nv]): the reported cliques of k_min + i vertices, the
        ones through every vertex and the size of the largest of those."""
        info = self.maximal_cliques_info()
        hist = np.full(info["k_hi"] - info["k_min"] + 1, SENTINEL_I32, dtype=np.int64)
        count = _out_i32(max(self.nv, 0))
        largest = _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_maximal_cliques_fetch(self._ctx, ptr(hist), ptr(count), ptr(largest)))
        return hist, count, largest

    def maximal_cliques_list(self):
        """(offset int64[n_cliques + 1], verts int32[n_verts]): every reported clique as an ascending tuple
        verts[offset[i]:offset[i + 1]], in lexicographic order (KOMB_ERR_LIMIT when the list was not kept)."""
        n, nw = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.komb_maximal_cliques_list(self._ctx, 0, 0, ctypes.byref(n), ctypes.byref(nw), None, None))
        offset = np.full(n.value + 1, SENTINEL_I32, dtype=np.int64)
        verts = _out_i32(nw.value)
        self._check(self._lib.komb_maximal_cliques_list(self._ctx, n.value, nw.value, ctypes.byref(n), ctypes.byref(nw), ptr(offset), ptr(verts)))
        return offset, verts

    def run_maximal_cliques(self, k_min=2, budget=0):
        """(hist, count, largest, info) of the maximal cliques of the last k-truss result."""
        self.maximal_cliques_run(k_min, budget)
        return self.maximal_cliques_fetch() + (self.maximal_cliques_info(),)

    # ---- k-clique communities of the held maximal cliques: clique percolation (include/komb_accel.h)
    CLIQUE_COMMUNITIES_INFO_FIELDS = ("k", "k_min", "n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap", "pair_tests", "ms")

    def clique_communities_run(self, k=3, budget=0):
        """Needs the list of a komb_maximal_cliques_run with k_min <= k on the current k-truss result.  budget: the cap on
        pair_tests, 0 for the default."""
        self._sync_env_options()
        self._check(self._lib.komb_clique_communities_run(self._ctx, k, budget))

    def clique_communities_info(self):
        """{"k", "k_min", "n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap", "pair_tests", "ms"} of the
        last komb_clique_communities_run."""
        i32 = [ctypes.c_int32() for _ in range(2)]
        i64 = [ctypes.c_int64() for _ in range(6)]
        ms = ctypes.c_double()
        self._check(self._lib.komb_clique_communities_info(self._ctx, *(ctypes.byref(x) for x in i32 + i64), ctypes.byref(ms)))
        return dict(zip(self.CLIQUE_COMMUNITIES_INFO_FIELDS, [x.value for x in i32 + i64] + [ms.value]))

    def clique_communities_count(self):
        """(n_communities, n_member_verts)."""
        n, nw = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.komb_clique_communities_count(self._ctx, ctypes.byref(n), ctypes.byref(nw)))
        return n.value, nw.value

    def clique_communities_fetch(self):
        """(label int32[n_cliques of the list], size int32[same]): the rep of every clique's community (-1 for a clique of
        fewer than k vertices) and the number of cliques of that community (0)."""
        self.clique_communities_count()                    # (the state check, before the list is asked for its length)
        n = ctypes.c_int64()
        self._check(self._lib.komb_maximal_cliques_list(self._ctx, 0, 0, ctypes.byref(n), None, None, None))
        label, size = _out_i32(n.value), _out_i32(n.value)
        self._check(self._lib.komb_clique_communities_fetch(self._ctx, ptr(label), ptr(size)))
        return label, size

    def clique_communities_fetch_communities(self):
        """(rep int32[n], n_cliques int32[n], offset int64[n + 1], verts int32[n_member_verts]): community c is
        verts[offset[c]:offset[c + 1]], ascending and distinct."""
        n, nw = self.clique_communities_count()
        rep, ncl = _out_i32(n), _out_i32(n)
        offset = np.full(n + 1, SENTINEL_I32, dtype=np.int64)
        verts = _out_i32(nw)
        self._check(self._lib.komb_clique_communities_fetch_communities(self._ctx, ptr(rep), ptr(ncl), ptr(offset), ptr(verts)))
        return rep, ncl, offset, verts

    def clique_communities_fetch_vertices(self):
        """(n_comm int32[nv], first int32[nv]): how many communities contain the vertex and the smallest of them (-1)."""
        n_comm, first = _out_i32(max(self.nv, 0)), _out_i32(max(self.nv, 0))
        self._check(self._lib.komb_clique_communities_fetch_vertices(self._ctx, ptr(n_comm), ptr(first)))
        return n_comm, first

    def run_clique_communities(self, k=3, budget=0):
        """(label, size, rep, n_cliques, offset, verts, n_comm, first, info) of the k-clique communities of the held maximal
        cliques."""
        self.clique_communities_run(k, budget)
        return (self.clique_communities_fetch() + self.clique_communities_fetch_communities() + self.clique_communities_fetch_vertices()
                + (self.clique_communities_info(),))

    # ---- CoreA (a9 + a10)
    def get_anomaly_score(self, degree, coreness):
        degree = as_c(degree, np.int32)
        coreness = as_c(coreness, np.int32)
        score = _out_f64(len(degree))
        self._sync_env_options()
        self._check(self._lib.komb_corea_scores(self._ctx, ptr(degree), ptr(coreness), len(degree), ptr(score)))
        return score

    def fractional_ranks(self, degree, coreness):
        degree = as_c(degree, np.int32)
        coreness = as_c(coreness, np.int32)
        rd = _out_f64(len(degree))
        rk = _out_f64(len(degree))
        self._sync_env_options()
        self._check(self._lib.komb_corea_ranks(self._ctx, ptr(degree), ptr(coreness), len(degree), ptr(rd), ptr(rk)))
        return rd, rk

    def densest_block(self, suspiciousness=None):
        """komb_densest_block: (order int32[2*nv], side int32[2*nv], n_block, max_density) of the resident graph."""
        n = int(self.nv)
        # (every one of the 2*nv entries is written: the peel removes every row and every column node once)
        order = _out_i32(max(2 * n, 1))
        side = _out_i32(max(2 * n, 1))
        self._sync_env_options()
        nb = ctypes.c_int64(0)
        dens = ctypes.c_double(0.0)
        susp = None if suspiciousness is None else as_c(suspiciousness, np.float64)
        self._check(self._lib.komb_densest_block(self._ctx, ptr(susp), ptr(order), ptr(side), ctypes.byref(nb), ctypes.byref(dens)))
        return order[: 2 * n], side[: 2 * n], int(nb.value), float(dens.value)

    def stats(self):
        st = KombStats()
        self._check(self._lib.komb_get_stats(self._ctx, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in KombStats._fields_}
