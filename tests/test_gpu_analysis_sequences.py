"""One context under seeded random plans over every entry point: all nineteen results of a komb_ctx in one sequence.

The per-analysis files test each analysis in depth, in its own file and in a fixed order.  Here the plans of
tests/sequence_model.py (make_plan: 8 graphs per plan, larger and smaller in turn, graphs whose arrays land in each other's
pool blocks) are driven through ONE KombAccel, so that analysis A's block, with A's plausible leftovers of another graph of
similar size in it, is handed to analysis B -- the [nv][64] doubles of betweenness and the all-ones masks of distances to the
peel, union-find and clique kernels, and theirs to seen[], front[], hpart[], sigma and delta; every lazily made array is first
asked for by each of its consumers; and every cell of the header's drop / keep table is exercised.  After every operation: the
status code is the model's (the model is written from include/komb_accel.h); a refused call has written nothing (every output
starts as 0xA5 bytes, with room for the largest output any reader writes); komb_stats is unchanged where the header says so;
what is held equals the references -- base inputs from the oracle, results from the restatements tests/*_ref.py through the
comparers of the per-analysis files -- exactly, every array and every integer of info, bc[] and harmonic[] as raw 64-bit
patterns.  The graphlet census, betweenness and distances are fed the oracle's CSR and canonical edges here, never the
library's own.  "stale" sets no POISON: a reused block holds real leftovers; "poisoned" starts at 0xFFFFFFFF and changes the
word between steps.  No call here fails an allocation or faults: every refusal is an ordinary error return.

A failure names the seed, the index of the operation and the plan up to it as a Python literal; replay it with
    run_plan(K, O, monkeypatch, seed, prefix, poisoned)
(seed: the ids of every graph but A-D are permuted by it, and the source lists follow the ids).

Figures, as measured:
  operations per plan: 591 / 585 / 587 / 577 (seeds 11, 23, 37, 41), 8 graphs each, 60 .. 85 per graph;
  coverage() of the four plans (tests/test_sequence_model_ref.py asserts the conditions): every run 32 .. 86 times (the census
  36, betweenness and distances 45 each); 96 / 96 drop cells probed, 470 / 470 keep cells verified; each of the twelve consumers
  of the canonical edge list first 2 .. 4 times and later 4 .. 68 times (the census 2 and 22); the canonical supports first by
  komb_truss_fetch_support 47 times, by a structural run 15 times, by the census 5 times; the communities' vertex pass first by
  fetch_vertices 19 times, by info 9 times; each refusable run refused with its result held and verified afterwards 2 .. 18
  times (betweenness and distances 18 each); each consumer straight after unprepare + truss_run 1 .. 2 times, betweenness and
  distances held across the pair and read after it 16 times each; source lists of 0 / 1 / 3 / 65 / 257 entries and every
  vertex: betweenness 16 / 3 / 1 / 11 / 8 / 6 runs, distances 17 / 3 / 1 / 11 / 8 / 5; the reuse transitions B->A 2, A->B 1,
  A|B->C 3, E->E' 2 times;
  reference CPU seconds per graph (one thread, the restatements alone, summed over what one plan asks of the graph; the
  oracle's base inputs of all 15 graphs take 0.3 .. 0.7 s per plan): A 0.09 .. 0.72, B 0.13 .. 0.54, C 0.14 .. 0.95,
  D 0.77 .. 2.27, E (K_60, 487 635 4-cliques) 2.2 .. 2.5, the strided-claim graph (524 549 vertices: its adjacency lists, the
  sparse census and three searches) 4.3, every other graph under 0.1; per plan 3.9 / 1.4 / 6.6 / 7.4 s, paid once per seed by
  the module's cache, so by the "stale" test of the seed;
  a run from any vertex of the strip C (about 4500 levels) takes 0.17 s (distances) and 0.73 s (betweenness) on the MI355X, with
  which the poisoned tests took 1.4 .. 1.5 s: C has the empty source list only (sequence_model.SOURCE_LENGTHS);
  wall time per test on the MI355X: see WALL_SECONDS below.
"""
import ctypes
import os
import time

import numpy as np
import pytest

import sequence_model as SM

import betweenness_ref
import biconnected_ref
import clique_census_ref
import clique_communities_ref
import community_hierarchy_ref
import components_ref
import densest_ref
import distances_ref
import graphlets_ref
import hierarchy_ref
import max_clique_ref
import maximal_cliques_ref
import nucleus_hierarchy_ref
import nucleus_ref
import onion_ref
import structural_ref
import truss_communities_ref

import test_gpu_betweenness as T_btw
import test_gpu_biconnected as T_bic
import test_gpu_clique_census as T_cens
import test_gpu_clique_communities as T_perc
import test_gpu_community_hierarchy as T_chier
import test_gpu_components as T_comp
import test_gpu_densest as T_dens
import test_gpu_dirty_memory as T_dirty
import test_gpu_distances as T_dist
import test_gpu_graphlets as T_gl
import test_gpu_hierarchy as T_hier
import test_gpu_max_clique as T_mclq
import test_gpu_maximal_cliques as T_mxl
import test_gpu_nucleus as T_nuc
import test_gpu_nucleus_hierarchy as T_nhier
import test_gpu_structural as T_sc
import test_gpu_truss_communities as T_comm

pytestmark = pytest.mark.gpu

OK, ARG, STATE = SM.OK, SM.ARG, SM.STATE

# wall seconds of test_sequence[seed-mode] on the MI355X, as measured (the stale test of a seed computes the seed's references)
WALL_SECONDS = {(11, "stale"): 5.00, (11, "poisoned"): 0.58, (23, "stale"): 2.00, (23, "poisoned"): 0.47, (37, "stale"): 7.19, (37, "poisoned"): 0.49,
                (41, "stale"): 8.02, (41, "poisoned"): 0.51, "test_full_caps_reserves_the_bounds_at_once": 0.19}
REFERENCE_SECONDS = {}


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


_GRAPHS = {}


def graphs_of(K, O, seed):
    """The graphs of one plan with everything the oracle says about them; kept for the module, shared by both modes."""
    if seed not in _GRAPHS:
        _GRAPHS[seed] = SM.build_graphs(K.gen_hug_edges, O, seed)
    return _GRAPHS[seed]


# ---- every reader of every result: (function, by-value arguments); the outputs are made by _probe from the signature
BIG = 1 << 20
READERS = {
    "core": (("komb_core_fetch", ()),),
    "onion": (("komb_onion_fetch", ()), ("komb_onion_info", ())),
    "comp": (("komb_components_fetch", ()), ("komb_components_info", ())),
    "hier": (("komb_hierarchy_count", ()), ("komb_hierarchy_fetch_nodes", ()), ("komb_hierarchy_fetch_vertices", ()), ("komb_hierarchy_info", ())),
    "dens": (("komb_densest_subgraph_fetch", ()), ("komb_densest_subgraph_profile", ()), ("komb_densest_subgraph_info", ())),
    "truss": (("komb_truss_count", ()), ("komb_truss_fetch", ()), ("komb_truss_fetch_support", ())),
    "comm": (("komb_truss_communities_fetch", ()), ("komb_truss_communities_fetch_vertices", ()), ("komb_truss_communities_info", ())),
    "bic": (("komb_biconnected_count", ()), ("komb_biconnected_fetch_edges", ()), ("komb_biconnected_fetch_vertices", ()),
            ("komb_biconnected_fetch_blocks", ()), ("komb_biconnected_info", ())),
    "chier": (("komb_community_hierarchy_count", ()), ("komb_community_hierarchy_fetch_nodes", ()), ("komb_community_hierarchy_fetch_edges", ()),
              ("komb_community_hierarchy_labels", (3,)), ("komb_community_hierarchy_info", ())),
    "sc": (("komb_structural_clusters_fetch", ()), ("komb_structural_clusters_fetch_edges", ()), ("komb_structural_clusters_info", ())),
    "nuc": (("komb_nucleus_count", ()), ("komb_nucleus_fetch", ()), ("komb_nucleus_fetch_edges", ()), ("komb_nucleus_fetch_vertices", ()),
            ("komb_nucleus_info", ())),
    "nhier": (("komb_nucleus_hierarchy_count", ()), ("komb_nucleus_hierarchy_fetch_nodes", ()), ("komb_nucleus_hierarchy_fetch_triangles", ()),
              ("komb_nucleus_hierarchy_labels", (1,)), ("komb_nucleus_hierarchy_nuclei", (1, BIG)), ("komb_nucleus_hierarchy_info", ())),
    "mclq": (("komb_max_clique_fetch", ()), ("komb_max_clique_list", (BIG,)), ("komb_max_clique_info", ())),
    "cens": (("komb_clique_census_fetch", ()), ("komb_clique_census_info", ())),
    "mxl": (("komb_maximal_cliques_fetch", ()), ("komb_maximal_cliques_list", (BIG, BIG)), ("komb_maximal_cliques_info", ())),
    "perc": (("komb_clique_communities_count", ()), ("komb_clique_communities_fetch", ()), ("komb_clique_communities_fetch_communities", ()),
             ("komb_clique_communities_fetch_vertices", ()), ("komb_clique_communities_info", ())),
    "gl": (("komb_graphlets_fetch_vertices", ()), ("komb_graphlets_fetch_edges", ()), ("komb_graphlets_info", ())),
    "btw": (("komb_betweenness_fetch", ()), ("komb_betweenness_fetch_sources", ()), ("komb_betweenness_info", ())),
    "dist": (("komb_distances_fetch", ()), ("komb_distances_fetch_sources", ()), ("komb_distances_histogram", (BIG,)), ("komb_distances_info", ())),
}
assert set(READERS) == set(SM.RESULTS) and set(SM.STATS_FROZEN) >= {"gl", "btw", "dist"}


class _Held:
    """The context for a comparer that runs the analysis before it fetches: here the run is the one the plan made."""

    def __init__(self, a):
        self.a, self.nv = a, a.nv

    def run_graphlets(self):
        cycles4, cliques4 = self.a.graphlets_fetch_edges()
        return self.a.graphlets_fetch_vertices(), cycles4, cliques4, self.a.graphlets_info()


def _probe(K, a, fname, byval, nbytes):
    """One raw call with every output a block of 0xA5 bytes: (status, whether every output is still untouched)."""
    _, args = K._lib.SIGNATURES[fname]
    call, arrays, scalars, byval = [a._ctx], [], [], list(byval)
    for t in args[1:]:
        if t is ctypes.c_void_p:
            arrays.append(np.full(nbytes, 0xA5, np.uint8))
            call.append(K._lib.ptr(arrays[-1]))
        elif isinstance(t, type) and issubclass(t, ctypes._Pointer):
            x = (t._type_ * 16)()                        # (one value, or the nine totals of komb_graphlets_info)
            ctypes.memset(x, 0xA5, ctypes.sizeof(x))
            scalars.append(x)
            call.append(x)
        else:
            call.append(byval.pop(0))
    rc = getattr(K._lib.load(), fname)(*call)
    clean = all(bool((b.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all()) for b in arrays) and all(bytes(x) == b"\xa5" * ctypes.sizeof(x) for x in scalars)
    return rc, clean


class _Fixed:
    """The rng of test_gpu_dirty_memory._fetch_varied, answering the order the plan names."""

    def __init__(self, order):
        self.order = order

    def integers(self, lo, hi):
        return self.order


class Driver:
    def __init__(self, K, O, monkeypatch, seed, poisoned):
        self.K, self.mp, self.poisoned = K, monkeypatch, poisoned
        self.graphs = graphs_of(K, O, seed)
        self.model = SM.Model()
        self.lib = K._lib.load()
        for name in SM.OPTIONS:
            for n in name.split("+"):
                monkeypatch.delenv("KOMB_" + n, raising=False)
        for name in T_dirty._SWITCHES:
            monkeypatch.delenv("KOMB_" + name, raising=False)
        if poisoned:
            monkeypatch.setenv("KOMB_POISON", SM.POISON_WORDS[0])
        self.a = K.KombAccel()
        self.checkpoints, self.after_load = {}, {}
        self.dist_words = None                           # the DIST_WORDS in force when the held distance result was made

    def close(self):
        self.a.close()

    # ---- helpers
    @property
    def g(self):
        return self.graphs[self.model.graph]

    def _code(self, call):
        try:
            call()
        except self.K.KombError as e:
            return e.code
        return OK

    def _mask(self, g, tag):
        return None if tag is None or g is None else g.masks[tag]

    def _k(self, k, top):
        return top + 1 if k == "above" else k

    def _nbytes(self):
        """Room for the largest output any reader can write: the fifteen orbits of every vertex."""
        g = self.graphs.get(self.model.graph)
        return 64 + 8 * (max(15 * g.nv, 4 * g.ne(), 1024) if g is not None else 1 << 16)

    # ---- one operation: the status code it answered (verification of what it read inside)
    def execute(self, op, want):
        a, name = self.a, op[0]
        return getattr(self, "x_" + name)(a, want, *op[1:])

    def x_load(self, a, want, gname, how):
        g = self.graphs[gname]
        rc = self._code((lambda: a.from_edges(g.nv, g.uv)) if how == "edges" else (lambda: a.from_csr(g.rowptr, g.col)))
        if rc == OK:
            assert (a.nv, a.ne) == (g.nv, g.ne())
            # everything of the graph before is gone: a context holds the same blocks after every load of the same graph
            blocks = a.alloc_info()["pool_blocks_in_use"]
            assert self.after_load.setdefault((gname, how), blocks) == blocks, ("pool blocks in use after the load", gname, how)
        return rc

    def x_load_bad(self, a, want, gname):
        g = self.graphs[gname]
        rc = self._code(lambda: a.from_edges(g.nv, np.concatenate([g.uv, [[0, g.nv]]]).astype(np.int64)))
        a.nv, a.ne = -1, 0
        assert self._code(a._info) == STATE                                  # komb_graph_info: no graph
        return rc

    def x_core(self, a, want, how):
        if how == "plain":
            return self._code(a.core_run)
        a._sync_env_options()
        return self.lib.komb_core_run_sharded(a._ctx, *((0, 1) if how == "sharded" else (1, 1)), None, None)

    def x_onion(self, a, want):
        return self._code(a.onion_run)

    def x_comp(self, a, want, kind, k):
        g = self.graphs.get(self.model_before_graph)
        if k == "above":
            k = 3 if g is None else (g.k_max_core() if kind == "core" else g.t_max(self.mask_before, 2)) + 1
        return self._code(lambda: a.components_run(kind, k))

    def x_hier(self, a, want, kind):
        return self._code(lambda: a.hierarchy_run(kind))

    def x_dens(self, a, want, iters):
        return self._code(lambda: a.densest_subgraph_run(iters))

    def x_truss(self, a, want, how, mask):
        m = self._mask(self.graphs.get(self.model_before_graph), mask)
        if how == "plain":
            return self._code(lambda: a.truss_run(m))
        a._sync_env_options()
        return self.lib.komb_truss_run_sharded(a._ctx, self.K._lib.ptr(m), 0, 1, None, None)

    def x_slice(self, a, want, rank, world, mask):
        m = self._mask(self.graphs.get(self.model_before_graph), mask)
        return self._code(lambda: a.truss_run_slice(rank, world, m))

    def x_prepare(self, a, want):
        return self._code(a.truss_prepare)

    def x_unprepare(self, a, want):
        return self._code(a.truss_unprepare)

    def _t_above(self, k, floor):
        g = self.graphs.get(self.model_before_graph)
        return g.t_max(self.mask_before, floor) + 1 if k == "above" and g is not None else (3 if k == "above" else k)

    def x_comm(self, a, want, k):
        return self._code(lambda: a.truss_communities_run(self._t_above(k, 2)))

    def x_bic(self, a, want, k):
        return self._code(lambda: a.biconnected_run(self._t_above(k, 2)))

    def x_chier(self, a, want):
        return self._code(a.community_hierarchy_run)

    def x_sc(self, a, want, *params):
        return self._code(lambda: a.structural_clusters_run(*params))

    def x_nuc(self, a, want):
        return self._code(a.nucleus_run)

    def x_nhier(self, a, want):
        return self._code(a.nucleus_hierarchy_run)

    def x_mclq(self, a, want, budget):
        return self._code(lambda: a.max_clique_run(budget))

    def x_cens(self, a, want, k_lo, k_hi, k_local):
        return self._code(lambda: a.clique_census_run(k_lo, k_hi, k_local))

    def x_mxl(self, a, want, k_min):
        return self._code(lambda: a.maximal_cliques_run(k_min))

    def x_perc(self, a, want, k):
        return self._code(lambda: a.clique_communities_run(self._t_above(k, 4)))

    def x_gl(self, a, want):
        return self._code(a.graphlets_run)

    def _sources_run(self, a, spec, run, raw):
        """A good spec through the wrapper; a bad one through the raw call, as the per-analysis error tests make it."""
        g = self.graphs.get(self.model_before_graph)
        if spec == "all" or spec[0] == "prefix":
            return self._code(lambda: run(None if g is None else g.sources(spec)))
        nv = 0 if g is None else g.nv
        n, ids = {"id_high": (3, [0, nv, 1]), "id_negative": (2, [0, -1]), "count": (-1, [0, 0])}[spec[1]]
        src = np.asarray(ids, np.int32)
        a._sync_env_options()
        rc = raw(a._ctx, n, self.K._lib.ptr(src))
        assert src.tolist() == ids
        return rc

    def x_btw(self, a, want, spec):
        return self._sources_run(a, spec, a.betweenness_run, self.lib.komb_betweenness_run)

    def x_dist(self, a, want, spec):
        words = {"1": 1, "2": 2}.get(os.environ.get("KOMB_DIST_WORDS"), T_dist.DEFAULT_WORDS)
        rc = self._sources_run(a, spec, a.distances_run, self.lib.komb_distances_run)
        if rc == OK:
            self.dist_words = words
        return rc

    def x_option(self, a, want, name, value):
        names = name.split("+")
        for n, v in zip(names, [None] * len(names) if value is None else value.split("+")):
            if v is None:
                self.mp.delenv("KOMB_" + n, raising=False)
            else:
                self.mp.setenv("KOMB_" + n, v)
        return OK

    def x_poison(self, a, want, word):
        if self.poisoned:
            self.mp.setenv("KOMB_POISON", word)
        return OK

    def x_stateless(self, a, want, name):
        g = self.graphs.get(self.model.graph)
        if name == "corea":
            rd, rk = a.fractional_ranks(g.deg, g.core)
            assert np.array_equal(rd, g.rd) and np.array_equal(rk, g.rk), "CoreA ranks"
            assert np.array_equal(a.get_anomaly_score(g.deg, g.core), g.score), "CoreA scores"
            return OK
        if want != OK:
            return self._code({"densest_block": a.densest_block, "moments": a.graph_moments, "get_csr": a.get_csr}[name])
        if name == "densest_block":
            order, side, nb, dens = a.densest_block()
            assert np.array_equal(order, g.merge[0]) and np.array_equal(side, g.merge[1]) and (nb, dens) == tuple(g.merge[2:]), "densest block"
        elif name == "moments":
            a.graph_moments()
            assert a.stats()["max_degree"] == (int(g.deg.max()) if g.ne() else 0)
        else:
            rowptr, col = a.get_csr()
            assert np.array_equal(rowptr, g.rowptr) and np.array_equal(col, g.col), "CSR"
        return OK

    def x_checkpoint(self, a, want):
        blocks = a.alloc_info()["pool_blocks_in_use"]
        key = (self.model.graph, frozenset(self.model.held))
        assert self.checkpoints.setdefault(key, blocks) == blocks, ("pool blocks in use at the checkpoint", key)
        return OK

    # ---- reads
    def x_read(self, a, want, result, arg=None):
        if want != OK:
            for fname, byval in READERS[result]:
                rc, clean = _probe(self.K, a, fname, byval, self._nbytes())
                assert clean, (fname, "a refused call wrote to its outputs")
                if rc != want:
                    return rc
            return want
        try:
            getattr(self, "v_" + result)(a, self.g, self.model.held[result], arg)
        except self.K.KombError as e:
            return e.code
        return OK

    def v_core(self, a, g, params, arg):
        deg, core = a.core_fetch()
        assert np.array_equal(deg, g.deg) and np.array_equal(core, g.core), "degree / coreness"

    def v_onion(self, a, g, params, arg):
        want, want_core, n = g.ref(("onion",), lambda: onion_ref.onion_layers(g.rowptr.astype(np.int64), g.col.astype(np.int64)))
        layer, core = a.onion_fetch()
        info = a.onion_info()
        assert layer.dtype == np.int32 and np.array_equal(layer, want), "onion layers"
        assert np.array_equal(core, want_core) and np.array_equal(core, g.core), "onion coreness"
        assert info["n_layers"] == n and info["max_coreness"] == g.k_max_core() and info["ms"] >= 0.0

    def v_comp(self, a, g, params, arg):
        kind, k, mask = params
        if kind == "core":
            kk = g.k_max_core() if k == -1 else self._k(k, g.k_max_core())
            want = g.ref(("comp", kind, kk), lambda: components_ref.core_components(g.rowptr, g.col, g.core, kk))
        else:
            eu, ev, tr, _ = g.base[mask]
            kk = g.t_max(mask, 2) if k == -1 else self._k(k, g.t_max(mask, 2))
            want = g.ref(("comp", kind, kk, mask), lambda: components_ref.truss_components(g.nv, eu, ev, tr, kk))
        T_comp._compare(a, kind, k, want, k_used=kk)

    def v_hier(self, a, g, params, arg):
        kind, mask = params
        if kind == "core":
            want = g.ref(("hier", kind), lambda: hierarchy_ref.core_hierarchy(g.rowptr, g.col, g.core))
        else:
            eu, ev, tr, _ = g.base[mask]
            want = g.ref(("hier", kind, mask), lambda: hierarchy_ref.truss_hierarchy(g.nv, eu, ev, tr))
        T_hier._compare(a, kind, want)

    def v_dens(self, a, g, params, arg):
        want = g.ref(("dens",) + params, lambda: densest_ref.densest(g.rowptr, g.col, g.core, params[0]))
        T_dens._same(T_dens._fetch_all(a), want, ("densest", params))

    def v_truss(self, a, g, params, arg):
        mask, lo, hi = params
        weu, wev, wtr, wsup = g.base[mask]
        hi = len(wtr) if hi is None else hi
        eu, ev, tr, sup = T_dirty._fetch_varied(a, _Fixed(arg or 0))
        assert np.array_equal(eu, weu) and np.array_equal(ev, wev), "canonical edge list"
        assert np.array_equal(tr[lo:hi], wtr[lo:hi]), "trussness"
        assert np.array_equal(sup[lo:hi], wsup[lo:hi]), "supports"
        assert not tr[:lo].any() and not tr[hi:].any() and not sup[:lo].any() and not sup[hi:].any(), "outside the slice"
        if mask is None and len(wtr):
            assert a.stats()["triangles"] == g.tri, "triangles"

    def v_comm(self, a, g, params, arg):
        k, mask = params
        eu, ev, tr, _ = g.base[mask]
        k = self._k(k, g.t_max(mask, 2))
        kk = T_comm._resolve(k, tr)
        tri = g.ref(("triangles", mask), lambda: truss_communities_ref.triangles(g.nv, eu, ev))
        want = g.ref(("comm", kk, mask), lambda: truss_communities_ref.communities(g.nv, eu, ev, tr, kk, tri))
        if arg == "vertices":
            a.truss_communities_fetch_vertices()
        elif arg == "info":
            a.truss_communities_info()
        T_comm._compare(a, k, eu, ev, tr, tri, want)

    def v_bic(self, a, g, params, arg):
        k, mask = params
        eu, ev, tr, _ = g.base[mask]
        k = self._k(k, g.t_max(mask, 2))
        kk = T_bic._resolve(k, tr)
        want = g.ref(("bic", kk, mask), lambda: biconnected_ref.biconnected(g.nv, eu, ev, tr, kk))
        T_bic._compare(a, k, eu, ev, tr, want=want)

    def v_chier(self, a, g, params, arg):
        mask, = params
        eu, ev, tr, _ = g.base[mask]
        want = g.ref(("chier", mask), lambda: community_hierarchy_ref.community_hierarchy(g.nv, eu, ev, tr))
        T_chier._compare(a, want)
        k = self._k(arg if arg is not None else 3, g.t_max(mask, 2))
        kk = g.t_max(mask, 2) if k == -1 else k
        wl, ws = community_hierarchy_ref.walk_up(want, tr, kk)
        label, size = a.community_hierarchy_labels(k)
        assert label.dtype == np.int32 and np.array_equal(label, wl) and np.array_equal(size, ws), ("community_hierarchy_labels", k)

    def v_sc(self, a, g, params, arg):
        p, mask = params[:3], params[3]
        eu, ev, _, sup = g.base[mask]
        want = g.ref(("sc", p, mask), lambda: structural_ref.clusters(g.nv, eu, ev, sup, *p))
        T_sc._compare(a, eu, ev, sup, p, want)

    def _nuc(self, g, mask):
        eu, ev, _, _ = g.base[mask]
        return g.ref(("nuc", mask), lambda: nucleus_ref.decompose(g.nv, eu, ev))

    def v_nuc(self, a, g, params, arg):
        T_nuc._compare(a, g.ne(params[0]), self._nuc(g, params[0]))

    def v_nhier(self, a, g, params, arg):
        mask, = params
        eu, ev, _, _ = g.base[mask]
        theta = self._nuc(g, mask)["theta"]
        h, dec = g.ref(("nhier", mask), lambda: nucleus_hierarchy_ref.hierarchy(g.nv, eu, ev, theta))
        T_nhier._compare_forest(a, h, dec)
        top = int(dec["theta"].max()) if len(dec["theta"]) else -1
        k = self._k(arg if arg is not None else 1, top)
        wl, ws = nucleus_hierarchy_ref.walk_up(h, dec["theta"], k)
        label, size = a.nucleus_hierarchy_labels(k)
        assert label.dtype == np.int32 and np.array_equal(label, wl) and np.array_equal(size, ws), ("nucleus_hierarchy_labels", k)
        got, want = a.nucleus_hierarchy_nuclei(k), nucleus_hierarchy_ref.nuclei(h, dec, k)
        for name in nucleus_hierarchy_ref.NUCLEI_FIELDS:
            assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), ("nucleus_hierarchy_nuclei", k, name)

    def v_mclq(self, a, g, params, arg):
        mask, = params
        eu, ev, _, _ = g.base[mask]
        T_mclq._compare(a, g.ref(("mclq", mask), lambda: max_clique_ref.solve(g.nv, eu, ev)))

    def v_cens(self, a, g, params, arg):
        k_lo, k_hi, k_local, mask = params
        eu, ev, _, _ = g.base[mask]
        T_cens._compare(a, g.ref(("cens",) + params, lambda: clique_census_ref.census(g.nv, eu, ev, k_lo, k_hi, k_local)))

    def _mxl(self, g, k_min, mask):
        eu, ev, _, _ = g.base[mask]
        return g.ref(("mxl", k_min, mask), lambda: maximal_cliques_ref.solve(g.nv, eu, ev, k_min))

    def v_mxl(self, a, g, params, arg):
        T_mxl._compare(a, self._mxl(g, *params))

    def v_perc(self, a, g, params, arg):
        k, k_min, mask = params
        k = self._k(k, g.t_max(mask, 4))
        cliques = self._mxl(g, k_min, mask)["cliques"]
        want, tests = g.ref(("perc", k, k_min, mask), lambda: (clique_communities_ref.solve(g.nv, cliques, k),
                                                               clique_communities_ref.pair_tests(cliques, k)))
        T_perc._compare(a, want, tests)

    def v_gl(self, a, g, params, arg):
        mask, = params
        eu, ev, _, sup = g.base[mask]
        want, items = g.ref(("gl", mask), lambda: (graphlets_ref.census(g.nv, eu, ev), graphlets_ref.ordered_items(g.nv, eu, ev)))
        T_gl._compare(_Held(a), eu, ev, sup, want, items)

    def _rows(self, g):
        """The adjacency lists of the oracle's CSR (never the library's own)."""
        return g.ref(("rows",), lambda: betweenness_ref.rows_of_csr(g.rowptr.tolist(), g.col.tolist()))

    def v_btw(self, a, g, spec, arg):
        rows = self._rows(g)
        want = g.ref(("btw", spec), lambda: betweenness_ref.betweenness(rows, g.sources(spec), cache=g.searches["btw"]))
        T_btw._same((a.betweenness_fetch(), a.betweenness_fetch_sources(), a.betweenness_info()), want)

    def v_dist(self, a, g, spec, arg):
        words = self.dist_words                          # (n_batches and n_level_steps follow it; harmonic[] must not)
        rows = self._rows(g)
        want = g.ref(("dist", spec, words), lambda: distances_ref.distances(rows, g.sources(spec), words, cache=g.searches["dist"]))
        T_dist._same((a.distances_fetch(), a.distances_fetch_sources(), a.distances_histogram(), a.distances_info()), want)

    # ---- one step
    def step(self, op):
        m = self.model
        self.model_before_graph = m.graph
        self.mask_before = m.truss["mask"] if m.truss else None
        frozen = op[0] in SM.STATS_FROZEN
        st = self.a.stats() if frozen else None
        want = m.apply(op)
        got = self.execute(op, want)
        assert got == want, ("status", got, "the header says", want, self.a._lib.komb_last_error(self.a._ctx).decode())
        if frozen:
            assert self.a.stats() == st, "komb_stats changed"


def run_plan(K, O, monkeypatch, seed, plan, poisoned):
    """Drive one fresh context through plan; a failure carries the seed, the index and the prefix that replays it."""
    d = Driver(K, O, monkeypatch, seed, poisoned)
    try:
        for i, op in enumerate(plan):
            try:
                d.step(op)
            except Exception as e:                       # noqa: BLE001 -- every failure gets the replay line
                raise AssertionError("seed %d, %s, operation %d %r on graph %r: %s: %s\nrun_plan(K, O, monkeypatch, %d, %r, %r)"
                                     % (seed, "poisoned" if poisoned else "stale", i, op, d.model_before_graph, type(e).__name__, e,
                                        seed, plan[:i + 1], poisoned)) from e
    finally:
        d.close()
    return d


@pytest.mark.parametrize("mode", ["stale", "poisoned"])
@pytest.mark.parametrize("seed", SM.SEEDS)
def test_sequence(K, O, monkeypatch, seed, mode):
    t = time.perf_counter()
    d = run_plan(K, O, monkeypatch, seed, SM.make_plan(seed), mode == "poisoned")
    for name, g in d.graphs.items():
        REFERENCE_SECONDS[seed, name] = round(g.seconds, 2)
    # (shown with -s: the wall time of this test and the reference seconds of the seed's graphs, which the docstring quotes)
    print("test_sequence[%d-%s]: %.2f s, references so far %s" % (seed, mode, time.perf_counter() - t,
                                                                   {n: s for (sd, n), s in REFERENCE_SECONDS.items() if sd == seed and s >= 0.05}))


def test_full_caps_reserves_the_bounds_at_once(K, monkeypatch):
    """K_320 has 53 triangles per edge: the default record stream's first reservation (two per edge) runs out and the
    enumeration runs once more (test_gpu_parity.py::test_cliques_and_hubs).  FULL_CAPS=1 reserves the bounds at once: no
    retry, still a stream build, the same results."""
    n = 320
    uv = np.stack(np.triu_indices(n, 1), axis=1).astype(np.int64)
    for name in T_dirty._SWITCHES + ("FULL_CAPS",):
        monkeypatch.delenv("KOMB_" + name, raising=False)
    with K.KombAccel() as a:
        a.from_edges(n, uv)
        want = a.run_truss(with_support=True)
        st = a.stats()
        assert st["stream_retries"] == 1 and st["index_layout"] == 0, st
    monkeypatch.setenv("KOMB_FULL_CAPS", "1")
    with K.KombAccel() as a:
        a.from_edges(n, uv)
        got = a.run_truss(with_support=True)
        st = a.stats()
        assert st["stream_retries"] == 0 and st["index_layout"] == 0, st
        assert st["triangles"] == n * (n - 1) * (n - 2) // 6
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert np.all(got[2] == n) and np.all(got[3] == n - 2)
