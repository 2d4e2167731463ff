"""GPU tests of what every entry point does when a device allocation FAILS.  Option ALLOC_FAIL_AT (komb_set_option) makes
request number n of the context -- every DevPool::get and every dev_malloc counts -- return out-of-memory before anything is
allocated; komb_alloc_info reports the count, whether the trigger fired, and what the pool has handed out.

For every entry and starting state (cold: the graph was just reloaded, nothing of the entry exists; warm: the same call has
succeeded once, with other arguments where it has any) a counting run gives N, the requests of the call, twice the same; then
EVERY n in 1..N is injected -- none is skipped -- and after each failed call
  - the call has returned KOMB_ERR_NOMEM, the trigger has fired, komb_last_error is not empty;
  - no host output array was written (they are pre-filled with a sentinel);
  - the pool has no more blocks handed out than before the call, but for what the call made on its way that stays valid and
    reachable (the canonical endpoints, the supports, the preparation: Case.may_keep);
  - the entry's own previous result reads as include/komb_accel.h says: exact for the previous arguments, or KOMB_ERR_STATE
    where the header says a failed run drops it;
  - another result held on the context (k-core, or the k-truss result) is still exact;
  - the same call, repeated without injection, succeeds and is exact, and after the usual fetches the pool has as many blocks
    handed out as after the fault-free sequence (the leak check).
n = N + 1 does not fire and the call succeeds.  ALLOC_TRIM_AT=n runs the same calls warm with the pool's cached blocks given
back to the driver before request n, the effect of a request the driver refused: every call succeeds and is exact.

The input is tests/replica.py's tile (97 vertices, 564 edges); every expected value comes from the plain references
(densest_ref, onion_ref, components_ref, hierarchy_ref, truss_communities_ref, replica.py's restatements of the others on a
union of one copy, the oracle for komb_densest_block), never from an earlier GPU call.  Every comparison is exact.

komb_max_clique_list makes no device request (the list is kept on the host): it is part of komb_max_clique_run's fetches here,
and test_entries_without_a_device_request pins that it has nothing to inject into.  komb_truss_run under the default index
layout is in test_truss_run_stream_layout: its record stream is an OPTIONAL allocation by design (ktruss.hip falls back to
the exact two-pass build when the memory for it is not there), so a failure injected into one of those requests is absorbed
-- the run succeeds and is exact -- where every other request fails the run as everywhere else."""
import ctypes

import numpy as np
import pytest

import community_hierarchy_ref as CH
import components_ref as C
import corea_inputs as CI
import densest_ref as D
import hierarchy_ref as H
import maximal_cliques_ref as MQ
import nucleus_hierarchy_ref as NH
import onion_ref as ON
import replica as RP
import structural_ref as S
import truss_communities_ref as TC
from test_gpu_structural import SOME

pytestmark = pytest.mark.gpu

OK, NOMEM, STATE = 0, -3, -5
ENDPOINTS, SUPPORT, PREP, SOURCES = 2, 1, 7, 1               # pool blocks of what is made on first use and kept (common.h)
S32 = -0x5A5A5A5B                                            # 0xA5A5A5A5: what every host output starts as

TILE = RP.tile()
NV, E = TILE
U = RP.build([(TILE, 1)], "blocked")
F = RP.Frame(U, *U.canonical())                              # (the canonical list is numpy's, not the library's)
ROWPTR, COL = D.csr_of_edges(NV, E)
DEG = np.diff(ROWPTR).astype(np.int32)
CORE = np.asarray(D.coreness(ROWPTR, COL), np.int32)
K5 = RP.filler("K5")                                         # the graph a load replaces
MASKS = {3: (CORE >= 3).astype(np.uint8), 5: (CORE >= 5).astype(np.uint8)}
_REF = {}


def ref(key, fn):
    """A reference result, computed once per process and never changed."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def tri():
    return ref("triangles", lambda: RP.Triangles(F))


def induced(kc):
    """(eu, ev, trussness, support) of the subgraph induced by the vertices of coreness >= kc, original ids."""
    def make():
        keep = MASKS[kc].astype(bool)
        e = E[keep[E[:, 0]] & keep[E[:, 1]]]
        eu, ev = e[:, 0].copy(), e[:, 1].copy()
        return eu, ev, RP.tile_trussness(NV, eu, ev), S.supports(NV, eu, ev)
    return ref(("induced", kc), make)


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def i32(n):
    return np.full(max(int(n), 0), S32, np.int32)


def f64(n):
    return np.full(max(int(n), 0), np.nan, np.float64)


def p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def pristine(out):
    """Every host output of a call still holds its sentinel."""
    for name, x in out.items():
        if isinstance(x, np.ndarray):
            kept = np.isnan(x).all() if x.dtype == np.float64 else (x == S32).all()
        else:
            kept = x.value == -7
        assert kept, name


def dropped(fn):
    """The result is gone: its fetch / info answers KOMB_ERR_STATE."""
    import komb_amd
    with pytest.raises(komb_amd.KombError) as e:
        fn()
    assert e.value.code == STATE


def same(got, want):
    return np.array_equal(np.asarray(got, np.int64), np.asarray(want, np.int64))


# ---- bystanders: results of OTHER analyses a failed call must leave exact

def core_exact(a):
    deg, core = a.core_fetch()
    assert same(deg, DEG) and same(core, CORE)


def truss_exact(a):
    """The trussness of the whole-graph result (no endpoints: the first fetch that asks for them would allocate them)."""
    tr = i32(len(E))
    a.truss_fetch_into(tr=tr)
    assert same(tr, RP.trussness(F))


def truss_full(a):
    eu, ev, tr, sup = a.truss_fetch(with_support=True)
    assert same(eu, F.eu) and same(ev, F.ev) and same(tr, RP.trussness(F)) and same(sup, RP.supports(F))


def load(a):
    a.from_edges(NV, E)


def load_core(a):
    load(a)
    a.core_run()


def load_truss(a):
    load_core(a)
    a.truss_run()


def load_nucleus(a):
    load_truss(a)
    a.nucleus_run()


def forest_exact(nodes, node, want, info, info_want):
    got = dict(nodes, node=node)
    assert RP.same_forest(got, want)
    for x in H.FIELDS + ("node",):
        assert np.array_equal(got[x], want[x]), x
    assert tuple(info) == tuple(info_want)


class Case:
    """One entry point.  setup(a) reloads the graph and runs what the entry needs; earlier(a) is the warm state's first,
    successful call (other arguments, and its fetches); call(a, out) is the injected call itself, straight on the C ABI, and
    returns its code; outputs() are its host outputs, pre-filled; verify(a, out) compares the result of a successful call with
    the reference, through the usual fetches; after(a, warm) is what the entry's own result and a bystander must read as
    after a failed call."""
    states = (False, True)

    def setup(self, a):
        load_core(a)

    def earlier(self, a):
        pass

    def may_keep(self, warm):
        """Pool blocks a call that fails may leave handed out beyond what was before it: only what it made on the way that
        stays reachable and valid (the canonical endpoints, the supports, the preparation)."""
        return 0

    def outputs(self):
        return {}


def run_state(a, case, warm):
    """The sweep of one (entry, state); returns N."""
    def start():
        case.setup(a)
        if warm:
            case.earlier(a)
    counts, steady = [], None
    for turn in range(2):
        start()
        a.set_option("ALLOC_FAIL_AT", "0")
        out = case.outputs()
        assert case.call(a, out) == OK, a._lib.komb_last_error(a._ctx)
        info = a.alloc_info()
        a.set_option("ALLOC_FAIL_AT", None)
        assert info["fired"] == 0
        counts.append(info["requests"])
        case.verify(a, out)
        if turn == 0:
            steady = a.alloc_info()["pool_blocks_in_use"]
        assert a.alloc_info()["pool_blocks_in_use"] == steady
    n_req = counts[0]
    assert n_req >= 1 and counts[1] == n_req, counts
    for n in range(1, n_req + 2):
        start()
        held = a.alloc_info()["pool_blocks_in_use"]
        a.set_option("ALLOC_FAIL_AT", str(n))
        out = case.outputs()
        rc = case.call(a, out)
        err = a._lib.komb_last_error(a._ctx)
        info = a.alloc_info()
        a.set_option("ALLOC_FAIL_AT", None)
        if n <= n_req:
            assert rc == NOMEM, (n, rc, err)
            assert info["fired"] == 1 and info["requests"] == n, (n, info)
            assert err, n
            assert info["pool_blocks_in_use"] <= held + case.may_keep(warm), (n, "the failed call kept blocks of its own")
            pristine(out)
            case.after(a, warm)
            out = case.outputs()
            assert case.call(a, out) == OK, (n, a._lib.komb_last_error(a._ctx))
        else:
            assert rc == OK and info["fired"] == 0 and info["requests"] == n_req, (n, rc, info)
        case.verify(a, out)
        assert a.alloc_info()["pool_blocks_in_use"] == steady, (n, "blocks left handed out")
    return n_req


def run_trim(a, case):
    """The same call, warm, with the pool's cached blocks given back before request n, for every n."""
    case.setup(a)
    case.earlier(a)
    a.set_option("ALLOC_FAIL_AT", "0")
    assert case.call(a, case.outputs()) == OK
    n_req = a.alloc_info()["requests"]
    a.set_option("ALLOC_FAIL_AT", None)
    for n in range(1, n_req + 1):
        case.setup(a)
        case.earlier(a)
        before = a.alloc_info()["trims"]
        a.set_option("ALLOC_TRIM_AT", str(n))
        out = case.outputs()
        rc = case.call(a, out)
        info = a.alloc_info()
        a.set_option("ALLOC_TRIM_AT", None)
        assert rc == OK, (n, a._lib.komb_last_error(a._ctx))
        # (a request outside the pool -- prim_unique_u64's counter -- has nothing to give back)
        assert info["trims"] - before in ((1,) if getattr(case, "pool_requests_only", True) else (0, 1)), (n, info)
        case.verify(a, out)
    return n_req


# ---- graph

class FromEdges(Case):
    states = (False,)                                        # (a load has one starting state: another graph with a result)
    pool_requests_only = False                               # (every request of a load is a dev_malloc: nothing to trim)

    def setup(self, a):
        a.from_edges(K5[0], K5[1])
        a.core_run()

    def call(self, a, out):
        uv = np.ascontiguousarray(E, np.int64)
        return a._lib.komb_graph_from_edges(a._ctx, NV, len(uv), p(uv))

    def after(self, a, warm):                                # a failed load leaves NO graph, and so no result
        nv, ne = ctypes.c_int64(-7), ctypes.c_int64(-7)
        assert a._lib.komb_graph_info(a._ctx, ctypes.byref(nv), ctypes.byref(ne)) == STATE and (nv.value, ne.value) == (-7, -7)
        assert a._lib.komb_core_fetch(a._ctx, None, None) == STATE
        assert a.alloc_info()["pool_blocks_in_use"] == 0

    def verify(self, a, out):
        a._info()
        assert (a.nv, a.ne) == (NV, len(E))
        rowptr, col = a.get_csr()
        assert same(rowptr, ROWPTR) and same(col, COL)


class FromCsr(FromEdges):
    def call(self, a, out):
        rowptr, col = np.ascontiguousarray(ROWPTR, np.int64), np.ascontiguousarray(COL, np.int32)
        return a._lib.komb_graph_from_csr(a._ctx, NV, p(rowptr), p(col))


class Moments(Case):
    def may_keep(self, warm):
        return 0 if warm else PREP + SOURCES

    def earlier(self, a):
        a.graph_moments()

    def call(self, a, out):
        return a._lib.komb_graph_moments(a._ctx)

    def after(self, a, warm):
        core_exact(a)
        st = a.stats()
        assert st["sum_deg_sq"] == (int((DEG.astype(np.int64) ** 2).sum()) if warm else 0)

    def verify(self, a, out):
        st = a.stats()
        assert st["sum_deg_sq"] == int((DEG.astype(np.int64) ** 2).sum()) and st["max_degree"] == int(DEG.max())
        assert st["oriented_items"] > 0 and st["wedge_items"] > 0


# ---- the core side

class CoreRun(Case):
    def setup(self, a):
        load(a)
        a.onion_run()

    def earlier(self, a):
        a.core_run()
        core_exact(a)

    def call(self, a, out):
        return a._lib.komb_core_run(a._ctx)

    def after(self, a, warm):                                # a failed run drops the previous k-core result
        dropped(a.core_fetch)
        OnionRun.exact(a)

    def verify(self, a, out):
        core_exact(a)
        assert a.stats()["max_coreness"] == int(CORE.max())


class OnionRun(Case):
    @staticmethod
    def exact(a):
        layer, core, n_layers = ref("onion", lambda: ON.onion_layers(ROWPTR, COL))
        got_layer, got_core = a.onion_fetch()
        assert same(got_layer, layer) and same(got_core, core) and same(core, CORE)
        info = a.onion_info()
        assert (info["n_layers"], info["max_coreness"]) == (n_layers, int(CORE.max()))

    def earlier(self, a):
        a.onion_run()
        self.exact(a)

    def call(self, a, out):
        return a._lib.komb_onion_run(a._ctx)

    def after(self, a, warm):                                # a failed run drops the previous onion result
        dropped(a.onion_fetch)
        dropped(a.onion_info)
        core_exact(a)

    def verify(self, a, out):
        self.exact(a)


class Components(Case):
    def __init__(self, kind, k, k_earlier):
        self.kind, self.k, self.k_earlier = kind, k, k_earlier

    def may_keep(self, warm):
        return ENDPOINTS if self.kind == "truss" and not warm else 0

    def setup(self, a):
        load_truss(a) if self.kind == "truss" else load_core(a)

    def exact(self, a, k):
        if self.kind == "core":
            want = ref(("comp", "core", k), lambda: C.core_components(ROWPTR, COL, CORE, k))
        else:
            want = ref(("comp", "truss", k), lambda: C.truss_components(NV, F.eu, F.ev, RP.trussness(F), k))
        label, size = a.components_fetch()
        assert same(label, want) and same(size, C.sizes(want))
        info = a.components_info()
        assert (info["k_used"], info["n_members"], info["n_components"], info["largest"]) == (k,) + C.summary(want)

    def earlier(self, a):
        a.components_run(self.kind, self.k_earlier)
        self.exact(a, self.k_earlier)

    def call(self, a, out):
        return a._lib.komb_components_run(a._ctx, a.COMP_KINDS[self.kind], self.k)

    def after(self, a, warm):                                # a failed run drops the previous snapshot
        dropped(a.components_fetch)
        dropped(a.components_info)
        core_exact(a)
        if self.kind == "truss":
            truss_exact(a)

    def verify(self, a, out):
        self.exact(a, self.k)


class Hierarchy(Case):
    """Warm: the hierarchy of the OTHER kind is held; a run that fails for memory leaves it readable."""

    def __init__(self, kind):
        self.kind, self.other = kind, "truss" if kind == "core" else "core"

    def may_keep(self, warm):
        return ENDPOINTS if self.kind == "truss" else 0

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a, kind):
        if kind == "core":
            want = ref("hier core", lambda: H.core_hierarchy(ROWPTR, COL, CORE))
        else:
            want = ref("hier truss", lambda: RP.truss_hierarchy(F))
        nodes, node = a.hierarchy_fetch_nodes(), a.hierarchy_fetch_vertices()
        info = a.hierarchy_info()
        assert info["kind"] == a.COMP_KINDS[kind]
        forest_exact(nodes, node, want, (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]), H.info(want, kind))

    def earlier(self, a):
        a.hierarchy_run(self.other)
        self.exact(a, self.other)

    def call(self, a, out):
        return a._lib.komb_hierarchy_run(a._ctx, a.COMP_KINDS[self.kind])

    def after(self, a, warm):
        if warm:
            self.exact(a, self.other)
        else:
            dropped(a.hierarchy_info)
            dropped(a.hierarchy_fetch_vertices)
        core_exact(a)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a, self.kind)


class Densest(Case):
    def may_keep(self, warm):                                # (member[] and load[]: pool blocks made by the first run, kept with the graph)
        return 0 if warm else 2

    @staticmethod
    def exact(a, iters):
        want = ref(("densest", iters), lambda: D.densest(ROWPTR, COL, CORE, iters))
        member, load_ = a.densest_subgraph_fetch()
        n_k, m_k = a.densest_subgraph_profile()
        info = a.densest_subgraph_info()
        assert same(member, want["member"]) and same(load_, want["load"]) and same(n_k, want["n_k"]) and same(m_k, want["m_k"])
        for x in D.INFO_FIELDS:
            assert info[x] == want[x], (x, iters)

    def earlier(self, a):
        a.densest_subgraph_run(2)
        self.exact(a, 2)

    def call(self, a, out):
        return a._lib.komb_densest_subgraph_run(a._ctx, 7)

    def after(self, a, warm):
        if warm:
            self.exact(a, 2)
        else:
            dropped(a.densest_subgraph_info)
        core_exact(a)

    def verify(self, a, out):
        self.exact(a, 7)


# ---- k-truss

class TrussPrepare(Case):
    states = (False,)                                        # (with a preparation it is a no-op: no request)

    def call(self, a, out):
        return a._lib.komb_truss_prepare(a._ctx)

    def after(self, a, warm):
        core_exact(a)
        assert a.stats()["truss_prepared"] == 0 and a.alloc_info()["pool_blocks_in_use"] == 0

    def verify(self, a, out):
        a.truss_run()
        assert a.stats()["truss_prepared"] == 0              # (the run found the preparation)
        truss_full(a)


class TrussRun(Case):
    """which: None (whole graph) | a coreness (the subgraph induced by the vertices of that coreness or more).  Warm: a run with
    OTHER vertices and the communities of its result are held.  A failed run leaves no k-truss result and none of the analyses
    that index one."""

    def __init__(self, which, finish="local"):
        self.which, self.finish = which, finish

    def may_keep(self, warm):                                # (the graph's preparation, made by its first whole-graph run)
        return 0 if self.which is not None else PREP + (SOURCES if self.finish == "lds" else 0)

    def exact(self, a, which):
        if which is None:
            truss_full(a)
            return
        eu, ev, tr, sup = induced(which)
        got = a.truss_fetch(with_support=True)
        assert same(got[0], eu) and same(got[1], ev) and same(got[2], tr) and same(got[3], sup)

    def earlier(self, a):
        other = 3 if self.which != 3 else 5
        a.truss_run(MASKS[other])
        self.exact(a, other)
        a.truss_communities_run(3)

    def call(self, a, out):
        mask = None if self.which is None else MASKS[self.which]
        return a._lib.komb_truss_run(a._ctx, p(mask))

    def after(self, a, warm):
        n = ctypes.c_int64(-7)
        assert a._lib.komb_truss_count(a._ctx, ctypes.byref(n)) == STATE and n.value == -7
        assert a._lib.komb_truss_fetch(a._ctx, None, None, None) == STATE
        assert a._lib.komb_truss_communities_info(a._ctx, None, None, None, None, None, None) == STATE
        core_exact(a)

    def verify(self, a, out):
        self.exact(a, self.which)
        assert a.stats()["max_trussness"] == int((RP.trussness(F) if self.which is None else induced(self.which)[2]).max())


class TrussRunEdgeless(Case):
    states = (False,)

    def setup(self, a):
        a.from_edges(5, np.zeros((0, 2), np.int64))
        a.core_run()

    def call(self, a, out):
        return a._lib.komb_truss_run(a._ctx, None)

    def after(self, a, warm):
        assert a._lib.komb_truss_count(a._ctx, None) == STATE
        assert a.alloc_info()["pool_blocks_in_use"] == 0     # (nothing of the four blocks stays handed out)
        deg, core = a.core_fetch()
        assert not deg.any() and not core.any()

    def verify(self, a, out):
        eu, ev, tr, sup = a.truss_fetch(with_support=True)
        assert len(eu) == len(ev) == len(tr) == len(sup) == 0


class TrussFetchEndpoints(Case):
    states = (False,)                                        # (the first fetch that asks for endpoints makes them: later ones ask nothing)

    def setup(self, a):
        load_truss(a)

    def outputs(self):
        return {"eu": i32(len(E)), "ev": i32(len(E)), "truss": i32(len(E))}

    def call(self, a, out):
        return a._lib.komb_truss_fetch(a._ctx, p(out["eu"]), p(out["ev"]), p(out["truss"]))

    def after(self, a, warm):                                # the result itself is untouched
        tr = i32(len(E))
        a.truss_fetch_into(tr=tr)
        assert same(tr, RP.trussness(F))
        core_exact(a)

    def verify(self, a, out):
        assert same(out["eu"], F.eu) and same(out["ev"], F.ev) and same(out["truss"], RP.trussness(F))


class TrussFetchSupport(TrussFetchEndpoints):
    def outputs(self):
        return {"support": i32(len(E))}

    def call(self, a, out):
        return a._lib.komb_truss_fetch_support(a._ctx, p(out["support"]))

    def verify(self, a, out):
        assert same(out["support"], RP.supports(F))


# ---- the analyses of a k-truss result

class Communities(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a, k):
        want = ref(("comm", k), lambda: TC.communities(NV, F.eu, F.ev, RP.trussness(F), k))
        label, size = a.truss_communities_fetch()
        assert same(label, want) and same(size, TC.sizes(want))
        assert same(a.truss_communities_fetch_vertices(), TC.vertex_multiplicity(NV, F.eu, F.ev, want))
        info = a.truss_communities_info()
        assert (info["k_used"], info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"]) == \
            (k,) + TC.summary(NV, F.eu, F.ev, want)

    def earlier(self, a):
        a.truss_communities_run(3)
        self.exact(a, 3)

    def call(self, a, out):
        return a._lib.komb_truss_communities_run(a._ctx, 4)

    def after(self, a, warm):                                # a failed run drops the previous communities
        dropped(a.truss_communities_fetch)
        dropped(a.truss_communities_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a, 4)


class CommunitiesVertices(Case):
    states = (False,)                                        # (the first fetch_vertices / info after a run makes n_comm[])
    pool_requests_only = False

    def setup(self, a):
        load_truss(a)
        a.truss_communities_run(4)

    def may_keep(self, warm):
        return 1                                             # (n_comm[], kept for the fetch that succeeds)

    def outputs(self):
        return {"n_comm": i32(NV)}

    def call(self, a, out):
        return a._lib.komb_truss_communities_fetch_vertices(a._ctx, p(out["n_comm"]))

    def after(self, a, warm):
        want = ref(("comm", 4), lambda: TC.communities(NV, F.eu, F.ev, RP.trussness(F), 4))
        label, size = a.truss_communities_fetch()
        assert same(label, want) and same(size, TC.sizes(want))
        truss_exact(a)

    def verify(self, a, out):
        want = ref(("comm", 4), lambda: TC.communities(NV, F.eu, F.ev, RP.trussness(F), 4))
        assert same(out["n_comm"], TC.vertex_multiplicity(NV, F.eu, F.ev, want))
        Communities.exact(a, 4)


BC_INFO = ("k_used", "n_member_edges", "n_member_vertices", "n_blocks", "n_bridges", "n_articulation", "largest_block", "n_ecc",
           "largest_ecc", "depth")


class Biconnected(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a, k):
        want = ref(("bc", k), lambda: RP.biconnected(F, k))
        block, size = a.biconnected_fetch_edges()
        n_blocks, ecc_label, ecc_size = a.biconnected_fetch_vertices()
        got = {"block": block, "size": size, "n_blocks": n_blocks, "ecc_label": ecc_label, "ecc_size": ecc_size}
        for name in got:
            assert same(got[name], want[name]), (name, k)
        blocks = a.biconnected_fetch_blocks()
        for name in ("rep", "n_edges", "n_verts"):
            assert same(blocks[name], want["blocks"][name]), (name, k)
        info = a.biconnected_info()
        assert tuple(info[x] for x in BC_INFO) == (k,) + tuple(want["info"][x] for x in BC_INFO[1:])

    def earlier(self, a):
        a.biconnected_run(4)
        self.exact(a, 4)

    def call(self, a, out):
        return a._lib.komb_biconnected_run(a._ctx, 2)

    def after(self, a, warm):                                # a failed run drops the previous blocks
        dropped(a.biconnected_count)
        dropped(a.biconnected_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a, 2)


class CommunityHierarchy(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a):
        want = ref("ch", lambda: RP.community_hierarchy(F))
        nodes, node = a.community_hierarchy_fetch_nodes(), a.community_hierarchy_fetch_edges()
        info = a.community_hierarchy_info()
        forest_exact(nodes, node, want, tuple(info[x] for x in ("n_nodes", "n_roots", "k_max", "depth", "n_member_edges")), CH.info(want))

    def earlier(self, a):
        a.community_hierarchy_run()
        self.exact(a)

    def call(self, a, out):
        return a._lib.komb_community_hierarchy_run(a._ctx)

    def after(self, a, warm):
        if warm:
            self.exact(a)
        else:
            dropped(a.community_hierarchy_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a)


class CommunityHierarchyLabels(Case):
    def setup(self, a):
        load_truss(a)
        a.community_hierarchy_run()

    @staticmethod
    def want(k):
        h = ref("ch", lambda: RP.community_hierarchy(F))
        return ref(("ch labels", k), lambda: CH.walk_up(h, RP.trussness(F), k))

    def earlier(self, a):
        label, size = a.community_hierarchy_labels(3)
        assert same(label, self.want(3)[0]) and same(size, self.want(3)[1])

    def outputs(self):
        return {"label": i32(len(E)), "size": i32(len(E))}

    def call(self, a, out):
        return a._lib.komb_community_hierarchy_labels(a._ctx, 4, p(out["label"]), p(out["size"]))

    def after(self, a, warm):
        CommunityHierarchy.exact(a)
        truss_exact(a)

    def verify(self, a, out):
        assert same(out["label"], self.want(4)[0]) and same(out["size"], self.want(4)[1])


ST_COUNTS = ("eps_num", "eps_den", "mu", "n_similar_edges", "n_cores", "n_borders", "n_hubs", "n_outliers", "n_clusters", "largest")


class Structural(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS + SUPPORT

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a, params):
        want = ref(("structural", params), lambda: RP.structural(F, *params))
        label, size, role, sim_deg = a.structural_clusters_fetch()
        got = {"label": label, "size": size, "role": role, "sim_deg": sim_deg, "similar": a.structural_clusters_fetch_edges()}
        for name in got:
            assert same(got[name], want[name]), (name, params)
        info = a.structural_clusters_info()
        assert tuple(info[x] for x in ST_COUNTS) == tuple(want["info"][x] for x in ST_COUNTS)

    def earlier(self, a):
        a.structural_clusters_run(*SOME[4])
        self.exact(a, SOME[4])

    def call(self, a, out):
        return a._lib.komb_structural_clusters_run(a._ctx, *SOME[1])

    def after(self, a, warm):
        if warm:
            self.exact(a, SOME[4])
        else:
            dropped(a.structural_clusters_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a, SOME[1])


NUC_COUNTS = ("n_triangles", "n_cliques4", "theta_max", "n_levels")


class Nucleus(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a):
        want = ref("nucleus", lambda: RP.nucleus(F, tri()))
        tris, edge_theta, vertex_theta = a.nucleus_fetch(), a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()
        for name in ("a", "b", "c", "key0", "theta"):
            assert same(tris[name], want[name]), name
        assert same(edge_theta, want["edge_theta"]) and same(vertex_theta, want["vertex_theta"])
        info = a.nucleus_info()
        assert {x: info[x] for x in NUC_COUNTS} == want["info"]

    def earlier(self, a):
        a.nucleus_run()
        self.exact(a)

    def call(self, a, out):
        return a._lib.komb_nucleus_run(a._ctx)

    def after(self, a, warm):
        if warm:
            self.exact(a)
        else:
            dropped(a.nucleus_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a)


def nh_want():
    return ref("nh", lambda: RP.nucleus_hierarchy(F, tri()))


def theta():
    return ref("nucleus", lambda: RP.nucleus(F, tri()))["theta"]


class NucleusHierarchy(Case):
    def setup(self, a):
        load_nucleus(a)

    @staticmethod
    def exact(a):
        nodes, node = a.nucleus_hierarchy_fetch_nodes(), a.nucleus_hierarchy_fetch_triangles()
        info = a.nucleus_hierarchy_info()
        forest_exact(nodes, node, nh_want(), tuple(info[x] for x in ("n_nodes", "n_roots", "theta_max", "depth", "n_member_triangles")),
                     NH.info(nh_want(), theta()))

    def earlier(self, a):
        a.nucleus_hierarchy_run()
        self.exact(a)

    def call(self, a, out):
        return a._lib.komb_nucleus_hierarchy_run(a._ctx)

    def after(self, a, warm):
        if warm:
            self.exact(a)
        else:
            dropped(a.nucleus_hierarchy_info)
        Nucleus.exact(a)

    def verify(self, a, out):
        self.exact(a)


class NucleusHierarchyLabels(Case):
    def setup(self, a):
        load_nucleus(a)
        a.nucleus_hierarchy_run()

    @staticmethod
    def want(k):
        return ref(("nh labels", k), lambda: NH.walk_up(nh_want(), theta(), k))

    def earlier(self, a):
        label, size = a.nucleus_hierarchy_labels(1)
        assert same(label, self.want(1)[0]) and same(size, self.want(1)[1])

    def outputs(self):
        return {"label": i32(tri().n), "size": i32(tri().n)}

    def call(self, a, out):
        return a._lib.komb_nucleus_hierarchy_labels(a._ctx, 2, p(out["label"]), p(out["size"]))

    def after(self, a, warm):
        NucleusHierarchy.exact(a)

    def verify(self, a, out):
        assert same(out["label"], self.want(2)[0]) and same(out["size"], self.want(2)[1])


class NucleusHierarchyNuclei(Case):
    FIELDS = ("rep", "n_triangles", "n_edges", "n_vertices")
    pool_requests_only = False

    def setup(self, a):
        load_nucleus(a)
        a.nucleus_hierarchy_run()

    @staticmethod
    def want(k):
        return ref(("nh nuclei", k), lambda: NH.nuclei(nh_want(), tri().dec[0], k))

    def earlier(self, a):
        got = a.nucleus_hierarchy_nuclei(1)
        for x in self.FIELDS:
            assert same(got[x], self.want(1)[x]), x

    def outputs(self):
        n = len(self.want(2)["rep"])
        return dict({x: i32(n) for x in self.FIELDS}, n_nuclei=ctypes.c_int64(-7))

    def call(self, a, out):
        return a._lib.komb_nucleus_hierarchy_nuclei(a._ctx, 2, len(out["rep"]), ctypes.byref(out["n_nuclei"]), *(p(out[x]) for x in self.FIELDS))

    def after(self, a, warm):
        NucleusHierarchy.exact(a)

    def verify(self, a, out):
        assert out["n_nuclei"].value == len(self.want(2)["rep"]) >= 1
        for x in self.FIELDS:
            assert same(out[x], self.want(2)[x]), x


# ---- the clique searches

class MaxClique(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a):
        want = ref("max clique", lambda: RP.max_clique(F))
        info = a.max_clique_info()
        count, witness = a.max_clique_fetch()
        assert info["flags"] == 7 == want["flags"]
        assert tuple(info[x] for x in ("omega", "upper", "t_max", "n_max_cliques")) == tuple(want[x] for x in ("omega", "upper", "t_max", "n_max_cliques"))
        assert same(count, want["count"])
        cliques = a.max_clique_list()                        # (komb_max_clique_list: host memory only)
        assert same(cliques, want["list"].rows) and same(witness, cliques[0])

    def earlier(self, a):
        a.max_clique_run(1 << 20)
        self.exact(a)

    def call(self, a, out):
        return a._lib.komb_max_clique_run(a._ctx, 0)

    def after(self, a, warm):
        if warm:
            self.exact(a)
        else:
            dropped(a.max_clique_info)
            n = ctypes.c_int64(-7)
            assert a._lib.komb_max_clique_list(a._ctx, 0, ctypes.byref(n), None) == STATE and n.value == -7
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a)


class CliqueCensus(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a, k_local):
        want = ref(("census", k_local), lambda: RP.clique_census(F, k_local))
        total, local = a.clique_census_fetch()
        info = a.clique_census_info()
        assert info["flags"] == 1 and (info["k_lo"], info["k_hi"], info["k_local"], info["t_max"], info["omega"]) == \
            (2, want["k_hi"], k_local, want["t_max"], want["omega"])
        assert [int(x) for x in total] == want["total"]
        if k_local:
            assert same(local.astype(np.int64), want["local"])

    def earlier(self, a):
        a.clique_census_run(2, -1, 0)
        self.exact(a, 0)

    def call(self, a, out):
        return a._lib.komb_clique_census_run(a._ctx, 2, -1, 4, 0)

    def after(self, a, warm):
        if warm:
            self.exact(a, 0)
        else:
            dropped(a.clique_census_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a, 4)


def mq_want():
    return ref("maximal", lambda: RP.maximal_cliques(F))


class MaximalCliques(Case):
    def may_keep(self, warm):
        return 0 if warm else ENDPOINTS

    def setup(self, a):
        load_truss(a)

    @staticmethod
    def exact(a, k_min):
        want = ref(("maximal", k_min), lambda: MQ.solve(NV, F.eu, F.ev, k_min))
        hist, count, largest = a.maximal_cliques_fetch()
        info = a.maximal_cliques_info()
        assert info["flags"] == 3
        assert tuple(info[x] for x in ("k_min", "k_hi", "t_max", "omega", "n_cliques")) == \
            (k_min,) + tuple(want[x] for x in ("k_hi", "t_max", "omega", "n_cliques"))
        assert same(hist, want["hist"]) and same(count, want["count"]) and same(largest, want["largest"])
        offset, verts = a.maximal_cliques_list()
        assert same(offset, np.concatenate([[0], np.cumsum([len(c) for c in want["cliques"]])]))
        assert same(verts, [v for c in want["cliques"] for v in c])

    def earlier(self, a):
        a.maximal_cliques_run(3)
        self.exact(a, 3)

    def call(self, a, out):
        return a._lib.komb_maximal_cliques_run(a._ctx, 2, 0)

    def after(self, a, warm):
        if warm:
            self.exact(a, 3)
        else:
            dropped(a.maximal_cliques_info)
        truss_exact(a)

    def verify(self, a, out):
        self.exact(a, 2)


class CliqueCommunities(Case):
    pool_requests_only = False                               # (prim_unique_u64's counter is a dev_malloc)

    def setup(self, a):
        load_truss(a)
        a.maximal_cliques_run(2)

    @staticmethod
    def exact(a, k):
        want = ref(("percolation", k), lambda: RP.clique_communities(F, mq_want(), k))
        label, size = a.clique_communities_fetch()
        rep, n_cliques = a.clique_communities_fetch_communities()[:2]
        n_comm, first = a.clique_communities_fetch_vertices()
        for got, name in ((label, "label"), (size, "size"), (rep, "rep"), (n_cliques, "n_cliques"), (n_comm, "n_comm"), (first, "first")):
            assert same(got, want[name]), (k, name)
        info = a.clique_communities_info()
        for x in ("n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap", "pair_tests"):
            assert info[x] == want[x], (k, x)

    def earlier(self, a):
        a.clique_communities_run(4)
        self.exact(a, 4)

    def call(self, a, out):
        return a._lib.komb_clique_communities_run(a._ctx, 3, 0)

    def after(self, a, warm):
        if warm:
            self.exact(a, 4)
        else:
            dropped(a.clique_communities_info)
        MaximalCliques.exact(a, 2)

    def verify(self, a, out):
        self.exact(a, 3)


# ---- CoreA and the densest block

class CoreaRanks(Case):
    states = (False,)                                        # (it keeps nothing: one state)

    def outputs(self):
        return {"rank_degree": f64(NV), "rank_key": f64(NV)}

    def call(self, a, out):
        return a._lib.komb_corea_ranks(a._ctx, p(DEG), p(CORE), NV, p(out["rank_degree"]), p(out["rank_key"]))

    def after(self, a, warm):
        core_exact(a)

    def verify(self, a, out):
        assert np.array_equal(out["rank_degree"], CI.np_fractional_rank(DEG.astype(np.int64)))
        assert np.array_equal(out["rank_key"], CI.np_fractional_rank(CI.keys_of(DEG, CORE)))


class DensestBlock(Case):
    states = (False,)
    oracle = None

    def outputs(self):
        return {"order": i32(2 * NV), "side": i32(2 * NV), "n_block": ctypes.c_int64(-7), "max_density": ctypes.c_double(-7.0)}

    def call(self, a, out):
        return a._lib.komb_densest_block(a._ctx, None, p(out["order"]), p(out["side"]), ctypes.byref(out["n_block"]), ctypes.byref(out["max_density"]))

    def after(self, a, warm):
        core_exact(a)

    def verify(self, a, out):
        want = ref("merge", lambda: self.oracle.run_merge(ROWPTR, COL, None))
        assert same(out["order"], want[0]) and same(out["side"], want[1])
        assert (out["n_block"].value, out["max_density"].value) == want[2:]


CASES = {
    "graph_from_edges": FromEdges(), "graph_from_csr": FromCsr(), "graph_moments": Moments(),
    "core_run": CoreRun(), "onion_run": OnionRun(),
    "components_run core": Components("core", 2, 1), "components_run truss": Components("truss", 4, 3),
    "hierarchy_run core": Hierarchy("core"), "hierarchy_run truss": Hierarchy("truss"),
    "truss_prepare": TrussPrepare(), "truss_run edgeless": TrussRunEdgeless(),
    "truss_fetch endpoints": TrussFetchEndpoints(), "truss_fetch_support": TrussFetchSupport(),
    "truss_communities_run": Communities(), "truss_communities_fetch_vertices": CommunitiesVertices(),
    "biconnected_run": Biconnected(), "community_hierarchy_run": CommunityHierarchy(),
    "community_hierarchy_labels": CommunityHierarchyLabels(), "structural_clusters_run": Structural(),
    "nucleus_run": Nucleus(), "nucleus_hierarchy_run": NucleusHierarchy(), "nucleus_hierarchy_labels": NucleusHierarchyLabels(),
    "nucleus_hierarchy_nuclei": NucleusHierarchyNuclei(),
    "max_clique_run": MaxClique(), "clique_census_run": CliqueCensus(), "maximal_cliques_run": MaximalCliques(),
    "clique_communities_run": CliqueCommunities(),
    "densest_subgraph_run": Densest(), "corea_ranks": CoreaRanks(), "densest_block": DensestBlock(),
}
TWO_PASS = {"INDEX": "two_pass"}


def _set(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)


def _sweep(K, case, label):
    with K.KombAccel() as a:
        for warm in case.states:
            n = run_state(a, case, warm)
            print("alloc failure sweep: %s, %s: N = %d" % (label, "warm" if warm else "cold", n))


@pytest.mark.parametrize("name", list(CASES))
def test_every_request_fails_once(K, O, name):
    DensestBlock.oracle = O
    _sweep(K, CASES[name], name)


@pytest.mark.parametrize("finish", ["lds", "none"])
@pytest.mark.parametrize("name", ["core_run", "onion_run"])
def test_peel_finishes(K, monkeypatch, name, finish):
    _set(monkeypatch, {"FINISH": finish})
    _sweep(K, CASES[name], "%s FINISH=%s" % (name, finish))


@pytest.mark.parametrize("finish", ["local", "lds", "none"])
@pytest.mark.parametrize("which", [None, 3], ids=["whole", "induced"])
def test_truss_run_two_pass(K, monkeypatch, which, finish):
    """komb_truss_run with the exact two-pass index build (option INDEX=two_pass), whole graph and induced by a vertex mask,
    under every finish of the peel."""
    _set(monkeypatch, dict(TWO_PASS, FINISH=finish))
    _sweep(K, TrussRun(which, finish), "truss_run %s INDEX=two_pass FINISH=%s" % ("whole" if which is None else "induced", finish))


def optional_requests(retries):
    """The requests of a stream-layout run it may do without (ktruss.hip, "no memory for the stream, or it ran out: exact
    two-pass build"): the record keys and values, the dense own-role region, its offsets and its cursors, and the wave-private
    record scratch of the first attempt; keys, values, region and scratch again for every attempt that follows one whose
    stream ran out (komb_stats.stream_retries); the two second buffers of the record sort."""
    return 6 + 4 * retries + 2


@pytest.mark.parametrize("finish", ["local", "lds", "none"])
@pytest.mark.parametrize("which", [None, 3], ids=["whole", "induced"])
def test_truss_run_stream_layout(K, monkeypatch, which, finish):
    """The default index layout.  As the sweep above, but a request the run may do without answers differently: the run
    succeeds, is exact, and komb_stats says which layout built the index.  Exactly optional_requests() requests are absorbed;
    every other one fails the run."""
    _set(monkeypatch, {"FINISH": finish})
    case = TrussRun(which, finish)
    with K.KombAccel() as a:
        for warm in case.states:
            def start():
                case.setup(a)
                if warm:
                    case.earlier(a)
            start()
            a.set_option("ALLOC_FAIL_AT", "0")
            assert case.call(a, {}) == OK
            n_req = a.alloc_info()["requests"]
            a.set_option("ALLOC_FAIL_AT", None)
            assert a.stats()["index_layout"] == 0
            retries = a.stats()["stream_retries"]
            case.verify(a, {})
            steady = a.alloc_info()["pool_blocks_in_use"]
            absorbed = 0
            for n in range(1, n_req + 1):
                start()
                held = a.alloc_info()["pool_blocks_in_use"]
                a.set_option("ALLOC_FAIL_AT", str(n))
                rc = case.call(a, {})
                err = a._lib.komb_last_error(a._ctx)
                info = a.alloc_info()
                a.set_option("ALLOC_FAIL_AT", None)
                assert info["fired"] == 1, n
                if rc == OK:
                    assert a.stats()["index_layout"] in (0, 2), n       # (0: only the scratch was missing)
                    absorbed += 1
                else:
                    assert rc == NOMEM and err, (n, rc)
                    assert info["pool_blocks_in_use"] <= held + case.may_keep(warm), n
                    case.after(a, warm)
                    assert case.call(a, {}) == OK
                    assert a.stats()["index_layout"] == 0
                case.verify(a, {})
                assert a.alloc_info()["pool_blocks_in_use"] == steady, n
            assert absorbed == optional_requests(retries), (absorbed, retries, n_req)
            print("alloc failure sweep: truss_run %s stream FINISH=%s, %s: N = %d" % ("whole" if which is None else "induced", finish,
                                                                                       "warm" if warm else "cold", n_req))


def test_entries_without_a_device_request(K):
    """komb_max_clique_list copies a list the run left on the host, and a second endpoint fetch finds the list the first one
    made: neither has a request to inject into."""
    with K.KombAccel() as a:
        load_truss(a)
        a.max_clique_run()
        truss_full(a)
        a.set_option("ALLOC_FAIL_AT", "1")
        MaxClique.exact(a)
        truss_full(a)
        info = a.alloc_info()
        assert info["requests"] == 0 and info["fired"] == 0
        a.set_option("ALLOC_FAIL_AT", None)


TRIM = ["core_run", "onion_run", "components_run core", "components_run truss", "hierarchy_run core", "hierarchy_run truss",
        "graph_moments", "truss_fetch endpoints", "truss_fetch_support", "truss_communities_run", "truss_communities_fetch_vertices",
        "biconnected_run", "community_hierarchy_run", "community_hierarchy_labels", "structural_clusters_run", "nucleus_run",
        "nucleus_hierarchy_run", "nucleus_hierarchy_labels", "nucleus_hierarchy_nuclei", "max_clique_run", "clique_census_run",
        "maximal_cliques_run", "clique_communities_run", "densest_subgraph_run", "corea_ranks", "densest_block"]


@pytest.mark.parametrize("name", TRIM)
def test_trim_before_every_request(K, O, name):
    """What a request the driver refuses does before it tries again -- every cached block goes back to the driver -- in front of
    every request of a warm call: blocks that were put back too early would be gone."""
    DensestBlock.oracle = O
    with K.KombAccel() as a:
        n = run_trim(a, CASES[name])
        print("trim sweep: %s: N = %d" % (name, n))


@pytest.mark.parametrize("which", [None, 3], ids=["whole", "induced"])
@pytest.mark.parametrize("index", ["stream", "two_pass"])
def test_trim_truss_run(K, monkeypatch, which, index):
    _set(monkeypatch, {"INDEX": index})
    with K.KombAccel() as a:
        n = run_trim(a, TrussRun(which))
        print("trim sweep: truss_run %s INDEX=%s: N = %d" % ("whole" if which is None else "induced", index, n))


def test_trim_and_failure_on_poisoned_memory(K, monkeypatch):
    """One combined case: every allocation filled with 0xFFFFFFFF first, the trim sweep and the failure sweep of the analyses
    that read the most scratch."""
    _set(monkeypatch, {"POISON": "0xFFFFFFFF"})
    with K.KombAccel() as a:
        run_trim(a, CASES["nucleus_hierarchy_run"])
        run_state(a, CASES["biconnected_run"], True)
