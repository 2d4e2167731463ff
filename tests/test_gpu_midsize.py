"""Mid-size GPU tests of the clique census, the maximal cliques, the maximum-clique search, the (3,4)-nucleus decomposition and
the nucleus hierarchy against the native references of oracle/komb_oracle.c (orc_clique_census, orc_maximal_cliques -- the
PIVOT-FREE form --, orc_nucleus, with the numpy / scipy helpers of oracle/oracle.py; tests/test_oracle_cliques.py ties those to
the Python restatements, networkx and one recorded run).  The references start at a vertex and intersect sorted CSR rows: they
share nothing with the library's edge roots, bit matrices, pivots and trussness cuts, nor with the one driver the three clique
analyses share (clique_root_dev.h), which the identities between those analyses cannot check.  Every comparison is exact
equality of whole integer arrays.

One context, one k-truss run and one set of reference results per graph, shared by its tests and never changed (a test runs
its own analysis on the context; none touches the graph or the k-truss result).

The graphs (m edges, T triangles, Q 4-cliques; the oracle's seconds are CPU time on one thread of the machine this was written
on, measured once per graph):
  G50   gen_hug_edges(50000, 122500, 2.6, 42): m 502 700, T 601 248 (just past 2048 x 256: nucleus.hip's sweep workgroups walk a
        second tile), Q 447 974, omega 16, t_max 17, 204 551 maximal cliques; 7 855 root chunks against 1 024 waves.
        Oracle: census 0.22 s per k_local (3.39 M cliques), maximal cliques 1.3 s, nucleus 0.6 s, the k-nuclei of every k
        1.2 s, trussness 1.4 s.
  G100  gen_hug_edges(100000, 245000, 2.6, 42): m 1 007 422, T 1 132 326, Q 835 985, omega 15, t_max 19, 384 369 maximal
        cliques.  Oracle: census 0.55 s per k_local (7.81 M cliques), maximal cliques 3.4 s, nucleus 1.4 s, the k-nuclei of
        every k 2.2 s, trussness 3.3 s.
        The 200 000-vertex graph of the same family (m 2 014 988, T 2 141 968, Q 1 562 626, omega 18) was measured and NOT kept:
        its census takes 1.5 s and its nucleus 2.9 s, but the pivot-free maximal cliques take 11.6 s (24.6 M cliques, each
        intersected with a full row) and the trussness 6.9 s.
  G50 under a vmask (coreness >= half the largest): 245 023 edges, T 332 049, Q 286 990, omega 16; the references run on the
        induced subgraph (under 1 s together).
  CAPPED (test_scratch_capped_grid has the construction): m 204 890, T 261 896, Q 192 853, omega 12, t_max 13; the one graph
        whose roots' scratch slots cut the launch grid.  Oracle: under 0.5 s each.

RECORDED holds what the library reported on an MI355X for every graph -- max_candidates, nodes, n_levels, n_subrounds; of
these the tests assert only what the contract fixes (nodes depend on pivot ties and on the option, n_subrounds on the
frontiers of the level-synchronous peel)."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

HUG = {"G50": (50000, 122500, 2.6, 42), "G100": (100000, 245000, 2.6, 42)}
MAXIMAL_LIST = 65536                                      # the default of option MAXIMAL_LIST

# as printed by a run of this file with -s on an MI355X, default options: census at (2, -1, 0), maximal cliques at k_min 2
RECORDED = {
    "G50": {"census": {"max_candidates": 159, "nodes": 1192939}, "maximal": {"max_candidates": 662, "nodes": 826108},
            "max_clique": {"nodes": 1530}, "nucleus": {"n_levels": 14, "n_subrounds": 78}},
    "G100": {"census": {"max_candidates": 159, "nodes": 2292755}, "maximal": {"max_candidates": 850, "nodes": 1600560},
             "max_clique": {"nodes": 7306}, "nucleus": {"n_levels": 15, "n_subrounds": 103}},
    "G50 vmask": {"census": {"max_candidates": 146, "nodes": 660113}, "maximal": {"max_candidates": 618, "nodes": 472095},
                  "max_clique": {"nodes": 1499}, "nucleus": {"n_levels": 14, "n_subrounds": 77}},
    "CAPPED": {"census": {"max_candidates": 3000, "nodes": 520327}, "maximal": {"max_candidates": 3000, "nodes": 358208},
               "max_clique": {"nodes": 2087}},
}

N_PAGES = 3000
CAPPED_HUG = (20000, 49000, 2.6, 5)


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


class Graph:
    """One graph on one context with its k-truss result (whole or under a vmask), and the references of H, the graph of that
    result, computed once on first use.  The references see H with its vertices renumbered 0 .. n_sub - 1 in ascending order
    (inv maps back), which keeps every order the contract defines."""

    def __init__(self, K, name, nv, uv, masked=False):
        self.name, self.nv = name, nv
        self.a = K.KombAccel()
        self.a.from_edges(nv, uv)
        rowptr, col = O.simplify(nv, uv)
        lr, lc = self.a.get_csr()
        assert np.array_equal(lr, rowptr) and np.array_equal(lc, col)
        self.lib_rowptr, self.lib_col = lr, lc
        vmask = None
        self.inv = np.arange(nv, dtype=np.int32)
        if masked:
            core = self.a.run_core()[1]
            assert np.array_equal(core, O.coreness(rowptr, col))
            vmask = (core >= max(int(core.max()) // 2, 1)).astype(np.uint8)
            rowptr, col, self.inv = O.induced_subgraph(rowptr, col, vmask)
        self.vmask, self.rowptr, self.col = vmask, rowptr, col
        self.eu, self.ev, self.tr = self.a.run_truss(vmask)
        su, sv = O.edge_list(rowptr, col)
        assert np.array_equal(self.eu, self.inv[su]) and np.array_equal(self.ev, self.inv[sv])
        assert np.array_equal(self.tr, O.trussness(rowptr, col))
        self.tmax = int(self.tr.max()) if len(self.tr) else 0
        self._cache = {}
        self.did = set()

    def close(self):
        self.a.close()

    def _once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def per_vertex(self, x, fill=0):
        out = np.full(self.nv, fill, dtype=x.dtype)
        out[self.inv] = x
        return out

    def counts(self, k_local):
        return self._once(("census", k_local), lambda: O.clique_counts(self.rowptr, self.col, k_local))

    def maximal_all(self):
        return self._once("maximal", lambda: O.maximal_cliques_all(self.rowptr, self.col, 2))

    def view(self, k_min):
        return self._once(("view", k_min), lambda: O.maximal_view(self.maximal_all(), self.tmax, k_min))

    def k_list(self):
        """The smallest k_min whose cliques the library holds as a list at the default MAXIMAL_LIST, from the oracle's histogram."""
        above = np.cumsum(self.maximal_all()["hist_all"][::-1])[::-1]         # above[k] = the maximal cliques of >= k vertices
        return max(int(np.flatnonzero(above <= MAXIMAL_LIST)[0]), 2)

    def nucleus(self):
        return self._once("nucleus", lambda: O.nucleus(self.rowptr, self.col))

    def labels(self, k):
        n = self.nucleus()
        return self._once(("labels", k), lambda: O.nuclei_labels(n["theta"], n["quads"], k))

    def run_nucleus(self):
        """The library's decomposition and forest, once per context (both depend on the k-truss result alone)."""
        if "nucleus" not in self.did:
            self.a.nucleus_run()
            self.a.nucleus_hierarchy_run()
            self.did.add("nucleus")


def _set(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)


# ---- the checks, one analysis each

def check_census(g, k_lo, k_hi, k_local):
    want = O.census_window(g.counts(k_local), g.tmax, k_lo, k_hi, k_local)
    assert g.counts(k_local)["nodes"] == int(g.counts(k_local)["total"].sum())      # (the oracle visited every clique: no closed form)
    total, local, info = g.a.run_clique_census(k_lo, k_hi, k_local)
    print("%s census (%d, %d, %d): %s; oracle %.2f s" % (g.name, k_lo, k_hi, k_local, info, g.counts(k_local)["seconds"]))
    for name in ("k_lo", "k_hi", "k_local", "t_max", "omega"):
        assert info[name] == want[name], name
    if (k_lo, k_hi, k_local) == (2, -1, 0):                                         # (the largest candidate set is the graph's, not the run's)
        assert info["max_candidates"] == RECORDED[g.name]["census"]["max_candidates"]
    assert info["flags"] == 1 == want["flags"]                                      # COMPLETE at the default budget, nothing saturated
    assert total.dtype == np.uint64 and np.array_equal(total, want["total"])
    if k_local:
        assert local.dtype == np.uint64 and np.array_equal(local, g.per_vertex(want["local"]))
    else:
        assert local is None
    return info


def check_maximal(g, k_min):
    want = g.view(k_min)
    hist, count, largest, info = g.a.run_maximal_cliques(k_min)
    print("%s maximal cliques k_min %d: %s; oracle %.2f s" % (g.name, k_min, info, g.maximal_all()["seconds"]))
    for name in ("k_min", "k_hi", "t_max", "omega", "n_cliques"):
        assert info[name] == want[name], name
    listed = want["n_cliques"] <= MAXIMAL_LIST
    assert info["flags"] == (3 if listed else 1)
    assert hist.dtype == np.int64 and np.array_equal(hist, want["hist"])
    assert count.dtype == np.int32 and np.array_equal(count, g.per_vertex(want["count"]))
    assert largest.dtype == np.int32 and np.array_equal(largest, g.per_vertex(want["largest"]))
    if listed:
        offset, verts = g.a.maximal_cliques_list()
        assert offset.dtype == np.int64 and np.array_equal(offset, want["offset"])
        assert verts.dtype == np.int32 and np.array_equal(verts, g.inv[want["verts"]])
    return info


def check_max_clique(g):
    want = O.maximum_cliques(g.view(2))
    info, count, witness = g.a.run_max_clique()
    print("%s maximum clique: %s" % (g.name, info))
    assert info["flags"] == 7 and info["omega"] == want["omega"] and info["upper"] >= want["omega"] and info["t_max"] == g.tmax
    assert info["upper"] == info["omega"]                                           # (EXACT)
    assert info["n_max_cliques"] == want["n_max_cliques"]
    assert count.dtype == np.int32 and np.array_equal(count, g.per_vertex(want["count"]))
    cliques = g.a.max_clique_list()
    assert cliques.dtype == np.int32 and np.array_equal(cliques, g.inv[want["list"]].reshape(cliques.shape))
    assert np.array_equal(witness, cliques[0]) and len(witness) == want["omega"] and (np.diff(witness) > 0).all()
    for i, u in enumerate(witness):                                                 # a clique in the library's own CSR
        row = g.lib_col[g.lib_rowptr[u]:g.lib_rowptr[u + 1]]
        assert np.isin(witness[i + 1:], row).all()
        assert g.vmask is None or g.vmask[u]
    return info


def check_nucleus(g):
    want = g.nucleus()
    g.run_nucleus()
    tris, edge_theta, vertex_theta = g.a.nucleus_fetch(), g.a.nucleus_fetch_edges(), g.a.nucleus_fetch_vertices()
    info = g.a.nucleus_info()
    print("%s nucleus: %s; oracle %.2f s" % (g.name, info, want["seconds"]))
    for name in ("a", "b", "c"):
        assert tris[name].dtype == np.int32 and np.array_equal(tris[name], g.inv[want[name]]), name
    for name in ("key0", "theta"):
        assert tris[name].dtype == np.int32 and np.array_equal(tris[name], want[name]), name
    assert np.array_equal(edge_theta, want["edge_theta"]) and np.array_equal(vertex_theta, g.per_vertex(want["vertex_theta"], -1))
    for name in ("n_triangles", "n_cliques4", "theta_max", "n_levels"):
        assert info[name] == want["info"][name], name
    assert info["n_levels"] <= info["n_subrounds"] <= max(info["n_triangles"], 0) and info["ms"] >= 0.0
    return info


def check_nuclei(g):
    """Labels and sizes of the k-nuclei for every k of the result (and the one above: nothing), and the forest's nodes level by
    level: a node is a class of its k that is no class of k + 1."""
    want = g.nucleus()
    g.run_nucleus()
    top = max(want["info"]["theta_max"], 0)
    classes = {}
    for k in range(1, top + 2):
        wl, ws = g.labels(k)
        label, size = g.a.nucleus_hierarchy_labels(k)
        assert label.dtype == np.int32 and np.array_equal(label, wl), k
        assert size.dtype == np.int32 and np.array_equal(size, ws), k
        classes[k] = set(zip(wl[wl >= 0].tolist(), ws[wl >= 0].tolist()))
    assert classes[top + 1] == set()
    nodes = g.a.nucleus_hierarchy_fetch_nodes()
    hinfo = g.a.nucleus_hierarchy_info()
    print("%s nucleus hierarchy: %s; classes per level %s" % (g.name, hinfo, [len(classes[k]) for k in range(1, top + 1)]))
    per_level = np.bincount(nodes["k"], minlength=top + 2)
    for k in range(1, top + 1):
        assert int(per_level[k]) == len(classes[k] - classes[k + 1]), k
    assert int(per_level[0]) == 0 and len(nodes["k"]) == hinfo["n_nodes"] == int(per_level.sum())
    want_nodes = sorted((k, r, s) for k in range(1, top + 1) for r, s in classes[k] - classes[k + 1])
    assert list(zip(nodes["k"].tolist(), nodes["rep"].tolist(), nodes["size"].tolist())) == want_nodes
    assert hinfo["theta_max"] == want["info"]["theta_max"] and hinfo["n_member_triangles"] == int((want["theta"] >= 1).sum())
    assert hinfo["n_roots"] == (len(classes[1]) if top else 0)                      # every 1-nucleus holds exactly one root


# ---- G50 and G100

def _hug(K, name):
    graph = Graph(K, name, HUG[name][0], K.gen_hug_edges(*HUG[name]))
    yield graph
    graph.close()


@pytest.fixture(scope="module")
def g50(K):
    yield from _hug(K, "G50")


@pytest.fixture(scope="module")
def g100(K):
    yield from _hug(K, "G100")


@pytest.fixture(params=["g50", "g100"])
def g(request):
    return request.getfixturevalue(request.param)


def test_shape(g):
    """The figures the module docstring quotes, from the references (so a change of the generator shows here first)."""
    shape = {"G50": (502700, 601248, 447974, 16, 17), "G100": (1007422, 1132326, 835985, 15, 19)}[g.name]
    c = g.counts(0)
    assert (len(g.eu), int(c["total"][3]), int(c["total"][4]), c["clique_number"]) == shape[:4]
    assert g.tmax == shape[4]
    if g.name == "G50":
        assert int(c["total"][3]) > 2048 * 256 and (len(g.eu) + 63) // 64 == 7855


@pytest.mark.parametrize("window", [(2, -1, 0), (2, -1, 3), (6, -1, 6)], ids=str)
def test_census(g, window):
    check_census(g, *window)


@pytest.mark.parametrize("opts", [{"CENSUS_LDS": "0"}, {"CENSUS_PIVOT": "first"}], ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_census_options(g50, monkeypatch, opts):
    _set(monkeypatch, opts)
    check_census(g50, 2, -1, 3)


def test_maximal_cliques_from_two_vertices(g):
    check_maximal(g, 2)


def test_maximal_cliques_listed(g):
    """From the smallest k_min whose cliques the default MAXIMAL_LIST holds: the whole sorted list."""
    k_min = g.k_list()
    assert 2 < k_min <= g.maximal_all()["omega"]
    info = check_maximal(g, k_min)
    assert info["flags"] == 3 and info["n_cliques"] > 0


def test_maximal_cliques_without_lds(g50, monkeypatch):
    _set(monkeypatch, {"MAXIMAL_LDS": "0"})
    check_maximal(g50, 2)
    assert check_maximal(g50, g50.k_list())["flags"] == 3


def test_max_clique(g):
    check_max_clique(g)


def test_nucleus(g):
    check_nucleus(g)


def test_nucleus_hierarchy(g):
    check_nuclei(g)


# ---- G50 under a vmask

@pytest.fixture(scope="module")
def masked(K):
    graph = Graph(K, "G50 vmask", HUG["G50"][0], K.gen_hug_edges(*HUG["G50"]), masked=True)
    yield graph
    graph.close()


def test_masked_cliques(masked):
    assert 0 < len(masked.inv) < masked.nv and 0 < len(masked.eu) < 502700
    check_census(masked, 2, -1, 3)
    check_maximal(masked, 2)
    check_maximal(masked, masked.k_list())
    check_max_clique(masked)


def test_masked_nucleus(masked):
    check_nucleus(masked)
    check_nuclei(masked)


# ---- the scratch-capped grid

K5S = ([2, 3, 4, 5, 6], [100, 101, 102, 103, 104], [5, 6, 200, 201, 202])       # among the pages; the first and the third share two
PATH = (1000, 1500)                                                              # pages 1000 - 1001 - ... - 1500


def capped_edges(K):
    """A book on the spine (0, 1) with N_PAGES pages 2 .. N_PAGES + 1, three K_5 and a path among the pages, and a disjoint
    power-law graph behind it."""
    pages = np.arange(2, 2 + N_PAGES)
    book = [np.stack([np.zeros_like(pages), pages], 1), np.stack([np.ones_like(pages), pages], 1), np.asarray([[0, 1]])]
    for five in K5S:
        book.append(np.asarray([(u, v) for i, u in enumerate(five) for v in five[i + 1:]]))
    book.append(np.stack([np.arange(PATH[0], PATH[1]), np.arange(PATH[0] + 1, PATH[1] + 1)], 1))
    first = 2 + N_PAGES
    uv = np.concatenate(book + [K.gen_hug_edges(*CAPPED_HUG) + first]).astype(np.int64)
    return first + CAPPED_HUG[0], first, uv


@pytest.fixture(scope="module")
def capped(K):
    nv, first, uv = capped_edges(K)
    graph = Graph(K, "CAPPED", nv, uv)
    graph.first = first
    yield graph
    graph.close()


def clq_grid(max_candidates, t_max, sets, n_edges):
    """(slot_bytes, fit, grid) by the arithmetic of clq_layout (clique_root_dev.h): a slot holds the candidates, their bit matrix
    and the stack -- `sets` sets per level -- and all slots of a launch together take at most 512 MiB."""
    align16 = lambda x: (x + 15) & ~15
    w_max = max(1, (max_candidates + 63) // 64)
    levels = min(max_candidates, max(t_max - 2, 0)) + 2
    off_stk = align16(4 * max_candidates) + 8 * max_candidates * w_max
    slot = align16(off_stk + 8 * levels * sets * w_max)
    fit = (512 << 20) // slot
    n_chunks = (n_edges + 63) // 64
    return slot, fit, min(n_chunks, 1024, max(fit, 1))


def book_cliques(k):
    """The k-cliques of the book: a clique of j pages (c_j of them: the pages, the path's edges, the subsets of the K_5s) with
    any subset of the spine."""
    from math import comb
    def c(j):
        if j < 0:
            return 0
        if j == 0:
            return 1
        if j == 1:
            return N_PAGES
        return 3 * comb(5, j) - comb(2, j) + (PATH[1] - PATH[0] if j == 2 else 0)
    return c(k) + 2 * c(k - 1) + c(k - 2)


@pytest.mark.parametrize("opts", [{}, {"CENSUS_LDS": "0", "MAXIMAL_LDS": "0", "MAXCLQ_LDS": "0", "MAXCLQ_SEED": "0"}], ids=["default", "lds 0"])
def test_scratch_capped_grid(capped, monkeypatch, opts):
    """clq_layout cuts the launch grid to fit = 512 MiB / slot_bytes workgroups when a root's scratch slot is large, and the
    suite's other graphs never get there (4094 candidates come with 130 chunks; K_515 has slots of 100 KB).  Here the root
    (0, 1) has N_PAGES = 3000 candidates -- every page --, so with c = 3000, W = ceil(c / 64) = 47 and t_max levels of stack
      slot_bytes = 4 c + 8 c W + 8 t_max W * sets = 12 000 + 1 128 000 + 376 * 13 * sets (+ padding to 16),
    which at the max_candidates = 3000 and t_max = 13 the runs report is 1 144 896 bytes and fit = 468 for the census (one set
    per level), 1 149 776 bytes and fit = 466 for the maximal cliques (two).  The power-law graph behind the book brings the
    edges to 204 890, 3 202 chunks of 64: min(n_chunks, 1024) = 1024 > fit, and the roots go through 468 / 466 workgroups.
    max_candidates and t_max are asserted, and the arithmetic is redone from the values the run reports, so a change of shape
    that leaves the path unreached fails here.  The maximal cliques count |X| + |P|: the same 3000 at the root (0, 1), which
    has no excluded vertex.  MAXCLQ_SEED=0 starts the search from the lower bound 1, so its first launch sees the root (0, 1)
    with every page too."""
    _set(monkeypatch, opts)
    g, m = capped, len(capped.eu)
    info = check_census(g, 2, -1, 0)
    assert info["max_candidates"] == N_PAGES and info["t_max"] == g.tmax
    slot, fit, grid = clq_grid(info["max_candidates"], info["t_max"], 1, m)
    print("CAPPED census: slot %d bytes, fit %d, grid %d, chunks %d" % (slot, fit, grid, (m + 63) // 64))
    assert fit < min((m + 63) // 64, 1024) and grid == fit
    check_census(g, 3, -1, 3)
    info = check_maximal(g, 2)
    assert info["max_candidates"] == N_PAGES and info["t_max"] == g.tmax
    slot, fit, grid = clq_grid(info["max_candidates"], info["t_max"], 2, m)
    print("CAPPED maximal cliques: slot %d bytes, fit %d, grid %d" % (slot, fit, grid))
    assert fit < min((m + 63) // 64, 1024) and grid == fit
    assert check_maximal(g, g.k_list())["flags"] == 3
    check_max_clique(g)


def test_scratch_capped_grid_book_in_closed_form(capped, K):
    """The book's share of what the library reports -- the whole graph's numbers minus the references' for the power-law part
    alone -- against the closed form, so the part that cuts the grid is checked without any enumeration."""
    g = capped
    hug_rowptr, hug_col = O.simplify(CAPPED_HUG[0], K.gen_hug_edges(*CAPPED_HUG))
    total, _, info = g.a.run_clique_census(2, -1, 0)
    assert info["flags"] == 1 and info["max_candidates"] == N_PAGES
    hug = O.clique_counts(hug_rowptr, hug_col, 0)["total"][2:]
    n = max(len(total), len(hug))
    diff = np.pad(total.astype(np.int64), (0, n - len(total))) - np.pad(hug.astype(np.int64), (0, n - len(hug)))
    assert diff.tolist() == [book_cliques(k) for k in range(2, n + 2)]
    hist, count, largest, info = g.a.run_maximal_cliques(2)
    assert info["flags"] & 1 and info["max_candidates"] == N_PAGES
    hug_mx = O.maximal_cliques_all(hug_rowptr, hug_col, 2, want_list=False)["hist_all"][2:]
    n = max(len(hist), len(hug_mx))
    diff = np.pad(hist, (0, n - len(hist))) - np.pad(hug_mx, (0, n - len(hug_mx)))
    in_a_five = len({v for five in K5S for v in five})
    want = {3: N_PAGES - in_a_five - (PATH[1] - PATH[0] + 1), 4: PATH[1] - PATH[0], 7: 3}   # a lone page, a path edge, a K_5 -- each with the spine
    assert {k + 2: int(x) for k, x in enumerate(diff) if x} == want
    assert count[:2].tolist() == [sum(want.values())] * 2 and largest[:2].tolist() == [7, 7]
    pages = np.arange(2, g.first)
    on_path = (pages >= PATH[0]) & (pages <= PATH[1])
    ends = (pages == PATH[0]) | (pages == PATH[1])
    fives = np.bincount([v for five in K5S for v in five], minlength=g.first)[2:]
    assert count[2:g.first].tolist() == np.where(fives > 0, fives, np.where(on_path, 2 - ends, 1)).tolist()
    assert largest[2:g.first].tolist() == np.where(fives > 0, 7, np.where(on_path, 4, 3)).tolist()
    assert g.first == 2 + N_PAGES and int(total[0]) == len(g.eu)
