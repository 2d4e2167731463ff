"""GPU tests of the analyses built on the k-truss result PAST ONE TILE PER WORKGROUP of their capped grids.  The counting and
finishing passes of biconnected.hip, structural.hip, nucleus.hip, densest.hip, forest.hip and clique_root_dev.h launch at most
2048 workgroups of 256 lanes (1024 for k_clq_tmax), so past N = 2048 * 256 items a workgroup walks several tiles and carries an
LDS partial sum, its ballots or a queue cursor from one to the next.  The plain-Python references cannot take such graphs; the
graphs here are replicas of a small tile (tests/replica.py, proved on the references by tests/test_replica_ref.py), whose every
expected value follows from the tile's own result.  Every entry of every output array of every copy is compared, on the
library's own run_truss() edge list (whose parity other tests own).

What these graphs do NOT do: no class of a replica is larger than a tile copy, so none spans two tiles of one workgroup, and the
`lead == first` branch (the LDS partial sum for the class a workgroup's first tile starts with) is taken in the first tile only;
in later tiles every class goes the global-atomic way.  A class across the tiles of one workgroup is what the giant components
of the generated graphs give: for biconnected.hip tests/test_gpu_midsize_structure.py (the giant block of a power-law graph of a
million edges, a grid that is one block, a tree of blocks with three of more than 300 tiles each), for the others
test_composite and the mid-size tests of tests/test_gpu_midsize.py."""
import numpy as np
import pytest

import community_hierarchy_ref as CH
import densest_ref as D
import hierarchy_ref as H
import nucleus_hierarchy_ref as NH
import replica as RP
from test_gpu_nucleus import PATHS
from test_gpu_structural import SOME

pytestmark = pytest.mark.gpu

N = 2048 * 256
TILE = RP.tile()
K1, K2, K3, K4, K5, K9 = (RP.filler(x) for x in ("K1", "K2", "K3", "K4", "K5", "K9"))
SETTINGS = [SOME[1], SOME[4]]            # (1/2, 3): clusters, borders, outliers; (1/1, 2): clusters, hubs, outliers
POISON = {"POISON": "0xFFFFFFFF"}


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _set(monkeypatch, opts):
    for k, v in opts.items():
        monkeypatch.setenv("KOMB_" + k, v)


def _padded(layout, nv, parts):
    """The union of `parts` padded with isolated vertices to nv vertices: half of them before the first part (part 1 of the
    union) and half behind it, the other parts last.  So the last ids, and with them the last canonical edges, belong to the
    fillers the caller puts last, and a workgroup's last, ragged tile holds labelled items."""
    pad = nv - sum(t[0] * c for t, c in parts)
    assert pad >= 0 and parts[-1][1] > 0 and parts[-1][0][0] > 1
    return RP.build([(K1, pad // 2), parts[0], (K1, pad - pad // 2)] + parts[1:], layout)


def _truss(a, u, with_support=False):
    """The k-truss run of the loaded union u: the Frame of the library's own edge list (its constructor asserts that the list's
    restriction to each copy is the tile's canonical list), trussness and supports compared with the tiles' own."""
    out = a.run_truss(with_support=with_support)
    f = RP.Frame(u, out[0], out[1])
    assert np.array_equal(out[2], RP.trussness(f))
    if with_support:
        assert np.array_equal(out[3], RP.supports(f))
    return f


# ---- biconnected components

BC_INFO = ("k_used", "n_member_edges", "n_member_vertices", "n_blocks", "n_bridges", "n_articulation", "largest_block", "n_ecc", "largest_ecc",
           "depth")


def _bc_parts(m=None, members4=None):
    """Tile copies and fillers with m edges in all, or with members4 edges of trussness >= 4 (535 per tile, 10 per K5, 6 per K4)."""
    if members4 is None:
        c = m // len(TILE[1])
        return [(TILE, c), (K2, m - c * len(TILE[1]))]
    m4 = int((RP.tile_trussness(TILE[0], TILE[1][:, 0], TILE[1][:, 1]) >= 4).sum())
    r = next(r for r in range(5) if (members4 - 6 * r) % 5 == 0)
    rest = members4 - 6 * r
    c = rest // m4
    if (rest - m4 * c) % 10:
        c -= 1
    if rest == m4 * c:
        c -= 2
    q = (rest - m4 * c) // 10
    assert m4 * c + 10 * q + 6 * r == members4 and q > 0
    return [(TILE, c), (K2, 5), (K3, 3), (K4, r), (K5, q)]


# vertices / member edges / m + 1 on N - 1, N, N + 1 and 2 N + 1, between them; k = 2: every edge is a member
BC_CASES = [("blocked", N - 1, dict(m=N - 2)), ("interleaved", N, dict(m=N - 1)), ("blocked", N + 1, dict(m=N)),
            ("interleaved", 2 * N + 1, dict(m=N + 1)), ("blocked", N + 1, dict(m=2 * N)), ("interleaved", N - 1, dict(m=2 * N + 1)),
            ("interleaved", N, dict(members4=N - 1)), ("blocked", N - 1, dict(members4=N)), ("interleaved", N + 1, dict(members4=N + 1)),
            ("blocked", 2 * N + 1, dict(members4=2 * N + 1))]


def _bc_compare(a, f, k):
    want = RP.biconnected(f, k)
    block, size = a.run_biconnected(k)
    n_blocks, ecc_label, ecc_size = a.biconnected_fetch_vertices()
    got = {"block": block, "size": size, "n_blocks": n_blocks, "ecc_label": ecc_label, "ecc_size": ecc_size}
    for name in got:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (name, k)
    blocks = a.biconnected_fetch_blocks()
    for name in ("rep", "n_edges", "n_verts"):
        assert np.array_equal(blocks[name], want["blocks"][name]), (name, k)
    info = a.biconnected_info()
    assert tuple(info[x] for x in BC_INFO) == (k,) + tuple(want["info"][x] for x in BC_INFO[1:]), k
    assert a.biconnected_count() == want["info"]["n_blocks"]
    return want


@pytest.mark.parametrize("layout,nv,sizes", BC_CASES, ids=lambda x: x if isinstance(x, str) else str(x))
def test_biconnected(K, layout, nv, sizes):
    u = _padded(layout, nv, _bc_parts(**sizes))
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        assert f.nv == nv and ("m" not in sizes or f.m == sizes["m"])
        w2, w4 = _bc_compare(a, f, 2), _bc_compare(a, f, 4)
        assert w2["info"]["n_member_edges"] == f.m and ("members4" not in sizes or w4["info"]["n_member_edges"] == sizes["members4"])
        assert w2["info"]["depth"] == f.tile_cached(1, ("biconnected", 2))["info"]["depth"] == 10         # the tile's


# ---- structural clusters

ST_COUNTS = ("eps_num", "eps_den", "mu", "n_similar_edges", "n_cores", "n_borders", "n_hubs", "n_outliers", "n_clusters", "largest")
ST_CASES = [("blocked", N - 1), ("interleaved", N), ("blocked", N + 1), ("interleaved", N + 1), ("blocked", 2 * N + 1),
            ("interleaved", 2 * N + 1)]


def _st_compare(a, f, params):
    want = RP.structural(f, *params)
    label, size, role, sim_deg = a.run_structural_clusters(*params)
    got = {"label": label, "size": size, "role": role, "sim_deg": sim_deg, "similar": a.structural_clusters_fetch_edges()}
    for name in got:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (name, params)
    info = a.structural_clusters_info()
    assert {x: info[x] for x in ST_COUNTS} == want["info"], params
    return want


def _st_union(layout, nv):
    return _padded(layout, nv, [(TILE, 1500), (K2, 7), (K3, 5), (K5, 3)])


@pytest.mark.parametrize("layout,nv", ST_CASES)
def test_structural_clusters(K, layout, nv):
    u = _st_union(layout, nv)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u, with_support=True)
        for params in SETTINGS:
            want = _st_compare(a, f, params)
            assert want["info"]["n_clusters"] > 1500 and want["info"]["n_outliers"] > nv - 1500 * 97
        assert want["info"]["n_hubs"] >= 1500                           # (the second setting; the first has the borders)


# ---- densest subgraph: not local, so the restatement runs on the whole union (vectorised but for one linear loop).  Two launches
# are capped: k_den_rows over the vertices, and k_den_keys / k_den_prefix_part over n_pruned, the vertices the prune keeps.

# 8 vertices, 13 edges, coreness 3 3 2 3 3 3 2 2: the best core is the whole gadget (13 / 8), a prefix of 6 is denser (10 / 6)
GADGET = RP.as_tile(8, [(0, 3), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4), (1, 5), (2, 5), (3, 5), (3, 6), (4, 5), (4, 7), (6, 7)])


def _den_check(a, monkeypatch, runs, check):
    rowptr, col = a.get_csr()
    _, core = a.run_core()
    for local, iters in runs:
        if local is None:
            monkeypatch.delenv("KOMB_DENSEST_LOCAL", raising=False)
        else:
            monkeypatch.setenv("KOMB_DENSEST_LOCAL", local)
        want = D.densest(rowptr, col, core, iters)
        check(want, iters)
        a.densest_subgraph_run(iters)
        member, load = a.densest_subgraph_fetch()
        n_k, m_k = a.densest_subgraph_profile()
        info = a.densest_subgraph_info()
        assert member.dtype == np.int32 and np.array_equal(member, want["member"])
        assert load.dtype == np.int32 and np.array_equal(load, want["load"])
        assert np.array_equal(n_k, want["n_k"]) and np.array_equal(m_k, want["m_k"])
        for x in D.INFO_FIELDS:
            assert info[x] == want[x], (x, iters, local)


@pytest.mark.parametrize("layout,nv", [("blocked", N + 3), ("interleaved", 2 * N + 5)])
def test_densest_subgraph(K, monkeypatch, layout, nv):
    """k_den_rows (the histogram, count and fill passes) over up to 3 tiles of vertices; the pruned set is 60 000 vertices, one
    tile of k_den_keys / k_den_prefix_part."""
    u = _padded(layout, nv, [(TILE, 1200), (K5, 9), (K2, 3)])
    def check(want, iters):
        assert want["n_pruned"] == 1200 * 50 and want["m_pruned"] == 1200 * 461
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        _den_check(a, monkeypatch, ((None, 7), ("0", 2), (None, 0)), check)


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_densest_prefix_past_one_tile(K, monkeypatch, layout):
    """The prune keeps 700 000 vertices (k_den_keys and k_den_prefix_part walk 2 tiles per workgroup) and the answer is a prefix
    that ends in the second tile: 525 000 vertices, denser than the best core."""
    copies = 87500
    u = RP.build([(K1, 3), (GADGET, copies), (K2, 3)], layout)
    def check(want, iters):                                  # (asserted on the restatement's side)
        assert want["n_pruned"] == 8 * copies > N and want["m_pruned"] == 13 * copies
        assert want["source"] == D.SOURCE_PREFIX and N < want["n_sub"] < want["n_pruned"]
        if iters == 7:
            assert (want["n_sub"], want["m_sub"]) == (6 * copies, 10 * copies)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        _den_check(a, monkeypatch, ((None, 7), ("0", 2)), check)


# ---- (3,4)-nucleus decomposition

NUC_COUNTS = ("n_triangles", "n_cliques4", "theta_max", "n_levels")


def _nuc_compare(a, f, tri):
    want = RP.nucleus(f, tri)
    tris, edge_theta, vertex_theta = a.nucleus_fetch(), a.nucleus_fetch_edges(), a.nucleus_fetch_vertices()
    for name in ("a", "b", "c", "key0", "theta"):
        assert tris[name].dtype == np.int32 and np.array_equal(tris[name], want[name]), name
    assert edge_theta.dtype == np.int32 and np.array_equal(edge_theta, want["edge_theta"])
    assert vertex_theta.dtype == np.int32 and np.array_equal(vertex_theta, want["vertex_theta"])
    info = a.nucleus_info()
    assert {x: info[x] for x in NUC_COUNTS} == want["info"]
    assert info["n_subrounds"] >= info["n_levels"]
    return want


def _nuc_union(layout, n_triangles):
    """Tile copies and K_3 (one triangle of theta 0 each) with n_triangles triangles in all."""
    c = n_triangles // 1559
    return RP.build([(K3, 200), (TILE, c), (K1, 5), (K3, n_triangles - 1559 * c - 200), (K2, 3)], layout)


def _frontier_union(layout):
    """About 50 tile copies beside enough K_5 that the first frontier of level 2 is longer than N: a K_5's 10 triangles have
    key0 = theta = 2 and no neighbour outside it, so all of them are in that frontier."""
    return RP.build([(TILE, 25), (K5, N // 10 + 2), (K3, 4), (TILE, 25)], layout)


@pytest.mark.parametrize("paths", [PATHS[0], PATHS[3]], ids=["default", "queued"])
@pytest.mark.parametrize("layout,n_triangles", [("blocked", N - 1), ("interleaved", N), ("blocked", N + 1), ("interleaved", N + 1)])
def test_nucleus_triangle_counts(K, monkeypatch, layout, n_triangles, paths):
    _set(monkeypatch, paths)
    u = _nuc_union(layout, n_triangles)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        a.nucleus_run()
        want = _nuc_compare(a, f, RP.Triangles(f))
        assert want["info"]["n_triangles"] == n_triangles and want["levels"] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_nucleus_smallest_key_behind_the_first_tile(K, layout):
    """k_nuc_min: N + 32 triangles of key 2 first (K_5), then 25 tile copies and one K_3.  Every live triangle of a key below 2
    has an index >= N, so the levels 0 and 1 exist only for a sweep that goes on past its first tile."""
    u = RP.build([(K5, N // 10 + 2), (TILE, 25), (K3, 1)], layout)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        a.nucleus_run()
        tri = RP.Triangles(f)
        want = _nuc_compare(a, f, tri)
        low = np.flatnonzero((want["key0"] < 2) | (want["theta"] < 2))          # (asserted on the reference's side)
        assert len(low) and int(low.min()) >= N and int(tri.gt[2][0, 0]) == tri.n - 1 and want["theta"][-1] == 0
        assert (want["key0"][:N] == 2).all() and want["levels"] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("paths", [PATHS[0], PATHS[3]], ids=["default", "queued"])
@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_nucleus_frontier_longer_than_the_grid(K, monkeypatch, layout, paths):
    _set(monkeypatch, paths)
    u = _frontier_union(layout)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        a.nucleus_run()
        tri = RP.Triangles(f)
        want = _nuc_compare(a, f, tri)
        k5 = tri.dec[1]
        assert set(k5["key0"].tolist()) == {2} and set(k5["theta"].tolist()) == {2} and k5["levels"] == [2]
        assert f.copies(1) * len(k5["theta"]) > N                                 # the level-2 frontier, on the reference's side
        assert want["info"]["n_triangles"] > N


# ---- the three nesting forests: CLAIM / ADOPT past their 2048 workgroups with triangles, edges and vertices as the items

def _forest_compare(nodes, node, want, info, info_want):
    got = dict(nodes, node=node)
    assert RP.same_forest(got, want)
    for x in H.FIELDS + ("node",):                           # and the node numbers: (k, rep) order is part of the contract
        assert np.array_equal(got[x], want[x]), x
    assert info == info_want


def _many_k3_union(layout):
    """More than N vertices and more than N edges at trussness 3, around 50 tile copies."""
    return RP.build([(TILE, 25), (K3, N // 3 + 2), (K2, 3), (TILE, 25), (K5, 4)], layout)


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_nucleus_hierarchy(K, layout):
    u = _frontier_union(layout)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        a.nucleus_run()
        tri = RP.Triangles(f)
        want = RP.nucleus_hierarchy(f, tri)
        theta = RP.nucleus(f, tri)["theta"]
        assert np.array_equal(a.nucleus_fetch()["theta"], theta) and int((theta >= 1).sum()) > N
        nodes, node = a.run_nucleus_hierarchy()
        info = a.nucleus_hierarchy_info()
        _forest_compare(nodes, node, want, tuple(info[x] for x in ("n_nodes", "n_roots", "theta_max", "depth", "n_member_triangles")),
                        NH.info(want, theta))
        label, size = a.nucleus_hierarchy_labels(2)
        wl, ws = NH.walk_up(want, theta, 2)
        assert np.array_equal(label, wl) and np.array_equal(size, ws)


@pytest.mark.parametrize("which", ["K5", "K3"])
@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_community_hierarchy(K, layout, which):
    u = _frontier_union(layout) if which == "K5" else _many_k3_union(layout)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        tr = RP.trussness(f)
        assert int((tr == (5 if which == "K5" else 3)).sum()) > N                 # more than N edges at one level
        want = RP.community_hierarchy(f)
        nodes, node = a.run_community_hierarchy()
        info = a.community_hierarchy_info()
        _forest_compare(nodes, node, want, tuple(info[x] for x in ("n_nodes", "n_roots", "k_max", "depth", "n_member_edges")), CH.info(want))
        label, size = a.community_hierarchy_labels(4)
        wl, ws = CH.walk_up(want, tr, 4)
        assert np.array_equal(label, wl) and np.array_equal(size, ws)


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_truss_hierarchy(K, layout):
    u = _many_k3_union(layout)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        tr = RP.trussness(f)
        lvl = H.truss_levels(f.nv, f.eu, f.ev, tr)
        assert int((lvl == 3).sum()) > N                                          # more than N vertices at one level
        want = RP.truss_hierarchy(f)
        nodes, node = a.run_hierarchy("truss")
        info = a.hierarchy_info()
        _forest_compare(nodes, node, want, (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]), H.info(want, "truss"))
        label, _ = a.run_components("truss", 4)
        assert np.array_equal(label, H.walk_up_labels(want, lvl, 4))


# ---- the clique searches: more than 262 144 edges (k_clq_tmax strides) and many chunks per wave (clq_next_chunk)

CLQ_COPIES = 1000
CLQ_LIST = {"MAXIMAL_LIST": "300000"}


def _clq_union(layout, k9=False):
    """k9: one K_9 behind everything else.  Its 36 edges are the last of the canonical list and the only ones of trussness 9,
    so k_clq_tmax finds the largest trussness only in the last stride of its 1024 workgroups."""
    return RP.build([(K3, 4), (TILE, CLQ_COPIES), (K1, 3), (K2, 2), (K5, 3)] + ([(K9, 1)] if k9 else []), layout)


def _clq_max_clique(a, f, top=8, n_top=CLQ_COPIES * 8):
    want = RP.max_clique(f)
    assert want["nodes"] < 2 ** 30 // 64                                          # far below the default budget (reference side)
    info, count, witness = a.run_max_clique()
    assert info["flags"] == 7 == want["flags"]
    assert (info["omega"], info["upper"], info["t_max"], info["n_max_cliques"]) == (top, top, top, n_top)
    assert (want["omega"], want["upper"], want["t_max"], want["n_max_cliques"]) == (top, top, top, n_top)
    assert count.dtype == np.int32 and np.array_equal(count, want["count"])
    cliques = a.max_clique_list()
    assert cliques.dtype == np.int32 and np.array_equal(cliques, want["list"].rows)
    assert np.array_equal(witness, cliques[0])
    w = witness.astype(np.int64)                                                  # the witness is a clique of the edge list
    pairs = w[np.stack(np.triu_indices(len(w), 1), 1)]
    keys = f.eu * f.nv + f.ev
    assert np.isin(pairs[:, 0] * f.nv + pairs[:, 1], keys).all() and (np.diff(w) > 0).all()


def _clq_census(a, f, top=8):
    for k_local in (0, 4, 8):
        want = RP.clique_census(f, k_local)
        total, local, info = a.run_clique_census(2, -1, k_local)
        assert info["flags"] == 1 and (info["k_lo"], info["k_hi"], info["t_max"], info["omega"]) == (2, top, top, top)
        assert [int(x) for x in total] == want["total"]
        if k_local:
            assert local.dtype == np.uint64 and np.array_equal(local.astype(np.int64), want["local"])
    tile = f.tile_cached(1, ("census", 0))["exact"][0]
    assert tile == [564, 1559, 2073, 1431, 544, 107, 8]
    assert want["total"][6] == CLQ_COPIES * 8 + (9 if top == 9 else 0) and want["total"][0] == f.m and len(want["total"]) == top - 1


def _clq_maximal(a, f, communities=True, top=8):
    want = RP.maximal_cliques(f)
    assert want["nodes"] < 2 ** 30 // 64                                          # far below the default budget (reference side)
    hist, count, largest, info = a.run_maximal_cliques(2)
    assert info["flags"] == 3                                                     # complete and listed: not cut by the budget
    assert (info["k_min"], info["k_hi"], info["t_max"], info["omega"], info["n_cliques"]) == (2, top, top, top, want["n_cliques"])
    assert np.array_equal(hist, want["hist"])
    assert np.array_equal(count, want["count"]) and np.array_equal(largest, want["largest"])
    offset, verts = a.maximal_cliques_list()
    w_offset, w_verts = want["list"].offset_verts()
    assert len(w_verts) + want["n_cliques"] == CLQ_COPIES * 1829 + 4 * 4 + 2 * 3 + 3 * 6 + (10 if top == 9 else 0) <= 2 ** 24      # the list's words
    assert np.array_equal(offset, w_offset) and np.array_equal(verts, w_verts)    # the whole sorted list
    for k in ((3, 4) if communities else ()):
        cw = RP.clique_communities(f, want, k)
        assert cw["pair_tests"] < 2 ** 32 // 64
        label, size, rep, n_cliques, _, _, n_comm, first, cinfo = a.run_clique_communities(k)
        for got, name in ((label, "label"), (size, "size"), (rep, "rep"), (n_cliques, "n_cliques"), (n_comm, "n_comm"), (first, "first")):
            assert got.dtype == np.int32 and np.array_equal(got, cw[name]), (k, name)
        for x in ("n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap", "pair_tests"):
            assert cinfo[x] == cw[x], (k, x)


@pytest.mark.parametrize("layout,lds", [("blocked", None), ("interleaved", None), ("interleaved", "0")],
                         ids=["blocked", "interleaved", "interleaved, lds 0"])
def test_clique_searches(K, monkeypatch, layout, lds):
    """Maximum clique, clique census, maximal cliques and k-clique communities of one loaded union."""
    _set(monkeypatch, CLQ_LIST)
    if lds is not None:
        _set(monkeypatch, {"MAXCLQ_LDS": lds, "CENSUS_LDS": lds, "MAXIMAL_LDS": lds})
    u = _clq_union(layout)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        assert f.m > 262144 and f.m // 64 > 8 * 1024
        _clq_max_clique(a, f)
        _clq_census(a, f)
        _clq_maximal(a, f, communities=lds is None)


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_clique_searches_largest_trussness_last(K, monkeypatch, layout):
    """k_clq_tmax past its first stride: the only edges of the largest trussness are the last 36 of 564 080."""
    _set(monkeypatch, CLQ_LIST)
    u = _clq_union(layout, k9=True)
    with K.KombAccel() as a:
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        tr = RP.trussness(f)                                                      # (asserted on the reference's side)
        assert int(tr.max()) == 9 and int(np.flatnonzero(tr == 9).min()) == f.m - 36 >= 2 * 1024 * 256 and int(tr[:f.m - 36].max()) == 8
        _clq_max_clique(a, f, top=9, n_top=1)
        _clq_census(a, f, top=9)
        _clq_maximal(a, f, top=9)


# ---- poisoned memory, and one context that goes large replica -> tiny graph -> large replica

def test_poisoned_memory(K, monkeypatch):
    """One configuration of each group with every allocation filled with garbage first."""
    _set(monkeypatch, dict(POISON, **CLQ_LIST))
    with K.KombAccel() as a:
        u = _padded("interleaved", N + 1, _bc_parts(m=2 * N))
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        _bc_compare(a, f, 2)
        _bc_compare(a, f, 4)
    with K.KombAccel() as a:
        u = _st_union("blocked", N + 1)
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u, with_support=True)
        _st_compare(a, f, SETTINGS[0])
        rowptr, col = a.get_csr()
        _, core = a.run_core()
        want = D.densest(rowptr, col, core, 3)
        member, load, info = a.run_densest_subgraph(3)
        assert np.array_equal(member, want["member"]) and np.array_equal(load, want["load"])
        assert all(info[x] == want[x] for x in D.INFO_FIELDS)
    with K.KombAccel() as a:
        u = _frontier_union("interleaved")
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        a.nucleus_run()
        tri = RP.Triangles(f)
        _nuc_compare(a, f, tri)
        nodes, node = a.run_nucleus_hierarchy()
        assert RP.same_forest(dict(nodes, node=node), RP.nucleus_hierarchy(f, tri))
        nodes, node = a.run_community_hierarchy()
        assert RP.same_forest(dict(nodes, node=node), RP.community_hierarchy(f))
        nodes, node = a.run_hierarchy("truss")
        assert RP.same_forest(dict(nodes, node=node), RP.truss_hierarchy(f))
    with K.KombAccel() as a:
        u = _clq_union("blocked")
        a.from_edges(u.nv, u.pairs)
        f = _truss(a, u)
        _clq_max_clique(a, f)
        _clq_maximal(a, f, communities=False)


def test_reused_context_large_tiny_large(K, monkeypatch):
    _set(monkeypatch, dict(POISON, **CLQ_LIST))
    big = _padded("blocked", N + 1, [(TILE, 950), (K5, N // 10 + 2), (K3, 5)])
    tiny = RP.build([(K1, 1), (TILE, 1), (K5, 1)], "blocked")
    with K.KombAccel() as a:
        for u in (big, tiny, big):
            a.from_edges(u.nv, u.pairs)
            f = _truss(a, u, with_support=True)
            _bc_compare(a, f, 2)
            _st_compare(a, f, SETTINGS[1])
            a.nucleus_run()
            tri = RP.Triangles(f)
            _nuc_compare(a, f, tri)
            nodes, node = a.run_nucleus_hierarchy()
            assert RP.same_forest(dict(nodes, node=node), RP.nucleus_hierarchy(f, tri))
            nodes, node = a.run_community_hierarchy()
            assert RP.same_forest(dict(nodes, node=node), RP.community_hierarchy(f))
            want = RP.maximal_cliques(f)
            hist, count, largest, info = a.run_maximal_cliques(2)
            assert info["flags"] & 1 and np.array_equal(hist, want["hist"]) and np.array_equal(count, want["count"])
            assert np.array_equal(largest, want["largest"])
