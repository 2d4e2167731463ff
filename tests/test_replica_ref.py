"""CPU proof of tests/replica.py: for every reference that tests/test_gpu_replicas.py relies on, the reference run on a whole
union (5 copies of the tile and a few fillers, both layouts) gives exactly what the harness derives from the tile's own result.
And the comparisons reject a label that is off by one copy and a swapped pair of copies.  No GPU, no library."""
import numpy as np
import pytest

import biconnected_ref as B
import clique_census_ref as CC
import clique_communities_ref as QC
import community_hierarchy_ref as CH
import densest_ref as D
import hierarchy_ref as H
import max_clique_ref as MC
import maximal_cliques_ref as MQ
import nucleus_hierarchy_ref as NH
import nucleus_ref as N
import replica as RP
import structural_ref as S
from test_gpu_structural import SOME

COPIES = 5
SETTINGS = [SOME[1], SOME[4]]                  # the two of test_gpu_structural.SOME that test_gpu_replicas uses


def _parts():
    return [(RP.filler("K3"), 4), (RP.tile(), COPIES), (RP.filler("K1"), 3), (RP.filler("K2"), 2), (RP.filler("K5"), 3)]


_FRAMES = {}


def _frame(layout):
    """(Union, Frame, trussness by the restatement's own peel of the whole union), made once per layout."""
    if layout not in _FRAMES:
        u = RP.build(_parts(), layout)
        eu, ev = u.canonical()
        _FRAMES[layout] = (u, RP.Frame(u, eu, ev), np.asarray(MC.trussness(u.nv, eu, ev), np.int64))
    return _FRAMES[layout]


def _same(want, got, names):
    for x in names:
        assert np.array_equal(np.asarray(want[x]), np.asarray(got[x])), x


def test_the_tile_is_the_one_described():
    nv, e = RP.tile()
    assert (nv, len(e)) == (97, 564) and nv % 64 != 0
    assert not np.isin(92, e)                                                    # an isolated vertex
    dec = N.decompose(nv, e[:, 0], e[:, 1])
    assert (dec["info"]["n_triangles"], dec["info"]["n_cliques4"]) == (1559, 2073)
    assert dec["levels"] == [0, 1, 2, 3, 4, 5] and dec["subrounds"] == [1, 4, 5, 6, 5, 2]
    tr = RP.tile_trussness(nv, e[:, 0], e[:, 1])
    assert np.bincount(tr)[2:].tolist() == [23, 6, 10, 21, 55, 202, 247]
    b = B.biconnected(nv, e[:, 0], e[:, 1], tr, 2)["info"]
    assert (b["n_blocks"], b["n_bridges"], b["n_articulation"]) == (17, 14, 10)
    k5 = RP.filler("K5")
    d5 = N.decompose(k5[0], k5[1][:, 0], k5[1][:, 1])
    assert d5["info"] == {"n_triangles": 10, "n_cliques4": 5, "theta_max": 2, "n_levels": 1} and set(d5["key0"].tolist()) == {2}
    for mu_eps in SETTINGS:                                                      # clusters, hubs and outliers between the two
        info = S.clusters(nv, e[:, 0], e[:, 1], S.supports(nv, e[:, 0], e[:, 1]), *mu_eps)["info"]
        assert info["n_clusters"] > 0 and info["n_outliers"] > 0
    infos = [S.clusters(nv, e[:, 0], e[:, 1], S.supports(nv, e[:, 0], e[:, 1]), *s)["info"] for s in SETTINGS]
    assert infos[0]["n_borders"] > 0 and infos[1]["n_hubs"] > 0


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_layouts_are_increasing_inside_a_copy(layout):
    u, f, _ = _frame(layout)
    seen = np.zeros(u.nv, np.int64)
    for m in u.maps:
        assert (np.diff(m, axis=1) > 0).all()
        np.add.at(seen, m.reshape(-1), 1)
    assert (seen == 1).all()
    tile_map = u.maps[1]
    if layout == "blocked":
        assert (np.diff(tile_map, axis=1) == 1).all()
    else:
        assert (np.diff(tile_map, axis=1) == COPIES).all() and (np.diff(tile_map[:, 0]) == 1).all()
    for p in f.parts():                                                          # positions() of the vertices is the map itself
        assert np.array_equal(RP.positions(u.copy_of_vertex(p)), u.maps[p])


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_trussness_and_supports(layout):
    u, f, tr = _frame(layout)
    assert np.array_equal(tr, RP.trussness(f))
    assert np.array_equal(S.supports(u.nv, f.eu, f.ev), RP.supports(f))


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_biconnected(layout, k):
    u, f, tr = _frame(layout)
    want, got = B.biconnected(u.nv, f.eu, f.ev, tr, k), RP.biconnected(f, k)
    _same(want, got, ("block", "size", "n_blocks", "ecc_label", "ecc_size"))
    _same(want["blocks"], got["blocks"], ("rep", "n_edges", "n_verts"))
    assert want["info"] == got["info"]
    tile_info = f.tile_cached(1, ("biconnected", k))["info"]
    assert got["info"]["depth"] == tile_info["depth"]                            # the depth is the tile's


@pytest.mark.parametrize("params", SETTINGS)
@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_structural(layout, params):
    u, f, _ = _frame(layout)
    want, got = S.clusters(u.nv, f.eu, f.ev, S.supports(u.nv, f.eu, f.ev), *params), RP.structural(f, *params)
    _same(want, got, ("similar", "sim_deg", "label", "size", "role"))
    assert want["info"] == got["info"]


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_nucleus_and_its_hierarchy(layout):
    u, f, _ = _frame(layout)
    tri = RP.Triangles(f)
    want, got = N.decompose(u.nv, f.eu, f.ev), RP.nucleus(f, tri)
    _same(want, got, ("a", "b", "c", "key0", "theta", "edge_theta", "vertex_theta"))
    assert want["info"] == got["info"] and want["levels"] == got["levels"]
    assert want["subrounds"] == tri.dec[1]["subrounds"]                          # (this union's: the fillers add no sub-round)
    h, hgot = NH.forest(want["theta"], want["cliques"]), RP.nucleus_hierarchy(f, tri)
    _same(h, hgot, H.FIELDS + ("node",))
    assert RP.same_forest(h, hgot)


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_truss_and_community_hierarchy(layout):
    u, f, tr = _frame(layout)
    for want, got in ((H.truss_hierarchy(u.nv, f.eu, f.ev, tr), RP.truss_hierarchy(f)),
                      (CH.community_hierarchy(u.nv, f.eu, f.ev, tr), RP.community_hierarchy(f))):
        _same(want, got, H.FIELDS + ("node",))
        assert RP.same_forest(want, got) and len(want["k"]) > 2 * COPIES


def test_densest_of_copies():
    """densest_ref.densest is not local (test_gpu_replicas runs it on the whole union); what IS fixed by the tile: the profile
    is copies x the tile's, and with it the best core, the prune and, without rounds, the members."""
    nv_t, e = RP.tile()
    rp_t, col_t = D.csr_of_edges(nv_t, e)
    tile = D.densest(rp_t, col_t, D.coreness(rp_t, col_t), 0)
    for layout in RP.LAYOUTS:
        u = RP.build([(RP.tile(), COPIES)], layout)
        rowptr, col = D.csr_of_edges(u.nv, u.pairs)
        got = D.densest(rowptr, col, D.coreness(rowptr, col), 0)
        assert np.array_equal(got["n_k"], COPIES * tile["n_k"]) and np.array_equal(got["m_k"], COPIES * tile["m_k"])
        assert (got["k_best"], got["k_prune"], got["k_max"]) == (tile["k_best"], tile["k_prune"], tile["k_max"])
        assert (got["n_sub"], got["m_sub"], got["n_pruned"]) == (COPIES * tile["n_sub"], COPIES * tile["m_sub"], COPIES * tile["n_pruned"])
        assert np.array_equal(got["member"], RP.spread(u.nv, [(u.maps[0], tile["member"])]))


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_max_clique(layout):
    u, f, _ = _frame(layout)
    want, got = MC.solve(u.nv, f.eu, f.ev), RP.max_clique(f)
    for x in ("omega", "upper", "flags", "t_max", "n_max_cliques"):
        assert want[x] == got[x], x
    assert (got["omega"], got["n_max_cliques"]) == (8, COPIES * 8)
    assert np.array_equal(want["count"], got["count"])
    assert np.array_equal(np.asarray(want["cliques"]), got["list"].rows) and tuple(got["witness"]) == want["witness"]


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_clique_census(layout):
    u, f, _ = _frame(layout)
    for k_local in (0, 3, 5, 8):
        want, got = CC.census(u.nv, f.eu, f.ev, 2, -1, k_local), RP.clique_census(f, k_local)
        assert want["exact"][0] == got["total"] and (want["k_hi"], want["t_max"], want["omega"]) == (got["k_hi"], got["t_max"], got["omega"])
        assert k_local == 0 or np.array_equal(np.asarray(want["exact"][1]), got["local"])
    tile = f.tile_cached(1, ("census", 0))["exact"][0]
    assert tile == [564, 1559, 2073, 1431, 544, 107, 8]


@pytest.mark.parametrize("layout", RP.LAYOUTS)
def test_maximal_cliques_and_clique_communities(layout):
    u, f, _ = _frame(layout)
    want, got = MQ.solve(u.nv, f.eu, f.ev, 2), RP.maximal_cliques(f)
    for x in ("k_hi", "t_max", "omega", "n_cliques"):
        assert want[x] == got[x], x
    _same(want, got, ("hist", "count", "largest"))
    offset, verts = got["list"].offset_verts()
    assert verts.tolist() == [v for c in want["cliques"] for v in c]
    assert np.diff(offset).tolist() == [len(c) for c in want["cliques"]]
    t = got["tiles"][1]
    assert (t["n_cliques"], sum(len(c) for c in t["cliques"])) == (295, 1534)          # 1829 list words: one more per clique
    for k in (3, 4):
        cw, cg = QC.solve(u.nv, want["cliques"], k), RP.clique_communities(f, got, k)
        _same(cw, cg, ("label", "size", "rep", "n_cliques", "n_comm", "first"))
        for x in ("n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap"):
            assert cw[x] == cg[x], (k, x)
        assert QC.pair_tests(want["cliques"], k) == cg["pair_tests"]


# ---- what the comparisons must reject

def test_positions_and_map_label_reject_a_label_off_by_one_copy():
    u, f, tr = _frame("interleaved")
    want = B.biconnected(u.nv, f.eu, f.ev, tr, 2)
    RP.biconnected(f, 2)
    g = f.ge[1]
    assert np.array_equal(RP.positions(u.copy_of_vertex(1)[f.eu]), g)
    tile_block = f.tile_cached(1, ("biconnected", 2))["block"]
    mapped = RP.map_label(tile_block, g)
    assert np.array_equal(want["block"][g], mapped)
    assert RP.map_label(np.asarray([-1, 0, 2]), g[:, :3]).tolist() == [[-1, int(r[0]), int(r[2])] for r in g]
    off = RP.map_label(tile_block, np.roll(g, 1, axis=0))                        # every copy labelled by its neighbour copy's items
    assert off.shape == mapped.shape and not np.array_equal(want["block"][g], off)
    one = mapped.copy()                                                          # one label of one copy, moved to the next copy
    one[2, 7] = RP.map_label(tile_block, g)[3, 7]
    assert not np.array_equal(want["block"][g], one)
    with pytest.raises(AssertionError):                                          # a copy that owns an item too many
        RP.positions(np.asarray([0, 0, 1, 1, 1, -1]))


def test_spread_rejects_swapped_copies_and_double_cover():
    u, f, _ = _frame("blocked")
    want = RP.supports(f)
    g = f.ge[1]
    swapped = g.copy()
    swapped[[1, 3]] = g[[3, 1]]
    vals = np.arange(g.size).reshape(g.shape)                                    # a value that differs from copy to copy
    pieces = lambda gg: [(f.ge[p], np.zeros(f.ge[p].shape[1], np.int64)) if p != 1 else (gg, vals) for p in f.parts()]
    assert not np.array_equal(RP.spread(f.m, pieces(g)), RP.spread(f.m, pieces(swapped)))
    assert np.array_equal(want, RP.spread(f.m, [(f.ge[p], f.tile_cached(p, "support")) for p in f.parts()]))
    with pytest.raises(AssertionError):
        RP.spread(f.m, pieces(g)[:-1])                                           # items nobody owns
    with pytest.raises(AssertionError):
        RP.spread(f.m, pieces(g) + [(g[:1], vals[:1])])                          # items owned twice


def test_the_forest_comparer_rejects_perturbed_forests():
    u, f, tr = _frame("interleaved")
    want = RP.community_hierarchy(f)
    ref = CH.community_hierarchy(u.nv, f.eu, f.ev, tr)
    assert RP.same_forest(ref, want)
    n = len(want["k"])
    perm = np.random.default_rng(5).permutation(n)                               # other node numbers, the same forest
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    renumbered = {x: np.asarray(ref[x], np.int64)[perm] for x in H.FIELDS}
    renumbered["parent"] = np.where(renumbered["parent"] >= 0, inv[np.maximum(renumbered["parent"], 0)], -1)
    renumbered["node"] = np.where(ref["node"] >= 0, inv[np.maximum(ref["node"], 0)], -1)
    assert RP.same_forest(renumbered, want)
    g = f.ge[1]
    def broken(field, at, value):
        h = {x: np.asarray(ref[x], np.int64).copy() for x in ref}
        h[field][at] = value
        return h
    child = int(np.flatnonzero(ref["parent"] >= 0)[0])
    reps_of_copy = [set(g[i].tolist()) for i in range(COPIES)]
    first = int(np.flatnonzero([int(r) in reps_of_copy[0] for r in ref["rep"]])[0])
    twin = int(np.flatnonzero((ref["k"] == ref["k"][first]) & np.asarray([int(r) in reps_of_copy[1] for r in ref["rep"]]))[0])
    assert not RP.same_forest(broken("rep", first, int(ref["rep"][first]) + 1), want)        # a representative off by one copy
    assert not RP.same_forest(broken("size", child, int(ref["size"][child]) + 1), want)
    assert not RP.same_forest(broken("shell", child, int(ref["shell"][child]) - 1), want)
    assert not RP.same_forest(broken("parent", child, -1), want)
    assert not RP.same_forest(broken("parent", child, twin if ref["parent"][child] != twin else first), want)
    e = int(np.flatnonzero(ref["node"] == first)[0])
    assert not RP.same_forest(broken("node", e, twin), want)                                 # an edge handed to the next copy's node
    assert not RP.same_forest(broken("node", e, -1), want)
    swapped = RP.replicate_forest(f.m, [(f.ge[p] if p != 1 else np.roll(g, 1, axis=0), f.tile_cached(p, "community_hierarchy"))
                                        for p in f.parts()])
    assert RP.same_forest(swapped, want)                       # whole copies swapped: the same union, and no difference
    half = g.copy()
    half[[0, 1], :5] = g[[1, 0], :5]                           # two copies that swap some of their edges: another forest
    mixed = RP.replicate_forest(f.m, [(f.ge[p] if p != 1 else half, f.tile_cached(p, "community_hierarchy")) for p in f.parts()])
    assert not RP.same_forest(mixed, want)
