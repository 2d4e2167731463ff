"""Mid-size GPU tests of the three analyses that tests/test_gpu_midsize.py and tests/test_gpu_midsize_structure.py left out: the
betweenness centrality, the distance analysis and the graphlet census, against the native references of oracle/komb_oracle.c
(orc_betweenness, orc_bfs_sources, orc_graphlets, orc_orbits_by_definition; tests/test_oracle_traversals.py ties those to the
Python restatements and to the stored fixtures bit for bit).  The references run one queue BFS per source over the sorted CSR
rows and fill dense arrays: they share nothing with the library's 64-source batches, bit masks, (d, id) order, hash tables and
canonical-edge roots.  They are fed the oracle's own CSR, which test_gpu_midsize.Graph asserts equal to the library's.

Every comparison is exact equality of whole arrays -- bc[] and harmonic[] as 64-bit patterns -- and of every integer info
field.  One context and one k-truss run per graph, shared by its tests and never changed; one reference per (graph, source
list), computed once.  Every statement about an input (an isolated source, a root above 2^32, a grid at its cap) is asserted
from the reference's side.

The graphs (seconds are the reference's CPU time on one thread of the machine this was written on; the machine with the MI355X
ran the same calls about three times as fast: 0.66 and 1.48 s for the betweenness lists of 65 and 129 entries, 0.86 and 1.09 s for
the distance lists, 1.29, 0.51 and 0.28 s for the three censuses, 0.20 and 0.56 s on the grid):
  G100  gen_hug_edges(100000, 245000, 2.6, 42): m 1 007 422, largest degree 7 059, 3 571 rows longer than 64 entries and 12
        longer than 2 048, 1 765 isolated vertices, depth 7 from the lists here.  More than 2048 x 4 and 2048 x 32 vertices: the
        default grids of the betweenness sweeps and of k_dist_level are at their cap, and every wave takes several turns, with
        no option set.  The lists are prefixes of one master list of 321 entries drawn from 200 vertices -- repeats, no order
        --, with the hub first and an isolated vertex and both ends of a 2-vertex component among the first entries:
        betweenness from 1, 65 and 129 entries (0.04, 2.5 and 4.4 s), distances from 257 and 321 at DIST_WORDS 1 and 4 (2.9
        and 3.8 s).  The lists are SHORTER than the 513 and 1 025 entries first planned: a reference search costs 38 ms
        (betweenness) and 10 ms (distances) per entry on this graph, so those lists would have taken 19 s and 10.5 s, against
        the 4.58 s of the slowest reference of the other two mid-size files.  129 is two batches of 64 and one entry; 321 is a
        batch of 256 and a second one of one full word and one entry at DIST_WORDS = 4, five batches and one entry at 1.
        Graphlets at the default options: reference 3.4 s.
  GRID300  a 300 x 300 grid, ids permuted by default_rng(7): depth 598 from a corner, where the path count to the opposite
        corner is C(598, 299), about 2^594 -- finite and far past 2^53, so almost every sigma and delta is an inexact double
        and the operation order decides most bits.  Betweenness from the four corners, the centre and 60 others (0.7 s);
        distances from those and 200 more (265 entries: two batches at DIST_WORDS = 4; 1.5 s), harmonic sums over hundreds
        of levels.
  STRIP  a 725 x 400 grid, ids permuted alike: from a corner sigma passes 2^1024 -- C(724 + r, r) at the far end of row r --, the
        reference answers its limit code (asserted first, on the CPU) and the library KOMB_ERR_LIMIT.
  G50   gen_hug_edges(50000, 122500, 2.6, 42): m 502 700, largest degree 4 372 (the hub's claw-centre count alone is
        C(4372, 3), about 1.4 x 10^10 > 2^32), and G50 under the usual vmask (coreness >= half the largest; 16 279 vertices,
        245 023 edges).  The whole census at the default options and at GRAPHLET_LDS=0, where every heavy root takes a dense
        table of 50 000 words that kGlParts = 64 workgroups share.  Reference: 1.3 s and 0.65 s.  On G50 200 vertices drawn by a
        fixed seed among those with an edge, no hub (the five largest degrees) as a neighbour and at most BALL = 3 000
        vertices within three hops (622 of the 50 000 qualify: most vertices are within two hops of a hub) are also counted
        straight from the definition (0.7 s with the search for them): up to 4 097 connected sets at one vertex.

RECORDED holds what the library reported on an MI355X; ms, cycle_items and the tier counts of GRAPHLET_DEBUG are never asserted.

WALL holds the wall times pytest reported for this file and for tests/test_gpu_midsize.py, which this change leaves as the
parent commit has it, one after the other in the same run on the same machine with an MI355X, the build done before: 16.6 s
for the 19 tests here against 19.5 s for the 26 there, most of both spent in the references."""
from math import comb

import numpy as np
import pytest

from graphlets_ref import ORBITS, check_identities
from oracle import oracle as O
from test_gpu_midsize import HUG, Graph, _set
from test_oracle_traversals import bits, ordered_items_np

pytestmark = pytest.mark.gpu

POISON = {"POISON": "0xFFFFFFFF"}
BTW_LISTS = (1, 65, 129)
DIST_LISTS = (257, 321)
N_MASTER = 321
BTW_GRID, BTW_WAVES, DIST_GRID, DIST_PER_GROUP = 2048, 4, 2048, 32        # the caps and the vertices a workgroup takes per turn
BALL = 3000
INFO_B = ("n_sources", "flags", "depth_max", "n_batches", "n_level_steps")
INFO_D = ("n_sources", "flags", "depth_max", "depth_min", "n_pairs", "sum_all", "n_batches", "n_level_steps")

# as printed by a run of this file with -s on an MI355X, default options unless named
RECORDED = {
    "G100": {"betweenness": {1: {"n_level_steps": 10, "ms": 3.90}, 65: {"n_level_steps": 24, "ms": 12.13}, 129: {"n_level_steps": 40, "ms": 22.04}},
             "distances": {(257, 1): {"n_level_steps": 38, "ms": 12.07}, (257, 4): {"n_level_steps": 14, "ms": 3.95},
                           (321, 1): {"n_level_steps": 46, "ms": 12.98}, (321, 4): {"n_level_steps": 15, "ms": 5.07}},
             "graphlets": {"cycle_items": 23326455, "roots": {"wave": 46299, "lds": 12165, "heavy": 785}, "ms": 48.73,
                           "ms_cycles": 6.34, "ms_triangles": 40.38, "ms_vertices": 0.59}},
    "GRID300": {"betweenness": {65: {"n_level_steps": 2150, "ms": 343.01}}, "distances": {(265, 4): {"n_level_steps": 1179, "ms": 275.93}}},
    "G50": {"graphlets": {"cycle_items": 11118059, "roots": {"wave": 23128, "lds": 6126, "heavy": 394}, "ms": 28.09, "ms_cycles": 2.97},
            "graphlets GRAPHLET_LDS=0": {"cycle_items": 11118059, "roots": {"wave": 0, "lds": 0, "heavy": 29648}, "ms": 76.41, "ms_cycles": 51.04}},
    "G50 vmask": {"graphlets": {"cycle_items": 6184532, "roots": {"wave": 9640, "lds": 3234, "heavy": 245}, "ms": 21.25, "ms_cycles": 1.59},
                  "graphlets GRAPHLET_LDS=0": {"cycle_items": 6184532, "roots": {"wave": 0, "lds": 0, "heavy": 13119}, "ms": 40.19, "ms_cycles": 21.58}},
}

# seconds of `pytest -m gpu` on one file, the build done before, on the same MI355X machine
WALL = {"tests/test_gpu_midsize_traversals.py": 16.64, "tests/test_gpu_midsize.py": 19.47}


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


# ---- the checks, one analysis each

def check_betweenness(g, src, key):
    want = g._once(("betweenness", key), lambda: O.betweenness(g.rowptr, g.col, src))
    bc, per, info = g.a.run_betweenness(src)
    print("%s betweenness %s: %s; oracle %.2f s" % (g.name, key, info, want["seconds"]))
    assert bc.dtype == np.float64 and len(bc) == g.nv
    diff = np.flatnonzero(bits(bc) != bits(want["bc"]))
    assert len(diff) == 0, (len(diff), diff[:5], bc[diff[:5]], want["bc"][diff[:5]])
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert per[name].dtype == want[name].dtype and np.array_equal(per[name], want[name]), name
    assert {k: info[k] for k in INFO_B} == {k: want[k] for k in INFO_B}
    assert info["ms"] >= 0.0
    return (bc, per, info), want


def check_distances(g, src, key, words):
    want = g._once(("distances", key), lambda: O.distances(g.rowptr, g.col, src))
    vert, per, pairs, info = g.a.run_distances(src)
    print("%s distances %s, %d words: %s; oracle %.2f s" % (g.name, key, words, info, want["seconds"]))
    assert vert["harmonic"].dtype == np.float64 and len(vert["harmonic"]) == g.nv
    diff = np.flatnonzero(bits(vert["harmonic"]) != bits(want["harmonic"]))
    assert len(diff) == 0, (len(diff), diff[:5], vert["harmonic"][diff[:5]], want["harmonic"][diff[:5]])
    for name in ("n_reached", "sum_dist", "ecc"):
        assert vert[name].dtype == want[name].dtype and np.array_equal(vert[name], want[name]), name
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert per[name].dtype == want["sources"][name].dtype and np.array_equal(per[name], want["sources"][name]), name
    assert pairs.dtype == np.int64 and np.array_equal(pairs, want["pairs"])
    assert {k: info[k] for k in INFO_D} == O.distances_info(want, words)
    assert info["ms"] >= 0.0
    return (vert, per, pairs, info), want


def check_graphlets(g):
    want = g._once("graphlets", lambda: O.graphlets(g.rowptr, g.col))
    items = g._once("items", lambda: ordered_items_np(g.rowptr, g.col))
    orbit, cyc, clq, info = g.a.run_graphlets()
    print("%s graphlets: %s; ordered items %d; oracle %.2f s" % (g.name, info, items, want["seconds"]))
    assert orbit.dtype == cyc.dtype == clq.dtype == np.uint64 and orbit.shape == (ORBITS, g.nv)
    assert np.array_equal(cyc, want["cycles4"]) and np.array_equal(clq, want["cliques4"])
    for o in range(ORBITS):
        assert np.array_equal(orbit[o], g.per_vertex(want["orbit"][o])), o
    assert info["total"] == want["total"] and info["flags"] == 0
    assert info["n_triangles"] == want["total"]["triangle"] and info["n_cliques4"] == want["total"]["clique4"]
    assert info["max_degree"] == int(want["orbit"][0].max()) and info["ms"] >= 0.0
    assert 0 <= info["cycle_items"] <= items, (info["cycle_items"], items)
    check_identities(orbit)
    total, _, _ = g.a.run_clique_census(3, 4)
    assert [int(x) for x in total] == [want["total"]["triangle"], want["total"]["clique4"]]
    return orbit, info, want


# ---- G100: betweenness and distances with both grids at their cap

@pytest.fixture(scope="module")
def g100(K):
    g = Graph(K, "G100", HUG["G100"][0], K.gen_hug_edges(*HUG["G100"]))
    deg = np.diff(g.rowptr)
    g.hub = int(deg.argmax())
    isolated = np.flatnonzero(deg == 0)
    leaves = np.flatnonzero(deg == 1)
    ends = leaves[deg[g.col[g.rowptr[leaves]]] == 1]                              # a leaf whose only neighbour is a leaf
    assert len(isolated) >= 2 and len(ends) >= 2
    g.isolated, g.pair = int(isolated[0]), (int(ends[0]), int(g.col[g.rowptr[ends[0]]]))
    rng = np.random.default_rng(5)
    master = rng.choice(rng.permutation(g.nv)[:200], size=N_MASTER)
    master[[0, 3, 10, 40, 41, 64, 70]] = [g.hub, g.isolated, g.pair[0], int(isolated[1]), g.isolated, g.hub, g.pair[1]]
    g.master = master.astype(np.int32)
    yield g
    g.close()


def test_g100_shape(g100):
    """What the docstring and the tests below rely on, from the oracle's CSR: the grids at their cap, the long rows, and the
    three kinds of source in every list of 65 entries or more."""
    g = g100
    deg = np.diff(g.rowptr)
    assert g.nv > BTW_GRID * BTW_WAVES and g.nv > DIST_GRID * DIST_PER_GROUP == 65536
    assert (len(g.eu), int(deg.max()), int((deg > 64).sum()), int((deg > 2048).sum()), int((deg == 0).sum())) == (1007422, 7059, 3571, 12, 1765)
    first = g.master[:65].tolist()
    assert first[0] == g.hub and g.isolated in first and g.pair[0] in first and len(set(g.master.tolist())) < len(g.master)
    want = g._once(("betweenness", 65), lambda: O.betweenness(g.rowptr, g.col, g.master[:65]))
    reached = dict(zip(want["source"].tolist(), want["n_reached"].tolist()))
    assert reached[g.isolated] == 1 and reached[g.pair[0]] == 2 and reached[g.hub] > g.nv // 2
    assert deg[g.hub] == deg.max()


@pytest.mark.parametrize("n", BTW_LISTS)
def test_g100_betweenness(g100, n):
    (bc, per, info), want = check_betweenness(g100, g100.master[:n], n)
    assert info["flags"] == 0 and info["n_batches"] == -(-n // 64) and bc.any()


@pytest.mark.parametrize("words", [1, 4])
@pytest.mark.parametrize("n", DIST_LISTS)
def test_g100_distances(g100, monkeypatch, n, words):
    _set(monkeypatch, {"DIST_WORDS": str(words)})
    (vert, per, pairs, info), want = check_distances(g100, g100.master[:n], n, words)
    assert info["n_batches"] == -(-n // (64 * words)) > 1 and int((want["ecc"] < 0).sum()) > 0


def test_g100_poisoned_memory_on_the_reused_context(g100, monkeypatch):
    _set(monkeypatch, POISON)
    check_betweenness(g100, g100.master[:65], 65)
    check_distances(g100, g100.master[:257], 257, 4)


def test_g100_per_source_integers_of_the_two_analyses_agree(g100):
    src = g100.master[:BTW_LISTS[-1]]
    (_, per_b, _), want = check_betweenness(g100, src, BTW_LISTS[-1])
    g100.a.distances_run(src)
    per_d = g100.a.distances_fetch_sources()
    for name in ("source", "n_reached", "sum_dist", "ecc"):
        assert per_d[name].dtype == per_b[name].dtype and np.array_equal(per_d[name], per_b[name]), name
        assert np.array_equal(per_d[name], want[name]), name


def test_g100_graphlets(g100):
    orbit, info, want = check_graphlets(g100)
    assert int(want["orbit"].max()) > 2 ** 32


# ---- GRID300: depth in the hundreds, path counts far past 2^53

SIDE = 300


def grid_edges(rows, cols):
    nv = rows * cols
    ids = np.random.default_rng(7).permutation(nv).reshape(rows, cols)
    uv = np.concatenate([np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1), np.stack([ids[:-1].ravel(), ids[1:].ravel()], 1)])
    return nv, ids, uv.astype(np.int64)


@pytest.fixture(scope="module")
def grid300(K):
    nv, ids, uv = grid_edges(SIDE, SIDE)
    g = Graph(K, "GRID300", nv, uv)
    corners = [int(ids[0, 0]), int(ids[0, -1]), int(ids[-1, 0]), int(ids[-1, -1])]
    others = np.random.default_rng(9).integers(0, nv, size=260).tolist()
    g.master = np.asarray(corners + [int(ids[SIDE // 2, SIDE // 2])] + others, dtype=np.int32)
    yield g
    g.close()


def test_grid300_betweenness_is_rounded_and_exact(grid300, K):
    g = grid300
    assert g.nv == 90000 > BTW_GRID * BTW_WAVES
    (bc, per, info), want = check_betweenness(g, g.master[:65], 65)
    assert want["ecc"][:5].tolist() == [2 * SIDE - 2] * 4 + [SIDE] and want["depth_max"] == 598
    assert want["flags"] == 1 == K._lib.KOMB_BETWEENNESS_ROUNDED == info["flags"]
    assert np.isfinite(want["bc"]).all() and comb(598, 299) > 2 ** 590


def test_grid300_distances(grid300, monkeypatch):
    g = grid300
    _set(monkeypatch, {"DIST_WORDS": "4"})
    assert g.nv > DIST_GRID * DIST_PER_GROUP
    (vert, per, pairs, info), want = check_distances(g, g.master, 265, 4)
    assert len(g.master) == 265 and info["n_batches"] == 2 and info["depth_max"] == 598 == len(want["pairs"]) - 1
    assert (want["n_reached"] == 265).all()


def test_strip_overflow_is_a_limit(K):
    """A 725 x 400 grid from a corner: the reference's limit code first, then the library's KOMB_ERR_LIMIT."""
    nv, ids, uv = grid_edges(400, 725)
    rowptr, col = O.simplify(nv, uv)
    corner = [int(ids[0, 0])]
    with pytest.raises(O.Limit):
        O.betweenness(rowptr, col, corner)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        with pytest.raises(K.KombError) as e:
            a.betweenness_run(corner)
        assert e.value.code == K._lib.KOMB_ERR_LIMIT


# ---- G50 and G50 under a vmask: the graphlet census

@pytest.fixture(scope="module")
def g50(K):
    g = Graph(K, "G50", HUG["G50"][0], K.gen_hug_edges(*HUG["G50"]))
    yield g
    g.close()


@pytest.fixture(scope="module")
def masked(K):
    g = Graph(K, "G50 vmask", HUG["G50"][0], K.gen_hug_edges(*HUG["G50"]), masked=True)
    yield g
    g.close()


@pytest.fixture(params=["g50", "masked"])
def gl(request):
    return request.getfixturevalue(request.param)


@pytest.mark.parametrize("opts", [{}, {"GRAPHLET_LDS": "0"}], ids=["default", "GRAPHLET_LDS=0"])
def test_g50_graphlets(gl, monkeypatch, opts):
    _set(monkeypatch, opts)
    orbit, info, want = check_graphlets(gl)
    if gl.name == "G50":
        assert info["max_degree"] == 4372 and comb(4372, 3) > 2 ** 32 and len(gl.eu) == 502700
        hub = int(want["orbit"][0].argmax())
        assert 2 ** 32 < int(want["orbit"][7, hub]) <= comb(4372, 3)             # (a real count above 32 bits, from many edges)
    else:                                                                       # (its largest count is 3 787 387 129, below 2^32)
        assert 0 < len(gl.inv) < gl.nv and 0 < len(gl.eu) < 502700
        assert not orbit[:, gl.vmask == 0].any() and int(want["orbit"].max()) > 2 ** 31


def test_g50_orbits_by_definition(g50):
    """200 vertices with an edge, no hub as a neighbour and at most BALL vertices within three hops, in the order of a seeded
    permutation: their orbit vectors straight from the definition against the library's columns (and the closed forms')."""
    g = g50
    want = g._once("graphlets", lambda: O.graphlets(g.rowptr, g.col))
    orbit = g.a.run_graphlets()[0]
    deg = np.diff(g.rowptr)
    hubs = np.argsort(deg, kind="stable")[-5:]
    beside = np.zeros(g.nv, dtype=bool)
    for h in hubs.tolist():
        beside[h] = True
        beside[g.col[g.rowptr[h]:g.rowptr[h + 1]]] = True
    picked, sets = [], 0
    for v in np.random.default_rng(1).permutation(np.flatnonzero(~beside & (deg >= 1))).tolist():
        vec, ball = O.orbits_by_definition(g.rowptr, g.col, v, BALL)
        if vec is None:
            continue
        assert ball <= BALL
        assert np.array_equal(vec, orbit[:, v]) and np.array_equal(vec, want["orbit"][:, v]), v
        picked.append(v)
        sets = max(sets, int(vec[1:].sum()))
        if len(picked) == 200:
            break
    print("G50 orbits by definition: %d vertices, at most %d sets at one" % (len(picked), sets))
    assert len(picked) >= 150 and sets > 1000
