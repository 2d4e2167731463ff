"""CPU tests of tests/biconnected_ref.py, the reference the GPU tests compare komb_biconnected_run with: against networkx
(biconnected_component_edges, articulation_points, bridges) and, for the 2-edge-connected components, scipy's
connected_components after deleting networkx's bridges, on random graphs of 2..18 vertices; and the closed forms."""
import networkx as nx
import numpy as np
import pytest

import biconnected_ref as R
import components_ref as CR


def _canon(nv, pairs):
    """Simple canonical edge list (eu < ev, sorted) of raw pairs."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    p = p[p[:, 0] != p[:, 1]]
    p = np.unique(np.sort(p, axis=1), axis=0)
    return p[:, 0].copy(), p[:, 1].copy()


def _against_networkx(nv, eu, ev, tr, k):
    res = R.biconnected(nv, eu, ev, tr, k)
    sel = tr >= k
    index = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(eu, ev))}
    G = nx.Graph()
    G.add_edges_from(zip(eu[sel].tolist(), ev[sel].tolist()))
    block, size = np.full(len(tr), -1, np.int64), np.zeros(len(tr), np.int64)
    n_blocks = np.zeros(nv, np.int64)
    blocks = []
    for comp in nx.biconnected_component_edges(G):
        ids = sorted(index[(min(a, b), max(a, b))] for a, b in comp)
        block[ids], size[ids] = ids[0], len(ids)
        vs = {a for a, _ in comp} | {b for _, b in comp}
        n_blocks[list(vs)] += 1
        blocks.append((ids[0], len(ids), len(vs)))
    blocks.sort()
    assert np.array_equal(res["block"], block) and np.array_equal(res["size"], size)
    assert np.array_equal(res["n_blocks"], n_blocks)
    assert sorted(np.flatnonzero(res["n_blocks"] >= 2).tolist()) == sorted(nx.articulation_points(G))
    bridges = sorted((min(a, b), max(a, b)) for a, b in nx.bridges(G))
    got = np.flatnonzero(res["size"] == 1)
    assert sorted(zip(eu[got].tolist(), ev[got].tolist())) == bridges
    got_blocks = list(zip(*(res["blocks"][x].tolist() for x in ("rep", "n_edges", "n_verts"))))
    assert got_blocks == blocks
    member = np.zeros(nv, bool)
    member[eu[sel]] = member[ev[sel]] = True
    H = G.copy()
    H.remove_edges_from(bridges)
    he = np.asarray(list(H.edges()), np.int64).reshape(-1, 2)
    ecc = CR.min_labels(nv, he[:, 0], he[:, 1], member)
    assert np.array_equal(res["ecc_label"], ecc) and np.array_equal(res["ecc_size"], CR.sizes(ecc))
    info = res["info"]
    assert info["n_member_edges"] == int(sel.sum()) and info["n_member_vertices"] == int(member.sum())
    assert info["n_blocks"] == len(blocks) and info["n_bridges"] == len(bridges)
    assert info["n_articulation"] == len(list(nx.articulation_points(G)))
    assert info["largest_block"] == max((b[1] for b in blocks), default=0)
    assert info["n_ecc"] == nx.number_connected_components(H) if sel.any() else info["n_ecc"] == 0
    assert info["largest_ecc"] == max((len(c) for c in nx.connected_components(H)), default=0)
    depth = 0
    for c in nx.connected_components(G):
        depth = max(depth, 1 + max(nx.single_source_shortest_path_length(G, min(c)).values()))
    assert info["depth"] == depth
    return res


@pytest.mark.parametrize("density", [0.08, 0.15, 0.3, 0.6])
def test_random_graphs_against_networkx(density):
    rng = np.random.default_rng(int(density * 100))
    for _ in range(100):
        nv = int(rng.integers(2, 19))
        n_raw = max(1, int(density * nv * (nv - 1) / 2 + rng.integers(0, 3)))
        eu, ev = _canon(nv, rng.integers(0, nv, (n_raw, 2)))
        if len(eu) == 0:
            continue
        tr = rng.integers(2, 5, len(eu))
        for k in (2, 3, 4, 5):
            _against_networkx(nv, eu, ev, tr, k)


def _run(nv, pairs, perm=None):
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if perm is not None:
        p = np.asarray(perm)[p]
    eu, ev = _canon(nv, p)
    return eu, ev, R.biconnected(nv, eu, ev, np.full(len(eu), 2), 2)


def _info(res):
    i = res["info"]
    return i["n_blocks"], i["n_articulation"], i["n_bridges"]


def test_closed_forms():
    perm = np.random.default_rng(5).permutation(64)
    for p in (None, perm):
        assert _info(_run(64, [[i, i + 1] for i in range(4)], p)[2]) == (4, 3, 4)                    # a path of 5
        for n in (5, 6):                                                                              # cycles
            res = _run(64, [[i, (i + 1) % n] for i in range(n)], p)[2]
            assert _info(res) == (1, 0, 0) and res["info"]["largest_block"] == n
        assert _info(_run(64, [[0, 1], [0, 2], [1, 2]], p)[2]) == (1, 0, 0)                           # a triangle
        res = _run(64, [[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]], p)[2]                        # two triangles, one vertex
        assert _info(res) == (2, 1, 0) and res["info"]["n_ecc"] == 1
        assert _info(_run(64, [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]], p)[2]) == (1, 0, 0)           # two triangles, one edge
        theta = [[0, 1], [1, 2], [2, 3], [0, 4], [4, 3], [0, 5], [5, 6], [6, 3]]
        assert _info(_run(64, theta, p)[2]) == (1, 0, 0)
    # a star: every edge a bridge, the hub in all of them
    eu, ev, res = _run(3001, [[0, i] for i in range(1, 3001)])
    assert _info(res) == (3000, 1, 3000) and res["n_blocks"][0] == 3000 and res["info"]["n_ecc"] == 3001
    assert res["info"]["depth"] == 2
    # a cactus of 50 triangles in a chain
    eu, ev, res = _run(101, [e for i in range(50) for e in ([2 * i, 2 * i + 1], [2 * i, 2 * i + 2], [2 * i + 1, 2 * i + 2])])
    assert _info(res) == (50, 49, 0) and np.all(res["blocks"]["n_verts"] == 3) and res["info"]["largest_ecc"] == 101
    # a grid: one block
    g = np.arange(900).reshape(30, 30)
    eu, ev, res = _run(900, np.concatenate([np.stack([g[:, :-1].ravel(), g[:, 1:].ravel()], 1), np.stack([g[:-1].ravel(), g[1:].ravel()], 1)]))
    assert _info(res) == (1, 0, 0) and res["info"]["largest_block"] == 2 * 30 * 29 and res["info"]["depth"] == 59
    # a long path beside a K5
    k5 = [[20000 + a, 20000 + b] for a in range(5) for b in range(a + 1, 5)]
    eu, ev, res = _run(20005, [[i, i + 1] for i in range(19999)] + k5)
    assert _info(res) == (20000, 19998, 19999) and res["info"]["depth"] == 20000 and res["info"]["largest_block"] == 10


def test_thresholds_members_and_invariants():
    # a triangle of trussness 3 with a pendant path of trussness 2, an isolated vertex
    eu, ev = np.asarray([0, 0, 1, 2, 3]), np.asarray([1, 2, 2, 3, 4])
    tr = np.asarray([3, 3, 3, 2, 2])
    res = R.biconnected(6, eu, ev, tr, 2)
    assert res["block"].tolist() == [0, 0, 0, 3, 4] and res["size"].tolist() == [3, 3, 3, 1, 1]
    assert res["n_blocks"].tolist() == [1, 1, 2, 2, 1, 0]
    assert res["ecc_label"].tolist() == [0, 0, 0, 3, 4, -1] and res["ecc_size"].tolist() == [3, 3, 3, 1, 1, 0]
    assert R.summary(res) == (5, 5, 3, 2, 2, 3, 3, 3, 4)
    res = R.biconnected(6, eu, ev, tr, 3)
    assert res["block"].tolist() == [0, 0, 0, -1, -1] and res["n_blocks"].tolist() == [1, 1, 1, 0, 0, 0]
    assert R.summary(res) == (3, 3, 1, 0, 0, 3, 1, 3, 2)
    res = R.biconnected(6, eu, ev, tr, 4)
    assert res["block"].tolist() == [-1] * 5 and R.summary(res) == (0,) * 9 and len(res["blocks"]["rep"]) == 0
    # the block-cut structure is a forest: sum over cut vertices of n_blocks = blocks + cut vertices - components
    rng = np.random.default_rng(8)
    for _ in range(50):
        nv = int(rng.integers(5, 60))
        eu, ev = _canon(nv, rng.integers(0, nv, (int(nv * 1.2), 2)))
        res = R.biconnected(nv, eu, ev, np.full(len(eu), 2), 2)
        nb, info = res["n_blocks"], res["info"]
        n_comp = int((CR.truss_components(nv, eu, ev, np.full(len(eu), 2), 2) == np.arange(nv)).sum())
        assert int(nb[nb >= 2].sum()) == info["n_blocks"] + info["n_articulation"] - n_comp
        assert int(res["blocks"]["n_edges"].sum()) == info["n_member_edges"]
        assert int(res["blocks"]["n_verts"].sum()) == int(nb.sum())
        assert np.array_equal(res["block"][res["blocks"]["rep"]], res["blocks"]["rep"])


def test_block_tree_closed_form():
    """tests/block_tree.py at a reduced size: what the construction fixes against the Hopcroft-Tarjan reference."""
    import block_tree as BT
    t = BT.block_tree(**BT.REDUCED)
    want = BT.closed_form(t)
    assert len(t["n_edges"]) == 315 and t["nv"] == int(t["n_verts"].sum()) - 314
    assert len(np.unique(np.sort(t["uv"], axis=1), axis=0)) == len(t["uv"]) and (t["uv"][:, 0] != t["uv"][:, 1]).all()
    assert (t["n_edges"] >= t["n_verts"]).all() and (t["n_edges"] <= t["n_verts"] + t["n_verts"] // 3).all()
    eu, ev = _canon(t["nv"], t["uv"])
    assert len(eu) == len(t["uv"])
    res = R.biconnected(t["nv"], eu, ev, np.full(len(eu), 2), 2)
    for name, value in want["info"].items():
        assert res["info"][name] == value, name
    assert np.array_equal(np.sort(res["blocks"]["n_edges"]), want["n_edges"]) and np.array_equal(np.sort(res["blocks"]["n_verts"]), want["n_verts"])
    assert np.array_equal(BT.sorted_pairs(res["blocks"]["n_edges"], res["blocks"]["n_verts"]), want["pairs"])
    assert np.array_equal(res["n_blocks"], want["n_blocks"])
    assert np.array_equal(np.flatnonzero(res["n_blocks"] >= 2), want["articulation"])
    assert (res["size"] > 1).all() and (res["ecc_label"] == 0).all()
    # every block of the construction is one class of the reference: the edges of block i carry one label
    canon = {(int(a), int(b)): j for j, (a, b) in enumerate(zip(eu, ev))}
    at = 0
    for n in t["n_edges"].tolist():
        rows = np.sort(t["uv"][at:at + n], axis=1)
        labels = {int(res["block"][canon[(int(a), int(b))]]) for a, b in rows}
        assert len(labels) == 1 and int(res["size"][labels.pop()]) == n
        at += n
