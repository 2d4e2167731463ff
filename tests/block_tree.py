"""A graph whose biconnected components are known by construction, for the tests of komb_biconnected_run and of its reference:
a tree of blocks.  Block i is a ring of s_i vertices with up to s_i // 3 random chords inside it (a ring is 2-connected and a
chord keeps it so); every block but the first is hung on one random vertex of the blocks before it, which is one vertex of
its ring -- so two blocks share at most that vertex, the blocks of the graph are exactly these, the articulation points are
the attachment vertices, and there is no bridge and one 2-edge-connected component.  The sizes are heavy-tailed: many rings
of 3 .. 30 vertices, fewer of 100 .. 5 000 (log-uniform), and a few giants.  Ids go through a fixed random permutation."""
import numpy as np

FULL = dict(n_small=6000, n_mid=240, giants=(61000, 64000, 70000))      # about 590 000 vertices, 780 000 edges
REDUCED = dict(n_small=300, n_mid=12, giants=(900, 1000, 1100))


def block_tree(n_small, n_mid, giants, seed=11):
    """{"nv", "uv": int64[m, 2] (no loop, no duplicate), "n_edges", "n_verts": int64[B] per block in the order of construction,
    "attach": int64[B] (the vertex block i hangs on, -1 for the first), "n_blocks": int64[nv] (the blocks through every vertex)}."""
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([rng.integers(3, 31, n_small), (100 * 50 ** rng.random(n_mid)).astype(np.int64), np.asarray(giants, np.int64)])
    sizes = sizes[rng.permutation(len(sizes))]
    nv = 0
    parts, n_edges, attach = [], [], []
    for i, s in enumerate(sizes.tolist()):
        at = int(rng.integers(0, nv)) if i else -1
        ring = np.arange(nv - (1 if i else 0), nv - (1 if i else 0) + s)
        if i:
            ring[0] = at
        nv += s - (1 if i else 0)
        edges = [np.stack([ring, np.roll(ring, -1)], 1)]
        if s >= 4:
            a = rng.integers(0, s, s // 3)
            b = (a + rng.integers(2, s - 1, s // 3)) % s                  # 2 .. s - 2 steps on: no ring edge, no loop
            chords = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
            edges.append(ring[chords])
        edges = np.concatenate(edges)
        parts.append(edges)
        n_edges.append(len(edges))
        attach.append(at)
    ids = np.random.default_rng(seed + 1).permutation(nv)
    attach = np.asarray(attach, np.int64)
    n_blocks = np.ones(nv, np.int64)
    np.add.at(n_blocks, attach[1:], 1)
    out_blocks = np.zeros(nv, np.int64)
    out_blocks[ids] = n_blocks
    return {"nv": nv, "uv": ids[np.concatenate(parts)].astype(np.int64), "n_edges": np.asarray(n_edges, np.int64), "n_verts": sizes.astype(np.int64),
            "attach": np.concatenate([[-1], ids[attach[1:]]]), "n_blocks": out_blocks}


def closed_form(t):
    """What komb_biconnected_run reports at k = 2 on block_tree()'s graph, without any search: the info fields that the
    construction fixes (depth is not one), the sorted block sizes, the articulation points and n_blocks[]."""
    cut = np.unique(t["attach"][1:])
    return {"info": {"n_member_edges": int(t["n_edges"].sum()), "n_member_vertices": t["nv"], "n_blocks": len(t["n_edges"]), "n_bridges": 0,
                     "n_articulation": len(cut), "largest_block": int(t["n_edges"].max()), "n_ecc": 1, "largest_ecc": t["nv"]},
            "n_edges": np.sort(t["n_edges"]), "n_verts": np.sort(t["n_verts"]), "pairs": sorted_pairs(t["n_edges"], t["n_verts"]),
            "articulation": cut, "n_blocks": t["n_blocks"]}


def sorted_pairs(n_edges, n_verts):
    """The blocks as (edges, vertices) rows in ascending order: what compares two lists of blocks whatever their order."""
    rows = np.stack([np.asarray(n_edges, np.int64), np.asarray(n_verts, np.int64)], 1)
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]
