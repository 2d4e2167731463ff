"""Replicas of a small tile: the disjoint union of many copies of a graph that the plain-Python references solve in
milliseconds, under an id map that is strictly increasing inside each copy.  Every output of the analyses built on the k-truss
result is local to a connected component up to "smallest id / smallest canonical index of the class" labels and to counters
that are sums or maxima, so the expected value of EVERY item of a union of any size follows from the tile's own result:
  - canonical edge order, triangle order and clique list order restricted to one copy are the tile's own order;
  - a local label l becomes g_i[l], g_i the ascending global positions of copy i's items;
  - a counter is copies x the tile's, or its maximum.
No GPU, no product code.  tests/test_replica_ref.py proves all of this on the references themselves."""
import numpy as np

import nucleus_ref as N

LAYOUTS = ("blocked", "interleaved")


def as_tile(nv, edges):
    """(nv, canonical edges int64[m, 2]) of any simple edge list: what build() takes as a tile."""
    e = np.asarray(N.canonical(edges), np.int64).reshape(-1, 2)
    assert not len(e) or int(e.max()) < nv
    return nv, e


def tile():
    """(nv, canonical edges int64[m, 2]): nucleus_ref.hand_graph() on 0..14, clique_union(60, 45, 2, 8, 3) on 15..74, a path
    of 10 on 75..84, a ring of 7 on 85..91, vertex 92 alone, pendant edges from vertex 3 to 93..96.  97 vertices, 564 edges,
    1559 triangles, 2073 4-cliques; 17 blocks, 14 bridges and 10 articulation points at k = 2; theta 0..5; trussness 2..8."""
    nv, edges = N.hand_graph()
    edges = list(edges) + [(u + 15, v + 15) for u, v in N.clique_union(60, 45, 2, 8, 3)]
    edges += [(75 + i, 76 + i) for i in range(9)]
    edges += [(85 + i, 85 + (i + 1) % 7) for i in range(7)]
    edges += [(3, 93 + i) for i in range(4)]
    return as_tile(97, edges)


_FILLERS = {}
_TILE_RESULTS = {}                                   # (what, tile) -> the reference's result: computed once per process, never changed


def filler(name):
    """The filler tiles: "K1" (an isolated vertex), "K2", "K3" (one triangle of theta 0), "K4" (6 edges of trussness 4: with the
    K5's 10 it lands a count of member edges at k = 4 on any number), "K5" (10 triangles of key0 = theta = 2, 5 four-cliques)
    and "K9" (36 edges of trussness 9: one copy behind everything else is the only place of the largest trussness)."""
    if name not in _FILLERS:
        n = {"K1": 1, "K2": 2, "K3": 3, "K4": 4, "K5": 5, "K9": 9}[name]
        _FILLERS[name] = as_tile(n, N.clique(range(n)))
    return _FILLERS[name]


class Union:
    """nv, pairs (the raw pairs, int64[m, 2], in no particular order) and, per part p, maps[p] (int64[copies, tile nv]: a
    copy's local vertex -> its global id) and tiles[p] (the part's (nv, edges))."""

    def __init__(self, nv, pairs, maps, tiles):
        self.nv, self.pairs, self.maps, self.tiles = nv, pairs, maps, tiles

    def copy_of_vertex(self, p):
        """int64[nv]: the copy of part p a vertex belongs to, -1 for the vertices of other parts."""
        out = np.full(self.nv, -1, np.int64)
        m = self.maps[p]
        if m.size:
            out[m] = np.arange(len(m))[:, None]
        return out

    def canonical(self):
        """(eu, ev) of the union as a k-truss result lists them: sorted by (eu, ev)."""
        key = np.sort(self.pairs[:, 0] * self.nv + self.pairs[:, 1])
        return key // self.nv, key % self.nv


def build(parts, layout):
    """parts = [((nv, canonical edges), copies), ...] -> Union.  Part p takes the id range after part p - 1's; inside it,
    "blocked" gives copy i the contiguous range base + i nv_t + v, "interleaved" gives local vertex v of copy i the id
    base + v copies + i.  Both are increasing inside a copy."""
    assert layout in LAYOUTS
    base, maps, pairs, tiles = 0, [], [], []
    for (nv_t, edges), c in parts:
        i, v = np.arange(c, dtype=np.int64)[:, None], np.arange(nv_t, dtype=np.int64)[None, :]
        m = base + (i * nv_t + v if layout == "blocked" else v * c + i)
        maps.append(m)
        tiles.append((nv_t, edges))
        if len(edges) and c:
            pairs.append(np.stack([m[:, edges[:, 0]].reshape(-1), m[:, edges[:, 1]].reshape(-1)], 1))
        base += c * nv_t
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    return Union(base, pairs, maps, tiles)


def positions(copy_of_item):
    """The g_i of one part as one matrix int64[copies, n]: row i holds, ascending, the global positions of the items whose
    entry is i; entries of -1 (the items of other parts) are left out.  Every copy must own the same number of items."""
    copy_of_item = np.asarray(copy_of_item, np.int64)
    idx = np.flatnonzero(copy_of_item >= 0)
    if not len(idx):
        return np.zeros((0, 0), np.int64)
    c = int(copy_of_item.max()) + 1
    counts = np.bincount(copy_of_item[idx], minlength=c)
    assert (counts == counts[0]).all(), "every copy owns the same number of items"
    return idx[np.argsort(copy_of_item[idx], kind="stable")].reshape(c, int(counts[0]))


def map_label(local_label, g):
    """A tile's label array (indices into the tile's own items, -1: none) as the labels of every copy: int64 of g's shape
    with out[i, j] = g[i, local_label[j]], -1 where the local label is -1.  g: int64[copies, n_labelled_items]."""
    l = np.asarray(local_label, np.int64)
    assert len(l) == 0 or (int(l.min()) >= -1 and int(l.max()) < g.shape[1])
    return np.where(l[None, :] >= 0, g[:, np.maximum(l, 0)], -1)


def spread(n_items, pieces, fill=None):
    """The expected global array: pieces = [(g, values), ...] with g int64[copies, n] and values of shape (n,) (the tile's,
    the same in every copy) or (copies, n) (mapped labels).  Without `fill` every item must be covered exactly once."""
    out = np.zeros(n_items, np.int64) if fill is None else np.full(n_items, fill, np.int64)
    seen = np.zeros(n_items, np.int64)
    for g, values in pieces:
        if g.size:
            out[g] = np.broadcast_to(np.asarray(values, np.int64), g.shape)
            np.add.at(seen, g.reshape(-1), 1)
    assert int(seen.max(initial=0)) <= 1, "an item belongs to one copy"
    assert fill is not None or int(seen.min(initial=1)) == 1, "every item belongs to a copy"
    return out


def replicate_forest(n_items, pieces):
    """The forest of a union in hierarchy_ref's layout (nodes in (k, rep) order, "node" per item), from pieces =
    [(g, tile forest), ...]: g int64[copies, tile items] over the items the forest is about (vertices, edges or triangles).
    A node keeps its level, size and shell; its representative and its parent's go through the copy's g."""
    cols = {x: [] for x in ("k", "rep", "parent", "size", "shell")}
    item_at, item_node, base = [], [], 0
    for g, h in pieces:
        c, n = len(g), len(h["k"])
        hk, hrep, hpar = (np.asarray(h[x], np.int64) for x in ("k", "rep", "parent"))
        off = base + np.arange(c, dtype=np.int64)[:, None] * n          # the copy's first node in the unsorted list
        cols["k"].append(np.tile(hk, c))
        cols["rep"].append(g[:, hrep].reshape(-1) if n else np.zeros(0, np.int64))
        cols["parent"].append(np.where(hpar[None, :] >= 0, off + hpar[None, :], -1).reshape(-1))
        cols["size"].append(np.tile(np.asarray(h["size"], np.int64), c))
        cols["shell"].append(np.tile(np.asarray(h["shell"], np.int64), c))
        tn = np.asarray(h["node"], np.int64)
        item_at.append(g.reshape(-1))
        item_node.append(np.where(tn[None, :] >= 0, off + tn[None, :], -1).reshape(-1))
        base += c * n
    cols = {x: np.concatenate(v) if v else np.zeros(0, np.int64) for x, v in cols.items()}
    order = np.lexsort((cols["rep"], cols["k"]))
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    out = {x: v[order] for x, v in cols.items()}
    out["parent"] = np.where(out["parent"] >= 0, inv[np.maximum(out["parent"], 0)], -1)
    node = np.full(n_items, -1, np.int64)
    if item_at:
        at, nd = np.concatenate(item_at), np.concatenate(item_node)
        node[at] = np.where(nd >= 0, inv[np.maximum(nd, 0)], -1)
    out["node"] = node
    return out


def forest_by_key(h):
    """A forest with its node numbers taken out: the nodes sorted by (level, representative) as rows (k, rep, parent's k,
    parent's rep, size, shell), -1 twice for a root, and per item the (k, rep) of its node, -1 twice without one."""
    k, rep, parent = (np.asarray(h[x], np.int64) for x in ("k", "rep", "parent"))
    has = parent >= 0
    pk = np.where(has, k[np.maximum(parent, 0)], -1) if len(k) else k
    prep = np.where(has, rep[np.maximum(parent, 0)], -1) if len(k) else k
    rows = np.stack([k, rep, pk, prep, np.asarray(h["size"], np.int64), np.asarray(h["shell"], np.int64)], 1)
    rows = rows[np.lexsort((rep, k))]
    node = np.asarray(h["node"], np.int64)
    if len(k):
        items = np.stack([np.where(node >= 0, k[np.maximum(node, 0)], -1), np.where(node >= 0, rep[np.maximum(node, 0)], -1)], 1)
    else:
        items = np.full((len(node), 2), -1, np.int64)
    return rows, items


def same_forest(got, want):
    """True when two forests (hierarchy_ref's layout with "node") are the same: nodes are matched by (level, representative),
    not by node number; parent, size, shell and every item's node are compared through that key."""
    if int(np.asarray(got["node"]).max(initial=-1)) >= len(got["k"]) or int(np.asarray(got["parent"]).max(initial=-1)) >= len(got["k"]):
        return False
    (gr, gi), (wr, wi) = forest_by_key(got), forest_by_key(want)
    keys = wr[:, 0] * (int(wr[:, 1].max(initial=0)) + 1) + wr[:, 1]
    assert len(np.unique(keys)) == len(keys), "(level, representative) names a node"
    return bool(np.array_equal(gr, wr) and np.array_equal(gi, wi))


# ---- a union with its canonical edge list, and the expected results of the analyses on it from the tiles' own

class Frame:
    """A Union and the canonical edges (eu, ev) of its k-truss result (the library's own list, or Union.canonical()):
    gv[p] / ge[p] are the positions matrices of part p's vertices / edges.  The constructor asserts that the list's
    restriction to each copy is the tile's canonical list under the copy's map."""

    def __init__(self, union, eu, ev):
        self.u, self.nv = union, union.nv
        self.eu, self.ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
        self.m = len(self.eu)
        assert self.m == len(union.pairs)
        self.gv = union.maps
        self.ge = []
        for p, (nv_t, e) in enumerate(union.tiles):
            g = positions(union.copy_of_vertex(p)[self.eu]) if len(e) and len(self.gv[p]) else np.zeros((len(self.gv[p]), len(e)), np.int64)
            assert g.shape == (len(self.gv[p]), len(e))
            assert np.array_equal(self.eu[g], self.gv[p][:, e[:, 0]]) and np.array_equal(self.ev[g], self.gv[p][:, e[:, 1]])
            self.ge.append(g)

    def parts(self):
        return range(len(self.u.tiles))

    def copies(self, p):
        return len(self.gv[p])

    def tile_result(self, p, what, fn):
        """fn(nv_t, teu, tev) of part p's tile, computed once per `what` and tile in the whole process."""
        nv_t, e = self.u.tiles[p]
        key = (what, nv_t, e.tobytes())
        if key not in _TILE_RESULTS:
            _TILE_RESULTS[key] = fn(nv_t, e[:, 0].copy(), e[:, 1].copy())
        return _TILE_RESULTS[key]

    def tile_cached(self, p, what):
        """The result tile_result(p, what, ...) has computed before (an expectation of this module made it)."""
        nv_t, e = self.u.tiles[p]
        key = (what, nv_t, e.tobytes())
        assert key in _TILE_RESULTS, "no %r of part %d's tile has been computed yet" % (what, p)
        return _TILE_RESULTS[key]

    def per_vertex(self, per_part, fill=None):
        return spread(self.nv, [(self.gv[p], per_part[p]) for p in self.parts()], fill)

    def per_edge(self, per_part):
        return spread(self.m, [(self.ge[p], per_part[p]) for p in self.parts()])

    def total(self, per_part):
        return sum(self.copies(p) * int(per_part[p]) for p in self.parts())

    def largest(self, per_part, empty=0):
        return max([int(per_part[p]) for p in self.parts() if self.copies(p)], default=empty)


def tile_trussness(nv_t, teu, tev):
    import max_clique_ref as MC
    return np.asarray(MC.trussness(nv_t, teu, tev), np.int64)


def trussness(f):
    return f.per_edge([f.tile_result(p, "truss", tile_trussness) for p in f.parts()])


def biconnected(f, k):
    """What biconnected_ref.biconnected(nv, eu, ev, tr, k) gives on the union, from the tiles' results."""
    import biconnected_ref as B
    def one(nv_t, teu, tev):
        return B.biconnected(nv_t, teu, tev, tile_trussness(nv_t, teu, tev), k)
    t = [f.tile_result(p, ("biconnected", k), one) for p in f.parts()]
    out = {"block": f.per_edge([map_label(t[p]["block"], f.ge[p]) for p in f.parts()]),
           "size": f.per_edge([t[p]["size"] for p in f.parts()]),
           "n_blocks": f.per_vertex([t[p]["n_blocks"] for p in f.parts()]),
           "ecc_label": f.per_vertex([map_label(t[p]["ecc_label"], f.gv[p]) for p in f.parts()]),
           "ecc_size": f.per_vertex([t[p]["ecc_size"] for p in f.parts()])}
    rep = np.concatenate([map_label(t[p]["blocks"]["rep"], f.ge[p]).reshape(-1) for p in f.parts()])
    order = np.argsort(rep)
    out["blocks"] = {"rep": rep[order]}
    for x in ("n_edges", "n_verts"):
        out["blocks"][x] = np.concatenate([np.tile(t[p]["blocks"][x], f.copies(p)) for p in f.parts()])[order]
    info = {}
    for x in B.INFO_FIELDS:
        vals = [t[p]["info"][x] for p in f.parts()]
        info[x] = f.largest(vals) if x in ("largest_block", "largest_ecc", "depth") else f.total(vals)
    out["info"] = info
    return out


def structural(f, eps_num, eps_den, mu):
    """What structural_ref.clusters gives on the union (supports included: structural_ref.supports of the tile)."""
    import structural_ref as S
    def one(nv_t, teu, tev):
        return S.clusters(nv_t, teu, tev, S.supports(nv_t, teu, tev), eps_num, eps_den, mu)
    t = [f.tile_result(p, ("structural", eps_num, eps_den, mu), one) for p in f.parts()]
    out = {"similar": f.per_edge([t[p]["similar"] for p in f.parts()]),
           "label": f.per_vertex([map_label(t[p]["label"], f.gv[p]) for p in f.parts()])}
    for x in ("sim_deg", "size", "role"):
        out[x] = f.per_vertex([t[p][x] for p in f.parts()])
    info = {"eps_num": eps_num, "eps_den": eps_den, "mu": mu}
    for x in ("n_similar_edges", "n_cores", "n_borders", "n_hubs", "n_outliers", "n_clusters"):
        info[x] = f.total([t[p]["info"][x] for p in f.parts()])
    info["largest"] = f.largest([t[p]["info"]["largest"] for p in f.parts()])
    out["info"] = info
    return out


def supports(f):
    import structural_ref as S
    return f.per_edge([f.tile_result(p, "support", S.supports) for p in f.parts()])


class Triangles:
    """The union's triangle list in triangle order (ascending (a, b, c)) from the tiles' own, and gt[p], the positions matrices
    of part p's triangles."""

    def __init__(self, f):
        self.f = f
        self.dec = [f.tile_result(p, "nucleus", N.decompose) for p in f.parts()]
        cols = [np.concatenate([f.gv[p][:, np.asarray(self.dec[p][x], np.int64)].reshape(-1) for p in f.parts()]) for x in "abc"]
        order = np.lexsort((cols[2], cols[1], cols[0]))
        self.a, self.b, self.c = (x[order] for x in cols)
        self.n = len(order)
        pos = np.empty(self.n, np.int64)
        pos[order] = np.arange(self.n)
        self.gt, at = [], 0
        for p in f.parts():
            n = f.copies(p) * len(self.dec[p]["a"])
            self.gt.append(pos[at:at + n].reshape(f.copies(p), len(self.dec[p]["a"])))
            at += n
        for g in self.gt:                                       # increasing inside a copy: the tile's own order
            assert g.shape[1] < 2 or (np.diff(g, axis=1) > 0).all()

    def per_triangle(self, per_part):
        return spread(self.n, [(self.gt[p], per_part[p]) for p in self.f.parts()])


def nucleus(f, tri=None):
    """What nucleus_ref.decompose gives on the union (without "cliques"; "levels" is the union of the tiles' levels)."""
    tri = tri or Triangles(f)
    d = tri.dec
    out = {"a": tri.a, "b": tri.b, "c": tri.c}
    for x in ("key0", "theta"):
        out[x] = tri.per_triangle([d[p][x] for p in f.parts()])
    out["edge_theta"] = f.per_edge([d[p]["edge_theta"] for p in f.parts()])
    out["vertex_theta"] = f.per_vertex([d[p]["vertex_theta"] for p in f.parts()])
    out["levels"] = sorted({k for p in f.parts() if f.copies(p) for k in d[p]["levels"]})
    out["info"] = {"n_triangles": tri.n, "n_cliques4": f.total([d[p]["info"]["n_cliques4"] for p in f.parts()]),
                   "theta_max": f.largest([d[p]["info"]["theta_max"] for p in f.parts()], -1), "n_levels": len(out["levels"])}
    return out


# ---- the three nesting forests

def _forest_of(h, node):
    return {**{x: h[x] for x in ("k", "rep", "parent", "size", "shell")}, "node": node}


def truss_hierarchy(f):
    """hierarchy_ref.truss_hierarchy of the union: the items are vertices."""
    import hierarchy_ref as H
    t = [f.tile_result(p, "truss_hierarchy", lambda nv_t, teu, tev: H.truss_hierarchy(nv_t, teu, tev, tile_trussness(nv_t, teu, tev)))
         for p in f.parts()]
    return replicate_forest(f.nv, [(f.gv[p], t[p]) for p in f.parts()])


def community_hierarchy(f):
    """community_hierarchy_ref.community_hierarchy of the union: the items are canonical edges."""
    import community_hierarchy_ref as CH
    t = [f.tile_result(p, "community_hierarchy",
                       lambda nv_t, teu, tev: CH.community_hierarchy(nv_t, teu, tev, tile_trussness(nv_t, teu, tev))) for p in f.parts()]
    return replicate_forest(f.m, [(f.ge[p], t[p]) for p in f.parts()])


def nucleus_hierarchy(f, tri=None):
    """nucleus_hierarchy_ref.forest of the union: the items are triangles."""
    import nucleus_hierarchy_ref as NH
    tri = tri or Triangles(f)
    t = [f.tile_result(p, "nucleus_hierarchy", lambda nv_t, teu, tev, p=p: NH.forest(tri.dec[p]["theta"], tri.dec[p]["cliques"]))
         for p in f.parts()]
    return replicate_forest(tri.n, [(tri.gt[p], t[p]) for p in f.parts()])


# ---- the clique searches

def _sorted_tuples(rows):
    """The order that sorts ascending tuples of different lengths lexicographically: rows int64[n, width], padded with -1."""
    return np.lexsort(tuple(rows[:, j] for j in range(rows.shape[1] - 1, -1, -1))) if rows.shape[1] else np.arange(len(rows))


class CliqueList:
    """A sorted list of cliques of the union from the tiles' own sorted lists: rows (int64[n, width], ascending tuples padded
    with -1, in lexicographic order), length, and gc[p], the positions matrices of part p's cliques in it."""

    def __init__(self, f, per_part):
        self.f = f
        width = max([len(c) for cl in per_part for c in cl], default=0)
        blocks = []
        for p in f.parts():
            local = np.full((len(per_part[p]), width), -1, np.int64)
            for i, c in enumerate(per_part[p]):
                local[i, :len(c)] = c
            mapped = np.where(local[None, :, :] >= 0, f.gv[p][:, np.maximum(local, 0)], -1)         # (copies, n, width)
            blocks.append(mapped.reshape(-1, width))
        rows = np.concatenate(blocks) if blocks else np.zeros((0, width), np.int64)
        order = _sorted_tuples(rows)
        self.rows = rows[order]
        self.length = (self.rows >= 0).sum(axis=1)
        self.n = len(order)
        pos = np.empty(self.n, np.int64)
        pos[order] = np.arange(self.n)
        self.gc, at = [], 0
        for p in f.parts():
            n = f.copies(p) * len(per_part[p])
            self.gc.append(pos[at:at + n].reshape(f.copies(p), len(per_part[p])))
            at += n
        for g in self.gc:                                       # increasing inside a copy: the tile's own order
            assert g.shape[1] < 2 or (np.diff(g, axis=1) > 0).all()

    def offset_verts(self):
        """The list as maximal_cliques_list gives it: (offset int64[n + 1], verts)."""
        return np.concatenate([[0], np.cumsum(self.length)]), self.rows[self.rows >= 0]


def max_clique(f):
    """max_clique_ref.solve of the union (no budget): omega, upper, flags, t_max, n_max_cliques, count, the sorted list as a
    CliqueList in "list", witness, and nodes (the sum of the tiles' searches: a figure of the restatement, not the union's)."""
    import max_clique_ref as MC
    t = [f.tile_result(p, "max_clique", lambda nv_t, teu, tev: MC.solve(nv_t, teu, tev)) for p in f.parts()]
    live = [p for p in f.parts() if f.copies(p)]
    omega = max([t[p]["omega"] for p in live], default=0)
    top = [t[p]["omega"] == omega and omega > 0 for p in f.parts()]
    lst = CliqueList(f, [t[p]["cliques"] if top[p] else [] for p in f.parts()])
    return {"omega": omega, "upper": omega, "flags": MC.EXACT | MC.ENUMERATED | MC.LISTED,
            "t_max": max([t[p]["t_max"] for p in live], default=0),
            "n_max_cliques": f.total([t[p]["n_max_cliques"] if top[p] else 0 for p in f.parts()]),
            "count": f.per_vertex([t[p]["count"] if top[p] else np.zeros(f.u.tiles[p][0], np.int64) for p in f.parts()]),
            "list": lst, "witness": lst.rows[0] if lst.n else np.zeros(0, np.int64),
            "nodes": f.total([t[p]["nodes"] for p in f.parts()])}


def clique_census(f, k_local=0):
    """clique_census_ref.census(k_lo = 2, k_hi = -1, k_local) of the union: k_hi, t_max, omega, total (Python ints for k = 2 ..
    k_hi) and local (int64[nv], or None)."""
    import clique_census_ref as CC
    def one(nv_t, teu, tev):
        if not len(teu):
            return {"t_max": 0, "omega": 0, "exact": ([], None), "k_hi": 2}
        tr = tile_trussness(nv_t, teu, tev)
        return CC.census(nv_t, teu, tev, 2, -1, k_local if 2 <= k_local <= int(tr.max()) else 0, truss=tr)
    t = [f.tile_result(p, ("census", k_local), one) for p in f.parts()]
    live = [p for p in f.parts() if f.copies(p)]
    t_max = max([t[p]["t_max"] for p in live], default=0)
    k_hi = max(t_max, 2)
    total = [0] * (k_hi - 1)
    for p in live:
        for i, x in enumerate(t[p]["exact"][0]):
            total[i] += f.copies(p) * x
    local = None
    if k_local:
        local = f.per_vertex([t[p]["exact"][1] if t[p]["exact"][1] is not None else np.zeros(f.u.tiles[p][0], np.int64) for p in f.parts()])
    return {"k_hi": k_hi, "t_max": t_max, "omega": max([t[p]["omega"] for p in live], default=0), "total": total, "local": local}


def maximal_cliques(f):
    """maximal_cliques_ref.solve(k_min = 2) of the union: k_hi, t_max, omega, n_cliques, hist, count, largest, the sorted list
    as a CliqueList in "list", and nodes (the sum of the tiles')."""
    import maximal_cliques_ref as MQ
    t = [f.tile_result(p, "maximal", lambda nv_t, teu, tev: MQ.solve(nv_t, teu, tev, 2)) for p in f.parts()]
    live = [p for p in f.parts() if f.copies(p)]
    t_max = max([t[p]["t_max"] for p in live], default=0)
    k_hi = max(t_max, 2)
    hist = np.zeros(k_hi - 1, np.int64)
    for p in live:
        hist[:len(t[p]["hist"])] += f.copies(p) * t[p]["hist"]
    return {"k_hi": k_hi, "t_max": t_max, "omega": max([t[p]["omega"] for p in live], default=0),
            "n_cliques": f.total([t[p]["n_cliques"] for p in f.parts()]), "hist": hist,
            "count": f.per_vertex([t[p]["count"] for p in f.parts()]), "largest": f.per_vertex([t[p]["largest"] for p in f.parts()]),
            "list": CliqueList(f, [t[p]["cliques"] for p in f.parts()]), "nodes": f.total([t[p]["nodes"] for p in f.parts()]),
            "tiles": t}


def clique_communities(f, mq, k):
    """clique_communities_ref.solve(nv, the union's maximal cliques, k) from mq = maximal_cliques(f): label, size (per clique
    of the list), rep, n_cliques (per community, ascending rep), n_comm, first (per vertex) and the counts of info with
    pair_tests."""
    import clique_communities_ref as QC
    def one(p):
        nv_t, cl = f.u.tiles[p][0], mq["tiles"][p]["cliques"]
        return f.tile_result(p, ("clique_communities", k), lambda *_: {**QC.solve(nv_t, cl, k), "pair_tests": QC.pair_tests(cl, k)})
    t = [one(p) for p in f.parts()]
    gc = mq["list"].gc
    n = mq["list"].n
    out = {"label": spread(n, [(gc[p], map_label(t[p]["label"], gc[p])) for p in f.parts()]),
           "size": spread(n, [(gc[p], t[p]["size"]) for p in f.parts()]),
           "n_comm": f.per_vertex([t[p]["n_comm"] for p in f.parts()])}
    rep = np.concatenate([map_label(t[p]["rep"], gc[p]).reshape(-1) for p in f.parts()])
    order = np.argsort(rep)
    number = np.empty(len(rep), np.int64)                    # the union's community number of (part, copy, tile community)
    number[order] = np.arange(len(rep))
    out["rep"] = rep[order]
    out["n_cliques"] = np.concatenate([np.tile(t[p]["n_cliques"], f.copies(p)) for p in f.parts()])[order]
    first, at = [], 0
    for p in f.parts():
        nc = len(t[p]["rep"])
        g = number[at:at + f.copies(p) * nc].reshape(f.copies(p), nc)
        first.append(map_label(t[p]["first"], g) if nc else np.full((f.copies(p), f.u.tiles[p][0]), -1, np.int64))
        at += f.copies(p) * nc
    out["first"] = f.per_vertex(first)
    for x in ("n_member_cliques", "n_communities", "n_covered", "n_overlap", "pair_tests"):
        out[x] = f.total([t[p][x] for p in f.parts()])
    out["largest"] = f.largest([t[p]["largest"] for p in f.parts()])
    return out
