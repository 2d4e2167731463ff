"""CPU reference of komb_nucleus_hierarchy_run for the tests, straight from the definition in include/komb_accel.h:
nucleus_ref.decompose gives theta and the 4-cliques, a clique links its first triangle to its other three with weight
min(theta), and hierarchy_ref._forest takes the ITEMS = triangles, level = theta (-1 where it is 0), k_min = 1, with the
k-nuclei of every level from hierarchy_ref._labels_by_weight.  No GPU, no product code."""
import numpy as np

import hierarchy_ref as H
import nucleus_ref as N

FIELDS = H.FIELDS
NUCLEI_FIELDS = ("rep", "n_triangles", "n_edges", "n_vertices")


def forest(theta, cliques):
    """{"k", "rep", "parent", "size", "shell"} per node and "node" per triangle, from theta[n_triangles] and the cliques as
    4-tuples of triangle ids."""
    theta = np.asarray(theta, np.int64).reshape(-1)
    nt = len(theta)
    q = np.asarray(cliques, np.int64).reshape(-1, 4)
    lu = np.repeat(q[:, 0], 3)
    lv = q[:, 1:].reshape(-1)
    w = np.repeat(theta[q].min(axis=1) if len(q) else np.zeros(0, np.int64), 3)
    lvl = np.where(theta >= 1, theta, -1)
    return H._forest(nt, lvl, 1, H._labels_by_weight(nt, lu, lv, w, lambda k, u, v: theta >= k))


def hierarchy(nv, eu, ev, theta=None):
    """(forest, decomposition) of the canonical edges of a k-truss result; theta, when given (the library's own), must be
    the restatement's."""
    dec = N.decompose(nv, eu, ev)
    if theta is not None:
        assert np.array_equal(np.asarray(theta), dec["theta"])
    return forest(dec["theta"], dec["cliques"]), dec


def hierarchy_edges(nv, edges):
    e = N.canonical(edges)
    return hierarchy(nv, [u for u, _ in e], [v for _, v in e])


def info(h, theta):
    """(n_nodes, n_roots, theta_max, depth, n_member_triangles)."""
    theta = np.asarray(theta, np.int64)
    n, roots, _, depth = H.info(h, "truss")
    return (n, roots, int(theta.max()) if len(theta) else -1, depth, int((theta >= 1).sum()))


def resolve_k(theta, k):
    """k as komb_nucleus_hierarchy_labels / _nuclei take it: -1 is the largest theta, then anything up to 1 runs as 1."""
    theta = np.asarray(theta, np.int64)
    if k == -1:
        k = int(theta.max()) if len(theta) else -1
    return max(int(k), 1)


def walk_up(h, theta, k):
    """(label, size) per triangle at threshold k, read off the forest: from node[t] up while the parent's level is still
    >= k."""
    theta = np.asarray(theta, np.int64)
    k = resolve_k(theta, k)
    kk, parent = h["k"].astype(np.int64), h["parent"].astype(np.int64)
    top = np.arange(len(kk))
    while len(kk):
        p = parent[top]
        up = (p >= 0) & (kk[np.maximum(p, 0)] >= k)
        if not up.any():
            break
        top = np.where(up, p, top)
    label, size = np.full(len(theta), -1, np.int64), np.zeros(len(theta), np.int64)
    mem = (h["node"] >= 0) & (theta >= k)
    at = top[h["node"][mem]]
    label[mem], size[mem] = h["rep"][at], h["size"][at]
    return label, size


def nuclei(h, dec, k):
    """The k-nuclei as subgraphs, in ascending rep order: rep, triangles, distinct edges, distinct vertices."""
    label, _ = walk_up(h, dec["theta"], k)
    mem = label >= 0
    lab = label[mem]
    a, b, c = (np.asarray(dec[x], np.int64)[mem] for x in "abc")
    reps, n_tri = np.unique(lab, return_counts=True)
    def distinct(x):                                      # distinct (label, x) pairs, counted per label
        if not len(lab):
            return np.zeros(len(reps), np.int64)
        item = np.unique(x, return_inverse=True)[1].reshape(-1)
        n_items = int(item.max()) + 1
        pairs = np.unique(lab3 * n_items + item)
        return np.bincount(np.searchsorted(reps, pairs // n_items), minlength=len(reps))
    lab3 = np.concatenate([lab, lab, lab])
    span = int(c.max()) + 1 if len(lab) else 1            # (a < b < c)
    n_vert = distinct(np.concatenate([a, b, c]))
    n_edge = distinct(np.concatenate([a, a, b]) * span + np.concatenate([b, c, c]))
    return {"rep": reps.astype(np.int32), "n_triangles": n_tri.astype(np.int32), "n_edges": n_edge.astype(np.int32),
            "n_vertices": n_vert.astype(np.int32)}


def check_invariants(h, theta):
    theta = np.asarray(theta, np.int64)
    H.check_invariants(h, False)
    assert (h["shell"] >= 0).all() and (h["size"] >= 4).all()           # a nucleus of k >= 1 holds a 4-clique
    assert np.array_equal(np.bincount(h["node"][h["node"] >= 0], minlength=len(h["k"])), h["shell"])
    assert int(h["shell"].sum()) == int((theta >= 1).sum())
    assert np.array_equal(h["node"] >= 0, theta >= 1)
    assert np.array_equal(h["k"][h["node"][theta >= 1]], theta[theta >= 1])
    roots = h["parent"] < 0
    assert int(h["size"][roots].sum()) == int((theta >= 1).sum())


# ---- graphs of the worked examples

def two_k5_sharing_an_edge():
    return 8, N.clique([0, 1, 2, 3, 4]) + N.clique([0, 1, 5, 6, 7])


def k6_plus_vertex():
    return 7, N.clique(range(6)) + [(6, 0), (6, 1), (6, 2)]


def two_k6_joined_by_a_band():
    return 12, N.clique(range(6)) + N.clique(range(6, 12)) + [(3, 6), (4, 6), (5, 6), (4, 7), (5, 7), (5, 8)]


def clique_chain(n):
    """K_4, K_5, ..., K_n, each sharing a triangle -- its first three vertices -- with the last three of the one before."""
    edges, start = [], 0
    for size in range(4, n + 1):
        edges += N.clique(range(start, start + size))
        start += size - 3
    return start + 3, N.canonical(edges)


def band(nv, width=3):
    return nv, [(i, i + d) for i in range(nv) for d in range(1, width + 1) if i + d < nv]


def disjoint_k4(n):
    return 4 * n, [e for i in range(n) for e in N.clique(range(4 * i, 4 * i + 4))]


def triangle_in_n_cliques(n):
    """K_3 plus n vertices, each joined to all three: one triangle in n 4-cliques."""
    return n + 3, N.clique([0, 1, 2]) + [(x, v) for v in range(3, n + 3) for x in (0, 1, 2)]
