"""CPU reference of komb_community_hierarchy_run for the tests, straight from the definition in include/komb_accel.h:
hierarchy_ref._forest over ITEMS = canonical edges, level = trussness (-1 where it is 2), k_min = 3, and the communities of
every C_k from truss_communities_ref with the triangle list made once.  No GPU, no product code."""
import numpy as np

import hierarchy_ref as H
import truss_communities_ref as C

FIELDS = H.FIELDS


def community_hierarchy(nv, eu, ev, tr):
    """{"k", "rep", "parent", "size", "shell"} per node and "node" per canonical edge."""
    eu, ev, tr = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(tr, np.int64)
    ne = len(tr)
    tri = C.triangles(nv, eu, ev)
    lvl = np.where(tr >= 3, tr, -1)
    return H._forest(ne, lvl, 3, lambda k: C.communities(nv, eu, ev, tr, k, tri))


def info(h):
    """(n_nodes, n_roots, k_max, depth, n_member_edges) of a forest."""
    return H.info(h, "truss") + (int((h["node"] >= 0).sum()),)


def walk_up(h, tr, k):
    """(label, size) per canonical edge at threshold k, read off the forest: from node[e] up while the parent's level is
    still >= k.  k <= 2 runs as 2: an edge without a node is a community of its own."""
    tr = np.asarray(tr, np.int64)
    k = max(int(k), 2)
    kk, parent = h["k"].astype(np.int64), h["parent"].astype(np.int64)
    top = np.arange(len(kk))
    while len(kk):
        p = parent[top]
        up = (p >= 0) & (kk[np.maximum(p, 0)] >= k)
        if not up.any():
            break
        top = np.where(up, p, top)
    label, size = np.full(len(tr), -1, np.int64), np.zeros(len(tr), np.int64)
    mem = (h["node"] >= 0) & (tr >= k)
    at = top[h["node"][mem]]
    label[mem], size[mem] = h["rep"][at], h["size"][at]
    if k == 2:
        alone = h["node"] < 0
        label[alone], size[alone] = np.flatnonzero(alone), 1
    return label, size


def check_invariants(h):
    H.check_invariants(h, False)
    assert (h["shell"] >= 0).all() and (h["size"] >= 3).all()           # a community of k >= 3 holds a triangle
    assert np.array_equal(np.bincount(h["node"][h["node"] >= 0], minlength=len(h["k"])), h["shell"])
