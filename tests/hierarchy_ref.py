"""CPU reference of komb_hierarchy_run for the tests, straight from the definition in include/komb_accel.h: the components
of every G_k by scipy (components_ref), a component is a node when its vertex set is not a component's of G_(k+1), a
node's parent is found by searching down the levels.  No GPU, no product code."""
import numpy as np

import components_ref as R

FIELDS = ("k", "rep", "parent", "size", "shell")


def _forest(nv, lvl, k_min, labels_at):
    """lvl[v]: the vertex' level (-1: non-member); labels_at(k): min-id labels of G_k's components (-1: non-member)."""
    lvl = np.asarray(lvl, np.int64)
    k_top = int(lvl.max()) if nv and lvl.max() >= k_min else k_min - 1
    ks = list(range(k_min, k_top + 1))
    labs = {k: labels_at(k).astype(np.int32) for k in ks}
    labs[k_top + 1] = np.full(nv, -1, np.int32)
    ids = np.arange(nv)
    out_k, out_rep, out_size = [], [], []
    index = {}                                              # level -> int32[nv]: node number at a node's rep, -1 elsewhere
    n = 0
    for k in ks:
        lab, nxt = labs[k], labs[k + 1]
        mem = lab >= 0
        # S (the component labelled r) is a component of G_(k+1) too iff all of S carries one label there
        differs = mem & ((nxt < 0) | (nxt != nxt[np.where(mem, lab, 0)]))
        is_node = np.zeros(nv, bool)
        is_node[lab[differs]] = True
        reps = ids[is_node]
        idx = np.full(nv, -1, np.int32)
        idx[reps] = n + np.arange(len(reps))
        index[k] = idx
        cnt = np.bincount(lab[mem], minlength=nv)
        out_k += [k] * len(reps); out_rep += reps.tolist(); out_size += cnt[reps].tolist()
        n += len(reps)
    k_arr, rep = np.asarray(out_k, np.int32), np.asarray(out_rep, np.int32)
    parent = np.full(n, -1, np.int32)
    open_ = np.ones(n, bool)
    for k in reversed(ks):                                  # search down: the nearest level below whose component around rep is a node
        cand = np.flatnonzero(open_ & (k_arr > k))
        if not len(cand):
            continue
        r = labs[k][rep[cand]]
        p = index[k][r]
        hit = p >= 0
        parent[cand[hit]] = p[hit]
        open_[cand[hit]] = False
    node = np.full(nv, -1, np.int32)
    for k in ks:
        at = lvl == k
        node[at] = index[k][labs[k][at]]
        assert (node[at] >= 0).all(), "a vertex of level k lies in a node of level k"
    shell = np.bincount(node[node >= 0], minlength=n).astype(np.int32)
    return {"k": k_arr, "rep": rep, "parent": parent, "size": np.asarray(out_size, np.int32), "shell": shell,
            "node": node}


def _labels_by_weight(nv, eu, ev, w, member_at):
    """labels_at(k) over the edges of weight >= k (sorted once, so that a level takes a prefix), through R.min_labels."""
    order = np.argsort(-w, kind="stable")
    eu, ev, neg = eu[order], ev[order], -w[order]
    def labels_at(k):
        n = int(np.searchsorted(neg, -k, side="right"))
        return R.min_labels(nv, eu[:n], ev[:n], member_at(k, eu[:n], ev[:n]))
    return labels_at


def core_hierarchy(rowptr, col, core):
    rowptr, col, core = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(core, np.int64)
    nv = len(core)
    src = np.repeat(np.arange(nv), np.diff(rowptr))
    once = src < col
    eu, ev = src[once], col[once]
    return _forest(nv, core, 0, _labels_by_weight(nv, eu, ev, np.minimum(core[eu], core[ev]), lambda k, u, v: core >= k))


def truss_levels(nv, eu, ev, tr):
    """lvl(v) = the largest trussness of an edge at v, -1 without one."""
    lvl = np.full(nv, -1, np.int64)
    np.maximum.at(lvl, np.asarray(eu, np.int64), np.asarray(tr, np.int64))
    np.maximum.at(lvl, np.asarray(ev, np.int64), np.asarray(tr, np.int64))
    return lvl


def truss_hierarchy(nv, eu, ev, tr):
    eu, ev, tr = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(tr, np.int64)
    def member_at(k, u, v):
        mem = np.zeros(nv, bool)
        mem[u] = True
        mem[v] = True
        return mem
    return _forest(nv, truss_levels(nv, eu, ev, tr), 2, _labels_by_weight(nv, eu, ev, tr, member_at))


def info(h, kind):
    """(n_nodes, n_roots, k_max, depth) of a forest."""
    n = len(h["k"])
    depth, a = np.zeros(n, np.int64) + (1 if n else 0), h["parent"].astype(np.int64)
    while n and (a >= 0).any():
        depth[a >= 0] += 1
        a = np.where(a >= 0, h["parent"][np.maximum(a, 0)], -1)
    return (n, int((h["parent"] < 0).sum()), int(h["k"].max()) if n else (0 if kind == "core" else 2),
            int(depth.max()) if n else 0)


def walk_up_labels(h, lvl, k):
    """label[v] for the members of G_k (lvl(v) >= k): from node[v] up while the parent's level is still >= k; the rep there."""
    kk, parent = h["k"].astype(np.int64), h["parent"].astype(np.int64)
    top = np.arange(len(kk))
    while True:
        p = parent[top]
        up = (p >= 0) & (kk[np.maximum(p, 0)] >= k)
        if not up.any():
            break
        top = np.where(up, p, top)
    lvl = np.asarray(lvl, np.int64)
    out = np.full(len(lvl), -1, np.int64)
    mem = lvl >= k
    out[mem] = h["rep"][top[h["node"][mem]]]
    return out


def check_invariants(h, core_kind):
    n = len(h["k"])
    assert (h["parent"] < np.arange(n)).all()
    kids = np.zeros(n, np.int64)
    has = h["parent"] >= 0
    np.add.at(kids, h["parent"][has], h["size"][has])
    assert np.array_equal(h["size"], h["shell"] + kids)
    assert (h["k"][h["parent"][has]] < h["k"][has]).all()
    order = np.lexsort((h["rep"], h["k"]))
    assert np.array_equal(order, np.arange(n))
    if core_kind:
        assert (h["shell"] >= 1).all()


# ---- graphs that both the CPU tests of this reference and the GPU tests use: (nv, raw pairs)

STRIDE_ISOLATED = 2048 * 256 + 257                          # the most workgroups CLAIM / ADOPT get, 256 items each, and 257 more


def strided_claim_graph():
    """STRIDE_ISOLATED isolated vertices, then a K_4 on the last four ids: level 0 takes the whole grid, whose workgroups
    0 and 1 go round a second time (256 items and 1) and meet roots that are not their first one's."""
    n = STRIDE_ISOLATED
    return n + 4, np.stack(np.triu_indices(4, 1), 1) + n


def shell_first_graph():
    """300 disjoint edges (level 1: 600 vertices but 300 hooks), two stars of 2 100 leaves whose hubs are joined to every
    vertex of a K_5 and of a K_30: level 1 has more vertices than hooks, so its last workgroups take their first root from
    the vertex list, and the hubs' rows (>= 2048 entries) are linked at two different core levels, 30 and 5."""
    parts, off = [np.stack([np.arange(0, 600, 2), np.arange(1, 600, 2)], 1)], 600
    for n in (5, 30):
        hub, clique, leaves = off, off + 1 + np.arange(n), off + 1 + n + np.arange(2100)
        parts += [np.stack(np.triu_indices(n, 1), 1) + off + 1, np.stack([np.full(n, hub), clique], 1), np.stack([np.full(2100, hub), leaves], 1)]
        off += 1 + n + 2100
    return off, np.concatenate(parts)
