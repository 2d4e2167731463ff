"""CPU reference of komb_biconnected_run for the tests: the blocks by an iterative Hopcroft-Tarjan depth-first search with
an edge stack in plain Python, everything derived from them with numpy / scipy.  No GPU, no product code.

The subject is the graph of the edges (eu[i], ev[i]) with tr[i] >= k; members are their endpoints.
  block[i]      smallest canonical index of the block of edge i, -1 for a non-member
  size[i]       edges of that block, 0 for a non-member (1: a bridge)
  n_blocks[v]   blocks that contain v (>= 2: an articulation point)
  ecc_label[v]  smallest id of v's 2-edge-connected component (components once the bridges are removed), -1 for a non-member
  ecc_size[v]   vertices of that component
  blocks        {"rep", "n_edges", "n_verts"} in ascending rep order
  depth         levels of the breadth-first forest rooted at the smallest id of every component (fixed by the graph)"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import shortest_path

import components_ref as CR

INFO_FIELDS = ("n_member_edges", "n_member_vertices", "n_blocks", "n_bridges", "n_articulation", "largest_block", "n_ecc",
               "largest_ecc", "depth")


def _csr(nv, u, v):
    nm = len(u)
    src, dst = np.concatenate([u, v]), np.concatenate([v, u])
    eid = np.concatenate([np.arange(nm), np.arange(nm)])
    order = np.argsort(src, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=nv))])
    return rowptr, dst[order], eid[order]


def _dfs_blocks(nv, rowptr, adj, aeid, nm):
    """blk[j] = the number of member edge j's block, in the order the search closes them."""
    rp, adj, aeid = rowptr.tolist(), adj.tolist(), aeid.tolist()
    disc, low, it = [-1] * nv, [0] * nv, rp[:-1]
    blk, n_blk, clock = [-1] * nm, 0, 0
    for s in range(nv):
        if disc[s] >= 0 or rp[s] == rp[s + 1]:
            continue
        disc[s] = low[s] = clock
        clock += 1
        vstack, pstack, estack = [s], [-1], []
        while vstack:
            x = vstack[-1]
            if it[x] < rp[x + 1]:
                i = it[x]
                it[x] = i + 1
                w, e = adj[i], aeid[i]
                if e == pstack[-1]:
                    continue
                if disc[w] < 0:
                    estack.append(e)
                    disc[w] = low[w] = clock
                    clock += 1
                    vstack.append(w)
                    pstack.append(e)
                elif disc[w] < disc[x]:
                    estack.append(e)
                    if disc[w] < low[x]:
                        low[x] = disc[w]
            else:
                vstack.pop()
                e = pstack.pop()
                if vstack:
                    p = vstack[-1]
                    if low[x] < low[p]:
                        low[p] = low[x]
                    if low[x] >= disc[p]:
                        while True:
                            f = estack.pop()
                            blk[f] = n_blk
                            if f == e:
                                break
                        n_blk += 1
    return np.asarray(blk, np.int64), n_blk


def _depth(nv, u, v, roots):
    """Levels of the breadth-first forest: hop distances from a source joined to every root."""
    rows, cols = np.concatenate([u, np.full(len(roots), nv)]), np.concatenate([v, roots])
    A = csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv + 1, nv + 1))
    d = shortest_path(A, method="D", directed=False, unweighted=True, indices=[nv])[0]
    return int(d[np.isfinite(d)].max())


def biconnected(nv, eu, ev, tr, k):
    eu, ev, tr = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(tr, np.int64)
    m = len(tr)
    mem = np.flatnonzero(tr >= k)
    u, v, nm = eu[mem], ev[mem], len(mem)
    block, size = np.full(m, -1, np.int64), np.zeros(m, np.int64)
    n_blocks, ecc_label, ecc_size = np.zeros(nv, np.int64), np.full(nv, -1, np.int64), np.zeros(nv, np.int64)
    out = {"block": block, "size": size, "n_blocks": n_blocks, "ecc_label": ecc_label, "ecc_size": ecc_size,
           "blocks": {x: np.zeros(0, np.int64) for x in ("rep", "n_edges", "n_verts")}, "info": dict.fromkeys(INFO_FIELDS, 0)}
    if nm == 0:
        return out
    rowptr, adj, aeid = _csr(nv, u, v)
    blk, n_blk = _dfs_blocks(nv, rowptr, adj, aeid, nm)
    assert blk.min() >= 0
    rep = np.full(n_blk, m, np.int64)
    np.minimum.at(rep, blk, mem)
    cnt = np.bincount(blk, minlength=n_blk)
    block[mem], size[mem] = rep[blk], cnt[blk]
    pairs = np.unique(np.concatenate([u * n_blk + blk, v * n_blk + blk]))      # the distinct (vertex, block) incidences
    n_blocks[:] = np.bincount(pairs // n_blk, minlength=nv)
    verts = np.bincount(pairs % n_blk, minlength=n_blk)
    order = np.argsort(rep)
    out["blocks"] = {"rep": rep[order], "n_edges": cnt[order], "n_verts": verts[order]}
    member = np.zeros(nv, bool)
    member[u] = member[v] = True
    keep = cnt[blk] > 1
    ecc_label[:] = CR.min_labels(nv, u[keep], v[keep], member)
    ecc_size[:] = CR.sizes(ecc_label)
    comp = CR.min_labels(nv, u, v, member)
    roots = np.flatnonzero(comp == np.arange(nv))
    out["info"] = {"n_member_edges": nm, "n_member_vertices": int(member.sum()), "n_blocks": n_blk, "n_bridges": int((cnt == 1).sum()),
                   "n_articulation": int((n_blocks >= 2).sum()), "largest_block": int(cnt.max()),
                   "n_ecc": int((ecc_label == np.arange(nv)).sum()), "largest_ecc": int(ecc_size.max()),
                   "depth": _depth(nv, u, v, roots)}
    return out


def summary(res):
    """The info fields as a tuple, in INFO_FIELDS order."""
    return tuple(res["info"][x] for x in INFO_FIELDS)
