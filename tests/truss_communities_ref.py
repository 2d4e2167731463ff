"""CPU reference of komb_truss_communities_run for the tests: the k-truss communities of Huang, Cheng, Qin, Tian, Yu
(SIGMOD 2014) -- the classes of the edges of trussness >= k under "two sides of a triangle of three such edges".
Triangles come from a (degree, id)-ordered wedge expansion in numpy, the classes from scipy's connected components over
EDGES, relabelled by the smallest edge index.  An independent brute force (all vertex triples, a plain union-find) checks
it on small graphs.  No GPU, no product code."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

WEDGE_CHUNK = 20_000_000


def triangles(nv, eu, ev):
    """Every triangle of the simple graph of the edges (eu[i], ev[i]) once, as three arrays of EDGE indices
    (e_ab, e_ac, e_bc) with a < b < c in (degree, id) order."""
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    ne = len(eu)
    empty = np.zeros(0, np.int64)
    if ne == 0:
        return empty, empty, empty
    deg = np.bincount(eu, minlength=nv) + np.bincount(ev, minlength=nv)
    rank = np.empty(nv, np.int64)
    rank[np.lexsort((np.arange(nv), deg))] = np.arange(nv)
    ru, rv = rank[eu], rank[ev]
    src, dst = np.minimum(ru, rv), np.maximum(ru, rv)
    key = src * nv + dst
    order = np.argsort(key, kind="stable")          # oriented slot -> edge index
    key, src, dst = key[order], src[order], dst[order]
    assert np.all(key[1:] > key[:-1]), "duplicate edges"
    row_end = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=nv), out=row_end[1:])
    slots = np.arange(ne)
    later = row_end[src + 1] - slots - 1            # slots of the same row behind this one: the wedges (a->b, a->c), b < c
    cum = np.concatenate([[0], np.cumsum(later)])
    out = [[], [], []]
    s0 = 0
    while s0 < ne:
        s1 = int(np.searchsorted(cum, cum[s0] + WEDGE_CHUNK, side="right")) - 1
        s1 = min(max(s1, s0 + 1), ne)
        n = later[s0:s1]
        first = np.repeat(slots[s0:s1], n)                              # slot of (a, b)
        second = first + 1 + (np.arange(int(n.sum())) - np.repeat(cum[s0:s1] - cum[s0], n))   # slot of (a, c)
        want = dst[first] * nv + dst[second]                            # key of (b, c)
        third = np.searchsorted(key, want)
        third[third >= ne] = ne - 1
        hit = key[third] == want
        out[0].append(order[first[hit]]); out[1].append(order[second[hit]]); out[2].append(order[third[hit]])
        s0 = s1
    return tuple(np.concatenate(x) if x else empty for x in out)


def communities(nv, eu, ev, tr, k, tri=None):
    """label[i] = smallest edge index of edge i's k-truss community, -1 for an edge of trussness < k (k <= 2: every edge
    is a member).  tri: triangles(nv, eu, ev), to share between thresholds."""
    tr = np.asarray(tr, np.int64)
    ne = len(tr)
    if ne == 0:
        return np.zeros(0, np.int64)
    member = tr >= max(int(k), 2)
    if tri is None:
        tri = triangles(nv, eu, ev)
    t0, t1, t2 = tri
    ok = member[t0] & member[t1] & member[t2]
    t0, t1, t2 = t0[ok], t1[ok], t2[ok]
    a, b = np.concatenate([t0, t0]), np.concatenate([t1, t2])
    A = csr_matrix((np.ones(len(a), np.int8), (a, b)), shape=(ne, ne))
    n, lab = connected_components(A, directed=False)
    first = np.full(n, ne, np.int64)
    np.minimum.at(first, lab, np.arange(ne))
    out = first[lab]
    out[~member] = -1
    return out


def sizes(label):
    """size[i] = edges that carry i's label, 0 for a non-member."""
    label = np.asarray(label, np.int64)
    ne = len(label)
    cnt = np.bincount(label[label >= 0], minlength=ne) if ne else np.zeros(0, np.int64)
    out = np.zeros(ne, np.int64)
    out[label >= 0] = cnt[label[label >= 0]]
    return out


def vertex_multiplicity(nv, eu, ev, label):
    """n_comm[v] = distinct labels among the member edges at v."""
    eu, ev, label = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(label, np.int64)
    sel = label >= 0
    ne = max(len(label), 1)
    pairs = np.unique(np.concatenate([eu[sel] * ne + label[sel], ev[sel] * ne + label[sel]]))
    return np.bincount(pairs // ne, minlength=nv).astype(np.int64)[:nv] if nv else np.zeros(0, np.int64)


def summary(nv, eu, ev, label):
    """(n_member_edges, n_communities, largest, n_multi_vertices) of a label vector."""
    label = np.asarray(label, np.int64)
    sz = sizes(label)
    roots = label == np.arange(len(label))
    multi = vertex_multiplicity(nv, eu, ev, label)
    return int((label >= 0).sum()), int(roots.sum()), int(sz.max()) if len(sz) else 0, int((multi > 1).sum())


def brute_force(nv, eu, ev, tr, k):
    """The same labels from the definition: every vertex triple, a plain union-find.  Small graphs only."""
    eu, ev, tr = [np.asarray(x, np.int64).tolist() for x in (eu, ev, tr)]
    k = max(int(k), 2)
    eid = {}
    for i, (u, v) in enumerate(zip(eu, ev)):
        if tr[i] >= k:
            eid[(min(u, v), max(u, v))] = i
    adj = [set() for _ in range(nv)]
    for (u, v) in eid:
        adj[u].add(v); adj[v].add(u)
    parent = list(range(len(eu)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def union(x, y):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)

    for a in range(nv):
        for b in adj[a]:
            if b <= a:
                continue
            for c in adj[a] & adj[b]:
                if c <= b:
                    continue
                union(eid[(a, b)], eid[(a, c)])
                union(eid[(a, b)], eid[(b, c)])
    return np.asarray([find(i) if tr[i] >= k else -1 for i in range(len(eu))], np.int64)


def brute_multiplicity(nv, eu, ev, label):
    seen = [set() for _ in range(nv)]
    for u, v, l in zip(np.asarray(eu).tolist(), np.asarray(ev).tolist(), np.asarray(label).tolist()):
        if l >= 0:
            seen[u].add(l); seen[v].add(l)
    return np.asarray([len(s) for s in seen], np.int64)
