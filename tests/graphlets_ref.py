"""Two independent CPU references of the graphlet census (komb_graphlets_run).

brute(nv, edges)      every 3- and 4-subset of the vertices, classified by (edge count, sorted degrees inside the subset) --
                      enough to tell the connected 3- and 4-vertex graphs apart.  Small graphs only.
census(nv, eu, ev)    the counting scheme of the library with none of its machinery: 4-cycles per edge by the dense identity
                      cycles4(u, v) = (A^3)[u, v] - d(u) - d(v) + 1 in float64 (exact below 2^53: nv <= 3000), 4-cliques per
                      edge by common-neighbour sets, the orbits by the closed forms.  Neither the (d, id) order nor a hash
                      table takes part in a count.  Above 3000 vertices (or as census_sparse) the 4-cycles per edge are
                      the sum over x in N(u) without v of |N(x) & N(v)| - 1 with plain sets; everything else is shared.
ordered_items(...)    the work formula of the degree-ordered 4-cycle pass.

Both return {"orbit": uint64[15, nv], "cycles4": uint64[m], "cliques4": uint64[m], "sup": int64[m], "total": {name: int}}
with the per-edge arrays in the order of the edges given.
"""
from bisect import bisect_left
from itertools import combinations

import numpy as np

ORBITS = 15
TYPES = ("edge", "wedge", "triangle", "path4", "claw", "cycle4", "paw", "diamond", "clique4")
# total = sum of orbit o over the vertices / divisor
TOTAL_OF = {"edge": (0, 2), "wedge": (2, 1), "triangle": (3, 3), "path4": (5, 2), "claw": (7, 1), "cycle4": (8, 4), "paw": (11, 1),
            "diamond": (13, 2), "clique4": (14, 4)}
# the six redundancy identities: sum of orbit a * fa == sum of orbit b * fb
IDENTITIES = ((1, 1, 2, 2), (4, 1, 5, 1), (6, 1, 7, 3), (9, 1, 11, 1), (10, 1, 11, 2), (12, 1, 13, 1))


def totals(orbit):
    out = {}
    for name, (o, div) in TOTAL_OF.items():
        s = sum(int(x) for x in orbit[o])
        assert s % div == 0, (name, s, div)
        out[name] = s // div
    return out


def check_identities(orbit):
    for a, fa, b, fb in IDENTITIES:
        sa, sb = sum(int(x) for x in orbit[a]), sum(int(x) for x in orbit[b])
        assert sa * fa == sb * fb, (a, fa, sa, b, fb, sb)


def _adj(nv, eu, ev):
    adj = [set() for _ in range(nv)]
    for u, v in zip(eu, ev):
        u, v = int(u), int(v)
        assert u != v and v not in adj[u], "simple graphs only"
        adj[u].add(v)
        adj[v].add(u)
    return adj


def brute(nv, edges):
    edges = [(int(u), int(v)) for u, v in edges]
    eu, ev = [e[0] for e in edges], [e[1] for e in edges]
    adj = _adj(nv, eu, ev)
    eid = {}
    for i, (u, v) in enumerate(edges):
        eid[(u, v)] = eid[(v, u)] = i
    orbit = np.zeros((ORBITS, nv), dtype=np.uint64)
    cyc = np.zeros(len(edges), dtype=np.uint64)
    clq = np.zeros(len(edges), dtype=np.uint64)
    sup = np.zeros(len(edges), dtype=np.int64)
    one = np.uint64(1)
    for v in range(nv):
        orbit[0, v] = len(adj[v])
    for s in combinations(range(nv), 3):
        deg = [sum(1 for y in s if y in adj[x]) for x in s]
        ne = sum(deg) // 2
        if ne == 2:
            for x, d in zip(s, deg):
                orbit[1 if d == 1 else 2, x] += one
        elif ne == 3:
            for x in s:
                orbit[3, x] += one
            for x, y in combinations(s, 2):
                sup[eid[(x, y)]] += 1
    for s in combinations(range(nv), 4):
        deg = [sum(1 for y in s if y in adj[x]) for x in s]
        ne = sum(deg) // 2
        if ne < 3:
            continue
        a, b, c, d = s
        for cycle in ((a, b, c, d), (a, b, d, c), (a, c, b, d)):           # the three 4-cycles on four vertices
            es = [(cycle[i], cycle[(i + 1) % 4]) for i in range(4)]
            if all(e in eid for e in es):
                for e in es:
                    cyc[eid[e]] += one
        key = (ne, tuple(sorted(deg)))
        if key == (3, (1, 1, 2, 2)):
            where = {1: 4, 2: 5}
        elif key == (3, (1, 1, 1, 3)):
            where = {1: 6, 3: 7}
        elif key == (3, (0, 2, 2, 2)):
            continue                                                        # a triangle and a stranger: not connected
        elif key == (4, (2, 2, 2, 2)):
            where = {2: 8}
        elif key == (4, (1, 2, 2, 3)):
            where = {1: 9, 2: 10, 3: 11}
        elif key == (5, (2, 2, 3, 3)):
            where = {2: 12, 3: 13}
        elif key == (6, (3, 3, 3, 3)):
            where = {3: 14}
            for x, y in combinations(s, 2):
                clq[eid[(x, y)]] += one
        else:
            raise AssertionError(key)
        for x, dx in zip(s, deg):
            orbit[where[dx], x] += one
    return {"orbit": orbit, "cycles4": cyc, "cliques4": clq, "sup": sup, "total": totals(orbit)}


def _comb2(x):
    return x * (x - 1) // 2


DENSE_MAX_NV = 3000


def _per_edge_dense(nv, eu, ev, adj, d):
    """(cycles4, sup, cliques4, common) per edge; the 4-cycles by the dense identity: the walks u-x-y-v of length 3 less those
    with x = v (d(v) of them) or y = u (d(u)), the walk u-v-u-v being in both."""
    assert nv <= DENSE_MAX_NV, "the dense identity is exact in float64 only while A^3 stays below 2^53"
    A = np.zeros((nv, nv), dtype=np.float64)
    A[eu, ev] = 1.0
    A[ev, eu] = 1.0
    A3 = A @ A @ A
    assert A3.max() < 2.0 ** 53
    cyc = np.rint(A3[eu, ev]).astype(np.int64) - d[eu] - d[ev] + 1
    return (cyc,) + _triangles_and_cliques(eu, ev, adj)


def _per_edge_sparse(nv, eu, ev, adj, d):
    """The same four with plain sets and no matrix: a 4-cycle through (u, v) is u-x-y-v with x a neighbour of u other than v and
    y a common neighbour of x and v other than u (u is always one of them): sum over x in N(u) without v of |N(x) & N(v)| - 1."""
    cyc = np.zeros(len(eu), dtype=np.int64)
    for i in range(len(eu)):
        u, v = int(eu[i]), int(ev[i])
        nv_set = adj[v]
        cyc[i] = sum(len(adj[x] & nv_set) - 1 for x in adj[u] if x != v)
    return (cyc,) + _triangles_and_cliques(eu, ev, adj)


def _triangles_and_cliques(eu, ev, adj):
    """(sup, cliques4, common): per edge its common neighbourhood, its size, and the edges inside it."""
    m = len(eu)
    sup = np.zeros(m, dtype=np.int64)
    clq = np.zeros(m, dtype=np.int64)
    common = []
    for i in range(m):
        c = adj[int(eu[i])] & adj[int(ev[i])]
        common.append(c)
        sup[i] = len(c)
        inside = sum(len(adj[w] & c) for w in c)
        assert inside % 2 == 0
        clq[i] = inside // 2
    return sup, clq, common


def census_sparse(nv, eu, ev):
    """census() without the dense A^3: any number of vertices, time in the sum of d(u) d(x) over the 2-paths."""
    return census(nv, eu, ev, dense=False)


def census(nv, eu, ev, dense=None):
    """dense: the 4-cycles per edge by A^3 (None: up to DENSE_MAX_NV vertices) or by common-neighbour sets."""
    eu = np.asarray(eu, dtype=np.int64)
    ev = np.asarray(ev, dtype=np.int64)
    m = len(eu)
    adj = _adj(nv, eu, ev)
    d = np.fromiter((len(a) for a in adj), dtype=np.int64, count=nv)
    orbit = np.zeros((ORBITS, nv), dtype=np.uint64)
    if m == 0:
        z = np.zeros(0, dtype=np.uint64)
        return {"orbit": orbit, "cycles4": z, "cliques4": z.copy(), "sup": np.zeros(0, dtype=np.int64), "total": totals(orbit)}

    # per edge (u, v): 4-cycles, triangles, 4-cliques (the edges inside the common neighbourhood)
    dense = nv <= DENSE_MAX_NV if dense is None else dense
    cyc, sup, clq, common = (_per_edge_dense if dense else _per_edge_sparse)(nv, eu, ev, adj, d)
    D2 = np.zeros(nv, dtype=np.int64)
    for i in range(m):
        for w in common[i]:                                                 # a triangle (w, eu, ev): its edge opposite w
            D2[w] += sup[i] - 1

    def at_vertices(x_to_u, x_to_v):
        out = np.zeros(nv, dtype=np.int64)
        np.add.at(out, eu, x_to_u)
        np.add.at(out, ev, x_to_v)
        return out

    T2 = at_vertices(sup, sup)
    assert (T2 % 2 == 0).all()
    t = T2 // 2
    K3 = at_vertices(clq, clq)
    assert (K3 % 3 == 0).all()
    K4 = K3 // 3
    C2 = at_vertices(cyc, cyc)
    assert (C2 % 2 == 0).all()
    C4 = C2 // 2
    D3 = at_vertices(_comb2(sup), _comb2(sup))
    S = at_vertices(d[ev] - 1, d[eu] - 1)
    W10 = at_vertices(sup * (d[ev] - 2), sup * (d[eu] - 2))
    N9 = at_vertices(t[ev] - sup, t[eu] - sup)
    B6 = at_vertices(_comb2(d[ev] - 1), _comb2(d[eu] - 1))
    SS = at_vertices(S[ev], S[eu])

    o = [None] * ORBITS
    o[0] = d
    o[3] = t
    o[2] = _comb2(d) - t
    o[1] = S - 2 * t
    o[14] = K4
    o[13] = D3 - 3 * K4
    o[12] = D2 - 3 * K4
    o[8] = C4 - o[12] - o[13] - 3 * K4
    o[11] = t * (d - 2) - 2 * o[13] - 3 * K4
    o[10] = W10 - 2 * o[13] - 2 * o[12] - 6 * K4
    o[9] = N9 - 2 * o[12] - 3 * K4
    o[7] = d * (d - 1) * (d - 2) // 6 - o[11] - o[13] - K4
    o[6] = B6 - o[9] - o[10] - o[13] - 2 * o[12] - 3 * K4
    o[4] = SS - d * (d - 1) - 2 * t - 2 * o[8] - 2 * o[9] - o[10] - 2 * o[13] - 4 * o[12] - 6 * K4
    o[5] = (d - 1) * S - 2 * t - 2 * o[8] - o[10] - 2 * o[11] - 4 * o[13] - 2 * o[12] - 6 * K4
    for i in range(ORBITS):
        assert (o[i] >= 0).all(), i
        orbit[i] = o[i].astype(np.uint64)
    return {"orbit": orbit, "cycles4": cyc.astype(np.uint64), "cliques4": clq.astype(np.uint64), "sup": sup, "total": totals(orbit)}


def ordered_items(nv, eu, ev):
    """sum over v, over the neighbours u of v below v in (d, id) order, of the neighbours of u below v"""
    adj = _adj(nv, eu, ev)
    order = sorted(range(nv), key=lambda v: (len(adj[v]), v))
    rank = [0] * nv
    for i, v in enumerate(order):
        rank[v] = i
    rows = [sorted(rank[w] for w in adj[v]) for v in range(nv)]
    items = 0
    for v in range(nv):
        r = rank[v]
        for u in adj[v]:
            if rank[u] < r:
                items += bisect_left(rows[u], r)
    return items
