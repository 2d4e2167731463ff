"""Restatement of the (3,4)-nucleus decomposition of include/komb_accel.h in plain Python: adjacency sets -> triangles ->
4-cliques -> a level peel without buckets.  It shares no code with the library; tests/test_nucleus_ref.py checks it against a
brute force that shares nothing with IT (no incidence lists, no decrements).

Input everywhere: nv and the canonical edges eu[i] < ev[i] sorted by (eu, ev) of a k-truss result (any simple edge list is
accepted: it is canonicalised first)."""
import numpy as np


def canonical(edges):
    """The distinct edges as sorted (u, v) pairs with u < v."""
    return sorted({(min(int(u), int(v)), max(int(u), int(v))) for u, v in edges if int(u) != int(v)})


def decompose(nv, eu, ev):
    """dict: a, b, c, key0, theta (int32[n_triangles], triangle order), edge_theta (int32[len(eu)], the order of the input
    edges), vertex_theta (int32[nv]), cliques (list of 4-tuples of triangle ids), levels (the distinct theta, ascending),
    subrounds (frontiers per level, same order) and info (what komb_nucleus_info reports except n_subrounds and ms)."""
    edges = [(int(u), int(v)) for u, v in zip(eu, ev)]
    assert edges == canonical(edges), "canonical edges expected"
    up = [set() for _ in range(nv)]                       # neighbours above the vertex
    for u, v in edges:
        up[u].add(v)
    tris, tid = [], {}
    for a, b in edges:                                    # ascending (a, b); c ascending inside: triangle order
        for c in sorted(up[a] & up[b]):
            tid[(a, b, c)] = len(tris)
            tris.append((a, b, c))
    cliques = []
    for t, (a, b, c) in enumerate(tris):
        for d in sorted(up[a] & up[b] & up[c]):
            cliques.append((t, tid[(a, b, d)], tid[(a, c, d)], tid[(b, c, d)]))
    n = len(tris)
    inc = [[] for _ in range(n)]
    for q, mem in enumerate(cliques):
        for t in mem:
            inc[t].append(q)
    key0 = np.asarray([len(x) for x in inc], dtype=np.int64).reshape(n)
    key = key0.copy()
    theta = np.full(n, -1, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    gone = [False] * len(cliques)
    levels, subrounds = [], []
    while alive.any():
        k = int(key[alive].min())
        frontier = np.flatnonzero(alive & (key <= k)).tolist()
        levels.append(k)
        rounds = 0
        while frontier:
            rounds += 1
            for t in frontier:                            # the stamp first: a frontier member takes no decrement
                theta[t] = k
                alive[t] = False
            nxt = []
            for t in frontier:
                for q in inc[t]:
                    if gone[q]:
                        continue
                    gone[q] = True
                    for u in cliques[q]:
                        if alive[u]:
                            key[u] -= 1
                            if key[u] == k:
                                nxt.append(u)
            frontier = nxt
        subrounds.append(rounds)
    pos = {e: i for i, e in enumerate(edges)}
    edge_theta = np.full(len(edges), -1, dtype=np.int64)
    vertex_theta = np.full(nv, -1, dtype=np.int64)
    for (a, b, c), th in zip(tris, theta.tolist()):
        for e in ((a, b), (a, c), (b, c)):
            edge_theta[pos[e]] = max(edge_theta[pos[e]], th)
        for v in (a, b, c):
            vertex_theta[v] = max(vertex_theta[v], th)
    t3 = np.asarray(tris, dtype=np.int32).reshape(n, 3)
    return {"a": t3[:, 0].copy(), "b": t3[:, 1].copy(), "c": t3[:, 2].copy(), "key0": key0.astype(np.int32), "theta": theta.astype(np.int32),
            "edge_theta": edge_theta.astype(np.int32), "vertex_theta": vertex_theta.astype(np.int32), "cliques": cliques,
            "levels": levels, "subrounds": subrounds,
            "info": {"n_triangles": n, "n_cliques4": len(cliques), "theta_max": int(theta.max()) if n else -1, "n_levels": len(levels)}}


def decompose_edges(nv, edges):
    """decompose() of any simple edge list."""
    e = canonical(edges)
    return decompose(nv, [u for u, _ in e], [v for _, v in e])


# ---- graphs

def clique(ids):
    ids = [int(x) for x in ids]
    return [(ids[i], ids[j]) for i in range(len(ids)) for j in range(i + 1, len(ids))]


def hand_cases():
    """(name, nv, edges, n_triangles, n_cliques4, sorted theta counts {theta: triangles}) of the graphs worked out by hand."""
    out = []
    for n, th in ((3, 0), (4, 1), (5, 2), (6, 3), (12, 9)):
        nt = n * (n - 1) * (n - 2) // 6
        out.append(("K_%d" % n, n, clique(range(n)), nt, nt * (n - 3) // 4, {th: nt}))
    out.append(("K_6 and a vertex on three of its vertices", 7, clique(range(6)) + [(6, 0), (6, 1), (6, 2)], 23, 16, {1: 3, 3: 20}))
    parts = [(0, 1), (2, 3), (4, 5), (6, 7)]
    k2222 = [(u, v) for i, p in enumerate(parts) for q in parts[i + 1:] for u in p for v in q]
    out.append(("K_2,2,2,2", 8, k2222, 32, 16, {2: 32}))
    wheel = [(0, i) for i in range(1, 9)] + [(i, i % 8 + 1) for i in range(1, 9)]
    out.append(("wheel W_8", 9, wheel, 8, 0, {0: 8}))
    out.append(("two K_5 sharing a triangle", 7, clique([0, 1, 2, 3, 4]) + clique([0, 1, 2, 5, 6]), 19, 10, {2: 19}))
    return out


def hand_graph():
    """One graph with several levels: a K_7, a K_5 sharing an edge with it, a K_4 hanging on a K_5 vertex, a lone triangle,
    a pendant path.  15 vertices."""
    edges = clique(range(7)) + clique([5, 6, 7, 8, 9]) + clique([9, 10, 11, 12]) + [(12, 13), (13, 14), (12, 14), (14, 3)]
    return 15, edges


def clique_union(nv, n_cliques, lo, hi, seed):
    """A seeded union of n_cliques random cliques of lo..hi vertices on nv vertices."""
    rng = np.random.default_rng(seed)
    edges = []
    for _ in range(n_cliques):
        edges += clique(rng.choice(nv, size=int(rng.integers(lo, hi + 1)), replace=False))
    return canonical(edges)
