"""The betweenness centrality of include/komb_accel.h (komb_betweenness_run) restated in plain Python floats, operation by
operation: per source a BFS with sorted levels, sigma summed over the row in ascending id, delta summed over the row in ascending
id with the division, the product and the addition rounded one after the other, bc summed over the sources in the order given.
Python's float is IEEE-754 binary64 and +, * and / round once each, so the result is the definition's, bit for bit.

Two switches make a deliberately DIFFERENT result, for the tests that show a fixture can tell the difference:
fused=True replaces acc + sigma * c by one exactly rounded fused operation (through fractions.Fraction), what a compiler does
when it contracts the two into a fused multiply-add; descending=True walks every row backwards."""
from fractions import Fraction

import numpy as np

ROUNDED = 1
TWO53 = 2.0 ** 53
INF = float("inf")


class Limit(Exception):
    """a sigma reached +inf: KOMB_ERR_LIMIT"""


def adjacency(nv, pairs):
    """The rows of the simple undirected graph of `pairs` (self loops and repeats dropped), ascending."""
    adj = [set() for _ in range(nv)]
    for u, v in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        if u != v:
            adj[u].add(v); adj[v].add(u)
    return [sorted(a) for a in adj]


def rows_of_csr(rowptr, col):
    return [[int(x) for x in col[rowptr[v]:rowptr[v + 1]]] for v in range(len(rowptr) - 1)]


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def one_source(rows, s, fused=False, descending=False):
    """(dist, sigma, delta, levels) of source s; dist[v] = -1 for an unreached vertex.  Raises Limit."""
    nv = len(rows)
    walk = (lambda v: reversed(rows[v])) if descending else (lambda v: rows[v])
    dist, sigma, delta = [-1] * nv, [0.0] * nv, [0.0] * nv
    dist[s], sigma[s] = 0, 1.0
    levels = [[s]]
    while True:
        L = len(levels)
        nxt = sorted({w for v in levels[-1] for w in rows[v] if dist[w] < 0})
        if not nxt:
            break
        for w in nxt:
            acc = 0.0
            for v in walk(w):
                if dist[v] == L - 1:
                    acc = acc + sigma[v]
            sigma[w] = acc
        for w in nxt:
            dist[w] = L
            if sigma[w] == INF:
                raise Limit(s)
        levels.append(nxt)
    for L in range(len(levels) - 1, -1, -1):
        for v in levels[L]:
            acc = 0.0
            for w in walk(v):
                if dist[w] == L + 1:
                    c = (1.0 + delta[w]) / sigma[w]
                    if fused:
                        acc = _fma(sigma[v], c, acc)
                    else:
                        p = sigma[v] * c
                        acc = acc + p
            delta[v] = acc
    return dist, sigma, delta, levels


def betweenness(rows, sources=None, fused=False, descending=False, cache=None):
    """What komb_betweenness_run / _fetch / _fetch_sources / _info give for the rows (ascending adjacency lists) and the sources
    (None: all): {"bc", "source", "n_reached", "sum_dist", "ecc", "flags", "depth_max", "n_sources", "n_batches",
    "n_level_steps"}.  Raises Limit where the library answers KOMB_ERR_LIMIT.  cache: a dict that keeps the search of every
    source vertex between calls on the same rows (bc is still summed entry by entry in the order given)."""
    nv = len(rows)
    src = list(range(nv)) if sources is None else [int(s) for s in sources]
    assert all(0 <= s < nv for s in src)
    cache = {} if cache is None else cache
    bc = [0.0] * nv
    reached, sumd, ecc, flags = [], [], [], 0
    for s in src:
        if (s, fused, descending) not in cache:
            dist, sigma, delta, levels = one_source(rows, s, fused, descending)
            cache[s, fused, descending] = (delta, sum(len(l) for l in levels), sum(L * len(l) for L, l in enumerate(levels)), len(levels) - 1,
                                           any(sigma[v] >= TWO53 for l in levels for v in l))
        delta, n, total, depth, rounded = cache[s, fused, descending]
        for v in range(nv):
            if v != s:
                bc[v] = bc[v] + delta[v]
        reached.append(n)
        sumd.append(total)
        ecc.append(depth)
        if rounded:
            flags |= ROUNDED
    batches = [ecc[i:i + 64] for i in range(0, len(src), 64)]
    steps = sum((max(b) + 1) + max(max(b) - 1, 0) for b in batches) if nv > 0 else 0
    return {"bc": np.asarray(bc, dtype=np.float64), "source": np.asarray(src, dtype=np.int32), "n_reached": np.asarray(reached, dtype=np.int64),
            "sum_dist": np.asarray(sumd, dtype=np.int64), "ecc": np.asarray(ecc, dtype=np.int32), "flags": flags,
            "depth_max": max(ecc, default=0), "n_sources": len(src), "n_batches": len(batches), "n_level_steps": steps}


def diamond_chain(k):
    """k diamonds in a row, 3 k + 1 vertices: joint i is vertex 3 i, and 3 i + 1, 3 i + 2 lie between joints i and i + 1.  The
    number of shortest paths from end to end is 2^k."""
    pairs = []
    for i in range(k):
        a, b = 3 * i, 3 * i + 3
        pairs += [(a, a + 1), (a, a + 2), (a + 1, b), (a + 2, b)]
    return 3 * k + 1, np.asarray(pairs, dtype=np.int64)


def layered(layers, width=16):
    """An apex (vertex 0) above `layers` layers of `width` vertices, consecutive layers joined completely: sigma from the apex
    is width^(l - 1) on layer l, so with width 16 it is finite up to layer 256 and +inf on layer 257."""
    pairs = [(0, 1 + j) for j in range(width)]
    for l in range(1, layers):
        a, b = 1 + (l - 1) * width, 1 + l * width
        pairs += [(a + i, b + j) for i in range(width) for j in range(width)]
    return 1 + layers * width, np.asarray(pairs, dtype=np.int64)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def sample_sources(nv, n, seed=1):
    """komb2's KOMB_BETWEENNESS=<n>[:<seed>]: the n vertices with the smallest splitmix64(seed ^ vid), ties by id, ascending."""
    if n >= nv:
        return list(range(nv))
    return sorted(sorted(range(nv), key=lambda v: (splitmix64(seed ^ v), v))[:n])
