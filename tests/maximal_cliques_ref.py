"""Restatement of the maximal-clique enumeration of include/komb_accel.h in plain Python: Bron-Kerbosch with pivoting over the
whole vertex set, Python ints as bit sets.  It shares no code with the library and not its decomposition either: the library
roots a clique at the edge of its two smallest ids, cuts candidates and excluded vertices by trussness and walks an explicit
stack; this recursion has no roots, no trussness filter (k_min only decides what is reported) and knows trussness only as t_max.
tests/test_maximal_cliques_ref.py checks it against networkx.find_cliques and the closed forms.

Input: nv and the canonical edges eu[i] < ev[i] sorted by (eu, ev) of a k-truss result."""
import sys

import numpy as np

from max_clique_ref import cocktail_party, trussness  # noqa: F401  (the peel is the restatements' own; CP(m) for the tests)

COMPLETE, LISTED = 1, 2


def complete_multipartite(parts):
    """(nv, edges) of the complete multipartite graph with the given part sizes, vertices numbered part by part."""
    part = [i for i, n in enumerate(parts) for _ in range(n)]
    nv = len(part)
    return nv, [(u, v) for u in range(nv) for v in range(u + 1, nv) if part[u] != part[v]]


def _count(x):
    return bin(x).count("1")


def solve(nv, eu, ev, k_min=2, pivot="max", list_cap=None, truss=None):
    """truss: the trussness of the edges where the caller has it (a K_515 is beyond the peel), else it is computed here.
    dict: k_min, k_hi, t_max, omega, flags, n_cliques, hist (int64[k_hi - k_min + 1]), count and largest (int32[nv]), cliques
    (every maximal clique of >= k_min vertices as an ascending tuple, sorted; None without LISTED) and nodes, the calls of this
    recursion (the contract fixes no node count).  ValueError for a k_min the library answers KOMB_ERR_ARG."""
    edges = [(int(u), int(v)) for u, v in zip(eu, ev)]
    assert all(u < v for u, v in edges) and edges == sorted(set(edges)), "canonical edges expected"
    if k_min < 2:
        raise ValueError("bad k_min")
    t_max = 0
    if edges:
        t_max = int(max(truss)) if truss is not None else max(trussness(nv, eu, ev))
    k_hi = max(k_min, t_max)
    adj = [0] * nv
    everything = 0
    for u, v in edges:
        adj[u] |= 1 << v
        adj[v] |= 1 << u
        everything |= (1 << u) | (1 << v)
    found = []
    state = {"nodes": 0}

    def bits(S):
        while S:
            low = S & -S
            yield low.bit_length() - 1
            S ^= low

    def node(P, X, held):
        state["nodes"] += 1
        if not P:
            if not X and len(held) >= k_min:
                found.append(tuple(sorted(held)))
            return
        n_p = _count(P)
        if len(held) + n_p < k_min:
            return
        if pivot == "first":
            u = (P & -P).bit_length() - 1
        else:
            u, best = -1, -1
            for x in bits(P | X):
                c = _count(P & adj[x])
                if c > best:
                    u, best = x, c
                    if c >= n_p - 1:                      # (no vertex of P does better, and one of X could only close the node)
                        break
        for v in bits(P & ~adj[u]):
            node(P & adj[v], X & adj[v], held + [v])
            P &= ~(1 << v)
            X |= 1 << v

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 2 * nv + 1000))
    try:
        if everything:
            node(everything, 0, [])
    finally:
        sys.setrecursionlimit(limit)
    found.sort()
    assert len(set(found)) == len(found)
    hist = np.zeros(k_hi - k_min + 1, np.int64)
    count = np.zeros(nv, np.int32)
    largest = np.zeros(nv, np.int32)
    for c in found:
        hist[len(c) - k_min] += 1
        for v in c:
            count[v] += 1
            largest[v] = max(largest[v], len(c))
    listed = list_cap is None or len(found) <= list_cap
    return {"k_min": k_min, "k_hi": k_hi, "t_max": t_max, "omega": max((len(c) for c in found), default=0),
            "flags": COMPLETE | (LISTED if listed else 0), "n_cliques": len(found), "hist": hist, "count": count, "largest": largest,
            "cliques": found if listed else None, "nodes": state["nodes"]}


def solve_edges(nv, edges, **kw):
    """solve() of any simple edge list."""
    e = sorted({(min(int(u), int(v)), max(int(u), int(v))) for u, v in edges if int(u) != int(v)})
    return solve(nv, [u for u, _ in e], [v for _, v in e], **kw)
