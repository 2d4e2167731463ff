"""Restatement of the clique census of include/komb_accel.h in plain Python: the number of k-cliques for every k of a window and
the k_local-cliques through every vertex, by pivoting (Jain and Seshadhri, WSDM 2020) with Python ints as bit sets and as
counts, saturated at 2^64 - 1 at the very end.  It shares no code with the library and not its decomposition either: the library
roots a clique at the edge of its two smallest ids, cuts the candidates by trussness and walks an explicit stack, this recursion
starts from the whole vertex set, holds nothing at the start and knows trussness only as t_max.
tests/test_clique_census_ref.py checks it against networkx.enumerate_all_cliques and the closed forms.

Input: nv and the canonical edges eu[i] < ev[i] sorted by (eu, ev) of a k-truss result."""
import sys
from math import comb

import numpy as np

from max_clique_ref import cocktail_party, trussness  # noqa: F401  (the peel is the restatements' own; CP(m) for the tests)

COMPLETE, SATURATED = 1, 2
SAT = 2 ** 64 - 1


def census(nv, eu, ev, k_lo=2, k_hi=-1, k_local=0, truss=None):
    """truss: the trussness of the edges where the caller has it (a K_515 is beyond the peel), else it is computed here.
    dict: k_lo, k_hi (as used), k_local, t_max, omega, flags, total (uint64[k_hi - k_lo + 1]), local (uint64[nv] or None) and
    exact, the same two as Python ints before saturation.  ValueError for arguments the library answers KOMB_ERR_ARG."""
    edges = [(int(u), int(v)) for u, v in zip(eu, ev)]
    assert all(u < v for u, v in edges) and edges == sorted(set(edges)), "canonical edges expected"
    t_max = 0
    if edges:
        t_max = int(max(truss)) if truss is not None else max(trussness(nv, eu, ev))
    if k_lo < 2 or (k_hi != -1 and k_hi < k_lo) or k_local < 0:
        raise ValueError("bad window")
    if k_hi == -1 or k_hi > t_max:
        k_hi = max(t_max, k_lo)
    if k_local and not k_lo <= k_local <= k_hi:
        raise ValueError("k_local outside the window")
    adj = [0] * nv
    everything = 0
    for u, v in edges:
        adj[u] |= 1 << v
        adj[v] |= 1 << u
        everything |= (1 << u) | (1 << v)
    total = [0] * (k_hi + 1)
    local = [0] * nv

    def bits(S):
        while S:
            low = S & -S
            yield low.bit_length() - 1
            S ^= low

    def node(S, held, pivots):
        h, p = len(held), len(pivots)
        if h > k_hi or h + p + bin(S).count("1") < k_lo:
            return
        if not S:
            for k in range(max(k_lo, h), min(k_hi, h + p) + 1):
                total[k] += comb(p, k - h)
            if k_local and h <= k_local <= h + p:
                for v in held:
                    local[v] += comb(p, k_local - h)
                if k_local > h:
                    for v in pivots:
                        local[v] += comb(p - 1, k_local - h - 1)
            return
        u = max(bits(S), key=lambda x: (bin(S & adj[x]).count("1"), -x))
        node(S & adj[u], held, pivots + [u])
        for v in bits(S & ~adj[u] & ~(1 << u)):
            S &= ~(1 << v)
            node(S & adj[v], held + [v], pivots)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 2 * nv + 1000))
    try:
        node(everything, [], [])
    finally:
        sys.setrecursionlimit(limit)
    window = total[k_lo:k_hi + 1]
    out_local = local if k_local else None
    sat = any(x >= SAT for x in window) or (k_local and any(x >= SAT for x in local))
    return {"k_lo": k_lo, "k_hi": k_hi, "k_local": k_local, "t_max": t_max,
            "omega": max([k for k in range(k_lo, k_hi + 1) if total[k]], default=0),
            "flags": COMPLETE | (SATURATED if sat else 0),
            "total": np.asarray([min(x, SAT) for x in window], dtype=np.uint64),
            "local": np.asarray([min(x, SAT) for x in local], dtype=np.uint64) if k_local else None,
            "exact": (window, out_local)}


def census_edges(nv, edges, **kw):
    """census() of any simple edge list."""
    e = sorted({(min(int(u), int(v)), max(int(u), int(v))) for u, v in edges if int(u) != int(v)})
    return census(nv, [u for u, _ in e], [v for _, v in e], **kw)
