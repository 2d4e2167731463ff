"""Restatement of the maximum-clique search of include/komb_accel.h in plain Python, with Python ints as bit sets: omega by a
branch and bound over a greedy colouring, then every maximum clique by the same recursion with the prune relaxed by one, the
per-vertex counts, the sorted list and t_max (a trussness peel of its own).  It shares no code with the library and not its
decomposition either: the library roots a clique at the edge of its two smallest ids and evaluates one candidate set at a time,
this recursion works on the whole vertex set in colour order.  tests/test_max_clique_ref.py checks it against
networkx.find_cliques.

Input: nv and the canonical edges eu[i] < ev[i] sorted by (eu, ev) of a k-truss result.  A NODE here is one call of the
recursion; the node counts are this restatement's own (the contract fixes what a budget that ran out means, not the count)."""
import heapq

import numpy as np

EXACT, ENUMERATED, LISTED = 1, 2, 4


class _Spent(Exception):
    pass


def trussness(nv, eu, ev):
    """Trussness (support + 2 convention: K_n gives n) of every edge, in the order of the input."""
    edges = [(int(u), int(v)) for u, v in zip(eu, ev)]
    adj = [set() for _ in range(nv)]
    for u, v in edges:
        adj[u].add(v)
        adj[v].add(u)
    index = {e: i for i, e in enumerate(edges)}
    sup = [len(adj[u] & adj[v]) for u, v in edges]
    heap = [(s, i) for i, s in enumerate(sup)]
    heapq.heapify(heap)
    truss = [0] * len(edges)
    k = 2
    while heap:
        s, i = heapq.heappop(heap)
        if truss[i] or s != sup[i]:
            continue
        k = max(k, s + 2)
        truss[i] = k
        u, v = edges[i]
        adj[u].discard(v)
        adj[v].discard(u)
        for w in adj[u] & adj[v]:
            for x, y in ((u, w), (v, w)):
                j = index[(x, y) if x < y else (y, x)]
                sup[j] -= 1
                heapq.heappush(heap, (sup[j], j))
    return truss


def _colour(P, adj):
    """The vertices of P in the order a sequential greedy colouring takes them, with their colours (ascending)."""
    order = []
    k = 0
    U = P
    while U:
        k += 1
        Q = U
        while Q:
            v = (Q & -Q).bit_length() - 1
            bit = 1 << v
            U &= ~bit
            Q &= ~(adj[v] | bit)
            order.append((v, k))
    return order


def solve(nv, eu, ev, budget=None, list_cap=None, truss=None):
    """truss: the trussness of the edges where the caller has it (a K_515 is beyond the peel above), else it is computed here.
    dict: omega, upper, flags, t_max, n_max_cliques, count (int32[nv]), cliques (every maximum clique as an ascending
    tuple, sorted; None without LISTED), witness (cliques[0] with LISTED, else the clique held), nodes."""
    edges = [(int(u), int(v)) for u, v in zip(eu, ev)]
    assert all(u < v for u, v in edges) and edges == sorted(set(edges)), "canonical edges expected"
    out = {"omega": 0, "upper": 0, "flags": EXACT | ENUMERATED | LISTED, "t_max": 0, "n_max_cliques": 0,
           "count": np.zeros(nv, np.int32), "cliques": [], "witness": (), "nodes": 0}
    if not edges:
        return out
    t_max = int(max(truss)) if truss is not None else max(trussness(nv, eu, ev))
    adj = [0] * nv
    for u, v in edges:
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    state = {"best": 1, "witness": (), "nodes": 0, "found": []}

    def node():
        if budget is not None and state["nodes"] >= budget:
            raise _Spent()
        state["nodes"] += 1

    def search(P, chosen):
        node()
        for v, k in reversed(_colour(P, adj)):
            if len(chosen) + k <= state["best"]:
                return
            rest = P & adj[v]
            if rest:
                search(rest, chosen + [v])
            elif len(chosen) + 1 > state["best"]:
                state["best"] = len(chosen) + 1
                state["witness"] = tuple(sorted(chosen + [v]))
            P &= ~(1 << v)

    def enumerate_all(P, chosen, omega):
        node()
        for v, k in reversed(_colour(P, adj)):
            if len(chosen) + k < omega:
                return
            rest = P & adj[v]
            if rest:
                enumerate_all(rest, chosen + [v], omega)
            elif len(chosen) + 1 == omega:
                state["found"].append(tuple(sorted(chosen + [v])))
            P &= ~(1 << v)

    everything = 0
    for u, v in edges:
        everything |= (1 << u) | (1 << v)
    out["t_max"] = t_max
    try:
        search(everything, [])
    except _Spent:
        pass
    else:
        out["flags"] = EXACT
    if not state["witness"]:                              # (the budget ran out before the first leaf: an edge is a clique)
        state["witness"] = edges[0]
    omega = len(state["witness"])
    exact = out["flags"] == EXACT or omega == t_max
    out.update(omega=omega, witness=state["witness"], upper=omega if exact else t_max, flags=EXACT if exact else 0,
               n_max_cliques=-1, cliques=None)
    enumerated = False
    if exact and not (budget is not None and state["nodes"] >= budget):
        try:
            enumerate_all(everything, [], omega)
            enumerated = True
        except _Spent:
            pass
    out["nodes"] = state["nodes"]
    if not enumerated:
        for v in out["witness"]:
            out["count"][v] = 1
        return out
    found = sorted(state["found"])
    assert len(set(found)) == len(found) and found
    out["flags"] |= ENUMERATED
    out["n_max_cliques"] = len(found)
    for c in found:
        for v in c:
            out["count"][v] += 1
    if list_cap is None or len(found) <= list_cap:
        out["flags"] |= LISTED
        out["cliques"] = found
        out["witness"] = found[0]
    return out


def solve_edges(nv, edges, **kw):
    """solve() of any simple edge list."""
    e = sorted({(min(int(u), int(v)), max(int(u), int(v))) for u, v in edges if int(u) != int(v)})
    return solve(nv, [u for u, _ in e], [v for _, v in e], **kw)


def cocktail_party(m):
    """CP(m): 2 m vertices, 2 i and 2 i + 1 not adjacent, every other pair adjacent."""
    return 2 * m, [(u, v) for u in range(2 * m) for v in range(u + 1, 2 * m) if u // 2 != v // 2]
