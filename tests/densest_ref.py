"""CPU restatement of komb_densest_subgraph_run (include/komb_accel.h): the core density profile, the prune, the integer
Frank-Wolfe rounds, the prefix extraction and the certificate, in numpy and Python integers -- every comparison of two
densities is a cross-multiplication of integers.  Plus the exact optimum by enumeration for graphs of up to 14 vertices."""
import numpy as np

SOURCE_CORE, SOURCE_PREFIX = 0, 1
LOAD_WORD_MAX = 2 ** 31 - 1
INFO_FIELDS = ("source", "k_best", "k_prune", "n_pruned", "m_pruned", "n_sub", "m_sub", "load_max", "iters", "k_max")


class LimitError(ValueError):
    """iters * (largest degree inside P) does not fit the 32-bit load word: the library answers KOMB_ERR_LIMIT."""


def edges_of_csr(rowptr, col):
    """(u, v) int64 arrays of the undirected edges of a symmetric CSR, u < v, in row order."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    src = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    keep = col > src
    return src[keep], col[keep]


def csr_of_edges(nv, uv):
    """Simple symmetric row-sorted CSR of raw pairs (loops and parallel edges dropped)."""
    uv = np.asarray(uv, np.int64).reshape(-1, 2)
    uv = uv[uv[:, 0] != uv[:, 1]]
    both = np.unique(np.concatenate([uv, uv[:, ::-1]]), axis=0) if len(uv) else np.zeros((0, 2), np.int64)
    rowptr = np.zeros(nv + 1, np.int64)
    np.add.at(rowptr, both[:, 0] + 1, 1)
    return np.cumsum(rowptr), both[:, 1].astype(np.int32)


def coreness(rowptr, col):
    """k-core numbers by the textbook peel (small graphs: the CPU tests have no library result to take them from)."""
    rowptr = np.asarray(rowptr, np.int64)
    nv = len(rowptr) - 1
    deg = np.diff(rowptr).astype(np.int64)
    core = np.zeros(nv, np.int32)
    alive = np.ones(nv, bool)
    k = 0
    for _ in range(nv):
        live = np.flatnonzero(alive)
        v = live[np.argmin(deg[live])]
        k = max(k, int(deg[v]))
        core[v] = k
        alive[v] = False
        for w in col[rowptr[v]:rowptr[v + 1]]:
            if alive[w]:
                deg[w] -= 1
    return core


def _best(cands):
    """cands: (m, n, order) with n >= 1; the largest m / n, ties to the largest order."""
    best = None
    for m, n, o in cands:
        if best is None or m * best[1] > best[0] * n or (m * best[1] == best[0] * n and o > best[2]):
            best = (m, n, o)
    return best


def densest(rowptr, col, core, iters):
    """Everything the ABI returns: {"member", "load": int32[nv]; "n_k", "m_k": int64[k_max + 1]; the INFO_FIELDS}."""
    if iters < 0:
        raise ValueError("iters < 0")
    core = np.asarray(core, np.int64)
    nv = len(core)
    out = {"member": np.zeros(nv, np.int32), "load": np.zeros(nv, np.int32), "iters": int(iters)}
    if nv == 0:
        out.update(n_k=np.zeros(1, np.int64), m_k=np.zeros(1, np.int64), source=SOURCE_CORE, k_best=0, k_prune=0, n_pruned=0,
                   m_pruned=0, n_sub=0, m_sub=0, load_max=0, k_max=0)
        return out
    eu, ev = edges_of_csr(rowptr, col)
    k_max = int(core.max())
    # 1. the core density profile
    vh = np.bincount(core, minlength=k_max + 1)
    eh = np.bincount(np.minimum(core[eu], core[ev]), minlength=k_max + 1)
    n_k = np.cumsum(vh[::-1])[::-1].astype(np.int64)
    m_k = np.cumsum(eh[::-1])[::-1].astype(np.int64)
    m_s, n_s, k_s = _best((int(m_k[k]), int(n_k[k]), k) for k in range(k_max + 1))
    # 2. the prune
    c = -(-m_s // n_s)
    in_p = core >= c
    pid = np.cumsum(in_p) - 1
    keep = in_p[eu] & in_p[ev]
    pu, pv = pid[eu[keep]], pid[ev[keep]]           # dense ids keep the order of the original ids: pu < pv
    n_p, m_p = int(in_p.sum()), int(keep.sum())
    deg_p = np.bincount(np.concatenate([pu, pv]), minlength=n_p) if m_p else np.zeros(n_p, np.int64)
    if iters * (int(deg_p.max()) if n_p else 0) > LOAD_WORD_MAX:
        raise LimitError("iters * degree exceeds the load word")
    # 3. the rounds
    load = np.zeros(n_p, np.int64)
    for t in range(iters if m_p else 0):
        lu, lv = load[pu], load[pv]
        to_u = (lu < lv) | ((lu == lv) & (t % 2 == 0))
        load = load + np.bincount(np.where(to_u, pu, pv), minlength=n_p)
    # 4. the best prefix of (load descending, id ascending)
    source, members = SOURCE_CORE, core >= k_s
    n_sub, m_sub = n_s, m_s
    if iters >= 1 and m_p:
        order = np.lexsort((np.arange(n_p), -load))
        rank = np.empty(n_p, np.int64)
        rank[order] = np.arange(n_p)
        m_i = np.cumsum(np.bincount(np.maximum(rank[pu], rank[pv]), minlength=n_p))
        bm, bi, _ = _best((int(m_i[i - 1]), i, -i) for i in range(1, n_p + 1))
        # 5. the prefix only when it is strictly denser than the best core
        if bm * n_s > m_s * bi:
            source, n_sub, m_sub = SOURCE_PREFIX, bi, bm
            members = np.zeros(nv, bool)
            members[np.flatnonzero(in_p)[order[:bi]]] = True
    out["member"] = members.astype(np.int32)
    out["load"][in_p] = load
    out.update(n_k=n_k, m_k=m_k, source=source, k_best=k_s, k_prune=c, n_pruned=n_p, m_pruned=m_p, n_sub=n_sub, m_sub=m_sub,
               load_max=int(load.max()) if n_p else 0, k_max=k_max)
    return out


def edges_inside(rowptr, col, member):
    eu, ev = edges_of_csr(rowptr, col)
    member = np.asarray(member).astype(bool)
    return int((member[eu] & member[ev]).sum())


def brute_force_optimum(rowptr, col):
    """(m, n) of a densest subgraph by enumerating every non-empty vertex set; nv <= 14."""
    nv = len(rowptr) - 1
    assert 1 <= nv <= 14
    eu, ev = edges_of_csr(rowptr, col)
    masks = np.arange(1, 1 << nv, dtype=np.int64)
    m = np.zeros(len(masks), np.int64)
    for u, v in zip(eu.tolist(), ev.tolist()):
        m += ((masks >> u) & (masks >> v) & 1)
    n = np.zeros(len(masks), np.int64)
    for b in range(nv):
        n += (masks >> b) & 1
    best = (0, 1)
    for mm, nn in set(zip(m.tolist(), n.tolist())):
        if mm * best[1] > best[0] * nn:
            best = (mm, nn)
    return best


def constructed_graph():
    """K_6 on 0..5, vertex 6 joined to {0, 1, 2}, vertex 7 to {1, 2, 3}, and 20 disjoint K_4: (nv, raw pairs)."""
    uv = [[a, b] for a in range(6) for b in range(a + 1, 6)] + [[6, 0], [6, 1], [6, 2], [7, 1], [7, 2], [7, 3]]
    for q in range(20):
        o = 8 + 4 * q
        uv += [[o + a, o + b] for a in range(4) for b in range(a + 1, 4)]
    return 88, np.asarray(uv, np.int64)
