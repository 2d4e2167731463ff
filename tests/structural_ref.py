"""CPU restatement of komb_structural_clusters_run for the tests (include/komb_accel.h has the definition): numpy, scipy's
connected components through components_ref.min_labels, Python integers for the similarity test wherever int64 could
overflow.  No GPU, no product code."""
import numpy as np

import components_ref as CR

OUTLIER, HUB, BORDER, CORE = 0, 1, 2, 3


def similar_edges(d, eu, ev, sup, eps_num, eps_den):
    """similar[i] of (sup+2)^2 eps_den^2 >= eps_num^2 (d(u)+1) (d(v)+1), exactly: int64 when both sides are proved to fit,
    Python integers otherwise."""
    s = np.asarray(sup, np.int64) + 2
    a = d[eu] + 1
    b = d[ev] + 1
    if len(s) == 0:
        return np.zeros(0, bool)
    lim = 2 ** 62
    if int(s.max()) ** 2 * eps_den ** 2 < lim and eps_num ** 2 * int(a.max()) * int(b.max()) < lim:
        return s * s * (eps_den * eps_den) >= (eps_num * eps_num) * a * b
    return np.fromiter(((int(x) ** 2) * eps_den ** 2 >= eps_num ** 2 * int(y) * int(z) for x, y, z in zip(s.tolist(), a.tolist(), b.tolist())),
                       bool, len(s))


def clusters(nv, eu, ev, sup, eps_num, eps_den, mu):
    """{"similar", "sim_deg", "label", "size", "role"} (int64 arrays; similar 0 | 1) and "info", the dict of
    komb_structural_clusters_info without ms, of the result edges (eu, ev) with supports sup on nv vertices."""
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    d = np.bincount(eu, minlength=nv) + np.bincount(ev, minlength=nv) if nv else np.zeros(0, np.int64)
    d = d.astype(np.int64)
    sim = similar_edges(d, eu, ev, sup, eps_num, eps_den)
    su, sv = eu[sim], ev[sim]
    sim_deg = (np.bincount(su, minlength=nv) + np.bincount(sv, minlength=nv)).astype(np.int64) if nv else np.zeros(0, np.int64)
    core = sim_deg + 1 >= mu
    cc = core[su] & core[sv]
    label = CR.min_labels(nv, su[cc], sv[cc], core)
    # borders: the smallest label among the cores at the other end of a similar edge
    best = np.full(nv, nv, np.int64)
    for a, b in ((su, sv), (sv, su)):
        sel = core[a] & ~core[b]
        np.minimum.at(best, b[sel], label[a[sel]])
    border = ~core & (best < nv)
    label[border] = best[border]
    # hubs: two differently labelled neighbours over any edge
    lo, hi = np.full(nv, nv, np.int64), np.full(nv, -1, np.int64)
    for a, b in ((eu, ev), (ev, eu)):
        sel = label[a] >= 0
        np.minimum.at(lo, b[sel], label[a[sel]])
        np.maximum.at(hi, b[sel], label[a[sel]])
    role = np.zeros(nv, np.int64)
    role[core] = CORE
    role[border] = BORDER
    role[(label < 0) & (hi >= 0) & (lo != hi)] = HUB
    size = CR.sizes(label)
    roots = label == np.arange(nv)
    info = {"eps_num": eps_num, "eps_den": eps_den, "mu": mu, "n_similar_edges": int(sim.sum()), "n_cores": int(core.sum()),
            "n_borders": int(border.sum()), "n_hubs": int((role == HUB).sum()), "n_outliers": int((role == OUTLIER).sum()),
            "n_clusters": int(roots.sum()), "largest": int(size[roots].max()) if roots.any() else 0}
    return {"similar": sim.astype(np.int64), "sim_deg": sim_deg, "label": label, "size": size, "role": role, "info": info}


def multi_borders(nv, eu, ev, out):
    """The borders with similar edges into more than one cluster."""
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    sim = out["similar"].astype(bool)
    core = out["role"] == CORE
    lo, hi = np.full(nv, nv, np.int64), np.full(nv, -1, np.int64)
    for a, b in ((eu[sim], ev[sim]), (ev[sim], eu[sim])):
        sel = core[a] & ~core[b]
        np.minimum.at(lo, b[sel], out["label"][a[sel]])
        np.maximum.at(hi, b[sel], out["label"][a[sel]])
    return int(((hi >= 0) & (lo != hi)).sum())


def supports(nv, eu, ev):
    """sup[i] = common neighbours of the ends of edge i in the graph of the edges themselves (small inputs: adjacency sets)."""
    adj = [set() for _ in range(nv)]
    for u, v in zip(np.asarray(eu).tolist(), np.asarray(ev).tolist()):
        adj[u].add(v); adj[v].add(u)
    return np.asarray([len(adj[u] & adj[v]) for u, v in zip(np.asarray(eu).tolist(), np.asarray(ev).tolist())], np.int64)


def canonical(edges):
    """Distinct (min, max) pairs without loops, in lexicographic order: (eu, ev)."""
    e = sorted({(min(u, v), max(u, v)) for u, v in edges if u != v})
    a = np.asarray(e, np.int64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def hand_graph():
    """K_5 on 0-4 and on 5-9; 10 adjacent to 0 and 5; 11 to 1; 12 to 2 and 3; 13 to 3, 4, 8 and 9: (nv, pairs)."""
    e = [(a, b) for a in range(5) for b in range(a + 1, 5)] + [(a, b) for a in range(5, 10) for b in range(a + 1, 10)]
    e += [(10, 0), (10, 5), (11, 1), (12, 2), (12, 3), (13, 3), (13, 4), (13, 8), (13, 9)]
    return 14, e
