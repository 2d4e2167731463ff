"""CPU restatement of the onion decomposition and an O(E) checker of a layering (test helpers, no GPU).

The definition is networkx.onion_layers (3.4.2) on a simple graph (Hebert-Dufresne, Grochow & Allard 2016): isolated
vertices form layer 1 (when there are any); then, starting with k = 1, repeat until the graph is empty: raise k to the
smallest live degree if that is larger, take EVERY live vertex of live degree <= k as the next layer, remove them all at
once and decrement their neighbours.  A vertex's coreness is the k it leaves at (0 if isolated).

Graphs are symmetric CSR arrays (rowptr [nv+1], col [2|E|]), rows without loops or duplicates.
"""
import numpy as np


def _rows_of(rowptr, col, vs):
    """The concatenated CSR rows of the vertices vs."""
    b = rowptr[vs].astype(np.int64)
    n = (rowptr[vs + 1] - rowptr[vs]).astype(np.int64)
    tot = int(n.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    start = np.repeat(b - np.cumsum(n) + n, n)
    return col[start + np.arange(tot, dtype=np.int64)]


def onion_layers(rowptr, col):
    """(layer int32[nv], coreness int32[nv], n_layers): one frontier per layer, its rows' neighbours counted at once."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    nv = len(rowptr) - 1
    d = np.diff(rowptr).astype(np.int64)
    layer = np.zeros(nv, np.int32)
    core = np.zeros(nv, np.int32)
    alive = d > 0
    cur = 1
    if nv and not alive.all():
        layer[~alive] = 1
        cur = 2
    n_alive = int(alive.sum())
    k = 1
    front = None                      # next layer, when the previous one's decrements produced it
    while n_alive:
        if front is None or len(front) == 0:
            live = np.flatnonzero(alive)
            k = max(k, int(d[live].min()))
            front = live[d[live] <= k]
        layer[front] = cur
        core[front] = k
        alive[front] = False
        n_alive -= len(front)
        cur += 1
        nb = _rows_of(rowptr, col, front)
        nb = nb[alive[nb]]
        if len(nb) * 16 < nv:
            touched, cnt = np.unique(nb, return_counts=True)
        else:
            cnt = np.bincount(nb, minlength=nv)
            touched = np.flatnonzero(cnt)
            cnt = cnt[touched]
        d[touched] -= cnt
        front = touched[d[touched] <= k]
    return layer, core, cur - 1 if nv else 0


def check_layering(rowptr, col, layer, core, want_core):
    """Proves (layer, core) is the onion decomposition without the sequential peel; returns a list of failed conditions.

    With L(v) the layer of v and k(l) the coreness of layer l:
      1. core equals want_core (the coreness computed independently);
      2. the layers are 1..n and none is empty;
      3. each layer has a single coreness and coreness never decreases from one layer to the next;
      4. every v: |{u in N(v): L(u) >= L(v)}| <= core(v)  (v's live degree when it is peeled);
      5. every v whose previous layer is not the layer of isolated vertices (nor absent):
         |{u in N(v): L(u) >= L(v) - 1}| > k(L(v) - 1)  (v was live and not taken one layer earlier).
    5 implies, by induction over the layers and 3, that a layer holds every live vertex of live degree <= its k."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    layer = np.asarray(layer, dtype=np.int64)
    core = np.asarray(core, dtype=np.int64)
    nv = len(rowptr) - 1
    bad = []
    if not np.array_equal(core, np.asarray(want_core, dtype=np.int64)):
        bad.append("coreness")
    if nv == 0:
        return bad
    n = int(layer.max())
    if layer.min() < 1 or len(np.unique(layer)) != n:
        return bad + ["layers not 1..n without gaps"]
    kmin = np.full(n + 1, np.iinfo(np.int64).max)
    kmax = np.full(n + 1, -1)
    np.minimum.at(kmin, layer, core)
    np.maximum.at(kmax, layer, core)
    if not np.array_equal(kmin[1:], kmax[1:]):
        bad.append("a layer with two corenesses")
    k = kmax
    if np.any(np.diff(k[1:]) < 0):
        bad.append("coreness decreases")
    deg = np.diff(rowptr)
    src = np.repeat(np.arange(nv, dtype=np.int64), deg)
    lu, lv = layer[col], layer[src]
    ge = np.bincount(src, weights=(lu >= lv), minlength=nv)
    if np.any(ge > core):
        bad.append("live degree above coreness when peeled")
    ge1 = np.bincount(src, weights=(lu >= lv - 1), minlength=nv)
    iso_layer = 1 if np.any(deg == 0) else 0
    prev = layer - 1
    has_prev = (prev >= 1) & (prev != iso_layer)
    if np.any(ge1[has_prev] <= k[prev[has_prev]]):
        bad.append("a vertex left live although its degree allowed it one layer earlier")
    return bad


def simple_csr(nv, uv):
    """Symmetric CSR of the simple graph of raw pairs (loops and duplicates dropped), rows ascending."""
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    uv = uv[uv[:, 0] != uv[:, 1]]
    a = np.concatenate([uv[:, 0], uv[:, 1]])
    b = np.concatenate([uv[:, 1], uv[:, 0]])
    key = np.unique(a * nv + b)
    src, dst = key // nv, key % nv
    rowptr = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=nv), out=rowptr[1:])
    return rowptr, dst.astype(np.int32)


def networkx_layers(nv, rowptr, col):
    """networkx.onion_layers on the same simple graph: (layer int32[nv], n_layers)."""
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(nv))
    src = np.repeat(np.arange(nv), np.diff(rowptr))
    sel = src < col
    g.add_edges_from(zip(src[sel].tolist(), np.asarray(col)[sel].tolist()))
    od = nx.onion_layers(g) if nv else {}
    out = np.array([od[v] for v in range(nv)], dtype=np.int32)
    return out, int(out.max()) if nv else 0
