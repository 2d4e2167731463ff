"""The distance analysis of include/komb_accel.h (komb_distances_run) restated in plain Python: one breadth-first search per
distinct source, then the per-vertex and per-source integers, the histogram of distances and harmonic[v] with the operation
order of the definition -- per block of 64 consecutive list entries a partial sum h_b that takes (double)c / (double)L at every
level L in ascending order, the partial sums added in block order.  numpy's float64 division and addition are IEEE-754 binary64
operations that round once each, so the result is the definition's, bit for bit.

order= makes a deliberately DIFFERENT harmonic[], for the test that shows the stored fixture can tell the difference:
"per_source" adds 1 / d one list entry at a time; "batch256" keeps one running sum over the levels for a whole batch of 256
entries (what a kernel that handles four words at once gets if it does not keep a partial sum per word)."""
import json
import os
from collections import deque

import numpy as np

ALL = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "distances_fixture.json")


def adjacency(nv, pairs):
    """The rows of the simple undirected graph of `pairs` (self loops and repeats dropped), ascending."""
    adj = [set() for _ in range(nv)]
    for u, v in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        if u != v:
            adj[u].add(v); adj[v].add(u)
    return [sorted(a) for a in adj]


def rows_of_csr(rowptr, col):
    return [[int(x) for x in col[rowptr[v]:rowptr[v + 1]]] for v in range(len(rowptr) - 1)]


def bfs(rows, s):
    """int32[nv]: the distance from s, -1 where there is none."""
    dist = [-1] * len(rows)
    dist[s] = 0
    todo = deque([s])
    while todo:
        v = todo.popleft()
        d = dist[v] + 1
        for w in rows[v]:
            if dist[w] < 0:
                dist[w] = d
                todo.append(w)
    return np.asarray(dist, dtype=np.int32)


def _harmonic_of(D, group):
    """The sum over the rows of D in groups of `group` rows: per group one running sum over the levels, the groups in order."""
    total = np.zeros(D.shape[1], dtype=np.float64)
    for first in range(0, D.shape[0], group):
        blk = D[first:first + group]
        h = np.zeros(D.shape[1], dtype=np.float64)
        for L in np.unique(blk[blk > 0]).tolist():
            c = (blk == L).sum(axis=0)
            q = c.astype(np.float64) / np.float64(L)
            h = np.where(c > 0, h + q, h)
        total = total + h
    return total


def distances(rows, sources=None, words=4, order="defined", cache=None):
    """What komb_distances_run / _fetch / _fetch_sources / _histogram / _info give for the rows (ascending adjacency lists), the
    sources (None: all) and DIST_WORDS = words: {"n_reached", "sum_dist", "ecc", "harmonic"} per vertex, "sources" = {"source",
    "n_reached", "sum_dist", "ecc"} per list entry, "pairs", and "info" (every field but ms).  cache: a dict that keeps the
    search of every source vertex between calls on the same rows."""
    nv = len(rows)
    src = list(range(nv)) if sources is None else [int(s) for s in sources]
    assert all(0 <= s < nv for s in src) and words in (1, 2, 4)
    cache = {} if cache is None else cache
    for s in src:
        if s not in cache:
            cache[s] = bfs(rows, s)
    D = np.stack([cache[s] for s in src]) if src else np.zeros((0, nv), dtype=np.int32)
    hit = D >= 0
    out = {"n_reached": hit.sum(axis=0).astype(np.int64), "sum_dist": np.where(hit, D, 0).sum(axis=0, dtype=np.int64),
           "ecc": D.max(axis=0).astype(np.int32) if src else np.full(nv, -1, dtype=np.int32)}
    if order == "defined":
        out["harmonic"] = _harmonic_of(D, 64)
    elif order == "batch256":
        out["harmonic"] = _harmonic_of(D, 256)
    else:
        assert order == "per_source"
        h = np.zeros(nv, dtype=np.float64)
        for i in range(len(src)):
            h = np.where(D[i] > 0, h + 1.0 / np.where(D[i] > 0, D[i], 1).astype(np.float64), h)
        out["harmonic"] = h
    ecc = D.max(axis=1).astype(np.int32) if nv else np.zeros(0, dtype=np.int32)
    out["sources"] = {"source": np.asarray(src, dtype=np.int32), "n_reached": hit.sum(axis=1).astype(np.int64),
                      "sum_dist": np.where(hit, D, 0).sum(axis=1, dtype=np.int64), "ecc": ecc}
    depth_max = int(ecc.max()) if len(src) else 0
    pairs = np.bincount(D[hit].astype(np.int64), minlength=depth_max + 1).astype(np.int64)
    per = 64 * words
    batches = [ecc[i:i + per] for i in range(0, len(src), per)]
    out["pairs"] = pairs
    out["info"] = {"n_sources": len(src), "flags": ALL if sources is None else 0, "depth_max": depth_max,
                   "depth_min": int(ecc.min()) if len(src) else 0, "n_pairs": int(pairs.sum()),
                   "sum_all": int((pairs * np.arange(len(pairs))).sum()), "n_batches": len(batches),
                   "n_level_steps": sum(int(b.max()) + 1 for b in batches) if nv else 0}
    return out


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def make_fixture(seed=20):
    """(nv, pairs, sources): a seeded graph of 160 vertices in several components and a list of 300 entries with repeats, in no
    order -- more than one batch at every DIST_WORDS, and more than one block in every batch but the last of DIST_WORDS=1."""
    rng = np.random.default_rng(seed)
    nv = 160
    pairs = np.concatenate([rng.integers(0, 120, size=(190, 2)), rng.integers(120, 150, size=(40, 2))])   # 150 .. 159 stay isolated
    sources = rng.integers(0, nv, size=300)
    return nv, pairs.astype(np.int64), sources.astype(np.int64)


def load_fixture():
    """(nv, pairs, sources, stored bit patterns of harmonic[])"""
    with open(FIXTURE) as f:
        d = json.load(f)
    return d["nv"], np.asarray(d["pairs"], dtype=np.int64), d["sources"], np.asarray([int(h, 16) for h in d["harmonic_hex"]], dtype=np.uint64)


if __name__ == "__main__":                                                   # writes the fixture anew
    nv, pairs, sources = make_fixture()
    got = distances(adjacency(nv, pairs), sources)
    with open(FIXTURE, "w") as f:
        json.dump({"nv": nv, "pairs": pairs.tolist(), "sources": sources.tolist(),
                   "harmonic_hex": ["%016x" % b for b in bits(got["harmonic"]).tolist()]}, f, separators=(",", ":"))
        f.write("\n")
