"""CPU reference of komb_components_run for the tests: scipy's connected components, relabelled by the smallest vertex
id of every component, on the subgraph a coreness / trussness threshold selects.  No GPU, no product code."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components


def min_labels(nv, eu, ev, member):
    """label[v] = smallest id of v's component in the graph of the edges (eu, ev) on nv vertices; -1 where not member."""
    eu, ev = np.asarray(eu, np.int64), np.asarray(ev, np.int64)
    member = np.asarray(member, bool)
    if nv == 0:
        return np.zeros(0, np.int64)
    A = csr_matrix((np.ones(len(eu), np.int8), (eu, ev)), shape=(nv, nv))
    n, lab = connected_components(A, directed=False)
    first = np.full(n, nv, np.int64)
    np.minimum.at(first, lab, np.arange(nv))
    out = first[lab]
    out[~member] = -1
    return out


def core_components(rowptr, col, core, k):
    """Components of the k-core: members are the vertices of coreness >= k, edges those between two members."""
    rowptr, col, core = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(core, np.int64)
    nv = len(rowptr) - 1
    member = core >= k
    src = np.repeat(np.arange(nv), np.diff(rowptr))
    sel = (src < col) & member[src] & member[col]
    return min_labels(nv, src[sel], col[sel], member)


def truss_components(nv, eu, ev, tr, k):
    """Components of the k-truss: edges of trussness >= k, members their endpoints."""
    eu, ev, tr = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(tr, np.int64)
    sel = tr >= k
    member = np.zeros(nv, bool)
    member[eu[sel]] = True
    member[ev[sel]] = True
    return min_labels(nv, eu[sel], ev[sel], member)


def sizes(label):
    """size[v] = vertices that carry v's label, 0 for a non-member."""
    label = np.asarray(label, np.int64)
    nv = len(label)
    cnt = np.bincount(label[label >= 0], minlength=nv) if nv else np.zeros(0, np.int64)
    out = np.zeros(nv, np.int64)
    out[label >= 0] = cnt[label[label >= 0]]
    return out


def summary(label):
    """(n_members, n_components, largest) of a label vector."""
    label = np.asarray(label, np.int64)
    sz = sizes(label)
    roots = label == np.arange(len(label))
    return int((label >= 0).sum()), int(roots.sum()), int(sz.max()) if len(sz) else 0


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


def composite_parts(gen, seed):
    """The pieces composite() is made of, before the ids are scattered: [(nv, edges)]."""
    parts = []
    for i, (nv, alpha) in enumerate([(300, 2.1), (2000, 2.2), (5000, 2.6), (20000, 2.2), (50000, 2.6),
                                     (1000, 2.6), (3000, 2.1), (8000, 2.2)]):
        parts.append((nv, np.asarray(gen(nv, int(2.45 * nv), alpha, 100 * seed + i), np.int64).reshape(-1, 2)))
    n = 100000; parts.append((n, np.stack([np.arange(n - 1), np.arange(1, n)], 1)))            # a path: deep trees
    n = 1000;   parts.append((n, np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)))         # a ring
    n = 5001;   parts.append((n, np.stack([np.zeros(n - 1, np.int64), np.arange(1, n)], 1)))   # a star
    sizes_ = [3, 4, 5, 6, 8, 12, 16, 24, 32, 40, 48, 64]                                       # cliques, joined in pairs
    for j in range(0, len(sizes_), 2):
        a, b = sizes_[j], sizes_[j + 1]
        ea = np.stack(np.triu_indices(a, 1), 1); eb = np.stack(np.triu_indices(b, 1), 1) + a
        if (j // 2) % 2 == 0: link, n = [[0, a]], a + b                                        # by a direct bridge edge
        else: link, n = [[0, a + b], [a + b, a]], a + b + 1                                    # through a vertex of degree 2
        parts.append((n, np.concatenate([ea, eb, np.asarray(link)])))
    return parts


def composite(gen, seed):
    """A test graph with many non-trivial components (gen is komb_amd.gen_hug_edges): (nv, raw pairs)."""
    rng = np.random.default_rng(seed)
    parts, off = [], 0
    def add(e, n):
        nonlocal off
        parts.append(np.asarray(e, np.int64).reshape(-1, 2) + off); off += n
    for n, e in composite_parts(gen, seed):
        add(e, n)
    off += 500                                                                      # isolated vertices
    nv, uv = off, np.concatenate(parts)
    uv = rng.permutation(nv)[uv]                   # ids scattered: a component's smallest id is not its first vertex
    dup = uv[rng.integers(0, len(uv), len(uv) // 10)]
    uv = np.concatenate([uv, dup, dup[: len(dup) // 2, ::-1], np.stack([np.arange(50)] * 2, 1)])   # duplicates, reversed, loops
    rng.shuffle(uv)
    return nv, uv
