"""CPU tests of tests/structural_ref.py, the restatement the GPU tests compare komb_structural_clusters_run with: against a
brute force written from the set definitions (fractions.Fraction on sigma^2, common neighbours from adjacency sets, nothing
of the support reused), its invariants, and the hand graph of the issue with the values computed there."""
import random
from fractions import Fraction

import numpy as np
import pytest

import structural_ref as R


def brute(nv, edges, eps_num, eps_den, mu):
    """label, role, sim_deg, {similar pairs} from the definitions alone."""
    adj = [set() for _ in range(nv)]
    for u, v in edges:
        if u != v:
            adj[u].add(v); adj[v].add(u)
    gam = [adj[v] | {v} for v in range(nv)]
    eps2 = Fraction(eps_num, eps_den) ** 2
    sim = {v: {w for w in adj[v] if Fraction(len(gam[v] & gam[w]) ** 2, len(gam[v]) * len(gam[w])) >= eps2} for v in range(nv)}
    core = [len(sim[v]) + 1 >= mu for v in range(nv)]
    label = [-1] * nv
    for v in range(nv):                              # ascending: the first core to reach a class is its smallest id
        if core[v] and label[v] < 0:
            label[v] = v
            todo = [v]
            while todo:
                x = todo.pop()
                for w in sim[x]:
                    if core[w] and label[w] < 0:
                        label[w] = v
                        todo.append(w)
    for v in range(nv):
        if not core[v]:
            ls = [label[w] for w in sim[v] if core[w]]
            if ls:
                label[v] = min(ls)
    role = []
    for v in range(nv):
        if core[v]:
            role.append(R.CORE)
        elif label[v] >= 0:
            role.append(R.BORDER)
        else:
            role.append(R.HUB if len({label[w] for w in adj[v] if label[w] >= 0}) >= 2 else R.OUTLIER)
    pairs = {(v, w) for v in range(nv) for w in sim[v] if v < w}
    return label, role, [len(sim[v]) for v in range(nv)], pairs


def _ref(nv, edges, eps_num, eps_den, mu):
    eu, ev = R.canonical(edges)
    return eu, ev, R.clusters(nv, eu, ev, R.supports(nv, eu, ev), eps_num, eps_den, mu)


def _invariants(nv, eu, ev, out):
    label, role, size = out["label"], out["role"], out["size"]
    has = label >= 0
    assert np.array_equal(label[label[has]], label[has])                         # the label of a label is itself
    assert np.all(role[label[has]] == R.CORE)                                    # every cluster holds a core: its label vertex
    assert np.array_equal(has, role >= R.BORDER)
    assert np.array_equal(size, np.where(has, np.bincount(label[has], minlength=nv)[np.where(has, label, 0)], 0))
    nb = [set() for _ in range(nv)]
    for u, v in zip(eu.tolist(), ev.tolist()):
        if label[v] >= 0: nb[u].add(int(label[v]))
        if label[u] >= 0: nb[v].add(int(label[u]))
    for v in range(nv):
        if role[v] == R.HUB:
            assert len(nb[v]) >= 2
        elif role[v] == R.OUTLIER:
            assert len(nb[v]) <= 1
    info = out["info"]
    assert info["n_cores"] + info["n_borders"] + info["n_hubs"] + info["n_outliers"] == nv
    assert info["n_clusters"] == len(set(label[has].tolist())) and info["n_similar_edges"] * 2 == int(out["sim_deg"].sum())
    assert info["largest"] == (int(size.max()) if nv else 0)


PARAMS = [(3, 10, 2), (1, 2, 3), (7, 10, 3), (6, 10, 2), (8, 10, 4), (1, 1, 2), (1, 100, 2), (2, 3, 5), (1, 2, 4), (2, 5, 4)]


def test_against_the_brute_force():
    rnd = random.Random(5)
    seen_roles, multi = set(), 0
    for g in range(60):
        nv = rnd.randint(4, 12)
        p = rnd.choice((0.2, 0.35, 0.5, 0.7))
        edges = [(a, b) for a in range(nv) for b in range(a + 1, nv) if rnd.random() < p]
        edges += [(b, a) for a, b in edges[:3]] + [(0, 0)]                       # reversed duplicates and a loop
        for eps_num, eps_den, mu in PARAMS:
            eu, ev, out = _ref(nv, edges, eps_num, eps_den, mu)
            label, role, sim_deg, pairs = brute(nv, edges, eps_num, eps_den, mu)
            assert out["label"].tolist() == label and out["role"].tolist() == role and out["sim_deg"].tolist() == sim_deg, (g, eps_num, eps_den, mu)
            assert {(u, v) for u, v, s in zip(eu.tolist(), ev.tolist(), out["similar"].tolist()) if s} == pairs
            _invariants(nv, eu, ev, out)
            seen_roles |= set(role)
            multi += R.multi_borders(nv, eu, ev, out)
    assert seen_roles == {0, 1, 2, 3} and multi > 0                             # the graphs exercise every branch


def test_hand_graph():
    nv, edges = R.hand_graph()
    eu, ev, out = _ref(nv, edges, 7, 10, 3)
    assert out["info"]["n_similar_edges"] == 21
    assert out["label"].tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, -1, -1, 0, -1]
    assert out["role"].tolist() == [3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 0, 2, 1]
    assert out["size"].tolist() == [6] * 5 + [5] * 5 + [0, 0, 6, 0]
    assert (out["info"]["n_clusters"], out["info"]["largest"]) == (2, 6)
    _invariants(nv, eu, ev, out)
    assert (out["label"].tolist(), out["role"].tolist()) == brute(nv, edges, 7, 10, 3)[:2]
    eu, ev, out = _ref(nv, edges, 8, 10, 4)
    assert out["info"]["n_similar_edges"] == 18
    assert out["role"][3] == R.BORDER and out["role"][12] == R.OUTLIER and out["label"][3] == 0 and out["label"][12] == -1
    assert (out["label"].tolist(), out["role"].tolist()) == brute(nv, edges, 8, 10, 4)[:2]
    _invariants(nv, eu, ev, out)


def test_wide_comparison_and_ties():
    """Both paths of the comparison agree, an exact tie is similar, and a product past 2^64 is compared exactly."""
    d = np.asarray([3, 8, 5000, 5000], np.int64)
    eu, ev, sup = np.asarray([0, 2]), np.asarray([1, 3]), np.asarray([1, 4999])
    assert R.similar_edges(d, eu, ev, sup, 1, 2).tolist() == [True, True]        # sigma = 3 / 6 exactly | 5001 / 5001
    assert R.similar_edges(d, eu, ev, sup, 500001, 1000000).tolist() == [False, True]
    assert 5001 ** 2 * 1000000 ** 2 > 2 ** 64
    d = np.asarray([5001, 5001], np.int64)
    assert R.similar_edges(d, eu[:1], ev[:1], np.asarray([5000]), 999999, 1000000).tolist() == [True]       # sigma = 1
    assert R.similar_edges(d, eu[:1], ev[:1], np.asarray([4999]), 999999, 1000000).tolist() == [False]      # 5001 / 5002 < eps
    assert R.similar_edges(d, eu[:1], ev[:1], np.asarray([4999]), 9997, 10000).tolist() == [True]
    rng = np.random.default_rng(2)
    d = rng.integers(0, 50, 40)
    eu, ev = rng.integers(0, 40, 300), rng.integers(0, 40, 300)
    sup = rng.integers(0, 30, 300)
    for num, den in ((1, 2), (7, 10), (999999, 1000000), (123457, 654321)):
        want = [(int(s) + 2) ** 2 * den ** 2 >= num ** 2 * (int(d[u]) + 1) * (int(d[v]) + 1) for u, v, s in zip(eu, ev, sup)]
        assert R.similar_edges(d, eu, ev, sup, num, den).tolist() == want


def test_degenerate():
    for nv in (0, 3):
        out = R.clusters(nv, [], [], [], 1, 2, 2)
        assert out["label"].tolist() == [-1] * nv and out["role"].tolist() == [0] * nv and out["size"].tolist() == [0] * nv
        assert out["info"]["n_outliers"] == nv and out["info"]["largest"] == 0 and out["info"]["n_clusters"] == 0
    out = R.clusters(2, [0], [1], [0], 1, 1, 2)                                  # one edge: sigma = 2 / 2
    assert out["label"].tolist() == [0, 0] and out["role"].tolist() == [3, 3] and out["similar"].tolist() == [1]
