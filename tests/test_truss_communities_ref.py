"""CPU tests of the k-truss communities reference (tests/truss_communities_ref.py) against its brute force, on hand
cases with the answers written out, and of the new entry points without a device."""
import numpy as np
import pytest

import components_ref as CR
import truss_communities_ref as R


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def _truss(O, nv, uv):
    rowptr, col = O.simplify(nv, np.asarray(uv, np.int64).reshape(-1, 2))
    eu, ev = O.edge_list(rowptr, col)
    return np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(O.trussness(rowptr, col), np.int64)


def _invariants(nv, eu, ev, tr, labels):
    """labels: {k: label vector}, for every k >= 3 that was computed."""
    for k, lab in labels.items():
        if k < 3:
            continue
        sz = R.sizes(lab)
        assert not np.any(sz == 1), k                                   # every member lies in k - 2 >= 1 member triangles
        assert np.array_equal(lab >= 0, tr >= k), k
        mem = lab >= 0
        assert np.array_equal(lab[lab[mem]], lab[mem]) and np.all(lab[mem] <= np.flatnonzero(mem)), k
        if k + 1 in labels:                                             # the communities at k + 1 refine those at k
            up = labels[k + 1]
            sel = up >= 0
            assert np.array_equal(lab[up[sel]], lab[sel]), k
        comp = CR.truss_components(nv, eu, ev, tr, k)                   # a community lies inside one vertex component
        assert np.array_equal(comp[eu[mem]], comp[ev[mem]]), k
        assert np.array_equal(comp[eu[mem]], comp[eu[lab[mem]]]), k


def _check_against_brute(nv, eu, ev, tr, name):
    tmax = int(tr.max()) if len(tr) else 2
    tri = R.triangles(nv, eu, ev)
    labels = {}
    for k in range(2, tmax + 2):
        lab = R.communities(nv, eu, ev, tr, k, tri)
        want = R.brute_force(nv, eu, ev, tr, k)
        assert np.array_equal(lab, want), (name, k)
        assert np.array_equal(R.vertex_multiplicity(nv, eu, ev, lab), R.brute_multiplicity(nv, eu, ev, lab)), (name, k)
        labels[k] = lab
    assert not np.any(labels[tmax + 1] >= 0), name
    _invariants(nv, eu, ev, tr, labels)
    return labels


def test_reference_equals_brute_force_on_golden_graphs(golden):
    n = 0
    for g in golden:
        if g["nv"] > 400 or len(g["eu"]) > 6000:
            continue
        n += 1
        eu, ev, tr = (np.asarray(g[x], np.int64) for x in ("eu", "ev", "trussness"))
        _check_against_brute(g["nv"], eu, ev, tr, g["name"])
        eu, ev, tr = (np.asarray(g[x], np.int64) for x in ("sub_eu", "sub_ev", "sub_trussness"))
        _check_against_brute(g["nv"], eu, ev, tr, g["name"] + " maxcore")
    assert n >= 3


@pytest.mark.parametrize("seed", range(36))
def test_reference_equals_brute_force_on_random_graphs(K, O, seed):
    rng = np.random.default_rng(1000 + seed)
    nv = int(rng.integers(5, 160))
    if seed % 3 == 0:
        uv = K.gen_hug_edges(nv, int(2.45 * nv), [2.1, 2.2, 2.6][seed % 9 // 3], seed)
    elif seed % 3 == 1:
        uv = rng.integers(0, nv, (int(nv * rng.uniform(1.0, 6.0)), 2))
    else:                                           # overlapping cliques: many communities sharing vertices
        parts = []
        for _ in range(int(rng.integers(2, 12))):
            mem = rng.choice(nv, int(rng.integers(3, min(9, nv))), replace=False)
            parts.append(mem[np.stack(np.triu_indices(len(mem), 1), 1)])
        uv = np.concatenate(parts)
    eu, ev, tr = _truss(O, nv, uv)
    _check_against_brute(nv, eu, ev, tr, seed)


def _run(O, nv, uv, k):
    eu, ev, tr = _truss(O, nv, uv)
    lab = R.communities(nv, eu, ev, tr, k)
    assert np.array_equal(lab, R.brute_force(nv, eu, ev, tr, k))
    return eu, ev, tr, lab


def _clique(ids):
    ids = np.asarray(ids)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)]


def test_hand_cases(O):
    # bow-tie: two triangles sharing vertex 2
    eu, ev, tr, lab = _run(O, 5, [[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]], 3)
    assert list(zip(eu.tolist(), ev.tolist())) == [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)]
    assert lab.tolist() == [0, 0, 0, 3, 3, 3] and R.sizes(lab).tolist() == [3] * 6
    assert R.vertex_multiplicity(5, eu, ev, lab).tolist() == [1, 1, 2, 1, 1]
    assert R.summary(5, eu, ev, lab) == (6, 2, 3, 1)
    # two K5 sharing one vertex: two communities at every k up to 5, the shared vertex in both
    uv = np.concatenate([_clique(range(5)), _clique(range(4, 9))])
    for k in (2, 3, 4, 5):
        eu, ev, tr, lab = _run(O, 9, uv, k)
        assert R.summary(9, eu, ev, lab) == (20, 2, 10, 1), k
        assert R.vertex_multiplicity(9, eu, ev, lab).tolist() == [1, 1, 1, 1, 2, 1, 1, 1, 1]
    # two K5 sharing one edge: triangles through the shared edge join them -- one community at k = 4
    uv = np.concatenate([_clique(range(5)), _clique(range(3, 8))])
    eu, ev, tr, lab = _run(O, 8, uv, 4)
    assert len(eu) == 19 and R.summary(8, eu, ev, lab) == (19, 1, 19, 0) and not lab.any()
    # two cliques joined by a bridge edge: the bridge is a singleton at k = 2 and a non-member at k = 3
    uv = np.concatenate([_clique(range(4)), _clique(range(4, 8)), [[3, 4]]])
    eu, ev, tr, lab = _run(O, 8, uv, 2)
    b = int(np.flatnonzero((eu == 3) & (ev == 4))[0])
    assert lab[b] == b and R.sizes(lab)[b] == 1 and R.summary(8, eu, ev, lab) == (13, 3, 6, 2)
    eu, ev, tr, lab = _run(O, 8, uv, 3)
    assert lab[b] == -1 and R.sizes(lab)[b] == 0 and R.summary(8, eu, ev, lab) == (12, 2, 6, 0)
    # triangle-free (a 4 x 5 grid): all singletons at k = 2, nothing at k = 3
    idx = np.arange(20).reshape(4, 5)
    uv = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    eu, ev, tr, lab = _run(O, 20, uv, 2)
    assert lab.tolist() == list(range(31)) and np.all(R.sizes(lab) == 1)
    assert R.vertex_multiplicity(20, eu, ev, lab).tolist() == (np.bincount(eu, minlength=20) + np.bincount(ev, minlength=20)).tolist()
    assert not np.any(_run(O, 20, uv, 3)[3] >= 0)
    # a book: the edge (0, 1) in 300 triangles -- one community of 601 edges
    pages = np.arange(2, 302)
    uv = np.concatenate([[[0, 1]], np.stack([np.zeros(300, np.int64), pages], 1), np.stack([np.ones(300, np.int64), pages], 1)])
    for k in (2, 3):
        eu, ev, tr, lab = _run(O, 302, uv, k)
        assert not lab.any() and R.summary(302, eu, ev, lab) == (601, 1, 601, 0)
    assert tr.max() == 3
    # k <= 2 means every edge; an empty edge list
    assert np.array_equal(R.communities(302, eu, ev, tr, 0), R.communities(302, eu, ev, tr, 2))
    assert len(R.communities(4, [], [], [], 3)) == 0 and R.summary(4, [], [], np.zeros(0)) == (0, 0, 0, 0)


def test_reference_reproduces_the_measured_table(K, O):
    """(member edges, communities, largest, vertices in more than one) of the graphs the feature was sized on."""
    nv, uv = CR.composite(K.gen_hug_edges, 1)
    eu, ev, tr = _truss(O, nv, uv)
    assert (nv, len(eu)) == (196066, 959288)
    tri = R.triangles(nv, eu, ev)
    assert len(tri[0]) == 1871684
    labels = {k: R.communities(nv, eu, ev, tr, k, tri) for k in (3, 4, 5)}
    assert R.summary(nv, eu, ev, labels[3]) == (801610, 24553, 352381, 38888)
    assert R.summary(nv, eu, ev, labels[4]) == (686578, 9132, 303258, 23157)
    assert len(np.unique(CR.truss_components(nv, eu, ev, tr, 3)[np.concatenate([eu, ev])[np.concatenate([tr, tr]) >= 3]])) == 20
    _invariants(nv, eu, ev, tr, labels)
    nv = 200000
    eu, ev, tr = _truss(O, nv, K.gen_hug_edges(nv, 490000, 2.6, 11))
    assert len(eu) == 2016538
    lab = R.communities(nv, eu, ev, tr, 3)
    assert R.summary(nv, eu, ev, lab) == (1835575, 129641, 1141628, 151835)
    _invariants(nv, eu, ev, tr, {3: lab})


def test_binding_declares_communities_and_fails_without_device(K):
    """The binding covers the four new entry points; without a GPU they answer KOMB_ERR_DEVICE (no CPU fallback)."""
    from komb_amd import _lib
    names = ("komb_truss_communities_run", "komb_truss_communities_fetch", "komb_truss_communities_fetch_vertices",
             "komb_truss_communities_info")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    for name in ("truss_communities_run", "truss_communities_fetch", "truss_communities_fetch_vertices",
                 "truss_communities_info", "run_truss_communities"):
        assert callable(getattr(K.KombAccel, name))
    assert _lib.KOMB_COMM_K_MAX == -1
    assert "COMM_SHORT" in K.api.OPTION_NAMES and "COMM_HEAVY" in K.api.OPTION_NAMES
    g = K.KombAccel()
    try:
        g.from_edges(3, [[0, 1]])
    except K.KombError as e:
        assert e.code == _lib.KOMB_ERR_DEVICE
    else:
        g.close()
        return                                   # a usable GPU is present: the GPU tests cover the calls
    for call in (lambda: g.truss_communities_run(3), g.truss_communities_fetch_vertices, g.truss_communities_info):
        with pytest.raises(K.KombError) as e:
            call()
        assert e.value.code == _lib.KOMB_ERR_DEVICE
    assert _lib.load().komb_truss_communities_fetch(g._ctx, None, None) == _lib.KOMB_ERR_DEVICE
    g.close()
