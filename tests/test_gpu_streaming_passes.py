"""GPU tests for the three streaming passes of the k-truss step: the oriented rows of the preparation (k_prep_rows: fill
groups of 4 trips whose loads are in flight together, a task's header requested one task ahead, batches of kRowCap = 512
entries), the bin counts of the index build (k_bin_count: 4 keys per thread per trip, the next bin requested ahead) and
the canonical results (k_truss_results; its version with 4 x 256 edges per workgroup and trip, which the edge counts below
sit around, was measured and not kept: DESIGN.md Appendix A).  Unrolled loops go wrong at their edges, so the inputs sit on
those edges; every value is compared with the oracle (trussness, and the supports through run_truss(with_support=True))."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the lengths of the oriented rows the rows pass is given: the wave width, 4 x 64, both sides of kRowCap = 512 (512 is the last
# length k_prep_rows ranks itself, 513 the first that goes to k_prep_rows_heavy) and both sides of 1024, the cap until now
ROW_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
HUG = (40000, 110000, 2.3, 21)
# edge counts around 4 x 256 edges for the results pass ...
RESULT_M = (1, 255, 1023, 1024, 1025, 4097)
# ... and around one and two bins of 2048 edges of the count pass
COUNT_M = (2047, 2048, 2049, 4097)


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _block(p, base):
    """B_p on vertices base .. base + 2p - 1: K_{p,p} plus a matching inside its second side.  First-side vertices have degree
    p, second-side vertices more, so every first-side oriented row has exactly p entries; every second-side vertex has an
    edge inside its side, and that edge closes a triangle through every first-side vertex -- through every slot of those
    rows.  (An odd side has no perfect matching: its last vertex is tied to its neighbour, which then has degree p + 2;
    p = 1 is a single edge.)"""
    a = base + np.arange(p, dtype=np.int64)
    b = base + p + np.arange(p, dtype=np.int64)
    bip = np.stack(np.meshgrid(a, b, indexing="ij"), axis=-1).reshape(-1, 2)
    pairs = np.stack([b[0:p - 1:2], b[1:p:2]], axis=1)
    parts = [bip, pairs]
    if p % 2 and p >= 3:
        parts.append(np.array([[b[p - 2], b[p - 1]]], dtype=np.int64))
    return np.concatenate(parts)


def _rows_graph(K):
    parts, base = [], 0
    for p in ROW_LENGTHS:
        parts.append(_block(p, base))
        base += 2 * p
    hug = np.asarray(K.gen_hug_edges(*HUG), dtype=np.int64).reshape(-1, 2)
    parts.append(hug + base)
    nv = base + HUG[0]
    assert nv % 64 != 0
    return nv, np.ascontiguousarray(np.concatenate(parts), dtype=np.int64)


@pytest.fixture(scope="module")
def rows_case(K, O):
    """The rows graph and its oracle results, computed once and left unchanged."""
    nv, uv = _rows_graph(K)
    rowptr, col = O.simplify(nv, uv)
    eu, ev = O.edge_list(rowptr, col)
    sup, tri = O.support(rowptr, col)
    # (the three blocks around 1024 are 3.1 M edges between rows of ~1025 slots: the OpenMP variant of the oracle's native
    # build where this box can build it -- tests/test_oracle.py ties it to orc_trussness --, else the single-thread restatement)
    if O.native_lib() is not None:
        import os
        tr = O.trussness_native(rowptr, col, min(16, len(os.sched_getaffinity(0))))
    else:
        tr = O.trussness(rowptr, col)
    for x in (rowptr, col, eu, ev, sup, tr):
        x.setflags(write=False)
    return dict(nv=nv, uv=uv, rowptr=rowptr, col=col, eu=eu, ev=ev, sup=sup, tri=tri, tr=tr)


def _path_triangle(m):
    """Exactly m edges: one triangle (m >= 4) and a path."""
    if m < 4:
        return m + 1, np.stack([np.arange(m), np.arange(1, m + 1)], axis=1).astype(np.int64)
    n = m - 3                                                      # path edges, on vertices 3 .. 3 + n
    tri = np.array([[0, 1], [1, 2], [0, 2]], dtype=np.int64)
    path = np.stack([np.arange(3, 3 + n), np.arange(4, 4 + n)], axis=1).astype(np.int64)
    return 4 + n, np.concatenate([tri, path])


def _strip(m):
    """Exactly m edges with triangles in every bin: a triangle strip (i, i+1), (i, i+2), and one pendant edge when m is even."""
    n = (m + 3) // 2
    uv = np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), np.stack([np.arange(n - 2), np.arange(2, n)], axis=1)])
    nv = n
    if len(uv) < m:
        uv = np.concatenate([uv, [[n - 1, n]]])
        nv = n + 1
    assert len(uv) == m
    return nv, uv.astype(np.int64)


def _check_whole(a, O, rowptr, col, want=None):
    eu, ev, tr, sup = a.run_truss(with_support=True)
    if want is None:
        oeu, oev = O.edge_list(rowptr, col)
        want = dict(eu=oeu, ev=oev, sup=O.support(rowptr, col)[0], tr=O.trussness(rowptr, col))
    assert np.array_equal(eu, want["eu"]) and np.array_equal(ev, want["ev"])
    assert np.array_equal(sup, want["sup"])
    assert np.array_equal(tr, want["tr"])
    return want


@pytest.mark.parametrize("stage", [None, "100"])
def test_rows_pass_row_lengths(K, O, rows_case, monkeypatch, stage):
    """Oriented rows of exactly 1 .. 1025 entries (ROW_LENGTHS: around the wave width, 4 x 64, kRowCap and twice kRowCap) next to a generator graph, on a vertex count that is no
    multiple of 64: a wrong rank, e2k entry, pivot or signature changes a support or a trussness.  Second run: the rows beyond
    kRowCap ranked out of global memory (KOMB_PREP_ROW_STAGE below their length)."""
    c = rows_case
    if stage:
        monkeypatch.setenv("KOMB_PREP_ROW_STAGE", stage)
    with K.KombAccel() as a:
        a.from_edges(c["nv"], c["uv"])
        rowptr, col = a.get_csr()
        assert np.array_equal(rowptr, c["rowptr"]) and np.array_equal(col, c["col"])
        # every first-side vertex of B_p has degree p and only higher-ranked neighbours: its oriented row has p entries
        deg = np.diff(rowptr)
        base = 0
        for p in ROW_LENGTHS:
            assert np.all(deg[base:base + p] == p) and np.all(deg[base + p:base + 2 * p] > p) or p == 1
            base += 2 * p
        _check_whole(a, O, rowptr, col, c)
        assert a.stats()["triangles"] == c["tri"]
    monkeypatch.delenv("KOMB_PREP_ROW_STAGE", raising=False)


def test_results_pass_on_the_rows_graph(K, O, rows_case, monkeypatch):
    """The results pass on the rows graph (4.6 M edges): slices of 3 ranks -- values inside
    the slice, zeros outside --, a vertex mask, and both sources of a value: the sub-round's level (every edge, with the
    finish switched off) and truss[] (the edges the local finish took over)."""
    c = rows_case
    ne = len(c["tr"])
    with K.KombAccel() as a:
        a.from_edges(c["nv"], c["uv"])
        for rank in range(3):
            a.truss_run_slice(rank, 3)
            eu, ev, tr, sup = a.truss_fetch(with_support=True)
            lo, hi = ne * rank // 3, ne * (rank + 1) // 3
            assert np.array_equal(eu, c["eu"]) and np.array_equal(ev, c["ev"])
            assert np.array_equal(tr[lo:hi], c["tr"][lo:hi]) and np.array_equal(sup[lo:hi], c["sup"][lo:hi]), rank
            assert not tr[:lo].any() and not tr[hi:].any() and not sup[:lo].any() and not sup[hi:].any(), rank
        both = False
        for env in ({"KOMB_FINISH": "none"}, {}, {"KOMB_FINISH": "local", "KOMB_LOCAL_LIMIT": "3000"}, {"KOMB_FINISH": "local", "KOMB_LOCAL_LIMIT": "300"}):
            for k, v in env.items(): monkeypatch.setenv(k, v)
            _check_whole(a, O, c["rowptr"], c["col"], c)
            st = a.stats()
            for k in env: monkeypatch.delenv(k, raising=False)
            print(env, "sub-rounds", st["truss_subrounds"], "local units", st["truss_local_units"])
            if env.get("KOMB_FINISH") == "none":
                assert st["truss_local_units"] == 0 and st["truss_subrounds"] > 0
            both = both or (st["truss_local_units"] > 0 and st["truss_subrounds"] > 0)
        assert both                                              # one run took values from rlevel[] AND from truss[]
        # (the mask drops the three blocks around 1024: the oracle needs half a minute for their rows)
        mask = (np.random.default_rng(6).random(c["nv"]) < 0.7).astype(np.uint8)
        small = 2 * sum(p for p in ROW_LENGTHS if p < 1000)
        mask[small:2 * sum(ROW_LENGTHS)] = 0
        seu, sev, stra = a.run_truss(mask)
        weu, wev, wtr = O.trussness_induced(c["rowptr"], c["col"], mask)
        assert np.array_equal(seu, weu) and np.array_equal(sev, wev) and np.array_equal(stra, wtr)


@pytest.mark.parametrize("m", RESULT_M)
def test_results_pass_tile_edges(K, O, m):
    """Exactly m edges (a triangle and a path) around 4 x 256 edges: the whole result, the slices of 3
    ranks, a vertex mask.  Graphs this small are handed to the local finish whole: every value comes from truss[]."""
    nv, uv = _path_triangle(m)
    rowptr, col = O.simplify(nv, uv)
    assert len(col) == 2 * m
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        want = _check_whole(a, O, rowptr, col)
        assert np.all(want["tr"][want["sup"] == 0] == 2) and (m < 4 or want["tr"].max() == 3)
        for rank in range(3):
            a.truss_run_slice(rank, 3)
            eu, ev, tr, sup = a.truss_fetch(with_support=True)
            lo, hi = m * rank // 3, m * (rank + 1) // 3
            assert np.array_equal(tr[lo:hi], want["tr"][lo:hi]) and np.array_equal(sup[lo:hi], want["sup"][lo:hi]), rank
            assert not tr[:lo].any() and not tr[hi:].any() and not sup[:lo].any() and not sup[hi:].any(), rank
        mask = np.ones(nv, np.uint8); mask[nv // 2::7] = 0
        seu, sev, stra = a.run_truss(mask)
        weu, wev, wtr = O.trussness_induced(rowptr, col, mask)
        assert np.array_equal(seu, weu) and np.array_equal(sev, wev) and np.array_equal(stra, wtr)
        _check_whole(a, O, rowptr, col, want)                     # a whole run afterwards


@pytest.mark.parametrize("m", COUNT_M)
def test_count_pass_bin_edges(K, O, monkeypatch, m):
    """Exactly m edges around one and two bins of 2048: a triangle-free path (no bin holds a record: every support 0, every
    trussness 2) and a triangle strip (records in every bin), by the default build, with every own-role entry sent through the
    record stream (KOMB_NO_OWN_DENSE: three records per triangle) and by the exact two-pass build."""
    path = (m + 1, np.stack([np.arange(m), np.arange(1, m + 1)], axis=1).astype(np.int64))
    for nv, uv in (path, _strip(m)):
        rowptr, col = O.simplify(nv, uv)
        assert len(col) == 2 * m
        with K.KombAccel() as a:
            a.from_edges(nv, uv)
            want = None
            for env in ({}, {"KOMB_NO_OWN_DENSE": "1"}, {"KOMB_INDEX": "two_pass"}):
                for k, v in env.items(): monkeypatch.setenv(k, v)
                want = _check_whole(a, O, rowptr, col, want)
                for k in env: monkeypatch.delenv(k, raising=False)
        if uv is path[1]:
            assert not want["sup"].any() and np.all(want["tr"] == 2)


def test_count_pass_layouts_agree(K, O, rows_case, monkeypatch):
    """The default index build against KOMB_INDEX=two_pass and KOMB_NO_OWN_DENSE=1 on the generator graph and on the rows
    graph: equal arrays."""
    env_names = ("KOMB_TWO_PASS", "KOMB_INDEX", "KOMB_OWN_DENSE_CAP", "KOMB_NO_OWN_DENSE", "KOMB_REC_CAP")
    for k in env_names:
        monkeypatch.delenv(k, raising=False)
    hug = np.asarray(K.gen_hug_edges(*HUG), dtype=np.int64).reshape(-1, 2)
    for nv, uv in ((HUG[0], hug), (rows_case["nv"], rows_case["uv"])):
        with K.KombAccel() as a:
            a.from_edges(nv, uv)
            r1 = a.run_truss(with_support=True)
            assert a.stats()["index_layout"] == 0
            if nv == HUG[0]:
                rowptr, col = a.get_csr()
                assert np.array_equal(r1[2], O.trussness(rowptr, col)) and np.array_equal(r1[3], O.support(rowptr, col)[0])
            else:
                assert np.array_equal(r1[2], rows_case["tr"]) and np.array_equal(r1[3], rows_case["sup"])
            for env, layout in (({"KOMB_INDEX": "two_pass"}, 2), ({"KOMB_NO_OWN_DENSE": "1"}, 0)):
                for k, v in env.items(): monkeypatch.setenv(k, v)
                r = a.run_truss(with_support=True)
                st = a.stats()
                for k in env: monkeypatch.delenv(k, raising=False)
                assert st["index_layout"] == layout, env
                for x, y in zip(r1, r):
                    assert np.array_equal(x, y), env
