"""GPU tests for the paths of the wedge enumeration (k_wedges, komb_amd/csrc/truss_wedge.h) whose code was restructured: the
four candidate tests of a chunk compacted in one step into a parking buffer of 63 + 4 x 64 words, the survivor look-up and
the record hand-over behind it at one place of the batch loop, one record append in a loop over the roles.  The inputs are
the smallest at which each of those can go wrong; every case compares per-edge support and trussness with the CPU oracle of
the parity suite, by the default index build (the wedge enumeration in record-stream mode) and by KOMB_INDEX=two_pass (the
wedge enumeration in count mode for the supports, the probe enumeration k_triangles for the index)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the library exposes none of the kernel's constants; these are komb_amd/csrc/truss_line.h and truss_tri.h
TRI_CAP = 256            # kTriCap: oriented slots a wavefront stages in LDS (and the largest slot number + 1 of a parked candidate)
TRI_REC = 384            # kTriRec: records of a staged sub-range the LDS buffer holds
REC_CHUNK = 1024         # kRecChunk: positions of the record stream a wavefront claims at a time

LAYOUTS = ({}, {"KOMB_INDEX": "two_pass"})
# a task groups min(32, |V| / 16384) light vertices (truss_prep.hip): with this many vertices, most of them isolated, it is 32
GROUPED_NV = 32 * 16384


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def K(built):
    import komb_amd
    return komb_amd


def _clique(n, base=0):
    """K_n on vertices base .. base + n - 1.  All degrees are equal, so the (degree, id) order is the id order: vertex
    base + i has an oriented row of n - 1 - i slots, and EVERY candidate behind an edge of that row is a triangle."""
    i, j = np.triu_indices(n, 1)
    return np.stack([i + base, j + base], axis=1).astype(np.int64)


def _path(first, length, base):
    """`length` new vertices base .. base + length - 1 hung on vertex `first` as a path: edges without a triangle."""
    v = np.concatenate([[first], base + np.arange(length)])
    return np.stack([v[:-1], v[1:]], axis=1).astype(np.int64)


def _check(K, O, monkeypatch, nv, uv, envs=LAYOUTS, extra_env=None):
    """Support and trussness of every edge against the oracle, once per environment of `envs` on one context; the oracle's
    results are computed once and left unchanged.  Returns them with the stats of the first (default) run."""
    uv = np.ascontiguousarray(uv, dtype=np.int64)
    rowptr, col = O.simplify(nv, uv)
    oeu, oev = O.edge_list(rowptr, col)
    osup, otri = O.support(rowptr, col)
    otr = O.trussness(rowptr, col)
    for x in (oeu, oev, osup, otr):
        x.setflags(write=False)
    first = None
    for k, v in (extra_env or {}).items(): monkeypatch.setenv(k, v)
    with K.KombAccel() as a:
        a.from_edges(nv, uv)
        for env in envs:
            for k, v in env.items(): monkeypatch.setenv(k, v)
            eu, ev, tr, sup = a.run_truss(with_support=True)
            st = a.stats()
            for k in env: monkeypatch.delenv(k, raising=False)
            assert np.array_equal(eu, oeu) and np.array_equal(ev, oev), env
            assert np.array_equal(sup, osup), env
            assert np.array_equal(tr, otr), env
            assert st["triangles"] == otri, env
            assert st["index_layout"] == (2 if env.get("KOMB_INDEX") == "two_pass" else 0), env
            first = first or st
    for k in (extra_env or {}): monkeypatch.delenv(k, raising=False)
    return dict(sup=osup, tr=otr, tri=otri, stats=first)


@pytest.mark.parametrize("n", [40, 70])
@pytest.mark.parametrize("pendant", [False, True])
def test_parking_buffer_fills_and_wraps(K, O, monkeypatch, n, pendant):
    """K_40 and K_70 alone: every candidate is a survivor, so a batch of 64 edges parks several hundred (the first 64 edges of
    row 0 of K_70: 2 336) -- the buffer takes up to 4 x 64 on top of a remainder trip after trip and is emptied from its top.
    With a pendant path on vertex 0 (which then has the highest degree and ranks last) batches mix full and empty lanes."""
    uv, nv = _clique(n), n
    if pendant:
        uv, nv = np.concatenate([uv, _path(0, 100, n)]), n + 100
    want = _check(K, O, monkeypatch, nv, uv)
    assert want["tr"].max() == n and want["tri"] == n * (n - 1) * (n - 2) // 6


@pytest.mark.parametrize("r", [2, 4, 5, 6, 64])
def test_compaction_at_chunk_edges(K, O, monkeypatch, r):
    """A vertex joined to r mutually adjacent higher-ranked vertices (K_{r+1}: its first row): 1, 3, 4, 5 and 63 candidates
    behind the row's first edge -- one slot of a chunk of 4, three, exactly one chunk, a chunk and one slot, and 16 chunks less
    one slot.  Three copies and a path, in a graph with enough (isolated) vertices that a task groups 32 of them: the rows
    of several vertices share a batch, so chunks of different rows meet in one trip."""
    parts, base = [], 0
    for _ in range(3):
        parts.append(_clique(r + 1, base))
        base += r + 1
    parts.append(_path(0, 7, base))
    want = _check(K, O, monkeypatch, GROUPED_NV, np.concatenate(parts))
    assert want["tri"] == 3 * (r + 1) * r * (r - 1) // 6


@pytest.mark.parametrize("slots", [TRI_CAP, TRI_CAP + 1])
def test_tri_cap_boundary(K, O, monkeypatch, slots):
    """A vertex whose oriented row has exactly kTriCap slots (K_257: staged, a parked candidate carries the largest slot
    number, 255) and one with kTriCap + 1 (K_258: that row runs unstaged, cut into parts, its candidates read from global
    memory, its triangles parked in the record buffer).  The library exposes no such constant: 256 and 257 are kTriCap and
    kTriCap + 1 of komb_amd/csrc/truss_line.h."""
    n = slots + 1
    want = _check(K, O, monkeypatch, n, _clique(n))
    assert want["tr"].max() == n


@pytest.mark.parametrize("scratch", [True, False])
def test_sub_range_beyond_the_record_buffer(K, O, monkeypatch, scratch):
    """K_100: row 0 has 99 slots, well under kTriCap, and C(99, 2) = 4 851 triangles, 12 times kTriRec -- the LDS record
    buffer fills again and again.  With the wavefront's scratch its records move there and the dense own-role block is still
    written; without it (KOMB_NO_REC_SCRATCH) the sub-range's own-role entries become records (the spilled branch)."""
    assert 99 < TRI_CAP and 99 * 98 // 2 > 4 * TRI_REC
    extra = None if scratch else {"KOMB_NO_REC_SCRATCH": "1"}
    want = _check(K, O, monkeypatch, 100, _clique(100), extra_env=extra)
    assert want["tri"] == 161700


def test_append_claim_runs_out_inside_one_append(K, O, monkeypatch):
    """K_48: row 0 is a task of its own (one wavefront) with C(47, 2) = 1 081 triangles, so that wavefront writes 1 081
    third-role records: more than one claim of kRecChunk = 1 024, fewer than two, and the first claim runs out inside an
    append of 64.  (In a graph this small every vertex is its own task.)"""
    t = 47 * 46 // 2
    assert REC_CHUNK < t < 2 * REC_CHUNK
    want = _check(K, O, monkeypatch, 48, _clique(48))
    assert want["stats"]["tri_records"] >= want["tri"]


@pytest.mark.parametrize("poison", [None, "0xFFFFFFFF", "0x00000001"])
def test_random_graph_with_planted_clique(K, O, monkeypatch, poison):
    """A seeded random graph of about 2 x 10^4 edges on 3 000 vertices with a planted K_30 (and isolated vertices up to
    GROUPED_NV, so that tasks group 32 rows), at both index layouts, on clean and on poisoned device memory."""
    rng = np.random.default_rng(20)
    nv = 3000
    uv = rng.integers(0, nv, size=(20000, 2), dtype=np.int64)
    uv = uv[uv[:, 0] != uv[:, 1]]
    members = rng.choice(nv, 30, replace=False).astype(np.int64)
    i, j = np.triu_indices(30, 1)
    uv = np.concatenate([uv, np.stack([members[i], members[j]], axis=1)])
    want = _check(K, O, monkeypatch, GROUPED_NV, uv, extra_env={"KOMB_POISON": poison} if poison else None)
    assert want["tr"].max() >= 30
