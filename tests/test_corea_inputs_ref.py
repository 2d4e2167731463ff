"""CPU tests of the CoreA host inputs (tests/corea_inputs.py): the oracle's 64-bit ranker against the numpy restatement on
every case, the closed forms, and the key ranges the families claim -- asserted from the inputs, so that the GPU test
that runs the same cases is known to reach keys of 2^31 and more."""
import numpy as np
import pytest

import corea_inputs as C


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def _exact_rank_sum(rank):
    twice = rank * 2.0                                   # ranks are half-integers: twice a rank is an exact integer
    assert np.array_equal(twice, np.floor(twice))
    return int(twice.astype(np.int64).sum())


@pytest.mark.parametrize("name", C.case_names())
def test_oracle_ranker_equals_numpy_restatement(O, name):
    _, deg, core = C.case(name)
    n = len(deg)
    key = C.keys_of(deg, core)
    assert int(key.max()).bit_length() == int(name.rsplit("-b", 1)[1])
    rank_key, rank_deg = C.np_fractional_rank(key), C.np_fractional_rank(deg)
    assert np.array_equal(O.fractional_rank_fast(key), rank_key)
    assert np.array_equal(O.fractional_rank_fast(deg.astype(np.int64)), rank_deg)
    for rank in (rank_key, rank_deg):
        assert rank.min() >= 1.0 and rank.max() <= n
        assert _exact_rank_sum(rank) == n * (n + 1)      # sum(rank) == n (n + 1) / 2

    family = C.family_of(name)
    if family == "zeros":
        assert np.array_equal(rank_deg, np.full(n, (n + 1) / 2.0)) and np.array_equal(rank_key, rank_deg)
    if family == "ones":
        want = np.full(n, n / 2.0)                       # positions 1 .. n-1, then n alone
        want[n - 1] = n
        assert np.array_equal(rank_deg, want)
    if family == "distinct":
        assert np.array_equal(np.sort(deg), np.arange(n))
        assert np.array_equal(rank_deg, (n - deg).astype(np.float64))
    if family.startswith("tworuns"):
        p = int(family.split("_p")[1])
        assert int((deg == deg.max()).sum()) == p and len(np.unique(deg)) == 2
        assert np.array_equal(rank_deg, np.where(deg == deg.max(), (1 + p) / 2.0, (p + 1 + n) / 2.0))
    if family == "degties":
        assert np.all(core == C.I32_MAX)
        assert np.array_equal(rank_key, rank_deg)


def test_families_reach_the_key_ranges_they_claim():
    seen = set()
    for name, deg, core in C.cases():
        family, n = C.family_of(name), len(deg)
        seen.add((family, n))
        bits = C.max_key_bits(deg, core)
        if family == "cross31":
            assert bits >= 32, name
        if family == "cross32" and n >= 2:               # (n = 1: the key is coreness + degree < 2^32; corea_inputs.py)
            assert bits >= 33, name
        if family == "wide" and n == C.BIG:
            assert bits >= 50, name
        if family == "pow2_max":
            assert int(deg.max()) == 2**31 - 1, name
        if family == "samelow":
            prod = core.astype(np.int64) * n
            assert len(np.unique(prod)) == 2 and len(np.unique(prod & 0xFFFFFFFF)) == 1 and not deg.any(), name
        if family == "difflow":
            prod = core.astype(np.int64) * n
            assert set(np.unique(core).tolist()) <= {0, 1} and int(prod.max() & 0xFFFFFFFF) == n, name
            assert int(deg.max()) < n, name
    for family in ("zeros", "ones", "distinct", "pow2_b1", "pow2_b8", "pow2_b16", "pow2_b30", "pow2_max", "cross31", "cross32",
                   "wide", "degties", "difflow"):
        for n in C.SIZES:
            assert (family, n) in seen, (family, n)
    for n in C.SIZES[1:]:
        for p in {1, n // 2, n - 1}:
            assert ("tworuns_p%d" % p, n) in seen
    assert {f for f, n in seen if n == C.BIG} == {"ones", "distinct", "cross31", "wide"}
    assert C.BIG > 4096 * 256
    assert sum(1 for f, _ in seen if f == "samelow") >= 2


def test_truncating_a_key_to_32_bits_changes_the_order():
    """A ranker that dropped the high word of the key would be caught: the ranks of key and of key & 0xFFFFFFFF differ."""
    changed = []
    for name, deg, core in C.cases():
        key = C.keys_of(deg, core)
        if not np.array_equal(C.np_fractional_rank(key), C.np_fractional_rank(key & 0xFFFFFFFF)):
            changed.append(C.family_of(name))
    assert {"cross32", "wide", "samelow"} <= set(changed)    # (cross31 keys fit in 32 unsigned bits)
    # ... and one that multiplied in 32 bits as well (sign-extended product, then + degree)
    changed = []
    for name, deg, core in C.cases():
        n = len(deg)
        wrapped = (core.astype(np.int64) * n).astype(np.int32).astype(np.int64) + deg
        if not np.array_equal(C.np_fractional_rank(C.keys_of(deg, core)), C.np_fractional_rank(wrapped)):
            changed.append(C.family_of(name))
    assert {"cross31", "cross32", "wide", "samelow"} <= set(changed)


def _small_int_keys():
    return [name for name, deg, core in C.cases() if len(deg) <= 4097 and C.max_key_bits(deg, core) <= 31]


@pytest.mark.parametrize("name", _small_int_keys())
def test_scores_faithful_equals_fast_below_2_31(O, name):
    """Where the reference's `int` key does not overflow, its O(U n) ranker and the sort-based one give the same scores;
    where the reference's own CoreA.h is built (oracle/_ref/corea_ref), its scores print the same "%f" text."""
    _, deg, core = C.case(name)
    fast = O.corea_scores(deg, core, faithful=False)
    assert np.array_equal(O.corea_scores(deg, core, faithful=True), fast)
    assert not np.isnan(fast).any()
    if O.ref_corea_path() is not None:
        ref = O.ref_corea_scores(deg, core)
        assert ["%f" % s for s in ref] == ["%f" % s for s in fast]
