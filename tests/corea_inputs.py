"""(degree, coreness) inputs for CoreA that no graph produces, and a second reference ranker.

CoreA ranks key = coreness * n + degree (64-bit) and degree.  Every (degree, coreness) a test takes from a graph keeps the
key below 2^31 and has power-law ties; the families here reach what those never do: keys of 32, 33 and 52 bits, keys equal
or different in their low word only, one run, two runs split at either end, all-distinct keys, degrees at the powers of
two where the number of sorted bits changes, and (marked BIG) an n above 4096 * 256, where the kernels' grid-stride loops
take a second turn.

Plain module, no GPU, shared by tests/test_corea_inputs_ref.py (CPU) and tests/test_gpu_host_inputs.py (GPU).

Two families cannot exist at every size, because degree and coreness are int32:
  * "cross32" at n = 1: the key is coreness + degree <= 2^31 + 4, so it cannot reach 2^32.  The case is still generated
    (coreness at its cap); the 33-bit claim is asserted for n >= 2.
  * "samelow" needs (c2 - c1) * n = 0 mod 2^32 with c2 - c1 < 2^31, that is n a multiple of 4: of the common sizes only
    256.  The family adds 512 and 4096 of its own so that it has more than one size.
"""
import functools

import numpy as np

SIZES = (1, 2, 255, 256, 257, 4097)
BIG = 4096 * 256 + 513                  # one more than a whole turn of 4096 blocks x 256 threads, plus an odd tail
I32_MAX = 2**31 - 1
SEED = 20240607


def np_fractional_rank(keys):
    """Descending fractional rank: a key with `greater` larger keys before it and `count` equals occupies the 1-based
    positions greater+1 .. greater+count, and gets their mean.  No sort of its own: np.unique does the grouping."""
    keys = np.asarray(keys, dtype=np.int64)
    if len(keys) == 0:
        return np.zeros(0, dtype=np.float64)
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    # np.unique is ascending: the keys greater than unique[j] are those of unique[j+1:]
    greater = (len(keys) - np.cumsum(counts))[inverse]
    count = counts[inverse]
    return ((greater + 1) + (greater + count)).astype(np.float64) / 2.0


def keys_of(deg, core):
    """The 64-bit key CoreA ranks besides the degree."""
    return core.astype(np.int64) * len(deg) + deg.astype(np.int64)


def max_key_bits(deg, core):
    return int(keys_of(deg, core).max()).bit_length() if len(deg) else 0


def _i32(x):
    x = np.asarray(x)
    assert x.min() >= 0 and x.max() <= I32_MAX
    return np.ascontiguousarray(x, dtype=np.int32)


def _families(rng, n, big):
    """(family name, deg, core) of every family that has a case at this n; big: only the families marked for n = BIG."""
    zero = np.zeros(n, dtype=np.int64)

    if not big:
        yield "zeros", zero, zero

    deg = np.ones(n, dtype=np.int64)
    deg[n - 1] = 0
    yield "ones", deg, zero

    yield "distinct", rng.permutation(n), zero

    if not big:
        for p in sorted({p for p in (1, n // 2, n - 1) if 1 <= p < n}):
            deg = np.full(n, 3, dtype=np.int64)
            deg[rng.permutation(n)[:p]] = 7
            yield "tworuns_p%d" % p, deg, zero

        for b in (1, 8, 16, 30):
            deg = rng.choice(np.array([2**b - 1, 2**b], dtype=np.int64), n)
            yield "pow2_b%d" % b, deg, zero
        deg = rng.choice(np.array([2**30, 2**31 - 2, I32_MAX], dtype=np.int64), n)
        deg[rng.integers(0, n)] = I32_MAX
        yield "pow2_max", deg, zero

    # the largest coreness of the range sits at one element, so that the family reaches its range at every n
    for name, top in (("cross31", 2**31), ("cross32", 2**32)):
        if big and name != "cross31":
            continue
        hi = min(top // n + 1, I32_MAX)
        core = rng.integers(0, hi + 1, n)
        deg = rng.integers(0, 6, n)
        at = rng.integers(0, n)
        core[at], deg[at] = hi, 5
        yield name, deg, core

    core = rng.integers(0, 2**31, n)
    deg = rng.integers(0, 2**31, n)
    core[rng.integers(0, n)] = I32_MAX
    yield "wide", deg, core

    if not big:
        core = np.full(n, I32_MAX, dtype=np.int64)
        yield "degties", rng.integers(0, 4, n), core

        core = rng.integers(0, 2, n)
        core[n - 1], core[0] = 0, 1
        yield "difflow", rng.integers(0, n, n), core


def _same_low_word(rng, n):
    """coreness * n takes two values with the same low 32 bits: c and c + 2^32 / gcd(n, 2^32)."""
    step = 2**32 // (n & -n)
    assert n % 4 == 0 and step < 2**31
    c = int(rng.integers(1, 2**31 - step))
    core = np.where(rng.integers(0, 2, n) == 1, c + step, c)
    core[0], core[n - 1] = c + step, c
    assert ((core * n) & 0xFFFFFFFF).min() == ((core * n) & 0xFFFFFFFF).max()
    return np.zeros(n, dtype=np.int64), core


@functools.lru_cache(maxsize=None)
def all_cases():
    """Tuple of (name, deg int32[n], core int32[n]); name = family-n<n>-b<bit length of the largest key>.  Read-only."""
    rng = np.random.default_rng(SEED)
    out = []

    def add(family, n, deg, core):
        deg, core = _i32(deg), _i32(core)
        deg.setflags(write=False)
        core.setflags(write=False)
        out.append(("%s-n%d-b%d" % (family, n, max_key_bits(deg, core)), deg, core))

    for n in SIZES:
        for family, deg, core in _families(rng, n, big=False):
            add(family, n, deg, core)
    for n in (256, 512, 4096):
        add("samelow", n, *_same_low_word(rng, n))
    for family, deg, core in _families(rng, BIG, big=True):
        add(family, BIG, deg, core)
    assert sum(1 for _, d, _ in out if len(d) == BIG) <= 4
    assert len({name for name, _, _ in out}) == len(out)
    return tuple(out)


def cases():
    """Yields (name, deg int32[n], core int32[n]) for every family and size, from a fixed seed."""
    yield from all_cases()


def case_names():
    return [name for name, _, _ in all_cases()]


def case(name):
    for c in all_cases():
        if c[0] == name:
            return c
    raise KeyError(name)


def family_of(name):
    return name.split("-")[0]
