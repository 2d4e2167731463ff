// nucleus_search_dev.h -- the 4-clique search over the oriented canonical edge list that nucleus.hip (the decomposition) and
// nucleus_hierarchy.hip (the nuclei and their forest) share: row a = the positions [rs[a], re[a]) with eu == a, their ev
// ascending.  DESIGN.md section 4.6h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace komb {

constexpr uint32_t kNucNone = 0xFFFFFFFFu;

struct NucTri {                             // per triangle: vertices (the result), the position of (a, b), of (a, c), of (b, c)
    int32_t *a, *b, *c;
    uint32_t *j, *pac, *pbc;
};

// the position of x in ev[lo, end) (ascending), kNucNone if it is not there
__device__ __forceinline__ uint32_t nuc_find(const int32_t *__restrict__ ev, int32_t x, uint32_t lo, uint32_t end)
{
    uint32_t hi = end;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ev[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < end && ev[lo] == x ? lo : kNucNone;
}

__device__ __forceinline__ unsigned long long nuc_below(int lane) { return (1ull << lane) - 1ull; }

// The three tails of triangle t = (a, b, c) a fourth vertex d > c can be in: row a behind (a, c), row b behind (b, c), all of
// row c.  [it, it + n) is the shortest and is walked; the other two are searched.
struct NucTails { uint32_t it, n, lo1, hi1, lo2, hi2; };

// the triangle given by value: its vertices and the positions of (a, c) and (b, c)
__device__ __forceinline__ NucTails nuc_tails(int32_t a, int32_t b, int32_t c, uint32_t pac, uint32_t pbc, const uint32_t *__restrict__ rs,
                                              const uint32_t *__restrict__ re)
{
    const uint32_t al = pac + 1, ah = re[a], bl = pbc + 1, bh = re[b], cl = rs[c], ch = re[c];
    const uint32_t na = ah - al, nb = bh - bl, nc = ch - cl;
    NucTails s;
    if (na <= nb && na <= nc) { s.it = al; s.n = na; s.lo1 = bl; s.hi1 = bh; s.lo2 = cl; s.hi2 = ch; }
    else if (nb <= nc) { s.it = bl; s.n = nb; s.lo1 = al; s.hi1 = ah; s.lo2 = cl; s.hi2 = ch; }
    else { s.it = cl; s.n = nc; s.lo1 = al; s.hi1 = ah; s.lo2 = bl; s.hi2 = bh; }
    return s;                                            // (the walked tail is the shortest: an empty tail gives n = 0)
}

__device__ __forceinline__ NucTails nuc_tails(const NucTri &o, const uint32_t *__restrict__ rs, const uint32_t *__restrict__ re, uint32_t t)
{
    return nuc_tails(o.a[t], o.b[t], o.c[t], o.pac[t], o.pbc[t], rs, re);
}

// entry x of the walked tail: a 4-clique iff its vertex d is in the other two tails as well; p1 / p2: where it is in them
// (with x itself the positions of (a, d), (b, d), (c, d) in some order), valid only when it returns true
__device__ __forceinline__ bool nuc_clq_entry(const int32_t *__restrict__ ev, const NucTails &s, uint32_t x, uint32_t *p1, uint32_t *p2)
{
    const int32_t d = ev[x];
    *p1 = nuc_find(ev, d, s.lo1, s.hi1);
    if (*p1 == kNucNone) return false;
    *p2 = nuc_find(ev, d, s.lo2, s.hi2);
    return *p2 != kNucNone;
}

__device__ __forceinline__ bool nuc_clq_entry(const int32_t *__restrict__ ev, const NucTails &s, uint32_t x)
{
    uint32_t p1, p2;
    return nuc_clq_entry(ev, s, x, &p1, &p2);
}

} // namespace komb
