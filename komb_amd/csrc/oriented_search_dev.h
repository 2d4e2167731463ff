// oriented_search_dev.h -- the one triangle and 4-clique search over the oriented canonical edge list: row a = the positions
// [rs[a], re[a]) with eu == a, their ev ascending.  Its users: communities.hip and community_hierarchy.hip (over their member
// lists), nucleus.hip, nucleus_hierarchy.hip, graphlets.hip and, through clique_root_dev.h, the three clique walks.  Here are
// the row bounds, the two sides of an edge, the three tails of a triangle, the one bisection and the triangle id.  What a hit
// does is each user's own.  DESIGN.md sections 4.6c, 4.6e, 4.6h.  The lane / wave tiers (wave_turns, from_lane, wave_walk,
// wave_walk_all) and THE WAVE RULE they come with are wave_dev.h's; here are from_lane's overloads for the two units.
#pragma once

#include "wave_dev.h"

namespace komb {

constexpr uint32_t kNucNone = 0xFFFFFFFFu;

struct NucTri {                             // per triangle: vertices (the result), the position of (a, b), of (a, c), of (b, c)
    int32_t *a, *b, *c;
    uint32_t *j, *pac, *pbc;
};

// ---- row bounds per original vertex (rs / re zeroed before: a vertex without a row has an empty one).  The list's length is m,
// or *n_mem when it is known on the device only; m is then the host's bound and sizes the grid.
static __global__ void k_rows(const int32_t *__restrict__ eu, uint32_t m, const uint32_t *__restrict__ n_mem, uint32_t *__restrict__ rs,
                              uint32_t *__restrict__ re)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x, n = n_mem ? *n_mem : m;
    if (j >= n) return;
    const int32_t u = eu[j];
    if (j == 0 || eu[j - 1] != u) rs[u] = j;
    if (j + 1 == n || eu[j + 1] != u) re[u] = j + 1;
}

// rs / re of the list eu[0, m) (m > 0; n_mem as above, or nullptr), nv words each from bufs
inline int oriented_rows(komb_ctx *ctx, DevBufs &bufs, const int32_t *eu, int64_t m, const uint32_t *n_mem, uint32_t **rs, uint32_t **re)
{
    hipStream_t s = ctx->stream;
    const size_t nv = (size_t)ctx->nv;
    KOMB_HIP(ctx, bufs.alloc(rs, nv));
    KOMB_HIP(ctx, bufs.alloc(re, nv));
    KOMB_HIP(ctx, hipMemsetAsync(*rs, 0, nv * sizeof(uint32_t), s));
    KOMB_HIP(ctx, hipMemsetAsync(*re, 0, nv * sizeof(uint32_t), s));
    k_rows<<<(int)((m + kBlock - 1) / kBlock), kBlock, 0, s>>>(eu, (uint32_t)m, n_mem, *rs, *re);
    return KOMB_OK;
}

// ---- the one bisection: the first position of a[lo, hi) (ascending) whose entry is not below x
template <class T>
__device__ __forceinline__ uint32_t row_lower(const T *__restrict__ a, T x, uint32_t lo, uint32_t hi)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the position of x in ev[lo, end) (ascending), kNucNone if it is not there
__device__ __forceinline__ uint32_t nuc_find(const int32_t *__restrict__ ev, int32_t x, uint32_t lo, uint32_t end)
{
    lo = row_lower(ev, x, lo, end);
    return lo < end && ev[lo] == x ? lo : kNucNone;
}

// the id of the triangle of the edge at position e whose third vertex is d: a bisection in e's ascending part of tc[].  Three
// edges of the result that close a triangle the triangle list does not hold (cannot happen; checked): *bad is set.
__device__ __forceinline__ uint32_t tri_id(const uint32_t *__restrict__ tri_ptr, const int32_t *__restrict__ tc, uint32_t e, int32_t d,
                                           uint32_t fallback, uint32_t *bad)
{
    uint32_t lo = tri_ptr[e];
    const uint32_t end = tri_ptr[e + 1];
    lo = row_lower(tc, d, lo, end);
    if (lo < end && tc[lo] == d) return lo;
    *bad = 1u;
    return fallback;
}

__device__ __forceinline__ unsigned long long nuc_below(int lane) { return (1ull << lane) - 1ull; }

// ---- the units
// The two sides of edge j = (a, b) a third vertex c > b can be in: row a behind j, and row b.  [it, it + n) is the shorter and
// is walked, [lo, hi) is searched; n <= hi - lo.  walk_a: the walked side is row a's, so x is the position of (a, c) and the
// hit that of (b, c); else the other way round.
struct EdgeSides { uint32_t it, n, lo, hi; bool walk_a; };

__device__ __forceinline__ EdgeSides edge_sides(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                                                const uint32_t *__restrict__ re, uint32_t j)
{
    const int32_t a = eu[j], b = ev[j];
    const uint32_t ab = j + 1, ae = re[a], bb = rs[b], be = re[b];   // (row a holds j: ae > j)
    const uint32_t la = ae - ab, lb = be - bb;
    EdgeSides s;
    s.walk_a = la <= lb;
    if (s.walk_a) { s.it = ab; s.n = la; s.lo = bb; s.hi = be; }
    else { s.it = bb; s.n = lb; s.lo = ab; s.hi = ae; }
    if (s.hi == s.lo) s.n = 0;
    return s;
}

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

// ---- a lane's unit handed to the whole wave (wave_turns)
__device__ __forceinline__ EdgeSides from_lane(const EdgeSides &s, int src)
{
    EdgeSides r;
    r.it = from_lane(s.it, src); r.n = from_lane(s.n, src); r.lo = from_lane(s.lo, src); r.hi = from_lane(s.hi, src);
    r.walk_a = from_lane((uint32_t)s.walk_a, src) != 0;
    return r;
}

__device__ __forceinline__ NucTails from_lane(const NucTails &s, int src)
{
    return NucTails{from_lane(s.it, src), from_lane(s.n, src), from_lane(s.lo1, src), from_lane(s.hi1, src), from_lane(s.lo2, src),
                    from_lane(s.hi2, src)};
}

} // namespace komb
