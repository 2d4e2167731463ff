// clique_root_dev.h -- the root of a clique subproblem over the oriented canonical edge list, shared by max_clique.hip (the
// maximum-clique search), clique_census.hip (the k-clique counts) and maximal_cliques.hip (the maximal cliques): row a = the
// positions [rs[a], re[a]) with eu == a, their ev ascending.  A clique is handled at its ROOT, the canonical edge (a, b) of its
// two smallest ids; its other vertices are in P = {c > b : (a, c) and (b, c) in H, both of trussness >= need}.  One wavefront (a
// workgroup of its own) owns a root: clq_cut cuts P, clq_matrix makes P's adjacency a bit matrix, rows of W = ceil(|P| / 64)
// 64-bit words, lane w owning word w of every row.  The maximal cliques also need the common neighbours below b: clq_cut_x cuts
// them from the lower rows, and clq_matrix takes X ++ P as it takes P.  DESIGN.md sections 4.6j, 4.6k and 4.6l.
#pragma once

#include "common.h"
#include "nucleus_search_dev.h"

namespace komb {

constexpr uint32_t kClqMaxCand = 4096;                // candidates of one root: one 64-bit word per lane

struct ClqGraph {
    const int32_t *eu, *ev, *tr;
    const uint32_t *rs, *re;
};

static __global__ void k_clq_rows(const int32_t *__restrict__ eu, uint32_t m, uint32_t *__restrict__ rs, uint32_t *__restrict__ re)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const int32_t u = eu[j];
    if (j == 0 || eu[j - 1] != u) rs[u] = j;
    if (j + 1 == m || eu[j + 1] != u) re[u] = j + 1;
}

__device__ __forceinline__ unsigned long long clq_shfl64(unsigned long long x, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int32_t)(uint32_t)x, src), hi = (uint32_t)__shfl((int32_t)(uint32_t)(x >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ int clq_sum(int x)
{
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// the first position of [lo, hi) whose entry is not below x
__device__ __forceinline__ uint32_t clq_lower(const int32_t *__restrict__ a, int32_t x, uint32_t lo, uint32_t hi)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// |P| of the root rj = (a, b): the shorter of (row a behind rj, row b) is walked 64 entries at a time, the other bisected; both
// are ascending, so P is.  With fill the first cap_p candidates go to P.  Every branch is uniform over the wave.
__device__ __forceinline__ uint32_t clq_cut(const ClqGraph &G, uint32_t rj, uint32_t need, int32_t *P, uint32_t cap_p, bool fill, int lane)
{
    const int32_t *__restrict__ ev = G.ev;
    const int32_t *__restrict__ tr = G.tr;
    const int32_t a = G.eu[rj], b = ev[rj];
    const uint32_t ab = rj + 1, ae = G.re[a], bb = G.rs[b], be = G.re[b];
    const bool walk_a = ae - ab <= be - bb;
    const uint32_t it = walk_a ? ab : bb, len = walk_a ? ae - ab : be - bb, lo = walk_a ? bb : ab, hi = walk_a ? be : ae;
    uint32_t n = 0;
    if (hi > lo)
        for (uint32_t x0 = it; x0 < it + len; x0 += kWave) {
            const uint32_t x = x0 + (uint32_t)lane;
            bool ok = false;
            int32_t c = 0;
            if (x < it + len && (uint32_t)tr[x] >= need) {
                c = ev[x];
                const uint32_t hit = nuc_find(ev, c, lo, hi);
                ok = hit != kNucNone && (uint32_t)tr[hit] >= need;
            }
            const unsigned long long hits = __ballot(ok);
            if (ok && fill) {
                const uint32_t pos = n + (uint32_t)__popcll(hits & nuc_below(lane));
                if (pos < cap_p) P[pos] = c;
            }
            n += (uint32_t)__popcll(hits);
        }
    return n;
}

// The LOWER ROWS (maximal_cliques.hip makes them, once per run): lower row b = the entries [ls[b], le[b]) of lu / lpos, one per
// canonical edge with ev == b, lu = its eu (ascending), lpos = its position in the canonical list.
struct ClqLower {
    const int32_t *lu;
    const uint32_t *lpos, *ls, *le;
};

// a part [lo, hi) of a row, ids ascending; entry i is the canonical edge pos[i], or i itself without pos (a row of the list)
struct ClqSpan {
    const int32_t *id;
    const uint32_t *pos;
    uint32_t lo, hi;
};

// The vertices of both spans whose two edges have trussness >= need, ascending, appended at X[n]: the shorter span is walked 64
// entries at a time, the other bisected.  With fill what lies below cap is written.  Returns the new n.
__device__ __forceinline__ uint32_t clq_meet(const int32_t *__restrict__ tr, ClqSpan r, ClqSpan s, uint32_t need, int32_t *X, uint32_t n, uint32_t cap,
                                             bool fill, int lane)
{
    const uint32_t nr = r.hi > r.lo ? r.hi - r.lo : 0u, ns = s.hi > s.lo ? s.hi - s.lo : 0u;
    if (nr == 0 || ns == 0) return n;
    if (nr > ns) { const ClqSpan t = r; r = s; s = t; }
    for (uint32_t x0 = r.lo; x0 < r.hi; x0 += kWave) {
        const uint32_t x = x0 + (uint32_t)lane;
        bool ok = false;
        int32_t c = 0;
        if (x < r.hi && (uint32_t)tr[r.pos ? r.pos[x] : x] >= need) {
            c = r.id[x];
            const uint32_t hit = nuc_find(s.id, c, s.lo, s.hi);
            ok = hit != kNucNone && (uint32_t)tr[s.pos ? s.pos[hit] : hit] >= need;
        }
        const unsigned long long hits = __ballot(ok);
        if (ok && fill) {
            const uint32_t pos = n + (uint32_t)__popcll(hits & nuc_below(lane));
            if (pos < cap) X[pos] = c;
        }
        n += (uint32_t)__popcll(hits);
    }
    return n;
}

// |X| of the root rj = (a, b), X = {x < b, x != a : (x, a) and (x, b) in H, both of trussness >= need}: x < a from the lower rows
// of a and b, a < x < b from row a before rj and the lower row of b behind a.  Both parts are ascending and the first lies below
// the second, so X is ascending.  With fill the first cap_x go to X.  Every branch is uniform over the wave.
__device__ __forceinline__ uint32_t clq_cut_x(const ClqGraph &G, const ClqLower &L, uint32_t rj, uint32_t need, int32_t *X, uint32_t cap_x, bool fill, int lane)
{
    const int32_t a = G.eu[rj], b = G.ev[rj];
    const uint32_t lb = L.ls[b], le = L.le[b];
    const uint32_t ia = clq_lower(L.lu, a, lb, le);      // (a itself is in the lower row of b: the edge rj)
    const uint32_t behind = ia < le ? ia + 1 : le;
    uint32_t n = clq_meet(G.tr, ClqSpan{L.lu, L.lpos, L.ls[a], L.le[a]}, ClqSpan{L.lu, L.lpos, lb, ia}, need, X, 0u, cap_x, fill, lane);
    n = clq_meet(G.tr, ClqSpan{G.ev, nullptr, G.rs[a], rj}, ClqSpan{L.lu, L.lpos, behind, le}, need, X, n, cap_x, fill, lane);
    return n;
}

// The bit matrix of P[0, n), n <= cap_p, which clq_cut has just written: bit j of row i <=> P[i] and P[j] are joined by an edge
// of trussness >= need.  mat (n * W words) is LDS or global; it is read with plain loads after the call.
__device__ __forceinline__ void clq_matrix(const ClqGraph &G, uint32_t need, const int32_t *P, uint32_t n, uint32_t W,
                                           unsigned long long *mat, int lane)
{
    const int32_t *__restrict__ ev = G.ev;
    const int32_t *__restrict__ tr = G.tr;
    __threadfence();                                     // (P: written by some lanes, read by all)
    __syncthreads();
    if (n == 0) return;                                  // (a single candidate still needs its zero row)
    for (uint32_t i = (uint32_t)lane; i < n * W; i += kWave) mat[i] = 0ull;
    __threadfence();
    __syncthreads();
    uint32_t *m32 = (uint32_t *)mat;
    const int32_t p_last = P[n - 1];
    for (uint32_t i = 0; i + 1 < n; ++i) {
        const int32_t c = P[i];
        const uint32_t ce = G.re[c];
        const uint32_t cs = clq_lower(ev, P[i + 1], G.rs[c], ce);   // (row c is above c; what is below P[i + 1] is not in P)
        for (uint32_t x0 = cs; x0 < ce; x0 += kWave) {
            const uint32_t x = x0 + (uint32_t)lane;
            bool past = false;
            if (x < ce) {
                const int32_t dd = ev[x];
                if (dd > p_last) past = true;
                else if ((uint32_t)tr[x] >= need) {
                    const uint32_t pos = clq_lower(P, dd, i + 1, n);
                    if (pos < n && P[pos] == dd) {
                        atomicOr(m32 + ((size_t)i * W * 2 + (pos >> 5)), 1u << (pos & 31u));
                        atomicOr(m32 + ((size_t)pos * W * 2 + (i >> 5)), 1u << (i & 31u));
                    }
                }
            }
            if (__any(past)) break;
        }
    }
    __threadfence();                                     // (the atomics went to L2: the rows are read with plain loads from here on)
    __syncthreads();
}

} // namespace komb
