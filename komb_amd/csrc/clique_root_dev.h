// clique_root_dev.h -- what the analyses that walk cliques from a root share: max_clique.hip (the maximum-clique search),
// clique_census.hip (the k-clique counts) and maximal_cliques.hip (the maximal cliques).  They read the oriented canonical edge
// list: row a = the positions [rs[a], re[a]) with eu == a, their ev ascending.  A clique is handled at its ROOT, the canonical
// edge (a, b) of its two smallest ids; its other vertices are in P = {c > b : (a, c) and (b, c) in H, both of trussness >= need}.
// One wavefront (a workgroup of its own) owns a root, lane w owning word w of every row and set.  Here are
//   * the root: clq_cut cuts P, clq_matrix makes P's adjacency a bit matrix, rows of W = ceil(|P| / 64) 64-bit words.  The maximal
//     cliques also need the common neighbours below b: clq_cut_x cuts them from the lower rows, and clq_matrix takes X ++ P as it
//     takes P;
//   * the driver: the launch constants, the control block ClqCtl with k_clq_tmax, a wave's bookkeeping (ClqWave, clq_node,
//     clq_count, clq_flush) and the hand-out of roots (clq_next_chunk, clq_finish);
//   * the layout: ClqLayout says where a root's candidates, matrix and stack live (LDS or the workgroup's slot of global scratch);
//     clq_layout sizes it on the host after the count launch, clq_place reads it on the device;
//   * the set idioms: clq_first, clq_prefix, and the max-neighbours pivot clq_pivot;
//   * the host's share of a run: clq_opt, clq_align16, clq_rows, clq_tmax.
// The walks are the analyses' own.  DESIGN.md sections 4.6j, 4.6k and 4.6l.
#pragma once

#include "oriented_search_dev.h"

#include <algorithm>

namespace komb {

constexpr uint32_t kClqMaxCand = 4096;                // candidates of one root: one 64-bit word per lane
constexpr uint32_t kClqNone = 0xFFFFFFFFu;
constexpr int kClqGrid = 1024;                        // wavefronts (workgroups of one) of a launch
constexpr uint32_t kClqBatch = 256;                   // nodes a wave adds to the counter at once, at most
static_assert((long long)kClqGrid * kClqBatch == KOMB_MAXCLQ_OVERSHOOT, "the documented overshoot");
constexpr uint32_t kClqLdsCand = 512;                 // default and largest *_LDS option: 512 x 8 words = 32 KiB
constexpr size_t kClqLdsBytes = 56u << 10;            // LDS of a workgroup (below the 64 KiB a launch gets without asking)
constexpr size_t kClqScratchBytes = 512ull << 20;     // all scratch slots of a launch together
constexpr long long kClqDefaultBudget = 1ll << 30;
constexpr long long kClqMaxBudget = 0x7FFFFFFFll - KOMB_MAXCLQ_OVERSHOOT;   // nodes (and so every per-vertex count) fit int32

struct ClqGraph {
    const int32_t *eu, *ev, *tr;
    const uint32_t *rs, *re;
};

__device__ __forceinline__ unsigned long long clq_shfl64(unsigned long long x, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int32_t)(uint32_t)x, src), hi = (uint32_t)__shfl((int32_t)(uint32_t)(x >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// x of lane src where src is a scalar (it comes from a ballot): two readlanes, no trip through the LDS crossbar
__device__ __forceinline__ unsigned long long clq_read64(unsigned long long x, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)x, src), hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(x >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ int clq_sum(int x)
{
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
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
    const uint32_t ia = row_lower(L.lu, a, lb, le);      // (a itself is in the lower row of b: the edge rj)
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
        const uint32_t cs = row_lower(ev, P[i + 1], G.rs[c], ce);   // (row c is above c; what is below P[i + 1] is not in P)
        for (uint32_t x0 = cs; x0 < ce; x0 += kWave) {
            const uint32_t x = x0 + (uint32_t)lane;
            bool past = false;
            if (x < ce) {
                const int32_t dd = ev[x];
                if (dd > p_last) past = true;
                else if ((uint32_t)tr[x] >= need) {
                    const uint32_t pos = row_lower(P, dd, i + 1, n);
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

// ---- the driver: one control block, a wave's bookkeeping, the hand-out of roots
struct ClqCtl {                                       // 64 bytes, zeroed before every run; an analysis leaves alone what it does not use
    unsigned long long nodes;                         // nodes spent, all launches
    unsigned long long n_roots;                       // roots opened
    unsigned long long n_cliques;                     // the search's enumeration: leaves of size omega
    unsigned long long list_words;                    // the maximal cliques: the stream's cursor, every report adds its size + 1
    uint32_t cursor;                                  // next chunk of 64 canonical edges (zeroed before every launch)
    uint32_t t_max;
    uint32_t max_cand;                                // count mode: the largest candidate list (|P|, or |X| + |P|)
    uint32_t bad;                                     // an inconsistency (cannot happen; checked)
    uint32_t stopped;                                 // a wave found the budget spent
    uint32_t best;                                    // the search: the largest clique found
    uint32_t saturated;                               // the census: an entry is 2^64 - 1
    uint32_t overflow;                                // the maximal cliques: a report found no room in the stream
};
static_assert(sizeof(ClqCtl) == 64, "ClqCtl layout");

// the largest trussness of the list, and best0 as the first lower bound (the search's; 0 leaves best alone)
static __global__ void k_clq_tmax(const int32_t *__restrict__ tr, uint32_t m, ClqCtl *ctl, uint32_t best0)
{
    int32_t hi = 0;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock) { const int32_t t = tr[j]; hi = t > hi ? t : hi; }
    for (int off = kWave / 2; off > 0; off >>= 1) { const int32_t other = __shfl_xor(hi, off); hi = other > hi ? other : hi; }
    if ((threadIdx.x & (kWave - 1)) == 0 && hi > 0) atomicMax(&ctl->t_max, (uint32_t)hi);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&ctl->best, best0);
}

__device__ __forceinline__ unsigned long long clq_nodes(ClqCtl *ctl) { return __hip_atomic_load(&ctl->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct ClqWave { uint32_t nodes, roots, max_cand; bool stop; };

__device__ __forceinline__ void clq_flush(ClqCtl *ctl, ClqWave &w, int lane)
{
    if (lane == 0 && w.nodes) atomicAdd(&ctl->nodes, (unsigned long long)w.nodes);
    w.nodes = 0;
}

// a node that needs no look at the budget: a root closed without a matrix, which the hand-out has just tested
__device__ __forceinline__ void clq_count(ClqCtl *ctl, ClqWave &w, int lane)
{
    if (w.nodes >= kClqBatch) clq_flush(ctl, w, lane);
    ++w.nodes;
}

// The top of every node of a walk: flush at the batch, stop at the budget, count the node.  False: the budget is spent and w.stop is
// set.  Every wave reads the counter at every node, so the overshoot is at most kClqBatch per wave (KOMB_MAXCLQ_OVERSHOOT in all).
__device__ __forceinline__ bool clq_node(ClqCtl *ctl, ClqWave &w, unsigned long long budget, int lane)
{
    if (w.nodes >= kClqBatch) clq_flush(ctl, w, lane);
    if (clq_nodes(ctl) + w.nodes >= budget) { w.stop = true; return false; }
    ++w.nodes;
    return true;
}

// The next chunk of 64 canonical edges off the cursor, false at the end of the list; tj = the trussness of this lane's edge of the
// chunk (0 behind the list).  The kernels ballot tj against their need and walk the ballot: root src is edge chunk * 64 + src.
__device__ __forceinline__ bool clq_next_chunk(ClqCtl *ctl, const int32_t *__restrict__ tr, uint32_t m, uint32_t n_chunks, uint32_t &chunk, uint32_t &tj,
                                               int lane)
{
    chunk = 0;
    if (lane == 0) chunk = atomicAdd(&ctl->cursor, 1u);
    chunk = (uint32_t)__shfl((int32_t)chunk, 0);
    if (chunk >= n_chunks) return false;
    const uint32_t j = chunk * kWave + (uint32_t)lane;
    tj = j < m ? (uint32_t)tr[j] : 0u;
    return true;
}

// the end of a kernel: what the wave still holds goes to the control block
__device__ __forceinline__ void clq_finish(ClqCtl *ctl, ClqWave &w, int lane)
{
    clq_flush(ctl, w, lane);
    if (lane == 0) {
        if (w.roots) atomicAdd(&ctl->n_roots, (unsigned long long)w.roots);
        if (w.max_cand) atomicMax(&ctl->max_cand, w.max_cand);
        if (w.stop) ctl->stopped = 1u;
    }
}

// ---- the layout: where the candidates, the matrix and the stack of a root live.  A stack level keeps `sets` candidate sets.
struct ClqLayout {
    unsigned char *scratch;                           // slot b: cand[cap] | mat[cap * w_max] | stk[levels * sets * w_max]
    size_t slot_bytes, off_mat, off_stk;
    uint32_t cap, levels;
    // LDS in 64-bit words: the index arrays, [levels] int32 each | the extra words | mat | stk; lds_levels == 0: the stack is global
    uint32_t lds_cand, lds_levels, lds_off_extra, lds_off_mat, lds_off_stk;
};

__device__ __forceinline__ unsigned char *clq_slot(const ClqLayout &L) { return L.scratch + (size_t)blockIdx.x * L.slot_bytes; }

struct ClqPlace { unsigned long long *mat, *stk; uint32_t levels; };

// A root of n candidates: the matrix in LDS up to lds_cand candidates, else in the slot; the stack beside it in LDS when it fits.
__device__ __forceinline__ ClqPlace clq_place(const ClqLayout &L, unsigned long long *smem, uint32_t n)
{
    unsigned char *slot = clq_slot(L);
    const bool in_lds = n <= L.lds_cand, stk_lds = in_lds && L.lds_levels > 0;
    return ClqPlace{in_lds ? smem + L.lds_off_mat : (unsigned long long *)(slot + L.off_mat),
                    stk_lds ? smem + L.lds_off_stk : (unsigned long long *)(slot + L.off_stk), stk_lds ? L.lds_levels : L.levels};
}

inline size_t clq_align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

struct ClqLaunch { int grid; size_t lds_bytes; bool fits; };   // fits: the head alone (index arrays, extra words) is within the LDS

// The layout after the count launch: roots of at most max_cand candidates, cliques of at most t_max vertices; idx index arrays
// and extra 64-bit words ahead of the matrix in LDS, `sets` per stack level, lds_opt the *_LDS option.  The launch that follows
// has the dynamic LDS and the grid returned: at most grid_cap workgroups, and no more than slots fit the scratch budget.
// L.scratch is the caller's to allocate, grid * slot_bytes.
inline ClqLaunch clq_layout(ClqLayout &L, uint32_t max_cand, uint32_t t_max, uint32_t idx, uint32_t extra, uint32_t sets, uint32_t lds_opt,
                            uint32_t n_chunks, int grid_cap)
{
    const uint32_t depth = t_max >= 2 ? t_max - 2 : 0;
    const uint32_t w_max = std::max<uint32_t>(1u, (max_cand + 63u) >> 6);
    L.cap = max_cand;
    L.levels = std::min(max_cand, depth) + 2;
    L.off_mat = clq_align16((size_t)max_cand * sizeof(int32_t));
    L.off_stk = L.off_mat + (size_t)max_cand * w_max * 8;
    L.slot_bytes = clq_align16(L.off_stk + (size_t)L.levels * sets * w_max * 8);
    // LDS: the head | the matrix of a root of up to lds_cand candidates | its stack, when that still fits
    const size_t head_words = clq_align16((size_t)L.levels * idx * sizeof(int32_t)) / 8 + extra;
    uint32_t n_l = std::min(max_cand, lds_opt);
    while (n_l > 0 && (head_words + (size_t)n_l * ((n_l + 63u) >> 6)) * 8 > kClqLdsBytes) n_l -= 1;
    const uint32_t w_l = (n_l + 63u) >> 6;
    L.lds_cand = n_l;
    L.lds_off_extra = (uint32_t)(head_words - extra);
    L.lds_off_mat = (uint32_t)head_words;
    L.lds_off_stk = L.lds_off_mat + n_l * w_l;
    L.lds_levels = std::min(n_l, depth) + 2;
    size_t lds_words = L.lds_off_stk;
    if (n_l > 0 && (lds_words + (size_t)L.lds_levels * sets * w_l) * 8 <= kClqLdsBytes) lds_words += (size_t)L.lds_levels * sets * w_l;
    else L.lds_levels = 0;
    int grid = (int)std::min<uint32_t>(n_chunks, (uint32_t)grid_cap);
    const size_t fit = kClqScratchBytes / L.slot_bytes;
    if ((size_t)grid > fit) grid = fit < 1 ? 1 : (int)fit;
    return ClqLaunch{grid, lds_words * 8, lds_words * 8 <= kClqLdsBytes};
}

// ---- sets spread over the wave, lane w holding word w
// bits [0, n) of the word that starts at bit base
__device__ __forceinline__ unsigned long long clq_prefix(uint32_t n, uint32_t base)
{
    if (n <= base) return 0ull;
    return n - base >= 64u ? ~0ull : (1ull << (n - base)) - 1ull;
}

// The first vertex of S, kClqNone when S is empty: the first lane with a bit, and that lane's first bit.  The lane is a scalar (it
// comes from the ballot), so its answer is read with one readlane and the result is a scalar too: a branch or a loop on it stays
// uniform over the wave for the compiler as well.
__device__ __forceinline__ uint32_t clq_first(unsigned long long S)
{
    const unsigned long long nz = __ballot(S != 0ull);
    if (!nz) return kClqNone;
    const int src = __ffsll((long long)nz) - 1;
    return (uint32_t)src * 64u + (uint32_t)__builtin_amdgcn_readlane(__ffsll((long long)S) - 1, src);
}

// The max-neighbours pivot: the vertex of U (not empty) with the most neighbours in P, the smallest such.
__device__ __forceinline__ uint32_t clq_pivot(unsigned long long P, unsigned long long U, const unsigned long long *mat, uint32_t W, int lane)
{
    const unsigned long long nzp = __ballot(P != 0ull);
    unsigned long long key = 0ull;                       // (neighbours + 1) << 32 | ~vertex: the largest wins
    for (unsigned long long wi = __ballot(U != 0ull); wi; wi &= wi - 1) {
        const int i = __ffsll((long long)wi) - 1;
        const bool in = (clq_read64(U, i) >> lane) & 1ull;
        const uint32_t u = (uint32_t)i * 64u + (uint32_t)lane;
        uint32_t c = 0;
        for (unsigned long long wj = nzp; wj; wj &= wj - 1) {
            const int j = __ffsll((long long)wj) - 1;
            const unsigned long long Pj = clq_read64(P, j);
            if (in) c += (uint32_t)__popcll(Pj & mat[(size_t)u * W + (uint32_t)j]);
        }
        const unsigned long long mine = ((unsigned long long)(c + 1u) << 32) | (0xFFFFFFFFu - u);
        if (in && mine > key) key = mine;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long other = clq_shfl64(key, lane ^ off);
        key = other > key ? other : key;
    }
    return 0xFFFFFFFFu - (uint32_t)key;
}

// ---- the host's share of a run; `who` is the public call the error texts name
inline long long clq_opt(const komb_ctx *ctx, const char *name, long long dflt, long long lo, long long hi)
{
    const char *e = ctx_opt(ctx, name);
    if (!e) return dflt;
    const long long v = strtoll(e, nullptr, 10);
    return v < lo ? lo : (v > hi ? hi : v);
}

// the rows of the canonical list (m > 0 edges) of the last k-truss result
inline int clq_rows(komb_ctx *ctx, DevBufs &bufs, ClqGraph *g)
{
    uint32_t *d_rs = nullptr, *d_re = nullptr;
    KOMB_TRY(oriented_rows(ctx, bufs, ctx->d_t_eu, ctx->t_ne, nullptr, &d_rs, &d_re));
    KOMB_HIP(ctx, hipGetLastError());
    *g = ClqGraph{ctx->d_t_eu, ctx->d_t_ev, ctx->d_t_truss, d_rs, d_re};
    return KOMB_OK;
}

// t_max of the list (m > 0 edges) into the zeroed control block, which comes back in *h; below 2 the run is refused
inline int clq_tmax(komb_ctx *ctx, const char *who, ClqCtl *ctl, uint32_t best0, ClqCtl *h)
{
    const int64_t m = ctx->t_ne;
    k_clq_tmax<<<(int)std::min<int64_t>((m + kBlock - 1) / kBlock, 1024), kBlock, 0, ctx->stream>>>(ctx->d_t_truss, (uint32_t)m, ctl, best0);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, d2h(ctx, h, ctl, sizeof(ClqCtl)));
    if (h->t_max < 2) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "%s: %lld edges and a largest trussness of %u", who, (long long)m, h->t_max);
    return KOMB_OK;
}

} // namespace komb
