// clique_census.hip -- the clique census (komb_clique_census_run): the exact number of k-cliques of the last complete k-truss
// result for every k of a window [k_lo, k_hi], and for one k_local the k_local-cliques through every vertex.  DESIGN.md section
// 4.6k.
//
// Input and roots are those of max_clique.hip: the canonical edges of the result as an oriented CSR, every clique handled at the
// canonical edge (a, b) of its two smallest ids, its other vertices in P = {c > b : (a, c) and (b, c) in H, both of trussness
// >= k_lo} (a clique of >= k_lo vertices uses only such edges), P's adjacency a bit matrix in LDS or in the workgroup's slot of
// global scratch (clique_root_dev.h).  One wavefront owns one root at a time and lane w owns word w of every set.
//
// Cliques are not enumerated: K_40 alone has 2^40.  They are counted by PIVOTING (Jain and Seshadhri, WSDM 2020).  A NODE is
// (S, h, p): a candidate set, h HELD vertices and p PIVOT vertices, held + pivot + S a subset of a + b + P; the root's is (P, 2, 0).
//   * S empty: a LEAF.  Every choice of pivots with all the held is a clique, and no clique is seen at two leaves: C(p, k - h) goes
//     to total[k] for k in [max(k_lo, h), min(k_hi, h + p)], and for k_local C(p, k_local - h) to every held vertex and
//     C(p - 1, k_local - h - 1) to every pivot vertex.  h == k_hi is a leaf whatever S holds: its subtree adds one clique, the held.
//   * h + p + |S| < k_lo: nothing below reaches the window.
//   * else a pivot u of S (the one with the most neighbours in S, or the first): the child (S & row(u), h, p + 1), then for every
//     v of S \ row(u) \ {u} in ascending order v leaves S and the child (S & row(v), h + 1, p) follows.
// The walk is iterative over an explicit stack: level d keeps its S (what is left of it), its pivot, and the vertex the current
// child took (with a bit that says pivot or held).  Held + pivot vertices are a clique, so h + p <= t_max bounds the depth and the
// binomials: one saturating Pascal table of (t_max + 1)^2 words made on the host.
//   * total[]: every wave adds into an array of its own in LDS and flushes it once with saturating compare-and-swap adds;
//     local[v]: saturating compare-and-swap adds in global memory at the leaf.  Saturating adds of non-negative numbers commute, so
//     a complete run's outputs do not depend on the scheduling.  Both are read by the host after the launch.
//   * nodes: as in the search, batches of at most 256 per wave to one counter that every node reads; a wave that finds the budget
//     spent stops.  What was added by then is a lower bound: every leaf adds real cliques, none twice.
// The launches of a run: k_clq_tmax, k_rows; k_cc_census in count mode (the largest |P| at need k_lo, which sizes the scratch
// slots and the LDS; above 4096 the run is refused) and in run mode; k_cc_saturated.  No workgroup waits for another.
#include "clique_root_dev.h"

#include <algorithm>

namespace komb {

namespace {

constexpr unsigned long long kCcSat = ~0ull;
constexpr int32_t kCcPivotBit = (int32_t)0x80000000u; // cur[d]: the child at level d + 1 took its vertex as a pivot

struct CcArgs {
    ClqGraph g;
    uint32_t m, n_chunks;
    ClqCtl *ctl;
    bool count_only, pivot_max;
    uint32_t k_lo, k_hi, k_local;                     // k_local 0: no per-vertex counts
    unsigned long long budget;
    ClqLayout lay;                                    // the candidates are P; LDS head: cur[levels], piv[levels] | tot[k_hi - k_lo + 1]; one set per stack level
    const unsigned long long *binom;                  // row n, entry i: min(C(n, i), 2^64 - 1)
    uint32_t binom_stride;
    unsigned long long *total, *local;
};

__device__ __forceinline__ unsigned long long cc_sat_add(unsigned long long x, unsigned long long y)
{
    const unsigned long long s = x + y;
    return s < x ? kCcSat : s;
}

// *p = min(*p + x, 2^64 - 1), x > 0: some lane's compare-and-swap succeeds in every round
__device__ __forceinline__ void cc_atomic_sat_add(unsigned long long *p, unsigned long long x)
{
    unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (old != kCcSat) {
        const unsigned long long seen = atomicCAS(p, old, cc_sat_add(old, x));
        if (seen == old) break;
        old = seen;
    }
}

// A leaf with h held and p pivot vertices: a, b (held) and the d vertices of cur[].
__device__ __forceinline__ void cc_leaf(const CcArgs &A, unsigned long long *tot, int32_t a, int32_t b, const int32_t *P, const volatile int32_t *cur,
                                        uint32_t d, uint32_t h, uint32_t p, int lane)
{
    const unsigned long long *row = A.binom + (size_t)p * A.binom_stride;
    const uint32_t k0 = A.k_lo > h ? A.k_lo : h, k1 = A.k_hi < h + p ? A.k_hi : h + p;
    for (uint32_t k = k0 + (uint32_t)lane; k <= k1; k += kWave) tot[k - A.k_lo] = cc_sat_add(tot[k - A.k_lo], row[k - h]);
    const uint32_t kl = A.k_local;
    if (kl < h || kl > h + p) return;
    const unsigned long long add_held = row[kl - h];
    const unsigned long long add_pivot = kl > h ? A.binom[(size_t)(p - 1) * A.binom_stride + (kl - h - 1)] : 0ull;   // (kl > h: p >= 1)
    for (uint32_t i = (uint32_t)lane; i < d + 2; i += kWave) {
        const int32_t c = i < 2 ? 0 : cur[i - 2];
        const int32_t v = i == 0 ? a : (i == 1 ? b : P[c & ~kCcPivotBit]);
        const unsigned long long add = c < 0 ? add_pivot : add_held;
        if (add) cc_atomic_sat_add(A.local + v, add);
    }
}

// One root: canonical edge rj = (a, b).  Every branch below is uniform over the wave.
__device__ void cc_root(const CcArgs &A, uint32_t rj, unsigned long long *smem, ClqWave &w, int lane)
{
    ClqCtl *ctl = A.ctl;
    const int32_t a = A.g.eu[rj], b = A.g.ev[rj];
    int32_t *P = (int32_t *)clq_slot(A.lay);
    const uint32_t n = clq_cut(A.g, rj, A.k_lo, P, A.lay.cap, !A.count_only, lane);
    if (A.count_only) { w.max_cand = n > w.max_cand ? n : w.max_cand; return; }
    ++w.roots;
    if (n > A.lay.cap || n > kClqMaxCand) { if (lane == 0) ctl->bad = 1u; return; }   // (the count launch saw every root at this need)
    volatile int32_t *cur = (int32_t *)smem, *piv = cur + A.lay.levels;   // (written by lane 0, read by every lane)
    unsigned long long *tot = smem + A.lay.lds_off_extra;
    if (n + 2u < A.k_lo || n == 0 || A.k_hi == 2u) {     // no clique of the window, or the edge alone: one node, no matrix
        clq_count(ctl, w, lane);
        if (n + 2u >= A.k_lo) cc_leaf(A, tot, a, b, P, cur, 0u, 2u, 0u, lane);
        return;
    }
    const uint32_t W = (n + 63u) >> 6;
    const ClqPlace at = clq_place(A.lay, smem, n);
    unsigned long long *mat = at.mat, *stk = at.stk;
    clq_matrix(A.g, A.k_lo, P, n, W, mat, lane);
    // ---- the walk: R is the set of the node at level d, h + p - 2 == d
    const bool mine = (uint32_t)lane < W;
    unsigned long long R = mine ? clq_prefix(n, (uint32_t)lane * 64u) : 0ull;
    uint32_t d = 0, h = 2, p = 0;
    bool enter = true;
    for (;;) {
        if (enter) {                                     // a node
            if (!clq_node(ctl, w, A.budget, lane)) break;
            const int cnt = clq_sum(__popcll(R));
            if (cnt == 0 || h >= A.k_hi) {
                if (h <= A.k_hi) cc_leaf(A, tot, a, b, P, cur, d, h, p, lane);
            } else if (h + p + (uint32_t)cnt >= A.k_lo) {
                const uint32_t u = !A.pivot_max || cnt == 1 ? clq_first(R) : clq_pivot(R, R, mat, W, lane);   // (of S itself; or the first)
                if (d + 1 >= at.levels || u >= n) { if (lane == 0) ctl->bad = 1u; break; }   // (a clique of more than t_max vertices)
                if (mine) {
                    stk[(size_t)d * W + lane] = R;
                    R &= mat[(size_t)u * W + lane];
                }
                if (lane == 0) { piv[d] = (int32_t)u; cur[d] = (int32_t)u | kCcPivotBit; }
                ++d; ++p;
                continue;
            }
        }
        // ---- back at the parent: its next vertex outside the pivot's row, if one is left
        if (d == 0) break;
        --d;
        if (cur[d] < 0) --p; else --h;
        const uint32_t u = (uint32_t)piv[d];
        R = mine ? stk[(size_t)d * W + lane] : 0ull;
        unsigned long long T = mine ? R & ~mat[(size_t)u * W + lane] : 0ull;
        if ((uint32_t)lane == (u >> 6)) T &= ~(1ull << (u & 63u));
        const uint32_t v = clq_first(T);
        enter = v != kClqNone;
        if (!enter) continue;
        if ((uint32_t)lane == (v >> 6)) R &= ~(1ull << (v & 63u));
        if (mine) {
            stk[(size_t)d * W + lane] = R;
            R &= mat[(size_t)v * W + lane];
        }
        if (lane == 0) cur[d] = (int32_t)v;
        ++d; ++h;
    }
    __syncthreads();                                     // (the next root writes P, mat and the stack again)
}

__global__ __launch_bounds__(kWave) void k_cc_census(CcArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const int lane = threadIdx.x;
    ClqCtl *ctl = A.ctl;
    ClqWave w{0u, 0u, 0u, false};
    unsigned long long *tot = smem + A.lay.lds_off_extra;
    const uint32_t n_k = A.k_hi - A.k_lo + 1u;
    if (!A.count_only) {                                 // (a count launch has no LDS)
        for (uint32_t i = (uint32_t)lane; i < n_k; i += kWave) tot[i] = 0ull;
        __syncthreads();
    }
    uint32_t chunk, tj;
    while (!w.stop && clq_next_chunk(ctl, A.g.tr, A.m, A.n_chunks, chunk, tj, lane)) {
        unsigned long long todo = __ballot(tj >= A.k_lo);
        while (todo && !w.stop) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            if (!A.count_only && clq_nodes(ctl) >= A.budget) { w.stop = true; break; }
            cc_root(A, chunk * kWave + (uint32_t)src, smem, w, lane);
        }
    }
    if (!A.count_only) {
        __syncthreads();
        for (uint32_t i = (uint32_t)lane; i < n_k; i += kWave)
            if (tot[i]) cc_atomic_sat_add(A.total + i, tot[i]);
    }
    clq_finish(ctl, w, lane);
}

// an entry of total[n_k] or local[nv] (null without one) that is 2^64 - 1
__global__ void k_cc_saturated(const unsigned long long *__restrict__ total, uint32_t n_k, const unsigned long long *__restrict__ local, uint32_t nv,
                               ClqCtl *ctl)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool sat = (i < n_k && total[i] == kCcSat) || (local && i < nv && local[i] == kCcSat);
    if (__any(sat) && (threadIdx.x & (kWave - 1)) == 0) ctl->saturated = 1u;
}

} // namespace

// the k-truss result it needs, the budget's sign and 2 <= k_lo are checked by the caller (api.cpp); the rest of the window needs
// t_max.  The result is built on the side and replaces the previous one only when the run has succeeded.
int clique_census_run(komb_ctx *ctx, int32_t k_lo, int32_t k_hi, int32_t k_local, int64_t budget)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));     // (a whole-graph result whose endpoints no fetch has asked for yet)
    Range r_all("komb_clique_census_run");
    komb_ctx::CliqueCensus res;                          // goes back to the pool unless it is installed
    const long long limit = budget == 0 ? kClqDefaultBudget : std::min<long long>(budget, kClqMaxBudget);
    DevBufs bufs(ctx);
    ClqCtl h{};
    CcArgs A{};
    KOMB_HIP(ctx, bufs.alloc(&A.ctl, 1));

    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(A.ctl, 0, sizeof(ClqCtl), s));
    const uint32_t um = (uint32_t)m;
    if (m > 0) KOMB_TRY(clq_tmax(ctx, "komb_clique_census_run", A.ctl, 0u, &h));
    const int32_t t_max = (int32_t)h.t_max;
    // the window: no clique has more than t_max vertices (and the fetch has at least one entry)
    if (k_hi == -1 || k_hi > t_max) k_hi = std::max(t_max, k_lo);
    if (k_hi < k_lo || (k_local != 0 && (k_local < k_lo || k_local > k_hi)))
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_clique_census_run: bad window k_lo %d, k_hi %d, k_local %d (t_max %d)", (int)k_lo, (int)k_hi, (int)k_local, (int)t_max);
    const uint32_t n_k = (uint32_t)(k_hi - k_lo + 1);
    res.k_lo = k_lo; res.k_hi = k_hi; res.k_local = k_local; res.t_max = t_max;
    res.total.assign(n_k, 0);
    if (k_local) {
        KOMB_HIP(ctx, ctx->pool.get((void **)res.local.slot(&ctx->pool), (size_t)nv * sizeof(unsigned long long)));
        if (nv > 0) KOMB_HIP(ctx, hipMemsetAsync(res.local, 0, (size_t)nv * sizeof(unsigned long long), s));
    }
    res.flags = KOMB_CENSUS_COMPLETE;
    if (m > 0 && k_lo <= t_max) {                        // (above t_max there is nothing to count)
        unsigned long long *d_binom = nullptr;
        KOMB_TRY(clq_rows(ctx, bufs, &A.g));
        KOMB_HIP(ctx, bufs.alloc(&A.total, (size_t)n_k));
        KOMB_HIP(ctx, hipMemsetAsync(A.total, 0, (size_t)n_k * sizeof(unsigned long long), s));
        // Pascal's triangle, saturating: row n, entry i = min(C(n, i), 2^64 - 1), 0 for i > n
        const size_t bs = (size_t)t_max + 1;
        std::vector<unsigned long long> binom(bs * bs, 0ull);
        for (size_t n = 0; n < bs; ++n) {
            binom[n * bs] = 1ull;
            for (size_t i = 1; i <= n; ++i) {
                const unsigned long long x = binom[(n - 1) * bs + i - 1], y = binom[(n - 1) * bs + i], z = x + y;
                binom[n * bs + i] = z < x ? kCcSat : z;
            }
        }
        KOMB_HIP(ctx, bufs.alloc(&d_binom, binom.size()));
        KOMB_HIP(ctx, staged_copy(ctx, d_binom, binom.data(), binom.size() * sizeof(unsigned long long), true));
        A.m = um; A.n_chunks = (um + kWave - 1) / kWave;
        A.k_lo = (uint32_t)k_lo; A.k_hi = (uint32_t)k_hi; A.k_local = (uint32_t)k_local;
        const char *pv = ctx_opt(ctx, "CENSUS_PIVOT");
        A.pivot_max = !(pv && strcmp(pv, "first") == 0);
        A.budget = (unsigned long long)limit;
        A.binom = d_binom; A.binom_stride = (uint32_t)bs;
        A.local = res.local;
        // ---- the largest |P| at need k_lo
        A.count_only = true;
        const int count_grid = (int)std::min<uint32_t>(A.n_chunks, (uint32_t)kClqGrid);
        k_cc_census<<<count_grid, kWave, 0, s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(ClqCtl)));
        const uint32_t max_p = h.max_cand;
        if (max_p > kClqMaxCand)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_census_run: a root edge has %u candidates of trussness >= %d; the limit is %u (one 64-bit word per lane)",
                      max_p, (int)k_lo, kClqMaxCand);
        // ---- the slots and the LDS, sized from it
        const ClqLaunch L = clq_layout(A.lay, max_p, (uint32_t)t_max, 2, n_k, 1, (uint32_t)clq_opt(ctx, "CENSUS_LDS", kClqLdsCand, 0, kClqLdsCand),
                                       A.n_chunks, kClqGrid);
        if (!L.fits)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_census_run: a window of %u sizes at t_max %d does not fit the LDS of a wavefront", n_k, (int)t_max);
        KOMB_HIP(ctx, bufs.alloc(&A.lay.scratch, (size_t)L.grid * A.lay.slot_bytes));
        A.count_only = false;
        KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->cursor, 0, sizeof(uint32_t), s));
        k_cc_census<<<L.grid, kWave, L.lds_bytes, s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        const uint32_t n_scan = std::max<uint32_t>(n_k, k_local ? (uint32_t)nv : 0u);
        k_cc_saturated<<<(int)((n_scan + kBlock - 1) / kBlock), kBlock, 0, s>>>(A.total, n_k, A.local, (uint32_t)nv, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(ClqCtl)));
        if (h.bad)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_census_run: the walk is inconsistent (k_lo %d, k_hi %d, largest candidate set %u)", (int)k_lo, (int)k_hi, max_p);
        KOMB_HIP(ctx, staged_copy(ctx, res.total.data(), A.total, (size_t)n_k * sizeof(unsigned long long), false));
        res.flags = (h.stopped ? 0 : KOMB_CENSUS_COMPLETE) | (h.saturated ? KOMB_CENSUS_SATURATED : 0);
        res.max_p = (int32_t)max_p;
        res.n_roots = (int64_t)h.n_roots;
        res.nodes = (int64_t)h.nodes;
    }
    res.ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    for (uint32_t i = 0; i < n_k; ++i)
        if (res.total[i]) res.omega = k_lo + (int32_t)i;
    if (ctx_flag(ctx, "CENSUS_DEBUG"))
        fprintf(stderr, "komb clique census: %lld edges, t_max %d, window %d .. %d, k_local %d, omega %d, flags %d, largest candidate set %d, %lld roots, "
                "%lld nodes of %lld, run %.3f ms\n", (long long)m, res.t_max, res.k_lo, res.k_hi, res.k_local, res.omega, res.flags, res.max_p,
                (long long)res.n_roots, (long long)res.nodes, limit, res.ms);
    res.done = true;
    ctx->cc = std::move(res);
    return KOMB_OK;
}

} // namespace komb
