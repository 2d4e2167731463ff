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
// The launches of a run: k_clq_rows, k_cc_tmax; k_cc_census in count mode (the largest |P| at need k_lo, which sizes the scratch
// slots and the LDS; above 4096 the run is refused) and in run mode; k_cc_saturated.  No workgroup waits for another.
#include "clique_root_dev.h"

#include <algorithm>

namespace komb {

namespace {

constexpr int kCcGrid = 1024;                         // wavefronts (workgroups of one) of a launch
constexpr uint32_t kCcBatch = 256;                    // nodes a wave adds to the counter at once, at most
static_assert((long long)kCcGrid * kCcBatch == KOMB_MAXCLQ_OVERSHOOT, "the documented overshoot");
constexpr uint32_t kCcLdsCand = 512;                  // default and largest CENSUS_LDS: 512 x 8 words = 32 KiB
constexpr size_t kCcLdsBytes = 56u << 10;             // LDS of a workgroup (below the 64 KiB a launch gets without asking)
constexpr size_t kCcScratchBytes = 512ull << 20;      // all scratch slots of a launch together
constexpr long long kCcDefaultBudget = 1ll << 30;
constexpr long long kCcMaxBudget = 0x7FFFFFFFll - KOMB_MAXCLQ_OVERSHOOT;   // the search's limit
constexpr unsigned long long kCcSat = ~0ull;
constexpr int32_t kCcPivotBit = (int32_t)0x80000000u; // cur[d]: the child at level d + 1 took its vertex as a pivot

struct CcCtl {                                        // 64 bytes, zeroed before every run
    unsigned long long nodes;
    unsigned long long n_roots;                       // roots opened
    uint32_t cursor;                                  // next chunk of 64 canonical edges (zeroed before every launch)
    uint32_t t_max;
    uint32_t max_p;                                   // count mode: the largest |P|
    uint32_t bad;                                     // an inconsistency (cannot happen; checked)
    uint32_t stopped;                                 // a wave found the budget spent
    uint32_t saturated;                               // k_cc_saturated: an entry is 2^64 - 1
    uint32_t pad[6];
};
static_assert(sizeof(CcCtl) == 64, "CcCtl layout");

struct CcArgs {
    ClqGraph g;
    uint32_t m, n_chunks;
    CcCtl *ctl;
    bool count_only, pivot_max;
    uint32_t k_lo, k_hi, k_local;                     // k_local 0: no per-vertex counts
    unsigned long long budget;
    unsigned char *scratch;                           // slot b: P[cap_p] | mat[cap_p * w_max] | stk[levels * w_max]
    size_t slot_bytes, off_mat, off_stk;
    uint32_t cap_p, levels;
    // LDS in 64-bit words: cur[levels] and piv[levels] (int32) | tot[k_hi - k_lo + 1] | mat | stk; lds_levels == 0: the stack is global
    uint32_t lds_cand, lds_levels, lds_off_tot, lds_off_mat, lds_off_stk;
    const unsigned long long *binom;                  // row n, entry i: min(C(n, i), 2^64 - 1)
    uint32_t binom_stride;
    unsigned long long *total, *local;
};

__global__ void k_cc_tmax(const int32_t *__restrict__ tr, uint32_t m, CcCtl *ctl)
{
    int32_t hi = 0;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock) { const int32_t t = tr[j]; hi = t > hi ? t : hi; }
    for (int off = kWave / 2; off > 0; off >>= 1) { const int32_t other = __shfl_xor(hi, off); hi = other > hi ? other : hi; }
    if ((threadIdx.x & (kWave - 1)) == 0 && hi > 0) atomicMax(&ctl->t_max, (uint32_t)hi);
}

__device__ __forceinline__ unsigned long long cc_nodes(CcCtl *ctl) { return __hip_atomic_load(&ctl->nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

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

struct CcWave { uint32_t nodes, roots, max_p; bool stop; };

__device__ __forceinline__ void cc_flush(CcCtl *ctl, CcWave &w, int lane)
{
    if (lane == 0 && w.nodes) atomicAdd(&ctl->nodes, (unsigned long long)w.nodes);
    w.nodes = 0;
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

// The pivot of S (lane w holds word w in R; S is not empty): the vertex with the most neighbours in S, the smallest such; or the first.
__device__ __forceinline__ uint32_t cc_pivot(const CcArgs &A, unsigned long long R, const unsigned long long *mat, uint32_t W, int cnt, int lane)
{
    const unsigned long long nz = __ballot(R != 0ull);
    if (!A.pivot_max || cnt == 1) {
        const int src = __ffsll((long long)nz) - 1;
        return (uint32_t)src * 64u + (uint32_t)(__ffsll((long long)clq_shfl64(R, src)) - 1);
    }
    unsigned long long key = 0ull;                       // (neighbours + 1) << 32 | ~vertex: the largest wins
    for (unsigned long long wi = nz; wi; wi &= wi - 1) {
        const int i = __ffsll((long long)wi) - 1;
        const bool in = (clq_shfl64(R, i) >> lane) & 1ull;
        const uint32_t u = (uint32_t)i * 64u + (uint32_t)lane;
        uint32_t c = 0;
        for (unsigned long long wj = nz; wj; wj &= wj - 1) {
            const int j = __ffsll((long long)wj) - 1;
            const unsigned long long Sj = clq_shfl64(R, j);
            if (in) c += (uint32_t)__popcll(Sj & mat[(size_t)u * W + (uint32_t)j]);
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

// One root: canonical edge rj = (a, b).  Every branch below is uniform over the wave.
__device__ void cc_root(const CcArgs &A, uint32_t rj, unsigned long long *smem, CcWave &w, int lane)
{
    CcCtl *ctl = A.ctl;
    const int32_t a = A.g.eu[rj], b = A.g.ev[rj];
    unsigned char *slot = A.scratch + (size_t)blockIdx.x * A.slot_bytes;
    int32_t *P = (int32_t *)slot;
    const uint32_t n = clq_cut(A.g, rj, A.k_lo, P, A.cap_p, !A.count_only, lane);
    if (A.count_only) { w.max_p = n > w.max_p ? n : w.max_p; return; }
    ++w.roots;
    if (n > A.cap_p || n > kClqMaxCand) { if (lane == 0) ctl->bad = 1u; return; }   // (the count launch saw every root at this need)
    volatile int32_t *cur = (int32_t *)smem, *piv = cur + A.levels;   // (written by lane 0, read by every lane)
    unsigned long long *tot = smem + A.lds_off_tot;
    if (n + 2u < A.k_lo || n == 0 || A.k_hi == 2u) {     // no clique of the window, or the edge alone: one node, no matrix
        if (w.nodes >= kCcBatch) cc_flush(ctl, w, lane);
        ++w.nodes;
        if (n + 2u >= A.k_lo) cc_leaf(A, tot, a, b, P, cur, 0u, 2u, 0u, lane);
        return;
    }
    const uint32_t W = (n + 63u) >> 6;
    const bool in_lds = n <= A.lds_cand;
    unsigned long long *mat = in_lds ? smem + A.lds_off_mat : (unsigned long long *)(slot + A.off_mat);
    const bool stk_lds = in_lds && A.lds_levels > 0;
    unsigned long long *stk = stk_lds ? smem + A.lds_off_stk : (unsigned long long *)(slot + A.off_stk);
    const uint32_t levels = stk_lds ? A.lds_levels : A.levels;
    clq_matrix(A.g, A.k_lo, P, n, W, mat, lane);
    // ---- the walk: R is the set of the node at level d, h + p - 2 == d
    const bool mine = (uint32_t)lane < W;
    unsigned long long R = 0ull;
    if (mine) {
        const uint32_t base = (uint32_t)lane * 64u;
        R = n - base >= 64u ? ~0ull : (1ull << (n - base)) - 1ull;
    }
    uint32_t d = 0, h = 2, p = 0;
    bool enter = true;
    for (;;) {
        if (enter) {                                     // a node
            if (w.nodes >= kCcBatch) cc_flush(ctl, w, lane);
            if (cc_nodes(ctl) + w.nodes >= A.budget) { w.stop = true; break; }
            ++w.nodes;
            const int cnt = clq_sum(__popcll(R));
            if (cnt == 0 || h >= A.k_hi) {
                if (h <= A.k_hi) cc_leaf(A, tot, a, b, P, cur, d, h, p, lane);
            } else if (h + p + (uint32_t)cnt >= A.k_lo) {
                const uint32_t u = cc_pivot(A, R, mat, W, cnt, lane);
                if (d + 1 >= levels || u >= n) { if (lane == 0) ctl->bad = 1u; break; }   // (a clique of more than t_max vertices)
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
        const unsigned long long nz = __ballot(T != 0ull);
        enter = nz != 0ull;
        if (!enter) continue;
        const int src = __ffsll((long long)nz) - 1;
        const int bit = __ffsll((long long)clq_shfl64(T, src)) - 1;
        const uint32_t v = (uint32_t)src * 64u + (uint32_t)bit;
        if (lane == src) R &= ~(1ull << bit);
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
    CcCtl *ctl = A.ctl;
    CcWave w{0u, 0u, 0u, false};
    unsigned long long *tot = smem + A.lds_off_tot;
    const uint32_t n_k = A.k_hi - A.k_lo + 1u;
    if (!A.count_only) {                                 // (a count launch has no LDS)
        for (uint32_t i = (uint32_t)lane; i < n_k; i += kWave) tot[i] = 0ull;
        __syncthreads();
    }
    while (!w.stop) {
        uint32_t chunk = 0;
        if (lane == 0) chunk = atomicAdd(&ctl->cursor, 1u);
        chunk = (uint32_t)__shfl((int32_t)chunk, 0);
        if (chunk >= A.n_chunks) break;
        const uint32_t j = chunk * kWave + (uint32_t)lane;
        const uint32_t tj = j < A.m ? (uint32_t)A.g.tr[j] : 0u;
        unsigned long long todo = __ballot(tj >= A.k_lo);
        while (todo && !w.stop) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            if (!A.count_only && cc_nodes(ctl) >= A.budget) { w.stop = true; break; }
            cc_root(A, chunk * kWave + (uint32_t)src, smem, w, lane);
        }
    }
    cc_flush(ctl, w, lane);
    if (!A.count_only) {
        __syncthreads();
        for (uint32_t i = (uint32_t)lane; i < n_k; i += kWave)
            if (tot[i]) cc_atomic_sat_add(A.total + i, tot[i]);
    }
    if (lane == 0) {
        if (w.roots) atomicAdd(&ctl->n_roots, (unsigned long long)w.roots);
        if (w.max_p) atomicMax(&ctl->max_p, w.max_p);
        if (w.stop) ctl->stopped = 1u;
    }
}

// an entry of total[n_k] or local[nv] (null without one) that is 2^64 - 1
__global__ void k_cc_saturated(const unsigned long long *__restrict__ total, uint32_t n_k, const unsigned long long *__restrict__ local, uint32_t nv,
                               CcCtl *ctl)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool sat = (i < n_k && total[i] == kCcSat) || (local && i < nv && local[i] == kCcSat);
    if (__any(sat) && (threadIdx.x & (kWave - 1)) == 0) ctl->saturated = 1u;
}

inline size_t cc_align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

long long cc_opt(const komb_ctx *ctx, const char *name, long long dflt, long long lo, long long hi)
{
    const char *e = ctx_opt(ctx, name);
    if (!e) return dflt;
    const long long v = strtoll(e, nullptr, 10);
    return v < lo ? lo : (v > hi ? hi : v);
}

} // namespace

void clique_census_drop(komb_ctx *ctx)
{
    ctx->pool.put(ctx->d_cc_local);
    ctx->d_cc_local = nullptr;
    ctx->cc = komb_ctx::CliqueCensus{};
    ctx->cc_done = false;
}

// the k-truss result it needs, the budget's sign and 2 <= k_lo are checked by the caller (api.cpp); the rest of the window needs
// t_max.  The result is built on the side and replaces the previous one only when the run has succeeded.
int clique_census_run(komb_ctx *ctx, int32_t k_lo, int32_t k_hi, int32_t k_local, int64_t budget)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));     // (a whole-graph result whose endpoints no fetch has asked for yet)
    Range r_all("komb_clique_census_run");
    struct Fresh { komb_ctx *c; unsigned long long *local; ~Fresh() { c->pool.put(local); } } fresh{ctx, nullptr};
    komb_ctx::CliqueCensus res;
    const long long limit = budget == 0 ? kCcDefaultBudget : std::min<long long>(budget, kCcMaxBudget);
    DevBufs bufs(ctx);
    CcCtl h{};
    CcArgs A{};
    KOMB_HIP(ctx, bufs.alloc(&A.ctl, 1));

    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(A.ctl, 0, sizeof(CcCtl), s));
    const uint32_t um = (uint32_t)m;
    if (m > 0) {
        k_cc_tmax<<<(int)std::min<int64_t>((m + kBlock - 1) / kBlock, 1024), kBlock, 0, s>>>(ctx->d_t_truss, um, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(CcCtl)));
        if (h.t_max < 2) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_census_run: %lld edges and a largest trussness of %u", (long long)m, h.t_max);
    }
    const int32_t t_max = (int32_t)h.t_max;
    // the window: no clique has more than t_max vertices (and the fetch has at least one entry)
    if (k_hi == -1 || k_hi > t_max) k_hi = std::max(t_max, k_lo);
    if (k_hi < k_lo || (k_local != 0 && (k_local < k_lo || k_local > k_hi)))
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_clique_census_run: bad window k_lo %d, k_hi %d, k_local %d (t_max %d)", (int)k_lo, (int)k_hi, (int)k_local, (int)t_max);
    const uint32_t n_k = (uint32_t)(k_hi - k_lo + 1);
    res.k_lo = k_lo; res.k_hi = k_hi; res.k_local = k_local; res.t_max = t_max;
    res.total.assign(n_k, 0);
    if (k_local) {
        KOMB_HIP(ctx, ctx->pool.get((void **)&fresh.local, (size_t)nv * sizeof(unsigned long long)));
        if (nv > 0) KOMB_HIP(ctx, hipMemsetAsync(fresh.local, 0, (size_t)nv * sizeof(unsigned long long), s));
    }
    res.flags = KOMB_CENSUS_COMPLETE;
    if (m > 0 && k_lo <= t_max) {                        // (above t_max there is nothing to count)
        uint32_t *d_rs = nullptr, *d_re = nullptr;
        unsigned long long *d_binom = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&d_rs, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_re, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&A.total, (size_t)n_k));
        KOMB_HIP(ctx, hipMemsetAsync(d_rs, 0, (size_t)nv * sizeof(uint32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(d_re, 0, (size_t)nv * sizeof(uint32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(A.total, 0, (size_t)n_k * sizeof(unsigned long long), s));
        k_clq_rows<<<(int)((m + kBlock - 1) / kBlock), kBlock, 0, s>>>(ctx->d_t_eu, um, d_rs, d_re);
        KOMB_HIP(ctx, hipGetLastError());
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
        A.g = ClqGraph{ctx->d_t_eu, ctx->d_t_ev, ctx->d_t_truss, d_rs, d_re};
        A.m = um; A.n_chunks = (um + kWave - 1) / kWave;
        A.k_lo = (uint32_t)k_lo; A.k_hi = (uint32_t)k_hi; A.k_local = (uint32_t)k_local;
        const char *pv = ctx_opt(ctx, "CENSUS_PIVOT");
        A.pivot_max = !(pv && strcmp(pv, "first") == 0);
        A.budget = (unsigned long long)limit;
        A.binom = d_binom; A.binom_stride = (uint32_t)bs;
        A.local = fresh.local;
        // ---- the largest |P| at need k_lo
        A.count_only = true;
        const int count_grid = (int)std::min<uint32_t>(A.n_chunks, (uint32_t)kCcGrid);
        k_cc_census<<<count_grid, kWave, 0, s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(CcCtl)));
        const uint32_t max_p = h.max_p;
        if (max_p > kClqMaxCand)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_census_run: a root edge has %u candidates of trussness >= %d; the limit is %u (one 64-bit word per lane)",
                      max_p, (int)k_lo, kClqMaxCand);
        // ---- the slots and the LDS, sized from it
        const uint32_t depth = (uint32_t)t_max - 2u;
        const uint32_t w_max = std::max<uint32_t>(1u, (max_p + 63u) >> 6);
        A.cap_p = max_p;
        A.levels = std::min(max_p, depth) + 2;
        A.off_mat = cc_align16((size_t)max_p * sizeof(int32_t));
        A.off_stk = A.off_mat + (size_t)max_p * w_max * 8;
        A.slot_bytes = cc_align16(A.off_stk + (size_t)A.levels * w_max * 8);
        const size_t head_words = cc_align16((size_t)A.levels * 2 * sizeof(int32_t)) / 8 + n_k;
        uint32_t n_l = std::min(max_p, (uint32_t)cc_opt(ctx, "CENSUS_LDS", kCcLdsCand, 0, kCcLdsCand));
        while (n_l > 0 && (head_words + (size_t)n_l * ((n_l + 63u) >> 6)) * 8 > kCcLdsBytes) n_l -= 1;
        const uint32_t w_l = (n_l + 63u) >> 6;
        A.lds_cand = n_l;
        A.lds_off_tot = (uint32_t)(head_words - n_k);
        A.lds_off_mat = (uint32_t)head_words;
        A.lds_off_stk = A.lds_off_mat + n_l * w_l;
        A.lds_levels = std::min(n_l, depth) + 2;
        size_t lds_words = A.lds_off_stk;
        if (n_l > 0 && (lds_words + (size_t)A.lds_levels * w_l) * 8 <= kCcLdsBytes) lds_words += (size_t)A.lds_levels * w_l;
        else A.lds_levels = 0;
        if (lds_words * 8 > kCcLdsBytes)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_census_run: a window of %u sizes at t_max %d does not fit the LDS of a wavefront", n_k, (int)t_max);
        int grid = (int)std::min<uint32_t>(A.n_chunks, (uint32_t)kCcGrid);
        const size_t fit = kCcScratchBytes / A.slot_bytes;
        if ((size_t)grid > fit) grid = fit < 1 ? 1 : (int)fit;
        KOMB_HIP(ctx, bufs.alloc(&A.scratch, (size_t)grid * A.slot_bytes));
        A.count_only = false;
        KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->cursor, 0, sizeof(uint32_t), s));
        k_cc_census<<<grid, kWave, lds_words * 8, s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        const uint32_t n_scan = std::max<uint32_t>(n_k, k_local ? (uint32_t)nv : 0u);
        k_cc_saturated<<<(int)((n_scan + kBlock - 1) / kBlock), kBlock, 0, s>>>(A.total, n_k, A.local, (uint32_t)nv, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(CcCtl)));
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
    clique_census_drop(ctx);
    ctx->d_cc_local = fresh.local;
    fresh.local = nullptr;
    ctx->cc = std::move(res);
    ctx->cc_done = true;
    return KOMB_OK;
}

} // namespace komb
