// distances.hip -- distance analysis from chosen sources, komb_distances_run: closeness and harmonic sums, eccentricities and the
// neighbourhood function.  The definition, with the order of the one floating-point sum, is in include/komb_accel.h; the design
// in DESIGN.md section 4.6q.
//
// Bit-parallel multi-source BFS (Then et al., VLDB 2014).  A batch is 64 W consecutive sources, W = 1, 2 or 4 (option
// DIST_WORDS); its whole state is three masks of W 64-bit words per vertex, laid out [vertex][W] so that one neighbour's frontier
// is one 8 W byte load: seen[v] = the sources that have reached v (and the idle lanes of a partial last batch), front[v] = those
// that have v on the previous level, next[v] = those that reach it on this one.  Nothing else is per batch: what a level finds
// goes straight into the run's per-vertex accumulators, which the vertex' own lane updates without atomics.
//
// A level step is a pull: a vertex that still misses sources ORs front[] over its row and stops as soon as the OR covers what it
// misses.  OR is order-free, so a row is split any way: eight lanes share a row of up to kDistShort entries (eight vertices per
// wave and turn), a longer row is walked by the whole wave, 64 entries at a time.  The one double, harmonic[v], has its order
// fixed by the definition: per 64-source word a partial h_b that takes (double)c / (double)L at every level L in ascending
// order, and the partials of a batch are added to harmonic[v] in word order when the batch ends -- so the value does not depend
// on W.  Written unfused (#pragma clang fp contract(off)), as betweenness.hip is.
#include "common.h"
#include "wave_dev.h"

#pragma clang fp contract(off)

namespace komb {

namespace {

using u64 = unsigned long long;

constexpr int kDistGrid = 2048;              // workgroups of a level step at most; option DIST_GRID lowers it
constexpr int kDistWaves = kBlock / kWave;
constexpr int kDistGroup = 8;                // lanes that share a short row
constexpr int kDistPer = kWave / kDistGroup; // vertices of a wave and turn
constexpr uint32_t kDistShort = 64;          // a longer row goes to the whole wave
constexpr int kDistWordsMax = 4;
constexpr uint32_t kDistWords = 4;           // W without option DIST_WORDS (DESIGN.md section 4.6q has the measurement)

struct DistCtl {
    u64 found;                               // (source, vertex) pairs discovered, all level steps so far (the host takes the difference)
    u64 visits, rows;                        // row entries looked at | the lengths of the rows walked (DIST_DEBUG)
};

template <int W> struct alignas(W == 1 ? 8 : 16) DistMask { u64 w[W]; };

struct DistIdle { u64 w[kDistWordsMax]; };   // the lanes of a partial last batch that stand for no source

struct DistAcc {                             // the run's per-vertex accumulators
    u64 *n_reached, *sum_dist;               // [nv]
    int32_t *ecc;                            // [nv]
    double *hpart;                           // [nv][W] the batch's partial harmonic sums, one per 64-source word
};

__device__ __forceinline__ u64 dist_shfl_xor(u64 x, int o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int32_t)(uint32_t)x, o), hi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(x >> 32), o);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 dist_lane_u64(u64 x, int k)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)x, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(x >> 32), k);
    return ((u64)hi << 32) | lo;
}
// OR over the lanes whose numbers differ in the bits below `span` (8: a group, 64: the wave); every lane gets the result
__device__ __forceinline__ u64 dist_or(u64 x, int span)
{
    for (int o = 1; o < span; o <<= 1) x |= dist_shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ u64 dist_wave_sum(u64 x)
{
    for (int o = kWave / 2; o > 0; o >>= 1) x += dist_shfl_xor(x, o);
    return x;
}
template <int W> __device__ __forceinline__ bool dist_covers(const DistMask<W> &acc, const DistMask<W> &want)
{
    u64 miss = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) miss |= want.w[k] & ~acc.w[k];
    return miss == 0;
}

// the masks and the partial sums of a batch
template <int W>
__global__ void k_dist_init(uint32_t nv, DistIdle idle, DistMask<W> *seen, DistMask<W> *front, double *hpart)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    DistMask<W> s, z;
#pragma unroll
    for (int k = 0; k < W; ++k) { s.w[k] = idle.w[k]; z.w[k] = 0; hpart[(size_t)v * W + k] = 0.0; }
    seen[v] = s; front[v] = z;
}

// entry i < n of the batch starts at src[i], at distance 0: several may start at one vertex
template <int W>
__global__ void k_dist_seed(const int32_t *__restrict__ src, int n, u64 *seen, u64 *front, DistAcc acc)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t s = (size_t)src[i];
    const u64 bit = 1ull << (i & 63);
    atomicOr(&seen[s * W + (i >> 6)], bit);
    atomicOr(&front[s * W + (i >> 6)], bit);
    atomicAdd(&acc.n_reached[s], 1ull);
    atomicMax(&acc.ecc[s], 0);
}

// level step to L >= 1.  reach / sumd / ecc_s: the batch's slice of the per-source integers, 64 W entries (order-free: atomics)
template <int W>
__global__ void __launch_bounds__(kBlock) k_dist_level(uint32_t nv, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       int32_t L, const DistMask<W> *__restrict__ front, DistMask<W> *__restrict__ next,
                                                       DistMask<W> *__restrict__ seen, DistAcc acc, DistCtl *ctl, u64 *reach, u64 *sumd,
                                                       int32_t *ecc_s)
{
    __shared__ uint32_t s_cnt[kDistWaves][W][kWave];
    const int lane = threadIdx.x & (kWave - 1), gl = lane & (kDistGroup - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kDistWaves * kDistPer;
    uint32_t cnt[W];                                                         // lane l, word k: the vertices that source 64 k + l reached here
#pragma unroll
    for (int k = 0; k < W; ++k) cnt[k] = 0;
    u64 found = 0, visits = 0, rows = 0;
    for (uint32_t base = (blockIdx.x * kDistWaves + wave) * kDistPer; base < nv; base += stride) {   // (wave-uniform)
        const uint32_t w = base + (uint32_t)(lane / kDistGroup);
        const bool has = w < nv;
        DistMask<W> old, want, got;
        uint32_t b = 0, e = 0;
        u64 any_want = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) { old.w[k] = ~0ull; got.w[k] = 0; }
        if (has) { old = seen[w]; b = rowptr[w]; e = rowptr[w + 1]; }
#pragma unroll
        for (int k = 0; k < W; ++k) { want.w[k] = ~old.w[k]; any_want |= want.w[k]; }
        const bool wants = any_want != 0 && e > b;
        // ---- short rows: the group's eight lanes take eight entries a trip
        bool act = wants && e - b <= kDistShort;
        uint32_t j0 = b;
        while (__ballot(act)) {
            const uint32_t j = j0 + (uint32_t)gl;
            DistMask<W> f;
#pragma unroll
            for (int k = 0; k < W; ++k) f.w[k] = 0;
            if (act && j < e) f = front[col[j]];
#pragma unroll
            for (int k = 0; k < W; ++k) got.w[k] |= dist_or(f.w[k], kDistGroup);
            if (act) {
                j0 += kDistGroup;
                if (j0 >= e || dist_covers<W>(got, want)) act = false;
            }
        }
        if (gl == 0 && wants && e - b <= kDistShort) { visits += (j0 < e ? j0 : e) - b; rows += e - b; }
        // ---- long rows: the whole wave, one row after the other
        wave_turns(wants && e - b > kDistShort && gl == 0, [&](int src) {
            const uint32_t ub = from_lane(b, src), ue = from_lane(e, src);
            DistMask<W> uwant, a;
#pragma unroll
            for (int k = 0; k < W; ++k) { uwant.w[k] = dist_lane_u64(want.w[k], src); a.w[k] = 0; }
            uint32_t x0 = ub;
            while (x0 < ue) {                                                // (wave-uniform: a is the same in every lane)
                const uint32_t x = x0 + (uint32_t)lane;
                DistMask<W> f;
#pragma unroll
                for (int k = 0; k < W; ++k) f.w[k] = 0;
                if (x < ue) f = front[col[x]];
#pragma unroll
                for (int k = 0; k < W; ++k) a.w[k] |= dist_or(f.w[k], kWave);
                x0 += kWave;
                if (dist_covers<W>(a, uwant)) break;
            }
            if (lane == src) { got = a; visits += (x0 < ue ? x0 : ue) - ub; rows += ue - ub; }
        });
        // ---- what is new at w: the group's first lane owns the vertex
        DistMask<W> nw;
        u64 any_new = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) { nw.w[k] = gl == 0 ? got.w[k] & want.w[k] : 0ull; any_new |= nw.w[k]; }
        if (has && gl == 0) {
            next[w] = nw;
            if (any_new) {
                DistMask<W> s;
                uint32_t c = 0;
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    s.w[k] = old.w[k] | nw.w[k];
                    const uint32_t ck = (uint32_t)__popcll(nw.w[k]);
                    if (ck) {
                        const double q = (double)ck / (double)L;
                        acc.hpart[(size_t)w * W + k] = acc.hpart[(size_t)w * W + k] + q;
                    }
                    c += ck;
                }
                seen[w] = s;
                acc.n_reached[w] += (u64)c;
                acc.sum_dist[w] += (u64)c * (u64)L;
                if (acc.ecc[w] < L) acc.ecc[w] = L;
                found += c;
            }
        }
        // ---- the per-source tallies: lane l counts for the sources 64 k + l
        u64 todo = __ballot(any_new != 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
#pragma unroll
            for (int k = 0; k < W; ++k) cnt[k] += (uint32_t)((dist_lane_u64(nw.w[k], src) >> lane) & 1ull);
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) s_cnt[wave][k][lane] = cnt[k];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            uint32_t c = 0;
            for (int i = 0; i < kDistWaves; ++i) c += s_cnt[i][k][lane];
            if (c) {
                atomicAdd(&reach[k * kWave + lane], (u64)c);
                atomicAdd(&sumd[k * kWave + lane], (u64)c * (u64)L);
                atomicMax(&ecc_s[k * kWave + lane], L);
            }
        }
    }
    found = dist_wave_sum(found); visits = dist_wave_sum(visits); rows = dist_wave_sum(rows);
    if (lane == 0) {
        if (found) atomicAdd(&ctl->found, found);
        if (rows) { atomicAdd(&ctl->visits, visits); atomicAdd(&ctl->rows, rows); }
    }
}

// the batch ends: harmonic[v] takes the partial sums in word order (a word that reached nothing adds 0.0, which changes no bit of a
// sum that is never -0.0)
template <int W>
__global__ void k_dist_fold(uint32_t nv, const double *__restrict__ hpart, double *__restrict__ harmonic)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    double h = harmonic[v];
#pragma unroll
    for (int k = 0; k < W; ++k) h = h + hpart[(size_t)v * W + k];
    harmonic[v] = h;
}

struct DistRun {                             // what the batches of a run share
    uint32_t nv;
    int grid;
    const uint32_t *rowptr;
    const int32_t *col;
    void *seen, *front[2];
    DistAcc acc;
    double *harmonic;
    DistCtl *ctl;
    const int32_t *src;
    u64 *reach, *sumd;
    int32_t *ecc_s;
};

// one batch of n <= 64 W sources from entry `first` of the list; E = its largest distance, pairs[L] += what level L found
template <int W>
int dist_batch(komb_ctx *ctx, const DistRun &r, int64_t first, int n, DistCtl &h, komb_ctx::Distances &res, int32_t *E_out)
{
    hipStream_t s = ctx->stream;
    DistIdle idle{};
    for (int k = 0; k < W; ++k) {
        const int left = n - k * kWave;
        idle.w[k] = left >= kWave ? 0ull : (left <= 0 ? ~0ull : ~0ull << left);
    }
    DistMask<W> *seen = (DistMask<W> *)r.seen, *front[2] = {(DistMask<W> *)r.front[0], (DistMask<W> *)r.front[1]};
    k_dist_init<W><<<tiles_of(r.nv), kBlock, 0, s>>>(r.nv, idle, seen, front[0], r.acc.hpart);
    k_dist_seed<W><<<tiles_of(n), kBlock, 0, s>>>(r.src + first, n, (u64 *)r.seen, (u64 *)r.front[0], r.acc);
    int cur = 0;
    int32_t E = 0;
    for (int32_t L = 1;; ++L) {
        const u64 before = h.found;
        k_dist_level<W><<<r.grid, kBlock, 0, s>>>(r.nv, r.rowptr, r.col, L, front[cur], front[cur ^ 1], seen, r.acc, r.ctl, r.reach + first,
                                                  r.sumd + first, r.ecc_s + first);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, r.ctl, sizeof(DistCtl)));
        ++res.n_level_steps;
        if (h.found == before) break;
        if ((size_t)L >= res.pairs.size()) res.pairs.resize((size_t)L + 1, 0);
        res.pairs[(size_t)L] += (int64_t)(h.found - before);
        E = L;
        cur ^= 1;
    }
    k_dist_fold<W><<<tiles_of(r.nv), kBlock, 0, s>>>(r.nv, r.acc.hpart, r.harmonic);
    KOMB_HIP(ctx, hipGetLastError());
    *E_out = E;
    return KOMB_OK;
}

} // namespace

// sources == nullptr: every vertex in ascending order.  The result is built in a record of its own and installed only when the
// run has succeeded: a run that fails (KOMB_ERR_ARG, KOMB_ERR_NOMEM, KOMB_ERR_DEVICE) leaves the previous one.
int distances_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources)
{
    hipStream_t s = ctx->stream;
    const int64_t nv = ctx->nv > 0 ? ctx->nv : 0;
    if (!sources) n_sources = nv;
    if (n_sources < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_distances_run: %lld sources", (long long)n_sources);
    for (int64_t i = 0; sources && i < n_sources; ++i)
        if (sources[i] < 0 || sources[i] >= nv)
            KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_distances_run: source %lld is vertex %d of %lld", (long long)i, sources[i], (long long)nv);
    Range r_all("komb_distances_run");
    const bool debug = ctx_flag(ctx, "DIST_DEBUG");
    const uint32_t words_opt = ctx_opt_u32(ctx, "DIST_WORDS", kDistWords);
    const int W = words_opt >= 4 ? 4 : (words_opt >= 2 ? 2 : 1);
    const int64_t per = (int64_t)kWave * W;
    komb_ctx::Distances res;                             // goes back to the pool unless it is installed
    res.words = W;
    res.flags = sources ? 0 : KOMB_DISTANCES_ALL;
    res.source.resize((size_t)n_sources);
    for (int64_t i = 0; i < n_sources; ++i) res.source[(size_t)i] = sources ? sources[i] : (int32_t)i;
    res.s_reached.assign((size_t)n_sources, 0); res.s_sum_dist.assign((size_t)n_sources, 0); res.s_ecc.assign((size_t)n_sources, 0);
    res.pairs.assign(1, n_sources);                      // every entry of the list reaches its own vertex at distance 0
    res.n_batches = (n_sources + per - 1) / per;
    if (nv > 0) {
        const uint32_t un = (uint32_t)nv;
        const uint32_t cap = ctx_opt_u32(ctx, "DIST_GRID", kDistGrid);
        int64_t want = (nv + kDistWaves * kDistPer - 1) / (kDistWaves * kDistPer);   // eight vertices per wave, up to the cap
        if (want > kDistGrid) want = kDistGrid;
        if (want > (int64_t)cap) want = cap;
        DevBufs bufs(ctx);
        KOMB_HIP(ctx, ctx->pool.get((void **)res.n_reached.slot(&ctx->pool), (size_t)nv * sizeof(int64_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.sum_dist.slot(&ctx->pool), (size_t)nv * sizeof(int64_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.ecc.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.harmonic.slot(&ctx->pool), (size_t)nv * sizeof(double)));
        ctx->timer.start(s);
        KOMB_HIP(ctx, hipMemsetAsync(res.n_reached, 0, (size_t)nv * sizeof(int64_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(res.sum_dist, 0, (size_t)nv * sizeof(int64_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(res.ecc, 0xFF, (size_t)nv * sizeof(int32_t), s));          // -1: no source reaches the vertex
        KOMB_HIP(ctx, hipMemsetAsync(res.harmonic, 0, (size_t)nv * sizeof(double), s));
        if (n_sources > 0) {
            DistRun r{};
            r.nv = un; r.grid = (int)want; r.rowptr = ctx->d_o_rowptr; r.col = ctx->d_o_col;
            r.acc.n_reached = (u64 *)res.n_reached.get(); r.acc.sum_dist = (u64 *)res.sum_dist.get(); r.acc.ecc = res.ecc;
            r.harmonic = res.harmonic;
            int32_t *d_src = nullptr;
            u64 *d_seen = nullptr, *d_front[2] = {nullptr, nullptr};
            const size_t slots = (size_t)res.n_batches * (size_t)per;                 // (whole batches: a step adds at its 64 W lanes)
            KOMB_HIP(ctx, bufs.alloc(&r.ctl, 1));
            KOMB_HIP(ctx, bufs.alloc(&d_src, (size_t)n_sources));
            KOMB_HIP(ctx, bufs.alloc(&r.reach, slots));
            KOMB_HIP(ctx, bufs.alloc(&r.sumd, slots));
            KOMB_HIP(ctx, bufs.alloc(&r.ecc_s, slots));
            KOMB_HIP(ctx, bufs.alloc(&r.acc.hpart, (size_t)nv * W));
            KOMB_HIP(ctx, bufs.alloc(&d_seen, (size_t)nv * W));
            KOMB_HIP(ctx, bufs.alloc(&d_front[0], (size_t)nv * W));
            KOMB_HIP(ctx, bufs.alloc(&d_front[1], (size_t)nv * W));
            r.src = d_src; r.seen = d_seen; r.front[0] = d_front[0]; r.front[1] = d_front[1];
            KOMB_HIP(ctx, staged_copy(ctx, d_src, res.source.data(), (size_t)n_sources * sizeof(int32_t), true));
            KOMB_HIP(ctx, hipMemsetAsync(r.ctl, 0, sizeof(DistCtl), s));
            KOMB_HIP(ctx, hipMemsetAsync(r.reach, 0, slots * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(r.sumd, 0, slots * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(r.ecc_s, 0, slots * sizeof(int32_t), s));
            DistCtl h{};
            for (int64_t batch = 0; batch < res.n_batches; ++batch) {
                const int64_t first = batch * per;
                const int n = (int)(n_sources - first < per ? n_sources - first : per);
                int32_t E = 0;
                KOMB_TRY(W == 4 ? dist_batch<4>(ctx, r, first, n, h, res, &E)
                                : (W == 2 ? dist_batch<2>(ctx, r, first, n, h, res, &E) : dist_batch<1>(ctx, r, first, n, h, res, &E)));
                if (E > res.depth_max) res.depth_max = E;
            }
            res.ms = ctx->timer.stop(s);
            KOMB_HIP(ctx, hipGetLastError());
            res.visits = (int64_t)h.visits; res.rows = (int64_t)h.rows;
            std::vector<u64> tmp((size_t)n_sources);
            KOMB_HIP(ctx, staged_copy(ctx, tmp.data(), r.reach, (size_t)n_sources * sizeof(u64), false));
            for (int64_t i = 0; i < n_sources; ++i) res.s_reached[(size_t)i] = (int64_t)tmp[(size_t)i] + 1;   // (the source itself)
            KOMB_HIP(ctx, staged_copy(ctx, tmp.data(), r.sumd, (size_t)n_sources * sizeof(u64), false));
            for (int64_t i = 0; i < n_sources; ++i) res.s_sum_dist[(size_t)i] = (int64_t)tmp[(size_t)i];
            KOMB_HIP(ctx, staged_copy(ctx, res.s_ecc.data(), r.ecc_s, (size_t)n_sources * sizeof(int32_t), false));
        } else {
            res.ms = ctx->timer.stop(s);
            KOMB_HIP(ctx, hipGetLastError());
        }
    }
    res.pairs.resize((size_t)res.depth_max + 1, 0);
    for (size_t L = 0; L < res.pairs.size(); ++L) { res.n_pairs += res.pairs[L]; res.sum_all += (int64_t)L * res.pairs[L]; }
    res.depth_min = n_sources > 0 ? res.s_ecc[0] : 0;
    for (int64_t i = 1; i < n_sources; ++i) if (res.s_ecc[(size_t)i] < res.depth_min) res.depth_min = res.s_ecc[(size_t)i];
    if (debug)
        fprintf(stderr, "komb distances: %lld vertices, %lld sources in %lld batches of %d words, depth %d, %lld level steps, %lld pairs, "
                "%lld of %lld row entries looked at, run %.3f ms\n", (long long)nv, (long long)n_sources, (long long)res.n_batches, W,
                res.depth_max, (long long)res.n_level_steps, (long long)res.n_pairs, (long long)res.visits, (long long)res.rows, res.ms);
    res.done = true;
    ctx->dist = std::move(res);
    return KOMB_OK;
}

} // namespace komb
