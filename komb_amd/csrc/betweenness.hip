// betweenness.hip -- betweenness centrality from chosen sources (Brandes 2001), komb_betweenness_run: the definition, with the
// order of every rounding operation, is in include/komb_accel.h; the design in DESIGN.md section 4.6p.
//
// Multi-source BFS with ONE LANE PER SOURCE (Then et al., VLDB 2014, on wave64).  A batch is up to 64 consecutive sources; its
// state is dist / sigma / delta[vertex][64], so whatever a wave loads of one vertex is one coalesced row and lane l only ever
// computes with source l's values.  One wave owns a vertex and walks its row once, in ascending order, with a wave-uniform
// neighbour: every lane accumulates for its own source in exactly the order of the definition -- no atomics and no cross-lane
// reduction on a floating-point value, so nothing depends on scheduling.  (The one ordered cross-lane sum, bc[v] over the lanes,
// is evaluated in lane order by every lane alike.)
//
// Masks, one 64-bit word per vertex: seen[v] = the lanes that have reached v (and the idle lanes of a partial batch),
// front[v] = the lanes that have v on the previous level.  A row is read 64 entries at a time, each lane fetches the mask of
// its entry, and a ballot names the entries some lane needs; only those cost a [64]-wide row of state.  The backward sweep uses
// the masks the same way: the mask of level L + 1 is the one the forward sweep ended with, or the one the previous backward step
// rebuilt from dist by a ballot, so two arrays serve every depth.  span[v] = the smallest and largest distance at v says
// whether v has any lane on level L without reading its dist row.
//
// Nothing of [vertex][64] is initialised: a lane's dist, sigma and delta at v are read only where seen[v] says they were written.
// Every floating-point operation below is written unfused (#pragma clang fp contract(off)): hipcc would otherwise contract
// acc + a * b into v_fmac_f64, which rounds once where the definition rounds twice.
#include "common.h"

#pragma clang fp contract(off)

namespace komb {

namespace {

using u64 = unsigned long long;

constexpr int kBtwGrid = 2048;               // workgroups of a sweep at most (4 waves each, one vertex per wave and turn); option BTW_GRID lowers it
constexpr int kBtwWaves = kBlock / kWave;
constexpr uint32_t kBtwInf = 2;              // BtwCtl::flags: a sigma became +inf (KOMB_BETWEENNESS_ROUNDED is bit 0)

struct BtwCtl {
    uint32_t hits;                           // waves that reached a vertex, all forward steps so far (the host compares it step to step)
    uint32_t flags;                          // KOMB_BETWEENNESS_ROUNDED | kBtwInf
    u64 visits, needed;                      // row entries looked at | of them, those some lane needed (BTW_DEBUG)
};

struct BtwState {                            // the arrays of a batch
    int32_t *dist;                           // [nv][64]
    double *sigma, *delta;                   // [nv][64]
    u64 *seen;                               // [nv]
    int2 *span;                              // [nv] smallest | largest distance at the vertex over the lanes that reached it
};

__device__ __forceinline__ int32_t lane_i32(int32_t x, int k) { return __builtin_amdgcn_readlane(x, k); }
__device__ __forceinline__ u64 lane_u64(u64 x, int k)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)x, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(x >> 32), k);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ double lane_f64(double x, int k) { return __longlong_as_double((long long)lane_u64((u64)__double_as_longlong(x), k)); }

// the wave's number in its workgroup, as a scalar: what is indexed by the wave's vertex is then loaded once per wave
__device__ __forceinline__ uint32_t btw_wave() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// the next entry of `todo` (a ballot over the 64 entries of a chunk), or the previous one again when none is left
__device__ __forceinline__ int btw_next(u64 &todo, int prev, bool &have)
{
    have = todo != 0;
    const int k = have ? __ffsll((long long)todo) - 1 : prev;
    todo &= todo - 1;
    return k;
}

__global__ void k_btw_init(uint32_t nv, u64 idle, u64 *seen, u64 *front, int2 *span)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    seen[v] = idle; front[v] = 0; span[v] = make_int2(0x7FFFFFFF, -1);
}

// lane i < n of the batch starts at src[i]: several lanes may start at one vertex
__global__ void k_btw_seed(const int32_t *__restrict__ src, int n, BtwState st, u64 *front)
{
    const int i = threadIdx.x;
    if (i >= n) return;
    const size_t s = (size_t)src[i];
    st.dist[s * kWave + i] = 0;
    st.sigma[s * kWave + i] = 1.0;
    atomicOr(&st.seen[s], 1ull << i);
    atomicOr(&front[s], 1ull << i);
    st.span[s] = make_int2(0, 0);                                            // (every lane that starts here writes the same)
}

// forward step to level L >= 1: sigma[w] = the sum of sigma[v] over the neighbours v of w on level L - 1, in row order, for
// every lane that has not seen w.  reach / sumd / ecc: the batch's slice of the per-source integers (order-free: atomics).
__global__ void __launch_bounds__(kBlock) k_btw_forward(uint32_t nv, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        int32_t L, const u64 *__restrict__ front, u64 *__restrict__ next, BtwState st,
                                                        BtwCtl *ctl, u64 *reach, u64 *sumd, int32_t *ecc)
{
    const int lane = threadIdx.x & (kWave - 1);
    const u64 bit = 1ull << lane;
    const uint32_t n_waves = gridDim.x * kBtwWaves;
    uint32_t cnt = 0, flags = 0;
    u64 visits = 0, needed = 0;
    bool any = false;
    for (uint32_t w = blockIdx.x * kBtwWaves + btw_wave(); w < nv; w += n_waves) {
        const u64 want = ~st.seen[w];                                        // (wave-uniform)
        if (!want) { if (lane == 0) next[w] = 0; continue; }                 // every lane is done with w
        const uint32_t b = rowptr[w], e = rowptr[w + 1];
        double acc = 0.0;
        u64 hit = 0;
        for (uint32_t j0 = b; j0 < e; j0 += kWave) {
            const uint32_t j = j0 + (uint32_t)lane;
            int32_t v = 0;
            u64 f = 0;
            if (j < e) { v = col[j]; f = front[v] & want; }
            u64 todo = __ballot(f != 0);
            visits += e - j0 < (uint32_t)kWave ? e - j0 : (uint32_t)kWave;
            needed += (u64)__popcll(todo);
            while (todo) {                                                   // four rows of sigma in flight; added in row order
                bool h0, h1, h2, h3;
                const int k0 = btw_next(todo, 0, h0), k1 = btw_next(todo, k0, h1), k2 = btw_next(todo, k1, h2), k3 = btw_next(todo, k2, h3);
                const u64 f0 = lane_u64(f, k0), f1 = h1 ? lane_u64(f, k1) : 0ull, f2 = h2 ? lane_u64(f, k2) : 0ull, f3 = h3 ? lane_u64(f, k3) : 0ull;
                const double x0 = st.sigma[(size_t)lane_i32(v, k0) * kWave + lane], x1 = st.sigma[(size_t)lane_i32(v, k1) * kWave + lane],
                             x2 = st.sigma[(size_t)lane_i32(v, k2) * kWave + lane], x3 = st.sigma[(size_t)lane_i32(v, k3) * kWave + lane];
                if (f0 & bit) acc = acc + x0;                                // (a lane without the bit has loaded what it must not use)
                if (f1 & bit) acc = acc + x1;
                if (f2 & bit) acc = acc + x2;
                if (f3 & bit) acc = acc + x3;
                hit |= f0 | f1 | f2 | f3;
            }
        }
        if (lane == 0) next[w] = hit;
        if (!hit) continue;
        any = true;
        if (lane == 0) {
            st.seen[w] = ~want | hit;
            const int2 sp = st.span[w];
            st.span[w] = make_int2(sp.x < L ? sp.x : L, L);
        }
        if (hit & bit) {
            st.dist[(size_t)w * kWave + lane] = L;
            st.sigma[(size_t)w * kWave + lane] = acc;
            ++cnt;
            if (acc >= 9007199254740992.0) flags |= acc > 1.7976931348623157e308 ? (KOMB_BETWEENNESS_ROUNDED | kBtwInf) : KOMB_BETWEENNESS_ROUNDED;
        }
    }
    if (cnt) {
        atomicAdd(&reach[lane], (u64)cnt);
        atomicAdd(&sumd[lane], (u64)cnt * (u64)L);
        atomicMax(&ecc[lane], L);
    }
    if (flags) atomicOr(&ctl->flags, flags);
    if (lane == 0) {
        if (any) atomicAdd(&ctl->hits, 1u);
        if (visits) { atomicAdd(&ctl->visits, visits); atomicAdd(&ctl->needed, needed); }
    }
}

// backward step at level L >= 1 (levels descending): delta[v] = the sum over the neighbours w of v on level L + 1, in row order,
// of sigma[v] * ((1 + delta[w]) / sigma[w]).  up[w] = the lanes that have w on level L + 1; own[v] is written for the step below.
// Level E, the deepest of the batch, has delta 0 without a step of its own: `top` says that L + 1 is that level.
__global__ void __launch_bounds__(kBlock) k_btw_backward(uint32_t nv, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         int32_t L, bool top, u64 idle, const u64 *__restrict__ up, u64 *__restrict__ own,
                                                         BtwState st, BtwCtl *ctl)
{
    const int lane = threadIdx.x & (kWave - 1);
    const u64 bit = 1ull << lane;
    const uint32_t n_waves = gridDim.x * kBtwWaves;
    u64 visits = 0, needed = 0;
    for (uint32_t v = blockIdx.x * kBtwWaves + btw_wave(); v < nv; v += n_waves) {
        const int2 sp = st.span[v];                                          // (wave-uniform)
        u64 m = 0;
        if (sp.x <= L && L <= sp.y) m = __ballot(st.dist[(size_t)v * kWave + lane] == L) & st.seen[v] & ~idle;
        if (lane == 0) own[v] = m;
        if (!m) continue;
        const double sv = st.sigma[(size_t)v * kWave + lane];                // (used by the lanes of m only)
        const uint32_t b = rowptr[v], e = rowptr[v + 1];
        double acc = 0.0;
        for (uint32_t j0 = b; j0 < e; j0 += kWave) {
            const uint32_t j = j0 + (uint32_t)lane;
            int32_t w = 0;
            u64 f = 0;
            if (j < e) { w = col[j]; f = up[w] & m; }
            u64 todo = __ballot(f != 0);
            visits += e - j0 < (uint32_t)kWave ? e - j0 : (uint32_t)kWave;
            needed += (u64)__popcll(todo);
            while (todo) {                                                   // two neighbours' sigma and delta rows in flight
                bool h0, h1;
                const int k0 = btw_next(todo, 0, h0), k1 = btw_next(todo, k0, h1);
                const u64 f0 = lane_u64(f, k0), f1 = h1 ? lane_u64(f, k1) : 0ull;
                const size_t i0 = (size_t)lane_i32(w, k0) * kWave + lane, i1 = (size_t)lane_i32(w, k1) * kWave + lane;
                const double s0 = st.sigma[i0], s1 = st.sigma[i1];
                double d0 = 0.0, d1 = 0.0;
                if (!top) { d0 = st.delta[i0]; d1 = st.delta[i1]; }
                if (f0 & bit) { const double c = (1.0 + d0) / s0; const double p = sv * c; acc = acc + p; }
                if (f1 & bit) { const double c = (1.0 + d1) / s1; const double p = sv * c; acc = acc + p; }
            }
        }
        if (m & bit) st.delta[(size_t)v * kWave + lane] = acc;
    }
    if (lane == 0 && visits) { atomicAdd(&ctl->visits, visits); atomicAdd(&ctl->needed, needed); }
}

// bc[v] += delta[v] of lane 0, 1, ..., in that order, for the lanes that reached v at a distance d > 0 (d = 0: v is the lane's
// own source; not reached, or on the batch's deepest level E: delta is 0, and adding 0.0 changes no bit of a sum that is never -0.0)
__global__ void __launch_bounds__(kBlock) k_btw_sum(uint32_t nv, int32_t E, u64 idle, BtwState st, double *__restrict__ bc)
{
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t n_waves = gridDim.x * kBtwWaves;
    for (uint32_t v = blockIdx.x * kBtwWaves + btw_wave(); v < nv; v += n_waves) {
        if (st.span[v].y <= 0) continue;
        const int32_t d = st.dist[(size_t)v * kWave + lane];
        u64 mk = __ballot(d > 0 && d < E) & st.seen[v] & ~idle;
        if (!mk) continue;
        const double x = st.delta[(size_t)v * kWave + lane];
        double acc = bc[v];
        while (mk) {
            const int k = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            acc = acc + lane_f64(x, k);
        }
        if (lane == 0) bc[v] = acc;
    }
}

} // namespace

// sources == nullptr: every vertex in ascending order.  The result is built in a record of its own and installed only when the
// run has succeeded: a run that fails (KOMB_ERR_ARG, KOMB_ERR_NOMEM, KOMB_ERR_LIMIT, KOMB_ERR_DEVICE) leaves the previous one.
int betweenness_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources)
{
    hipStream_t s = ctx->stream;
    const int64_t nv = ctx->nv > 0 ? ctx->nv : 0;
    if (!sources) n_sources = nv;
    if (n_sources < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_betweenness_run: %lld sources", (long long)n_sources);
    for (int64_t i = 0; sources && i < n_sources; ++i)
        if (sources[i] < 0 || sources[i] >= nv)
            KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_betweenness_run: source %lld is vertex %d of %lld", (long long)i, sources[i], (long long)nv);
    Range r_all("komb_betweenness_run");
    const bool debug = ctx_flag(ctx, "BTW_DEBUG");
    komb_ctx::Betweenness res;                           // goes back to the pool unless it is installed
    res.source.resize((size_t)n_sources);
    for (int64_t i = 0; i < n_sources; ++i) res.source[(size_t)i] = sources ? sources[i] : (int32_t)i;
    res.n_reached.assign((size_t)n_sources, 0); res.sum_dist.assign((size_t)n_sources, 0); res.ecc.assign((size_t)n_sources, 0);
    res.n_batches = (n_sources + kWave - 1) / kWave;
    std::string trace;
    if (nv > 0) {
        const uint32_t un = (uint32_t)nv;
        const uint32_t cap = ctx_opt_u32(ctx, "BTW_GRID", kBtwGrid);
        int64_t want = (nv + kBtwWaves - 1) / kBtwWaves;                     // one wave per vertex, up to the cap
        if (want > kBtwGrid) want = kBtwGrid;
        if (want > (int64_t)cap) want = cap;
        const int grid = (int)want;
        DevBufs bufs(ctx);
        KOMB_HIP(ctx, ctx->pool.get((void **)res.bc.slot(&ctx->pool), (size_t)nv * sizeof(double)));
        ctx->timer.start(s);
        KOMB_HIP(ctx, hipMemsetAsync(res.bc, 0, (size_t)nv * sizeof(double), s));
        if (n_sources > 0) {
            BtwState st{};
            BtwCtl *d_ctl = nullptr;
            int32_t *d_src = nullptr, *d_ecc = nullptr;
            u64 *d_front[2] = {nullptr, nullptr}, *d_reach = nullptr, *d_sumd = nullptr;
            KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
            KOMB_HIP(ctx, bufs.alloc(&d_src, (size_t)n_sources));
            KOMB_HIP(ctx, bufs.alloc(&d_reach, (size_t)res.n_batches * kWave));     // (whole batches: a step adds at its 64 lanes)
            KOMB_HIP(ctx, bufs.alloc(&d_sumd, (size_t)res.n_batches * kWave));
            KOMB_HIP(ctx, bufs.alloc(&d_ecc, (size_t)res.n_batches * kWave));
            KOMB_HIP(ctx, bufs.alloc(&st.dist, (size_t)nv * kWave));
            KOMB_HIP(ctx, bufs.alloc(&st.sigma, (size_t)nv * kWave));
            KOMB_HIP(ctx, bufs.alloc(&st.delta, (size_t)nv * kWave));
            KOMB_HIP(ctx, bufs.alloc(&st.seen, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&st.span, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&d_front[0], (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&d_front[1], (size_t)nv));
            KOMB_HIP(ctx, staged_copy(ctx, d_src, res.source.data(), (size_t)n_sources * sizeof(int32_t), true));
            KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(BtwCtl), s));
            KOMB_HIP(ctx, hipMemsetAsync(d_reach, 0, (size_t)res.n_batches * kWave * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(d_sumd, 0, (size_t)res.n_batches * kWave * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(d_ecc, 0, (size_t)res.n_batches * kWave * sizeof(int32_t), s));
            BtwCtl h{};
            for (int64_t batch = 0; batch < res.n_batches; ++batch) {
                const auto t0 = std::chrono::steady_clock::now();
                const int64_t first = batch * kWave;
                const int n = (int)(n_sources - first < kWave ? n_sources - first : kWave);
                const u64 idle = n == kWave ? 0ull : ~0ull << n;
                int cur = 0;
                k_btw_init<<<tiles_of(nv), kBlock, 0, s>>>(un, idle, st.seen, d_front[0], st.span);
                k_btw_seed<<<1, kWave, 0, s>>>(d_src + first, n, st, d_front[0]);
                // ---- forward: level by level until a step reaches nothing
                int32_t E = 0;
                for (int32_t L = 1;; ++L) {
                    const uint32_t hits = h.hits;
                    k_btw_forward<<<grid, kBlock, 0, s>>>(un, ctx->d_o_rowptr, ctx->d_o_col, L, d_front[cur], d_front[cur ^ 1], st, d_ctl,
                                                          d_reach + first, d_sumd + first, d_ecc + first);
                    KOMB_HIP(ctx, hipGetLastError());
                    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(BtwCtl)));
                    ++res.n_level_steps;
                    if (h.flags & kBtwInf)
                        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_betweenness_run: the number of shortest paths from a source of batch %lld exceeds "
                                  "the binary64 range at distance %d", (long long)batch, L);
                    if (h.hits == hits) break;           // (d_front[cur] still holds level E: the step wrote zeros to the other)
                    E = L;
                    cur ^= 1;
                }
                // ---- backward: levels E - 1 .. 1 (level E has delta 0; the sources' own delta is not part of bc)
                for (int32_t L = E - 1; L >= 1; --L) {
                    k_btw_backward<<<grid, kBlock, 0, s>>>(un, ctx->d_o_rowptr, ctx->d_o_col, L, L + 1 == E, idle, d_front[cur], d_front[cur ^ 1],
                                                           st, d_ctl);
                    ++res.n_level_steps;
                    cur ^= 1;
                }
                if (E > 1) k_btw_sum<<<grid, kBlock, 0, s>>>(un, E, idle, st, res.bc);
                KOMB_HIP(ctx, hipGetLastError());
                if (E > res.depth_max) res.depth_max = E;
                if (debug) {
                    KOMB_HIP(ctx, hipStreamSynchronize(s));
                    char line[96];
                    snprintf(line, sizeof(line), " [%lld: %d levels, %.3f ms]", (long long)batch, (int)E,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                    if (trace.size() < 4096) trace += line;
                }
            }
            res.ms = ctx->timer.stop(s);
            KOMB_HIP(ctx, hipGetLastError());
            KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(BtwCtl)));
            res.flags = (int32_t)(h.flags & KOMB_BETWEENNESS_ROUNDED);
            res.visits = (int64_t)h.visits; res.needed = (int64_t)h.needed;
            std::vector<u64> tmp((size_t)n_sources);
            KOMB_HIP(ctx, staged_copy(ctx, tmp.data(), d_reach, (size_t)n_sources * sizeof(u64), false));
            for (int64_t i = 0; i < n_sources; ++i) res.n_reached[(size_t)i] = (int64_t)tmp[(size_t)i] + 1;   // (the source itself)
            KOMB_HIP(ctx, staged_copy(ctx, tmp.data(), d_sumd, (size_t)n_sources * sizeof(u64), false));
            for (int64_t i = 0; i < n_sources; ++i) res.sum_dist[(size_t)i] = (int64_t)tmp[(size_t)i];
            KOMB_HIP(ctx, staged_copy(ctx, res.ecc.data(), d_ecc, (size_t)n_sources * sizeof(int32_t), false));
        } else {
            res.ms = ctx->timer.stop(s);
            KOMB_HIP(ctx, hipGetLastError());
        }
    }
    if (debug)
        fprintf(stderr, "komb betweenness: %lld vertices, %lld sources in %lld batches, depth %d, %lld level steps, %lld row entries "
                "looked at, %lld needed, run %.3f ms; batches (host time):%s\n", (long long)nv, (long long)n_sources, (long long)res.n_batches,
                res.depth_max, (long long)res.n_level_steps, (long long)res.visits, (long long)res.needed, res.ms, trace.c_str());
    res.done = true;
    ctx->btw = std::move(res);
    return KOMB_OK;
}

} // namespace komb
