// graph_build.hip -- row a1 of the hot-path table: the simple undirected graph
// igraph_create + igraph_simplify(multiple=true, loops=true) would hold
// (reference src/graph.cpp:418, src/graph.cpp:438), built on the device and
// left resident in HBM.
//
// What stays resident (common.h, komb_ctx): the symmetric CSR in the caller's (ORIGINAL) vertex ids, rows ascending --
// komb_graph_get_csr, the k-core peel, the canonical edge order of every result.  Nothing else: what only the k-truss path
// reads (the (degree,id) renumbering, the oriented CSR, the canonical edge map, the enumeration's lines and tasks) is made
// by the first k-truss call of the graph, inside that call (truss_prep.hip) -- rounds 1-4 built it here.
//
// How: both directions of every raw pair as 64-bit keys (src << vb | dst, vb = bits of a vertex id), radix-sorted on the
// 2*vb significant bits and uniqued -> the CSR.
//
// The raw pairs arrive in pageable host memory (1.8 GB at |E| = 100M): they are staged through pinned buffers by a few
// host threads (a single-threaded staging copy runs at 8-12 GB/s, a third of what the link takes).
#include "common.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <system_error>
#include <thread>

// ---------------------------------------------------------------- host -> device staging
struct H2DStager {
    static constexpr int kThreads = 8, kBufs = 2;
    static constexpr size_t kChunk = 8u << 20;
    void *pin[kThreads][kBufs] = {};
    hipStream_t st[kThreads] = {};
    hipEvent_t ev[kThreads][kBufs] = {};
    bool ok = false;
};

namespace komb {

void stager_free(komb_ctx *ctx)
{
    H2DStager *g = ctx->stager;
    if (!g) return;
    for (int t = 0; t < H2DStager::kThreads; ++t) {
        for (int b = 0; b < H2DStager::kBufs; ++b) {
            if (g->pin[t][b]) (void)hipHostFree(g->pin[t][b]);
            if (g->ev[t][b]) (void)hipEventDestroy(g->ev[t][b]);
        }
        if (g->st[t]) (void)hipStreamDestroy(g->st[t]);
    }
    delete g;
    ctx->stager = nullptr;
}

namespace {

H2DStager *stager_get(komb_ctx *ctx)
{
    if (ctx->stager) return ctx->stager->ok ? ctx->stager : nullptr;
    H2DStager *g = new (std::nothrow) H2DStager();
    if (!g) return nullptr;
    ctx->stager = g;
    bool ok = true;
    for (int t = 0; t < H2DStager::kThreads && ok; ++t) {
        ok = hipStreamCreate(&g->st[t]) == hipSuccess;
        for (int b = 0; b < H2DStager::kBufs && ok; ++b)
            ok = hipHostMalloc(&g->pin[t][b], H2DStager::kChunk, hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&g->ev[t][b], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    g->ok = ok;
    return ok ? g : nullptr;
}

} // namespace

// blocking copy between pageable host memory and the device through the pinned staging buffers, a few host threads each with
// a stream of its own; complete on return.  to_device = false: device -> host (the ranks of CoreA, the result fetches).
hipError_t staged_copy(komb_ctx *ctx, void *dst, const void *src, size_t bytes, bool to_device)
{
    H2DStager *g = bytes >= (32u << 20) ? stager_get(ctx) : nullptr;
    if (!g) {
        hipError_t e = hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream);
        return e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
    }
    // (device -> host: what the context's stream has written must be complete before the staging streams read it)
    if (!to_device) { const hipError_t e0 = hipStreamSynchronize(ctx->stream); if (e0 != hipSuccess) return e0; }
    const size_t nchunks = (bytes + H2DStager::kChunk - 1) / H2DStager::kChunk;
    hipError_t err[H2DStager::kThreads];
    std::thread th[H2DStager::kThreads];
    const int dev = ctx->device;
    // thread t copies chunks t, t + started, ...: `started` is how many threads could be created (a process at its thread
    // limit gets fewer, or none: then this thread does the staged copy alone -- an exception must not cross the C ABI)
    auto work = [=, &err](int t, int stride) {
        hipError_t e = hipSetDevice(dev);
        size_t turn = 0;
        size_t pend_off[H2DStager::kBufs] = {}, pend_len[H2DStager::kBufs] = {};      // device -> host: chunks in flight into the pinned buffers
        for (size_t c = (size_t)t; c < nchunks && e == hipSuccess; c += (size_t)stride, ++turn) {
            const int b = (int)(turn % H2DStager::kBufs);
            if (turn >= (size_t)H2DStager::kBufs) {
                e = hipEventSynchronize(g->ev[t][b]);                                 // the buffer's previous copy is done
                if (e == hipSuccess && !to_device) memcpy((char *)dst + pend_off[b], g->pin[t][b], pend_len[b]);
            }
            if (e != hipSuccess) break;
            const size_t off = c * H2DStager::kChunk, len = std::min(H2DStager::kChunk, bytes - off);
            if (to_device) {
                memcpy(g->pin[t][b], (const char *)src + off, len);
                e = hipMemcpyAsync((char *)dst + off, g->pin[t][b], len, hipMemcpyHostToDevice, g->st[t]);
            } else {
                e = hipMemcpyAsync(g->pin[t][b], (const char *)src + off, len, hipMemcpyDeviceToHost, g->st[t]);
                pend_off[b] = off; pend_len[b] = len;
            }
            if (e == hipSuccess) e = hipEventRecord(g->ev[t][b], g->st[t]);
        }
        const hipError_t e2 = hipStreamSynchronize(g->st[t]);
        if (!to_device && e == hipSuccess && e2 == hipSuccess) {
            // the last (up to kBufs) chunks of this thread are still in the pinned buffers
            const size_t done = turn;
            for (size_t q = done > (size_t)H2DStager::kBufs ? done - H2DStager::kBufs : 0; q < done; ++q) {
                const int b = (int)(q % H2DStager::kBufs);
                memcpy((char *)dst + pend_off[b], g->pin[t][b], pend_len[b]);
            }
        }
        err[t] = e != hipSuccess ? e : e2;
    };
    // how many threads can be had is known only by trying: the stride is fixed before the first one starts copying
    int started = 0;
    struct Gate { std::atomic<int> stride{0}; } gate;
    for (int t = 0; t < H2DStager::kThreads; ++t) {
        err[t] = hipSuccess;
        try {
            th[t] = std::thread([&gate, &work, t]() {
                int stride;
                while ((stride = gate.stride.load(std::memory_order_acquire)) == 0) std::this_thread::yield();
                if (stride > 0) work(t, stride);
            });
            ++started;
        } catch (const std::system_error &) { break; }
    }
    if (started == 0) { work(0, 1); return err[0]; }
    gate.stride.store(started, std::memory_order_release);
    hipError_t e = hipSuccess;
    for (int t = 0; t < started; ++t) { th[t].join(); if (err[t] != hipSuccess) e = err[t]; }
    return e;
}

namespace {

inline hipError_t h2d_staged(komb_ctx *ctx, void *dst, const void *src, size_t bytes) { return staged_copy(ctx, dst, src, bytes, true); }

// ---------------------------------------------------------------- kernels
inline int grid_for(int64_t n)
{
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;
    return (int)g;
}

// both directions of every raw pair as keys (src << vb | dst); loops and padding become the drop key (all ones in the
// 2*vb sorted bits = the loop on vertex 2^vb - 1, which no valid key is), which sorts to the end
__global__ __launch_bounds__(kBlock) void k_make_keys(const int64_t *__restrict__ uv, int64_t n_raw, int64_t nv, int vb,
                                                      uint64_t *__restrict__ keys, int *__restrict__ bad)
{
    const uint64_t drop = (1ull << (2 * vb)) - 1ull;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_raw; i += (int64_t)gridDim.x * kBlock) {
        const longlong2 p = reinterpret_cast<const longlong2 *>(uv)[i];
        const int64_t u = p.x, v = p.y;
        uint64_t k0 = drop, k1 = drop;
        if (u < 0 || v < 0 || u >= nv || v >= nv) *bad = 1;
        else if (u != v) {
            k0 = ((uint64_t)u << vb) | (uint64_t)v;
            k1 = ((uint64_t)v << vb) | (uint64_t)u;
        }
        reinterpret_cast<ulonglong2 *>(keys)[i] = make_ulonglong2(k0, k1);
    }
}

// uniq[0..ns) sorted by (src,dst): col[j] = dst, rowptr[v] = first slot with src >= v
__global__ __launch_bounds__(kBlock) void k_keys_to_csr(const uint64_t *__restrict__ uniq, int64_t ns, int64_t nv, int vb,
                                                        uint32_t *__restrict__ rowptr, int32_t *__restrict__ col)
{
    const uint64_t mask = (1ull << vb) - 1ull;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < ns; j += (int64_t)gridDim.x * kBlock) {
        const uint64_t k = uniq[j];
        const int64_t s = (int64_t)(k >> vb);
        col[j] = (int32_t)(k & mask);
        const int64_t p = (j == 0) ? -1 : (int64_t)(uniq[j - 1] >> vb);
        for (int64_t v = p + 1; v <= s; ++v) rowptr[v] = (uint32_t)j;
        if (j == ns - 1)
            for (int64_t v = s + 1; v <= nv; ++v) rowptr[v] = (uint32_t)ns;
    }
}

__global__ __launch_bounds__(kBlock) void k_fill_u32(uint32_t *p, int64_t n, uint32_t val)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) p[i] = val;
}

__global__ __launch_bounds__(kBlock) void k_rowptr_narrow(const int64_t *__restrict__ in, int64_t n,
                                                          uint32_t *__restrict__ out, int *__restrict__ bad)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t x = in[i];
        if (x < 0 || x > 0xFFFFFFFFll || (i > 0 && in[i - 1] > x)) *bad = 1;
        out[i] = (uint32_t)x;
    }
}

// simple + sorted + symmetric check of a caller-supplied CSR (one thread per slot's row)
__global__ __launch_bounds__(kBlock) void k_validate_csr(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         int64_t nv, int *__restrict__ bad)
{
    for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < nv; u += (int64_t)gridDim.x * kBlock) {
        const uint32_t b = rowptr[u], e = rowptr[u + 1];
        for (uint32_t j = b; j < e; ++j) {
            const int32_t v = col[j];
            if (v < 0 || v >= nv || v == (int32_t)u || (j > b && col[j - 1] >= v)) { *bad = 1; continue; }
            uint32_t lo = rowptr[v], hi = rowptr[v + 1];          // u must be in row v
            bool found = false;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                const int32_t c = col[mid];
                if (c < (int32_t)u) lo = mid + 1; else if (c > (int32_t)u) hi = mid; else { found = true; break; }
            }
            if (!found) *bad = 1;
        }
    }
}

struct Scratch {                                   // device scratch of one build: freed on every way out
    komb_ctx *ctx;
    std::vector<void *> v;
    explicit Scratch(komb_ctx *c) : ctx(c) {}
    template <class T> hipError_t get(T **out, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = dev_malloc(ctx, &q, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) { v.push_back(q); *out = (T *)q; }
        return e;
    }
    void drop(void *p) { for (auto &q : v) if (q == p && p) { (void)hipFree(p); q = nullptr; } }
    ~Scratch() { for (void *q : v) if (q) (void)hipFree(q); }
};

template <class T> hipError_t resident(komb_ctx *ctx, T **out, size_t count) { return dev_malloc(ctx, (void **)out, (count ? count : 1) * sizeof(T)); }

inline int id_bits(int64_t nv)
{
    int vb = 1;
    while (vb < 31 && (1ll << vb) < nv) ++vb;
    return vb;
}

double wall_ms(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void publish_stats(komb_ctx *ctx, int64_t nv, int64_t ne)
{
    ctx->nv = nv;
    ctx->ne = ne;
    ctx->stats = komb_stats{};
    ctx->stats.nv = nv; ctx->stats.ne = ne;
}

} // namespace

void warm_up(komb_ctx *ctx)
{
    const bool dbg = ctx->opts.verbosity > 1;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t *d = nullptr;
    if (dev_malloc(ctx, (void **)&d, 256) == hipSuccess) {
        k_fill_u32<<<1, kBlock, 0, ctx->stream>>>(d, 64, 0u);        // the library's code object is loaded by its first launch
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d);
    }
    if (dbg) fprintf(stderr, "komb warm-up: first kernel launch %.1f ms\n", wall_ms(t0));
    // the upload's pinned staging buffers + streams (128 MB, 60 ms): only for a caller that says it will upload a big graph
    // (komb2 does, beside its SAM parse); everyone else gets them on the first upload of 64 MB or more
    if (ctx->opts.reserved[0] & KOMB_CREATE_WARM_UPLOAD) {
        const auto t1 = std::chrono::steady_clock::now();
        (void)stager_get(ctx);
        if (dbg) fprintf(stderr, "komb warm-up: staging buffers %.1f ms\n", wall_ms(t1));
    }
    (void)hipGetLastError();
}

void graph_free(komb_ctx *ctx)
{
    truss_free(ctx);
    prep_free(ctx, &ctx->prep);
    // the results with the graph's lifetime (those of a k-truss result went with truss_free)
    ctx->core = {}; ctx->onion = {}; ctx->comp = {}; ctx->hier = {}; ctx->dens = {}; ctx->btw = {}; ctx->dist = {};
    if (ctx->d_o_rowptr) (void)hipFree(ctx->d_o_rowptr);
    if (ctx->d_o_col) (void)hipFree(ctx->d_o_col);
    ctx->d_o_rowptr = nullptr; ctx->d_o_col = nullptr;
    ctx->nv = -1; ctx->ne = 0;
    ctx->cap_hint.nv = -1; ctx->cap_hint.m = -1;
    if (ctx->d_ceu) ctx->pool.put(ctx->d_ceu);
    if (ctx->d_cev) ctx->pool.put(ctx->d_cev);
    ctx->d_ceu = ctx->d_cev = nullptr;
    ctx->pool.clear();                                   // scratch sized for the old graph; no record holds a block of it any more
}

int graph_from_edges(komb_ctx *ctx, int64_t nv, int64_t n_raw, const int64_t *uv)
{
    graph_free(ctx);
    if (nv < 0 || nv > INT32_MAX - 1 || n_raw < 0 || (n_raw > 0 && !uv))
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "graph_from_edges: bad nv=%lld n_raw=%lld", (long long)nv, (long long)n_raw);
    if (n_raw > (int64_t)1 << 36)                        // (what bounds a graph is its simple form: 2^32-16 slots, checked below)
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "graph_from_edges: %lld raw pairs", (long long)n_raw);
    hipStream_t s = ctx->stream;
    Range r_all("komb_graph_from_edges");
    const auto t_all = std::chrono::steady_clock::now();
    const int vb = id_bits(nv);
    double ms_h2d = 0.0;
    struct Fail { komb_ctx *c; bool armed = true; ~Fail() { if (armed) graph_free(c); } } fail{ctx};   // nothing half-built stays behind

    Scratch sc(ctx);
    KOMB_HIP(ctx, resident(ctx, &ctx->d_o_rowptr, (size_t)nv + 1));
    int64_t ns = 0;
    uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
    const bool dbg = ctx->opts.verbosity > 1 || ctx_flag(ctx, "BUILD_DEBUG");
    if (n_raw > 0) {
        int64_t *d_uv = nullptr; int *d_bad = nullptr;
        const int64_t nk = 2 * n_raw;
        KOMB_HIP(ctx, sc.get(&d_uv, (size_t)nk));
        KOMB_HIP(ctx, sc.get(&d_k0, (size_t)nk));
        KOMB_HIP(ctx, sc.get(&d_k1, (size_t)nk));
        KOMB_HIP(ctx, sc.get(&d_bad, 1));
        KOMB_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(int), s));
        if (dbg) fprintf(stderr, "komb build: allocations %.1f ms\n", wall_ms(t_all));
        const auto t_st = std::chrono::steady_clock::now();
        (void)stager_get(ctx);
        if (dbg) fprintf(stderr, "komb build: staging buffers %.1f ms\n", wall_ms(t_st));
        const auto t_h2d = std::chrono::steady_clock::now();
        KOMB_HIP(ctx, h2d_staged(ctx, d_uv, uv, (size_t)nk * sizeof(int64_t)));
        ms_h2d = wall_ms(t_h2d);
        if (dbg) fprintf(stderr, "komb build: copy %.1f ms\n", ms_h2d);
        k_make_keys<<<grid_for(n_raw), kBlock, 0, s>>>(d_uv, n_raw, nv, vb, d_k0, d_bad);
        int bad = 0;
        KOMB_HIP(ctx, d2h(ctx, &bad, d_bad, sizeof(int)));
        if (bad) KOMB_FAIL(ctx, KOMB_ERR_ARG, "graph_from_edges: vertex id outside [0,%lld)", (long long)nv);
        sc.drop(d_uv);

        uint64_t *sorted = nullptr;
        KOMB_TRY(prim_sort_u64(ctx, d_k0, d_k1, nk, 2 * vb, &sorted));
        uint64_t *other = (sorted == d_k0) ? d_k1 : d_k0;
        int64_t nu = 0;
        KOMB_TRY(prim_unique_u64(ctx, sorted, other, nk, &nu));
        // the drop key, if present, is the last unique key
        if (nu > 0) {
            uint64_t last = 0;
            KOMB_HIP(ctx, d2h(ctx, &last, other + (nu - 1), sizeof(uint64_t)));
            if (last == (1ull << (2 * vb)) - 1ull) --nu;
        }
        ns = nu;
        if (ns > 0xFFFFFFF0ll) KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "graph has %lld slots; limit is 2^32-16", (long long)ns);
        if (ns / 2 > INT32_MAX - 16) KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "graph has %lld edges; limit is 2^31-16", (long long)(ns / 2));
        KOMB_HIP(ctx, resident(ctx, &ctx->d_o_col, (size_t)ns));
        if (ns > 0) k_keys_to_csr<<<grid_for(ns), kBlock, 0, s>>>(other, ns, nv, vb, ctx->d_o_rowptr, ctx->d_o_col);
        else k_fill_u32<<<grid_for(nv + 1), kBlock, 0, s>>>(ctx->d_o_rowptr, nv + 1, 0u);
    } else {
        KOMB_HIP(ctx, resident(ctx, &ctx->d_o_col, 1));
        k_fill_u32<<<grid_for(nv + 1), kBlock, 0, s>>>(ctx->d_o_rowptr, nv + 1, 0u);
    }
    KOMB_HIP(ctx, hipStreamSynchronize(s));
    if (dbg) fprintf(stderr, "komb build: CSR done at %.1f ms\n", wall_ms(t_all));
    fail.armed = false;
    publish_stats(ctx, nv, ns / 2);
    ctx->stats.ms_build = wall_ms(t_all);
    ctx->stats.ms_build_h2d = ms_h2d;
    ctx->stats.ms_build_relabel = 0.0;                   // (rounds 1-4: the k-truss side was built here; now truss_prep.hip, stats.ms_prepare)
    return KOMB_OK;
}

int graph_from_csr(komb_ctx *ctx, int64_t nv, const int64_t *rowptr, const int32_t *col)
{
    graph_free(ctx);
    if (nv < 0 || nv > INT32_MAX - 1 || !rowptr)
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "graph_from_csr: bad nv=%lld", (long long)nv);
    const int64_t ns = rowptr[nv];
    if (rowptr[0] != 0 || ns < 0 || (ns & 1) || (ns > 0 && !col))
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "graph_from_csr: rowptr[0]=%lld rowptr[nv]=%lld is not a symmetric CSR", (long long)rowptr[0], (long long)ns);
    if (ns > 0xFFFFFFF0ll || ns / 2 > INT32_MAX - 16)
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "graph has %lld slots; limit is 2^32-16", (long long)ns);
    hipStream_t s = ctx->stream;
    const auto t_all = std::chrono::steady_clock::now();
    struct Fail { komb_ctx *c; bool armed = true; ~Fail() { if (armed) graph_free(c); } } fail{ctx};
    Scratch sc(ctx);
    int64_t *d_rp64 = nullptr; int *d_bad = nullptr;
    KOMB_HIP(ctx, resident(ctx, &ctx->d_o_rowptr, (size_t)nv + 1));
    KOMB_HIP(ctx, resident(ctx, &ctx->d_o_col, (size_t)ns));
    KOMB_HIP(ctx, sc.get(&d_rp64, (size_t)nv + 1));
    KOMB_HIP(ctx, sc.get(&d_bad, 1));
    KOMB_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(int), s));
    const auto t_h2d = std::chrono::steady_clock::now();
    KOMB_HIP(ctx, h2d_staged(ctx, d_rp64, rowptr, (size_t)(nv + 1) * sizeof(int64_t)));
    if (ns > 0) KOMB_HIP(ctx, h2d_staged(ctx, ctx->d_o_col, col, (size_t)ns * sizeof(int32_t)));
    const double ms_h2d = wall_ms(t_h2d);
    int bad = 0;
    k_rowptr_narrow<<<grid_for(nv + 1), kBlock, 0, s>>>(d_rp64, nv + 1, ctx->d_o_rowptr, d_bad);
    KOMB_HIP(ctx, d2h(ctx, &bad, d_bad, sizeof(int)));
    if (!bad && nv > 0) {                                        // rowptr is sane: rows can be walked safely
        k_validate_csr<<<grid_for(nv), kBlock, 0, s>>>(ctx->d_o_rowptr, ctx->d_o_col, nv, d_bad);
        KOMB_HIP(ctx, d2h(ctx, &bad, d_bad, sizeof(int)));
    }
    if (bad) KOMB_FAIL(ctx, KOMB_ERR_ARG, "graph_from_csr: CSR is not simple, symmetric and row-sorted");
    sc.drop(d_rp64);
    KOMB_HIP(ctx, hipStreamSynchronize(s));
    fail.armed = false;
    publish_stats(ctx, nv, ns / 2);
    ctx->stats.ms_build = wall_ms(t_all);
    ctx->stats.ms_build_h2d = ms_h2d;
    ctx->stats.ms_build_relabel = 0.0;
    return KOMB_OK;
}

} // namespace komb
