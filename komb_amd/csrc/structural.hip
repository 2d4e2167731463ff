// structural.hip -- structural clustering (komb_structural_clusters_run): the roles core / border / hub / outlier and the
// clusters of Xu, Yuret, Feng, Schweiger ("SCAN: a structural clustering algorithm for networks", KDD 2007), index-free as in
// pSCAN (Chang et al., ICDE 2016), on the last complete k-truss result.  DESIGN.md section 4.6g.
//
// Input: the canonical edges (eu[i] < ev[i], sorted by (eu, ev), original ids) of that result and the supports sup[i] the
// peel started from: sup[i] is the number of common neighbours of the two ends, the only expensive ingredient of the
// method, and it is resident already.  With d(v) the number of result edges at v, edge i is SIMILAR iff
//     (sup + 2)^2 * eps_den^2 >= eps_num^2 * (d(u) + 1) * (d(v) + 1),
// evaluated in 128-bit integers (the left side reaches 2^102): no floating point anywhere.
//
// The launches of a run (a constant number):
//   k_sc_init      per vertex: d (row length of a whole-graph result, else 0), sim_deg = 0, parent = v, the scratch words
//   k_sc_degree    vmask results only: d counted over the endpoints
//   k_sc_similar   THE HOT PASS, one lane per edge: the test, one byte of similar[], sim_deg of both ends
//   k_sc_link      similar edges between two cores: comp_link (unionfind_dev.h)
//   k_sc_flatten   x 2: a compressing pass, then a store-free labelling pass (components.hip's header says why)
//   k_sc_border    similar edges between a core and a non-core: atomicMin of the core's label onto the non-core
//   k_sc_hub       every edge: an unlabelled end takes the min and the max of the other end's label
//   k_class_count (unionfind_dev.h), k_sc_finish   sizes, roles, the counts of the control block
//
// Canonical order puts the edges with the same eu next to each other, so what an edge pass adds to its eu end is a
// segmented reduction inside the wave: a ballot of the run heads, a ballot of the contributing lanes and one add per run
// and wave (seg_run).  Only the ev end takes a global atomic per contributing edge.
//
// Which word is written when: k_sc_border's atomics go to the label words of NON-cores, its reads to those of cores;
// k_sc_hub reads label[] and writes lo[] / hi[] only; k_sc_finish writes label[v] from v's own lane.  An atomicMin /
// atomicMax is skipped when a relaxed read of its word shows it cannot change it: such a word only ever moves one way, so
// a stale read errs on the side of issuing the atomic.
#include "unionfind_dev.h"

namespace komb {

namespace {

typedef unsigned __int128 u128;

constexpr int32_t kScNone = 0x7FFFFFFF;     // label word of a vertex without a label (until k_sc_finish writes -1); empty lo[]

struct ScCtl {                              // 64 bytes, zeroed before every run, read by the host once after it
    uint32_t n_similar, n_cores, n_borders, n_hubs, n_outliers, n_clusters, largest;
    uint32_t pad[9];
};
static_assert(sizeof(ScCtl) == 64, "ScCtl layout");

__global__ void k_sc_init(uint32_t nv, const uint32_t *__restrict__ rowptr, uint32_t *__restrict__ deg, uint32_t *__restrict__ simdeg,
                          int32_t *__restrict__ parent, int32_t *__restrict__ lo, int32_t *__restrict__ hi, uint32_t *__restrict__ cnt)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    deg[v] = rowptr ? rowptr[v + 1] - rowptr[v] : 0u;
    simdeg[v] = 0u;
    parent[v] = (int32_t)v;
    lo[v] = kScNone; hi[v] = -1;
    cnt[v] = 0u;
}

// The lanes of a wave hold consecutive canonical edges, u = eu of the lane's edge (-1 past the end): the lanes with equal u
// are one run.  Returns, in the FIRST lane of every run, the number of lanes of the run with `on` set; 0 in the others.
// Every lane of the wave calls it.
__device__ __forceinline__ uint32_t seg_run(int32_t u, bool on, int lane)
{
    const int32_t prev = __shfl_up(u, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != u);
    const unsigned long long ons = __ballot(on);
    if (!((heads >> lane) & 1ull)) return 0u;
    const unsigned long long above = lane == kWave - 1 ? 0ull : heads & ~((2ull << lane) - 1ull);   // heads of later runs
    const unsigned long long upto = above ? ((1ull << (__ffsll((long long)above) - 1)) - 1ull) : ~0ull;
    return (uint32_t)__popcll(ons & upto & ~((1ull << lane) - 1ull));
}

// d(v) of a vmask result: the result edges at v
__global__ void k_sc_degree(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, uint32_t m, uint32_t *deg)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = i < m;
    const int32_t u = act ? eu[i] : -1;
    const uint32_t n = seg_run(u, act, lane);
    if (n) atomicAdd(deg + u, n);
    if (act) atomicAdd(deg + ev[i], 1u);
}

__device__ __forceinline__ bool sc_similar(uint32_t sup, uint32_t du, uint32_t dv, uint64_t num2, uint64_t den2)
{
    const uint64_t s = (uint64_t)sup + 2ull;
    const u128 lhs = (u128)(s * s) * (u128)den2;                                     // < 2^64 * 2^40
    const u128 rhs = (u128)num2 * (u128)(((uint64_t)du + 1ull) * ((uint64_t)dv + 1ull));
    return lhs >= rhs;
}

// the hot pass: coalesced eu / ev / sup, two gathers of d, the exact test, one byte out; sim_deg[eu] by runs, sim_deg[ev] by atomics
__global__ void k_sc_similar(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ sup, uint32_t m,
                             const uint32_t *__restrict__ deg, uint64_t num2, uint64_t den2, uint8_t *__restrict__ similar,
                             uint32_t *simdeg, ScCtl *ctl)
{
    __shared__ uint32_t s_sim;
    if (threadIdx.x == 0) s_sim = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = i < m;
    int32_t u = -1, v = -1;
    bool sim = false;
    if (act) {
        u = eu[i]; v = ev[i];
        sim = sc_similar((uint32_t)sup[i], deg[u], deg[v], num2, den2);
        similar[i] = sim ? 1 : 0;
    }
    const uint32_t n = seg_run(u, sim, lane);
    if (n) atomicAdd(simdeg + u, n);
    if (sim) atomicAdd(simdeg + v, 1u);
    const unsigned long long b = __ballot(sim);
    if (lane == 0 && b) atomicAdd(&s_sim, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && s_sim) atomicAdd(&ctl->n_similar, s_sim);
}

__device__ __forceinline__ bool sc_core(const uint32_t *simdeg, int32_t v, uint32_t mu) { return simdeg[v] + 1u >= mu; }

__global__ void k_sc_link(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint8_t *__restrict__ similar, uint32_t m,
                          const uint32_t *__restrict__ simdeg, uint32_t mu, int32_t *parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || !similar[i]) return;
    const int32_t u = eu[i], v = ev[i];
    if (sc_core(simdeg, u, mu) && sc_core(simdeg, v, mu)) comp_link(parent, u, v);
}

// !kFinal: every core points itself at the root it finds, its walk splitting the paths it passes.  kFinal: read-only walks;
// label[v] = the root of a core, kScNone for everybody else.  (A non-core is never linked: no walk passes through one.)
template <bool kFinal>
__global__ void k_sc_flatten(uint32_t nv, const uint32_t *__restrict__ simdeg, uint32_t mu, int32_t *parent, int32_t *__restrict__ label)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const bool core = sc_core(simdeg, (int32_t)v, mu);
    if (kFinal) { label[v] = core ? comp_find_ro(parent, (int32_t)v) : kScNone; return; }
    if (!core) return;
    comp_flatten<false>(parent, v);
}

__device__ __forceinline__ void sc_min(int32_t *p, int32_t x) { if (x < pload(p)) atomicMin(p, x); }
__device__ __forceinline__ void sc_max(int32_t *p, int32_t x) { if (x > pload(p)) atomicMax(p, x); }

// a non-core with a similar edge to a core takes the smallest label among those cores
__global__ void k_sc_border(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint8_t *__restrict__ similar, uint32_t m,
                            const uint32_t *__restrict__ simdeg, uint32_t mu, int32_t *label)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || !similar[i]) return;
    const int32_t u = eu[i], v = ev[i];
    const bool cu = sc_core(simdeg, u, mu), cv = sc_core(simdeg, v, mu);
    if (cu == cv) return;
    if (cu) sc_min(label + v, pload(label + u));          // (a core's word: nothing writes it in this launch)
    else sc_min(label + u, pload(label + v));
}

// an end without a label collects the smallest and the largest label among its neighbours, over every edge of the result
__global__ void k_sc_hub(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, uint32_t m, const int32_t *__restrict__ label,
                         int32_t *lo, int32_t *hi)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int32_t u = eu[i], v = ev[i];
    const int32_t lu = label[u], lv = label[v];
    if ((lu == kScNone) == (lv == kScNone)) return;       // both labelled: nothing to tell; neither: nothing to say
    const int32_t x = lu == kScNone ? u : v, l = lu == kScNone ? lv : lu;
    sc_min(lo + x, l);
    sc_max(hi + x, l);
}

// label (-1 without one), size, role and sim_deg of every vertex; the counts of the control block summed up per workgroup
__global__ void k_sc_finish(uint32_t nv, const uint32_t *__restrict__ simdeg, uint32_t mu, const int32_t *__restrict__ lo,
                            const int32_t *__restrict__ hi, const uint32_t *__restrict__ cnt, int32_t *label, int32_t *__restrict__ size,
                            int32_t *__restrict__ role, ScCtl *ctl)
{
    __shared__ uint32_t s_n[5], s_max;      // outliers, hubs, borders, cores (by role value), clusters
    if (threadIdx.x < 5) s_n[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t n[5] = {0u, 0u, 0u, 0u, 0u}, mx = 0u;
    for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nv; v += gridDim.x * kBlock) {
        const int32_t lab = label[v];
        int32_t r;
        uint32_t sz = 0u;
        if (lab != kScNone) {
            r = sc_core(simdeg, (int32_t)v, mu) ? KOMB_SC_CORE : KOMB_SC_BORDER;
            sz = cnt[lab];
            if (lab == (int32_t)v) { ++n[4]; mx = sz > mx ? sz : mx; }
        } else {
            const int32_t a = lo[v];
            r = a != kScNone && hi[v] != a ? KOMB_SC_HUB : KOMB_SC_OUTLIER;
            label[v] = -1;
        }
        size[v] = (int32_t)sz;
        role[v] = r;
        for (int j = 0; j < 4; ++j) n[j] += r == j ? 1u : 0u;
    }
    for (int j = 0; j < 5; ++j) n[j] = wave_sum(n[j]);
    mx = wave_max(mx);
    if (lane == 0) {
        for (int j = 0; j < 5; ++j) if (n[j]) atomicAdd(&s_n[j], n[j]);
        if (mx) atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_n[KOMB_SC_OUTLIER]) atomicAdd(&ctl->n_outliers, s_n[KOMB_SC_OUTLIER]);
        if (s_n[KOMB_SC_HUB]) atomicAdd(&ctl->n_hubs, s_n[KOMB_SC_HUB]);
        if (s_n[KOMB_SC_BORDER]) atomicAdd(&ctl->n_borders, s_n[KOMB_SC_BORDER]);
        if (s_n[KOMB_SC_CORE]) atomicAdd(&ctl->n_cores, s_n[KOMB_SC_CORE]);
        if (s_n[4]) { atomicAdd(&ctl->n_clusters, s_n[4]); atomicMax(&ctl->largest, s_max); }
    }
}

// similar[] as the 32-bit words komb_structural_clusters_fetch_edges hands out
__global__ void k_sc_widen(const uint8_t *__restrict__ similar, uint32_t m, int32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < m) out[i] = similar[i] ? 1 : 0;
}

} // namespace

// the parameters and the k-truss result it needs are checked by the caller (api.cpp).  The result is built in blocks of its
// own and replaces the previous one only when the run has succeeded.
int structural_run(komb_ctx *ctx, int32_t eps_num, int32_t eps_den, int32_t mu)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv;
    if (m > 0) {
        KOMB_TRY(truss_edges_canonical(ctx));           // (a whole-graph result whose endpoints no fetch has asked for yet)
        KOMB_TRY(truss_support_canonical(ctx));         // (... whose supports no fetch has put in canonical order yet)
    }
    Range r_all("komb_structural_clusters_run");
    komb_ctx::Structural res;                            // goes back to the pool unless it is installed
    res.eps_num = eps_num; res.eps_den = eps_den; res.mu = mu;
    if (nv > 0) {
        KOMB_HIP(ctx, ctx->pool.get((void **)res.label.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.size.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.role.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.simdeg.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.similar.slot(&ctx->pool), (size_t)(m > 0 ? m : 1)));
        DevBufs bufs(ctx);
        ScCtl *d_ctl = nullptr;
        uint32_t *d_deg = nullptr, *d_cnt = nullptr;
        int32_t *d_parent = nullptr, *d_lo = nullptr, *d_hi = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&d_deg, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_cnt, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_parent, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_lo, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_hi, (size_t)nv));
        EventSet evs;
        hipEvent_t e0 = nullptr, e1 = nullptr;              // around the similarity pass (read after the run's own synchronisation)
        KOMB_HIP(ctx, evs.make(&e0));
        KOMB_HIP(ctx, evs.make(&e1));

        const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *sup = ctx->d_t_sup;
        const bool whole = !ctx->t_own_edges;               // d(v) is the resident row length; a vmask result counts its endpoints
        uint32_t *simdeg = (uint32_t *)res.simdeg.get();
        const uint32_t un = (uint32_t)nv, um = (uint32_t)m, umu = (uint32_t)mu;
        const uint64_t num2 = (uint64_t)eps_num * (uint64_t)eps_num, den2 = (uint64_t)eps_den * (uint64_t)eps_den;
        const int gv = tiles_of(nv), ge = tiles_of(m);
        ctx->timer.start(s);
        KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(ScCtl), s));
        k_sc_init<<<gv, kBlock, 0, s>>>(un, whole ? ctx->d_o_rowptr : nullptr, d_deg, simdeg, d_parent, d_lo, d_hi, d_cnt);
        if (m > 0) {
            if (!whole) k_sc_degree<<<ge, kBlock, 0, s>>>(eu, ev, um, d_deg);
            (void)hipEventRecord(e0, s);
            k_sc_similar<<<ge, kBlock, 0, s>>>(eu, ev, sup, um, d_deg, num2, den2, res.similar, simdeg, d_ctl);
            (void)hipEventRecord(e1, s);
            k_sc_link<<<ge, kBlock, 0, s>>>(eu, ev, res.similar, um, simdeg, umu, d_parent);
            k_sc_flatten<false><<<gv, kBlock, 0, s>>>(un, simdeg, umu, d_parent, res.label);
        }
        k_sc_flatten<true><<<gv, kBlock, 0, s>>>(un, simdeg, umu, d_parent, res.label);
        if (m > 0) {
            k_sc_border<<<ge, kBlock, 0, s>>>(eu, ev, res.similar, um, simdeg, umu, res.label);
            k_sc_hub<<<ge, kBlock, 0, s>>>(eu, ev, um, res.label, d_lo, d_hi);
        }
        class_count(ctx, nv, nullptr, res.label, d_cnt);
        k_sc_finish<<<class_tail_grid(nv), kBlock, 0, s>>>(un, simdeg, umu, d_lo, d_hi, d_cnt, res.label, res.size, res.role, d_ctl);
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
        ScCtl h;
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(ScCtl)));
        if (m > 0) {
            float f = 0.f;
            if (hipEventElapsedTime(&f, e0, e1) == hipSuccess) res.ms_similar = (double)f;
        }
        res.n_similar = (int64_t)h.n_similar; res.n_cores = (int64_t)h.n_cores; res.n_borders = (int64_t)h.n_borders;
        res.n_hubs = (int64_t)h.n_hubs; res.n_outliers = (int64_t)h.n_outliers; res.n_clusters = (int64_t)h.n_clusters;
        res.largest = (int64_t)h.largest;
        if (ctx_flag(ctx, "STRUCT_DEBUG"))
            fprintf(stderr, "komb structural: %lld vertices, %lld edges, run %.3f ms, similarity pass %.3f ms\n",
                    (long long)nv, (long long)m, res.ms, res.ms_similar);
    }
    res.done = true;
    ctx->sc = std::move(res);
    return KOMB_OK;
}

// similar[ne_sub] of the last run as 0 | 1 words into host memory
int structural_fetch_edges(komb_ctx *ctx, int32_t *similar)
{
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0;
    if (m == 0 || ctx->nv <= 0 || !similar) return KOMB_OK;
    DevBufs bufs(ctx);
    int32_t *d_out = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_out, (size_t)m));
    k_sc_widen<<<tiles_of(m), kBlock, 0, ctx->stream>>>(ctx->sc.similar, (uint32_t)m, d_out);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    KOMB_HIP(ctx, staged_copy(ctx, similar, d_out, (size_t)m * sizeof(int32_t), false));
    return KOMB_OK;
}

} // namespace komb
