// components.hip -- connected components of a k-core or of a k-truss subgraph (komb_components_run): a union-find by
// hooking over ORIGINAL vertex ids.  DESIGN.md section 4.6b.
//
// parent[v] (the result's label array itself) starts as v.  Two trees are joined by a compare-and-swap on a ROOT that
// hangs the larger id under the smaller: parent[x] <= x always, every walk goes through strictly decreasing ids (so
// it ends, whatever it reads), there are no cycles, and the root of a finished component is its smallest id -- the
// label the interface promises, whatever the schedule.  The number of launches of a call is a constant.
//
// Why stale reads are harmless (per-XCD L2s are not coherent, a CU's L1 is not refreshed by other CUs' stores):
//  * A word of parent[] changes in two ways only.  A HOOK: the CAS parent[r]: r -> s, s < r, s in the other tree.  It
//    succeeds on a true root only (the CAS is a device-scope atomic: it compares with the word's current value, not
//    with what the lane read before) and makes r a non-root for good.  A COMPRESSION: a store parent[x] = a to an x
//    that was READ as a non-root (so it is one for good: hooks never touch it again) with an a that was read out of
//    parent[] on the way up from x.  By induction every value parent[x] ever held, and so every value a stale read
//    can return, is a vertex of x's tree: trees only ever merge, and a compression keeps x (and what hangs under it)
//    in the tree it was in.  A compression can therefore neither undo a hook (it never writes a root, never writes
//    x into parent[x]) nor move a vertex to another tree, and two racing compressions leave one of two valid values.
//  * find() ends at an r it READ as a root, which may be stale.  link() never trusts that: it hooks with a CAS that
//    expects r in parent[r]; when r is no root any more the CAS fails and returns r's current parent, a smaller id of
//    the same tree, and the walk continues from there.  Nothing waits for another wave: every iteration either
//    hooks or strictly lowers one of the two ids.  A successful hook under an s that has meanwhile been hooked
//    itself is still a correct union (s is in the other tree and smaller).
//  * The labels are read by a LATER launch (k_comp_flatten<true>), after every linking launch has completed: no hook is
//    in flight then and every hook is visible (a kernel boundary), so a vertex read as a root is one, and a root reached
//    through vertices of v's tree is the root of v's tree: the smallest id of v's component.  That launch's walks store
//    nothing (a compression of parent[v] by a walk passing through v could land on top of v's label): its only store
//    is label[v], by v's own lane, and a walk that reads it finds the root a step earlier.  The compressing flatten
//    runs in a launch before it.
// Every access to parent[] inside the linking launches is a relaxed agent-scope atomic load / store (it bypasses the
// L1, so a walk sees a hook soon, and no dirty line of parent[] waits in an L2 behind an atomic of another XCD).
#include "unionfind_dev.h"   // pload / pstore, comp_find, comp_link, the class tail (shared with communities.hip); wave_dev.h

namespace komb {

namespace {

constexpr uint32_t kCompShort = 16;         // rows up to this long: the row's own lane
constexpr uint32_t kCompHeavy = 2048;       // rows from this length on: several workgroups of k_comp_heavy (rows between: their wave)
constexpr uint32_t kCompWindow = 16;        // sampling pass: entries of a row it looks at for its two neighbours
constexpr int kCompSamples = 1024;          // vertices whose roots vote for the giant component
constexpr int kCompHeavyGrid = 256, kCompHeavyChunks = 8;   // k_comp_heavy: rows side by side x workgroups along a row

struct CompCtl {                            // 64 bytes, zeroed before every run
    int32_t  giant;                         // root of the most frequent component of the sample (-1: none)
    uint32_t n_heavy;                       // rows queued for k_comp_heavy
    uint32_t n_members, n_components, largest;
    uint32_t pad[11];
};
static_assert(sizeof(CompCtl) == 64, "CompCtl layout");

// parent[v] = v; flag[v] = member (core kind: coreness >= k, everyone when k == 0; truss kind: 0, the edge pass sets it); cnt[v] = 0
__global__ void k_comp_init(uint32_t nv, const int32_t *__restrict__ core, int32_t k, bool all, bool none,
                            int32_t *__restrict__ parent, int32_t *__restrict__ flag, uint32_t *__restrict__ cnt)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    parent[v] = (int32_t)v;
    flag[v] = none ? 0 : (all ? 1 : (core[v] >= k ? 1 : 0));
    cnt[v] = 0u;
}

template <bool kAll>
__device__ __forceinline__ bool comp_member(const int32_t *core, int32_t k, int32_t w)
{
    return kAll || core[w] >= k;
}

// sampling pass: every member row links its last two member neighbours among its last kCompWindow entries (rows
// ascend: the first entries of most rows are the same few hubs, and 10 M walks through their words queue up)
template <bool kAll>
__global__ void k_comp_sample(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ core,
                              int32_t k, uint32_t nv, int32_t *parent, const int32_t *__restrict__ flag)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv || !flag[v]) return;
    const uint32_t b = rowptr[v], e = rowptr[v + 1];
    const uint32_t lim = e - b > kCompWindow ? e - kCompWindow : b;
    int found = 0;
    for (uint32_t i = e; i > lim && found < 2; --i) {
        const int32_t w = col[i - 1];
        if (!comp_member<kAll>(core, k, w)) continue;
        comp_link(parent, (int32_t)v, w);
        ++found;
    }
}

// !kFinal: every member points itself at the root it finds, its walk splitting the paths it passes (a hint: it may be
// overwritten by another walk's compression).  kFinal: label[v] = root of v (members), -1 (others); read-only walks.
template <bool kFinal>
__global__ void k_comp_flatten(uint32_t nv, int32_t *parent, const int32_t *__restrict__ flag)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    if (!flag[v]) { if (kFinal) pstore(parent + v, -1); return; }
    comp_flatten<kFinal>(parent, v);
}

// the most frequent root among kCompSamples evenly spaced vertices (ties: the smaller id); one workgroup
__global__ void __launch_bounds__(kCompSamples) k_comp_pick(uint32_t nv, const int32_t *__restrict__ parent, const int32_t *__restrict__ flag, CompCtl *ctl)
{
    __shared__ int32_t s_lab[kCompSamples];
    __shared__ unsigned long long s_best;
    const int t = threadIdx.x;
    const uint32_t v = (uint32_t)(((uint64_t)t * nv) / kCompSamples);
    const int32_t lab = flag[v] ? parent[v] : -1;
    s_lab[t] = lab;
    if (t == 0) s_best = 0ull;
    __syncthreads();
    uint32_t c = 0;
    if (lab >= 0) for (int j = 0; j < kCompSamples; ++j) c += s_lab[j] == lab ? 1u : 0u;
    if (c) atomicMax(&s_best, ((unsigned long long)c << 32) | (uint32_t)(0x7FFFFFFF - lab));
    __syncthreads();
    if (t == 0) ctl->giant = s_best ? 0x7FFFFFFF - (int32_t)(uint32_t)(s_best & 0xFFFFFFFFull) : -1;
}

// one entry w of member row v.  kBoth: every entry (the rows of the giant component are skipped, so an edge into it is
// seen from this side only); else each undirected edge once, from its smaller endpoint.
template <bool kAll, bool kBoth>
__device__ __forceinline__ void comp_entry(const int32_t *core, int32_t k, int32_t *parent, int32_t v, int32_t w)
{
    if (!kBoth && w < v) return;
    if (!comp_member<kAll>(core, k, w)) return;
    comp_link(parent, v, w);
}

// the linking pass over the rows: one lane per vertex.  Short rows stay with their lane, longer ones are walked by the
// whole wave one after the other, the longest are queued for k_comp_heavy.  kBoth: rows whose label is the giant's are skipped.
template <bool kAll, bool kBoth>
__global__ void k_comp_rows(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ core,
                            int32_t k, uint32_t nv, int32_t *parent, const int32_t *__restrict__ flag, CompCtl *ctl,
                            int32_t *__restrict__ heavy, uint32_t heavy_cap)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    bool act = v < nv && flag[v] != 0;
    if (kBoth && act) act = pload(parent + v) != ctl->giant;
    uint32_t b = 0, e = 0;
    if (act) { b = rowptr[v]; e = rowptr[v + 1]; }
    const uint32_t deg = e - b;
    if (act && deg >= kCompHeavy) {
        const uint32_t slot = atomicAdd(&ctl->n_heavy, 1u);
        if (slot < heavy_cap) heavy[slot] = (int32_t)v;     // (cannot overflow: heavy_cap counts every row this long)
        act = false;
    }
    const bool mid = act && deg > kCompShort;
    if (act && !mid)
        for (uint32_t i = b; i < e; ++i) comp_entry<kAll, kBoth>(core, k, parent, (int32_t)v, col[i]);
    wave_turns(mid, [&](int src) {
        const int32_t rv = (int32_t)from_lane(v, src);
        const uint32_t rb = from_lane(b, src), rn = from_lane(deg, src);
        wave_walk(rb, rn, lane, [&](uint32_t i) { comp_entry<kAll, kBoth>(core, k, parent, rv, col[i]); });
    });
}

// the queued rows: block (x, y) takes the rows x, x + gridDim.x, ... and of each the entries y * kBlock + lane, stepping gridDim.y * kBlock
template <bool kAll, bool kBoth>
__global__ void k_comp_heavy(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ core,
                             int32_t k, int32_t *parent, const CompCtl *ctl, const int32_t *__restrict__ heavy, uint32_t heavy_cap)
{
    uint32_t n = ctl->n_heavy;
    if (n > heavy_cap) n = heavy_cap;
    const uint32_t t = blockIdx.y * kBlock + threadIdx.x, stride = gridDim.y * kBlock;
    for (uint32_t h = blockIdx.x; h < n; h += gridDim.x) {
        const int32_t v = heavy[h];
        const uint32_t b = rowptr[v], e = rowptr[v + 1];
        for (uint32_t i = b + t; i < e; i += stride) comp_entry<kAll, kBoth>(core, k, parent, v, col[i]);
    }
}

// truss kind: one lane per canonical edge of the result; an edge of trussness >= k makes both endpoints members and links them
__global__ void k_comp_truss(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ truss,
                             uint32_t m, int32_t k, int32_t *parent, int32_t *flag)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || truss[i] < k) return;
    const int32_t u = eu[i], v = ev[i];
    flag[u] = 1; flag[v] = 1;                // (every writer stores the same word; read by the next launch)
    comp_link(parent, u, v);
}

// size[v] = cnt[label[v]] (0 for a non-member); members, components (label[v] == v) and the largest size summed up per workgroup
__global__ void k_comp_finish(uint32_t nv, const int32_t *__restrict__ label, const uint32_t *__restrict__ cnt, int32_t *__restrict__ size, CompCtl *ctl)
{
    uint32_t n_mem = 0, n_root = 0, mx = 0;
    for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nv; v += gridDim.x * kBlock) {
        const int32_t lab = label[v];
        const uint32_t sz = lab >= 0 ? cnt[lab] : 0u;
        size[v] = (int32_t)sz;
        n_mem += lab >= 0 ? 1u : 0u;
        if (lab == (int32_t)v) { ++n_root; mx = sz > mx ? sz : mx; }
    }
    class_totals(n_mem, n_root, mx, &ctl->n_members, &ctl->n_components, &ctl->largest);
}

// the linking launches of the core kind (kAll: k == 0, no coreness is read)
template <bool kAll>
void comp_link_rows(komb_ctx *ctx, bool sample, int32_t k, int32_t *parent, const int32_t *flag, CompCtl *ctl, int32_t *heavy, uint32_t heavy_cap)
{
    hipStream_t s = ctx->stream;
    const uint32_t nv = (uint32_t)ctx->nv;
    const int grid = tiles_of(nv);
    const uint32_t *rp = ctx->d_o_rowptr; const int32_t *col = ctx->d_o_col, *core = ctx->core.core;
    if (sample) {
        k_comp_sample<kAll><<<grid, kBlock, 0, s>>>(rp, col, core, k, nv, parent, flag);
        k_comp_flatten<false><<<grid, kBlock, 0, s>>>(nv, parent, flag);
        k_comp_pick<<<1, kCompSamples, 0, s>>>(nv, parent, flag, ctl);
        k_comp_rows<kAll, true><<<grid, kBlock, 0, s>>>(rp, col, core, k, nv, parent, flag, ctl, heavy, heavy_cap);
        k_comp_heavy<kAll, true><<<dim3(kCompHeavyGrid, kCompHeavyChunks), kBlock, 0, s>>>(rp, col, core, k, parent, ctl, heavy, heavy_cap);
    } else {
        k_comp_rows<kAll, false><<<grid, kBlock, 0, s>>>(rp, col, core, k, nv, parent, flag, ctl, heavy, heavy_cap);
        k_comp_heavy<kAll, false><<<dim3(kCompHeavyGrid, kCompHeavyChunks), kBlock, 0, s>>>(rp, col, core, k, parent, ctl, heavy, heavy_cap);
    }
}

} // namespace

// kind and k are checked by the caller (api.cpp); k is the resolved threshold
int components_run(komb_ctx *ctx, int32_t kind, int32_t k)
{
    const int64_t nv = ctx->nv;
    hipStream_t s = ctx->stream;
    ctx->comp.done = false;
    if (!ctx->comp.label) {
        const size_t bytes = (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t);
        KOMB_HIP(ctx, dev_malloc_pair(ctx, ctx->comp.label.slot(nullptr), bytes, ctx->comp.size.slot(nullptr), bytes));
    }
    ctx->comp.kind = kind; ctx->comp.k = k;
    ctx->comp.members = ctx->comp.count = ctx->comp.largest = 0; ctx->comp.ms = 0.0;
    if (nv == 0) { ctx->comp.done = true; return KOMB_OK; }

    const bool truss = kind == KOMB_COMP_TRUSS;
    const int64_t m = truss ? ctx->t_ne : 0;
    if (truss && m > 0) KOMB_TRY(truss_edges_canonical(ctx));       // (a whole-graph result whose endpoints no fetch has asked for yet)

    Range r_all("komb_components_run");
    DevBufs bufs(ctx);
    const uint32_t heavy_cap = (uint32_t)((2 * ctx->ne) / kCompHeavy + 64);   // rows of kCompHeavy entries or more: at most this many
    CompCtl *d_ctl = nullptr; uint32_t *d_cnt = nullptr; int32_t *d_heavy = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
    KOMB_HIP(ctx, bufs.alloc(&d_cnt, (size_t)nv));
    if (!truss) KOMB_HIP(ctx, bufs.alloc(&d_heavy, (size_t)heavy_cap));
    const char *so = ctx_opt(ctx, "COMP_SAMPLE");
    const bool sample = so ? strcmp(so, "0") != 0 : true;

    int32_t *parent = ctx->comp.label, *flag = ctx->comp.size;
    const int grid = tiles_of(nv);
    const bool all = !truss && k == 0;
    // (core kind above the largest coreness: nobody is a member, and nothing is linked)
    const bool none = truss || (k > 0 && k > ctx->stats.max_coreness);
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(CompCtl), s));
    k_comp_init<<<grid, kBlock, 0, s>>>((uint32_t)nv, ctx->core.core, k, all, none, parent, flag, d_cnt);
    if (truss) {
        if (m > 0) k_comp_truss<<<tiles_of(m), kBlock, 0, s>>>(ctx->d_t_eu, ctx->d_t_ev, ctx->d_t_truss, (uint32_t)m, k, parent, flag);
    } else if (!none && ctx->ne > 0) {
        if (all) comp_link_rows<true>(ctx, sample, k, parent, flag, d_ctl, d_heavy, heavy_cap);
        else comp_link_rows<false>(ctx, sample, k, parent, flag, d_ctl, d_heavy, heavy_cap);
    }
    // two passes: the first compresses (every member points at the root it finds, its walk splitting the paths it
    // passes), the second labels -- read-only walks of a step or two
    k_comp_flatten<false><<<grid, kBlock, 0, s>>>((uint32_t)nv, parent, flag);
    k_comp_flatten<true><<<grid, kBlock, 0, s>>>((uint32_t)nv, parent, flag);
    class_count(ctx, nv, nullptr, parent, d_cnt);
    k_comp_finish<<<class_tail_grid(nv), kBlock, 0, s>>>((uint32_t)nv, parent, d_cnt, ctx->comp.size, d_ctl);
    const double ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    CompCtl h;
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(CompCtl)));
    ctx->comp.members = (int64_t)h.n_members; ctx->comp.count = (int64_t)h.n_components; ctx->comp.largest = (int64_t)h.largest;
    ctx->comp.ms = ms;
    ctx->comp.done = true;
    return KOMB_OK;
}

} // namespace komb
