// hierarchy.hip -- the nesting forest of the k-core / k-truss components over all k (komb_hierarchy_run): which component of
// G_k lies inside which component of G_(k-1).  DESIGN.md section 4.6d; the definition is in include/komb_accel.h.
//
// The forest builder (forest.hip; its header comment has CLAIM, ADOPT, the tail and why they are right) over ORIGINAL vertex
// ids.  What is this file's: the ITEMS are the vertices, bucketed by coreness, or by the largest trussness at the vertex; the
// LINKS are the edges of weight k -- weight = min(coreness) of the two ends, or the trussness -- so that after the levels
// >= k the trees are the components of G_k.  A level links only ITS edges: the rows of the vertices of coreness exactly k
// (entries of coreness >= k; short rows: their lane, longer: their wave, the longest: k_hier_heavy), or the edges of
// trussness exactly k; everything heavier is linked already.  The vertices and edges are bucketed by level once, up front
// (a radix sort and the bucket boundaries), and the boundaries are read by the host once: they size every launch of the loop,
// which reads nothing back and waits for nothing.
//
// Why every node has a hooked vertex: a vertex that enters G_k at level k has an edge of this level, which hooks one end of
// it -- before, it was alone.  The exception is the core kind's level 0, the isolated vertices: nothing is linked there, and
// the builder is told so.
#include "forest_dev.h"

namespace komb {

namespace {

constexpr uint32_t kHierShort = 16;         // rows up to this long: the row's own lane
constexpr uint32_t kHierHeavy = 2048;       // rows from this length on: several workgroups of k_hier_heavy (rows between: their wave)
constexpr int kHierHeavyGrid = 64, kHierHeavyChunks = 8;   // k_hier_heavy: rows side by side x workgroups along a row

struct HierCtl {                            // 64 bytes, zeroed before every run
    ForestCtl f;
    uint32_t n_heavy;                       // rows queued for k_hier_heavy so far: it runs on across the levels, each level's
    uint32_t pad[11];                       // rows behind those of the levels before it (a vertex has one coreness)
};
static_assert(sizeof(HierCtl) == 64 && offsetof(HierCtl, f) == 0, "HierCtl layout");

__global__ void k_hier_init(uint32_t nv, int32_t *__restrict__ parent, int32_t *__restrict__ cur, int32_t *__restrict__ claimk,
                            uint32_t *__restrict__ cnt, int32_t *__restrict__ vnode, int32_t *__restrict__ lvl)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    parent[v] = (int32_t)v;
    cur[v] = -1;                             // the node this vertex stands for as a root (the latest)
    claimk[v] = 0x7FFFFFFF;                  // the level that node was made at
    cnt[v] = 0u;
    vnode[v] = -1;
    if (lvl) lvl[v] = 0;
}

__device__ __forceinline__ uint32_t hier_clamp(int32_t x, uint32_t levels)
{
    return x < 0 ? 0u : ((uint32_t)x < levels ? (uint32_t)x : levels - 1u);
}

// core kind: (coreness, vertex) pairs for the sort; rows for k_hier_heavy counted per level
__global__ void k_hier_keys_core(uint32_t nv, const int32_t *__restrict__ core, const uint32_t *__restrict__ rowptr, uint32_t levels,
                                 uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *heavy_hist)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const uint32_t c = hier_clamp(core[v], levels);
    keys[v] = c; vals[v] = v;
    if (rowptr[v + 1] - rowptr[v] >= kHierHeavy) atomicAdd(heavy_hist + c, 1u);
}

// truss kind: (trussness, edge) pairs for the sort; lvl[v] = the largest trussness at v (0: no edge).  The plain read may
// be stale: lvl only grows, so a stale read costs an atomic that changes nothing.
__global__ void k_hier_keys_edges(uint32_t m, const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ truss,
                                  uint32_t levels, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, int32_t *lvl)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int32_t t = (int32_t)hier_clamp(truss[i], levels);
    keys[i] = (uint32_t)t; vals[i] = i;
    const int32_t u = eu[i], v = ev[i];
    if (lvl[u] < t) atomicMax(lvl + u, t);
    if (lvl[v] < t) atomicMax(lvl + v, t);
}

__global__ void k_hier_keys_lvl(uint32_t nv, const int32_t *__restrict__ lvl, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    keys[v] = (uint32_t)lvl[v]; vals[v] = v;
}

// one hook into the log, per lane: the callers sit in row loops whose trip counts differ from lane to lane, where the
// wave-wide ballot of forest_log_wave would miss the lanes that have left
__device__ __forceinline__ void hier_log(HierCtl *ctl, int32_t *log, uint32_t cap, int32_t hooked)
{
    if (hooked < 0) return;
    const uint32_t slot = atomicAdd(&ctl->f.log_n, 1u);
    if (slot < cap) log[slot] = hooked;      // (cannot overflow: a vertex is hooked once)
}

// one entry w of the row of v, a vertex of coreness exactly k: an edge of this level when coreness(w) >= k (between two
// vertices of this level: taken from the smaller one)
__device__ __forceinline__ void hier_entry(const int32_t *core, int32_t k, int32_t *parent, HierCtl *ctl, int32_t *log, uint32_t cap,
                                           int32_t v, int32_t w)
{
    const int32_t cw = core[w];
    if (cw < k || (cw == k && w < v)) return;
    hier_log(ctl, log, cap, comp_link_hooked(parent, v, w));
}

// LINK, core kind: one lane per vertex of the level (vord[sh_b .. sh_b + sh_n)); the row classes of k_comp_rows
__global__ void k_hier_rows(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ core, int32_t k,
                            const uint32_t *__restrict__ vord, uint32_t sh_b, uint32_t sh_n, int32_t *parent, HierCtl *ctl,
                            int32_t *__restrict__ heavy, uint32_t heavy_cap, int32_t *log, uint32_t cap)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    bool act = j < sh_n;
    const int32_t v = act ? (int32_t)vord[sh_b + j] : 0;
    uint32_t b = 0, e = 0;
    if (act) { b = rowptr[v]; e = rowptr[v + 1]; }
    const uint32_t deg = e - b;
    if (act && deg >= kHierHeavy) {
        const uint32_t slot = atomicAdd(&ctl->n_heavy, 1u);
        if (slot < heavy_cap) heavy[slot] = v;              // (cannot overflow: heavy_cap counts every row this long)
        act = false;
    }
    const bool mid = act && deg > kHierShort;
    if (act && !mid)
        for (uint32_t i = b; i < e; ++i) hier_entry(core, k, parent, ctl, log, cap, v, col[i]);
    unsigned long long m = __ballot(mid);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int32_t rv = __shfl(v, src);
        const uint32_t rb = (uint32_t)__shfl((int32_t)b, src), re = (uint32_t)__shfl((int32_t)e, src);
        for (uint32_t i = rb + (uint32_t)lane; i < re; i += kWave) hier_entry(core, k, parent, ctl, log, cap, rv, col[i]);
    }
}

// the level's queued rows heavy[h_b .. h_b + h_n) (the host knows both: the rows this long were counted per level up front): block
// (x, y) takes the rows x, x + gridDim.x, ... and of each the entries y * kBlock + lane, stepping gridDim.y * kBlock
__global__ void k_hier_heavy(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ core, int32_t k,
                             int32_t *parent, HierCtl *ctl, const int32_t *__restrict__ heavy, uint32_t h_b, uint32_t h_n, uint32_t heavy_cap,
                             int32_t *log, uint32_t cap)
{
    if (h_b > heavy_cap) h_b = heavy_cap;
    const uint32_t n = h_n < heavy_cap - h_b ? h_n : heavy_cap - h_b;
    const uint32_t t = blockIdx.y * kBlock + threadIdx.x, stride = gridDim.y * kBlock;
    for (uint32_t h = blockIdx.x; h < n; h += gridDim.x) {
        const int32_t v = heavy[h_b + h];
        if ((uint32_t)v >= cap) continue;                    // (cannot happen: the slot was written at this level; cap is the number of vertices)
        const uint32_t b = rowptr[v], e = rowptr[v + 1];
        for (uint32_t i = b + t; i < e; i += stride) hier_entry(core, k, parent, ctl, log, cap, v, col[i]);
    }
}

// LINK, truss kind: one lane per edge of the level (eord[e_b .. e_b + e_n): canonical edge indices)
__global__ void k_hier_edges(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint32_t *__restrict__ eord,
                             uint32_t e_b, uint32_t e_n, int32_t *parent, HierCtl *ctl, int32_t *log, uint32_t cap)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= e_n) return;
    const uint32_t i = eord[e_b + j];
    hier_log(ctl, log, cap, comp_link_hooked(parent, eu[i], ev[i]));
}

__global__ void k_hier_vertices_out(uint32_t nv, const int32_t *__restrict__ vnode, const int32_t *__restrict__ rank, int32_t *__restrict__ out)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int32_t i = vnode[v];
    out[v] = i >= 0 ? rank[i] : -1;
}

} // namespace

// kind and the state it needs are checked by the caller (api.cpp)
int hierarchy_run(komb_ctx *ctx, int32_t kind)
{
    const int64_t nv = ctx->nv;
    hipStream_t s = ctx->stream;
    const bool truss = kind == KOMB_COMP_TRUSS;
    const size_t cap = (size_t)(nv > 0 ? nv : 1);            // nodes <= vertices (forest.hip)
    if (!ctx->hier.nodes)
        KOMB_HIP(ctx, dev_malloc_pair(ctx, ctx->hier.nodes.slot(nullptr), 5 * cap * sizeof(int32_t), ctx->hier.vnode.slot(nullptr), cap * sizeof(int32_t)));
    // The result arrays are written by the last kernels of the run only, behind every allocation of the run, and the figures
    // are installed at the end: a run that fails for memory leaves the previous result readable (include/komb_accel.h).
    if (nv == 0) {
        ctx->hier.kind = kind; ctx->hier.n_nodes = ctx->hier.n_roots = 0; ctx->hier.depth = 0; ctx->hier.ms = 0.0;
        ctx->hier.kmax = truss ? 2 : 0;
        ctx->hier.done = true;
        return KOMB_OK;
    }

    const int64_t m = truss ? ctx->t_ne : 0;
    if (truss && m > 0) KOMB_TRY(truss_edges_canonical(ctx));       // (a whole-graph result whose endpoints no fetch has asked for yet)

    Range r_all("komb_hierarchy_run");
    DevBufs bufs(ctx);
    const int32_t top = truss ? (m > 0 && ctx->stats.max_trussness > 2 ? ctx->stats.max_trussness : 2) : ctx->stats.max_coreness;
    const uint32_t levels = (uint32_t)(top > 0 ? top : 0) + 1u;     // level numbers 0 .. levels - 1
    const int32_t k_min = truss ? 2 : 0;
    const uint32_t heavy_cap = (uint32_t)((2 * ctx->ne) / kHierHeavy + 64);

    HierCtl *d_ctl = nullptr;
    int32_t *parent = nullptr, *cur = nullptr, *claimk = nullptr, *vnode = nullptr, *lvl = nullptr, *log = nullptr, *d_heavy = nullptr;
    uint32_t *cnt = nullptr, *vkeys = nullptr, *vkeys2 = nullptr, *vvals = nullptr, *vvals2 = nullptr;
    uint32_t *ekeys = nullptr, *ekeys2 = nullptr, *evals = nullptr, *evals2 = nullptr, *d_tab = nullptr;
    ForestNodes t{};
    KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
    KOMB_HIP(ctx, bufs.alloc(&parent, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&cur, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&claimk, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&cnt, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&vnode, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&log, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&t.k, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&t.rep, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&t.par, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&t.size, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&t.shell, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&vkeys, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&vkeys2, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&vvals, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&vvals2, (size_t)nv));
    if (truss) {
        KOMB_HIP(ctx, bufs.alloc(&lvl, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&ekeys, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&ekeys2, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&evals, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&evals2, (size_t)m));
    } else {
        KOMB_HIP(ctx, bufs.alloc(&d_heavy, (size_t)heavy_cap));
    }
    // the level table the host reads once: voff[levels + 1] | eoff[levels + 1] (truss) or heavy rows per level [levels + 1] (core)
    const size_t tab_words = 2 * ((size_t)levels + 1);
    KOMB_HIP(ctx, bufs.alloc(&d_tab, tab_words));
    uint32_t *d_voff = d_tab, *d_second = d_tab + levels + 1;

    const int grid = tiles_of(nv);
    const int bits = forest_bits(levels);
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(HierCtl), s));
    KOMB_HIP(ctx, hipMemsetAsync(d_tab, 0, tab_words * sizeof(uint32_t), s));
    k_hier_init<<<grid, kBlock, 0, s>>>((uint32_t)nv, parent, cur, claimk, cnt, vnode, lvl);
    uint32_t *vord = nullptr, *eord = nullptr, *sorted_keys = nullptr;
    if (truss) {
        if (m > 0) k_hier_keys_edges<<<tiles_of(m), kBlock, 0, s>>>((uint32_t)m, ctx->d_t_eu, ctx->d_t_ev, ctx->d_t_truss, levels, ekeys, evals, lvl);
        KOMB_TRY(prim_sort_pairs_u32_u32(ctx, ekeys, ekeys2, evals, evals2, m, bits, &sorted_keys, &eord));
        forest_offsets(ctx, (uint32_t)m, sorted_keys, levels, d_second);
        k_hier_keys_lvl<<<grid, kBlock, 0, s>>>((uint32_t)nv, lvl, vkeys, vvals);
    } else {
        k_hier_keys_core<<<grid, kBlock, 0, s>>>((uint32_t)nv, ctx->core.core, ctx->d_o_rowptr, levels, vkeys, vvals, d_second);
    }
    KOMB_TRY(prim_sort_pairs_u32_u32(ctx, vkeys, vkeys2, vvals, vvals2, nv, bits, &sorted_keys, &vord));
    forest_offsets(ctx, (uint32_t)nv, sorted_keys, levels, d_voff);
    KOMB_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> tab(tab_words);
    KOMB_HIP(ctx, d2h(ctx, tab.data(), d_tab, tab_words * sizeof(uint32_t)));     // the one read before the loop
    const uint32_t *voff = tab.data(), *second = tab.data() + levels + 1;

    // populated levels: the core kind's have a vertex, the truss kind's an edge
    auto level_vertices = [&](int32_t k) { return voff[k + 1] - voff[k]; };
    auto level_edges = [&](int32_t k) { return second[k + 1] - second[k]; };
    uint32_t n_levels = 0;
    for (int32_t k = (int32_t)levels - 1; k >= k_min; --k) n_levels += (truss ? level_edges(k) : level_vertices(k)) ? 1u : 0u;
    uint32_t *seg = nullptr;                                  // seg[i]: where the i-th populated level's hooks start in the log
    KOMB_HIP(ctx, bufs.alloc(&seg, (size_t)n_levels + 1));
    KOMB_HIP(ctx, hipMemsetAsync(seg, 0, ((size_t)n_levels + 1) * sizeof(uint32_t), s));

    const ForestState f{parent, log, claimk, cur, cnt, seg, vnode, t, &d_ctl->f, (uint32_t)nv};
    int32_t k_top = k_min;
    uint32_t li = 0, heavy_done = 0;                         // heavy_done: the queued rows of the levels behind us
    for (int32_t k = (int32_t)levels - 1; k >= k_min; --k) {  // no read and no wait in this loop
        const uint32_t sh_b = voff[k], sh_n = level_vertices(k);
        const uint32_t e_n = truss ? level_edges(k) : 0u;
        if (!(truss ? e_n : sh_n)) continue;
        if (li == 0) k_top = k;
        uint64_t hooks;                                      // at most this many hooks at this level
        if (truss) {
            k_hier_edges<<<tiles_of(e_n), kBlock, 0, s>>>(ctx->d_t_eu, ctx->d_t_ev, eord, second[k], e_n, parent, d_ctl, log, (uint32_t)nv);
            hooks = e_n < (uint64_t)nv ? e_n : (uint64_t)nv;
        } else {
            if (k > 0) {                                     // (coreness 0: no row has an entry)
                k_hier_rows<<<tiles_of(sh_n), kBlock, 0, s>>>(ctx->d_o_rowptr, ctx->d_o_col, ctx->core.core, k, vord, sh_b, sh_n, parent, d_ctl,
                                                               d_heavy, heavy_cap, log, (uint32_t)nv);
                if (second[k])
                    k_hier_heavy<<<dim3(second[k] < (uint32_t)kHierHeavyGrid ? second[k] : kHierHeavyGrid, kHierHeavyChunks), kBlock, 0, s>>>(
                        ctx->d_o_rowptr, ctx->d_o_col, ctx->core.core, k, parent, d_ctl, d_heavy, heavy_done, second[k], heavy_cap, log, (uint32_t)nv);
                heavy_done += second[k];
            }
            hooks = (uint64_t)nv - voff[k];                  // the vertices of coreness >= k
        }
        forest_level(ctx, f, k, li, !truss && k == 0, vord, sh_b, sh_n, hooks);
        ++li;
    }
    KOMB_HIP(ctx, hipGetLastError());
    HierCtl h;
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(HierCtl)));     // the number of nodes sizes the tail
    if (h.f.n_nodes > (uint64_t)nv || h.f.log_n > (uint64_t)nv)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_hierarchy_run: inconsistent state (%u nodes, %u hooks, %lld vertices)", h.f.n_nodes, h.f.log_n, (long long)nv);
    if (h.n_heavy != heavy_done)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_hierarchy_run: inconsistent state (%u long rows queued, %u counted)", h.n_heavy, heavy_done);
    const uint32_t n = h.f.n_nodes;

    ForestNodes out{ctx->hier.nodes, ctx->hier.nodes + cap, ctx->hier.nodes + 2 * cap,
                    (uint32_t *)ctx->hier.nodes.get() + 3 * cap, (uint32_t *)ctx->hier.nodes.get() + 4 * cap};
    int32_t *rank = cur;                                      // (cur[] has served; n <= nv)
    if (n > 0) KOMB_TRY(forest_tail(ctx, bufs, f, n, bits, out, rank, nullptr, vvals, vvals2));   // (the vertices' sort has served: n <= nv)
    ctx->hier.done = false;                                   // from here on the previous result is being overwritten
    k_hier_vertices_out<<<grid, kBlock, 0, s>>>((uint32_t)nv, vnode, rank, ctx->hier.vnode);
    const double ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(HierCtl)));
    ctx->hier.kind = kind;
    ctx->hier.n_nodes = (int64_t)n; ctx->hier.n_roots = (int64_t)h.f.n_roots; ctx->hier.depth = h.f.depth;
    ctx->hier.kmax = n > 0 ? k_top : k_min;
    ctx->hier.ms = ms;
    ctx->hier.done = true;
    return KOMB_OK;
}

} // namespace komb
