// hierarchy.hip -- the nesting forest of the k-core / k-truss components over all k (komb_hierarchy_run): which component of
// G_k lies inside which component of G_(k-1).  DESIGN.md section 4.6d; the definition is in include/komb_accel.h.
//
// One union-find over ORIGINAL vertex ids (unionfind_dev.h: a root is the smallest id of its tree, whatever the schedule)
// takes the levels from the largest k down: after the edges of weight >= k are linked -- weight = min(coreness) of the two
// ends, or the trussness -- its trees are the components of G_k.  A level links only ITS edges: the rows of the vertices of
// coreness exactly k (entries of coreness >= k), or the edges of trussness exactly k; everything heavier is linked already.
// The vertices and edges are bucketed by level once, up front (a radix sort and the bucket boundaries), and the boundaries
// are read by the host once: they size every launch of the loop, which reads nothing back and waits for nothing.
//
// What a level changes is told by its HOOKS.  comp_link_hooked reports the root it hung under a smaller id; a vertex is
// hooked at most once in the whole run (it is never a root again), so one log of nv entries holds all levels, each a
// segment.  The vertex set of a component changed at level k exactly when one of its vertices was hooked at level k (a
// vertex that enters G_k at level k has an edge of this level, which hooks one end of it: before, it was alone): the roots of
// the hooked vertices are this level's nodes, every node has a hooked vertex of its own (or is an isolated vertex, core kind,
// k = 0), and so there are at most nv nodes.
//
// Per populated level, in launches of their own (a kernel boundary between them: no hook is in flight when roots are read,
// and a word written by one launch is read by a later one only):
//   LINK   the level's rows (short: their lane, longer: their wave, the longest: k_hier_heavy) or edges; hooks to the log
//   CLAIM  for every hooked x: cnt[root] += cnt[x] (x was a root before this level: cnt[x] is final), and ONE lane per root
//          -- an atomicMin on the level the root was last claimed at -- makes the node (k, root); a node the root stood for
//          before becomes its child.  For every vertex of this level: cnt[root] += 1.
//   ADOPT  for every hooked x that stood for a node: that node's parent is its root's node.  For every vertex of this level:
//          node[v] = its root's node, whose shell counts it.  A node's size is its root's count.
// The tail sorts the nodes by (k, rep), which numbers them, and maps parents and node[] through the ranks.
// Every access to parent[] is a relaxed agent-scope atomic (the header comment of components.hip says why that suffices).
#include "common.h"
#include "unionfind_dev.h"

namespace komb {

namespace {

constexpr uint32_t kHierShort = 16;         // rows up to this long: the row's own lane
constexpr uint32_t kHierHeavy = 2048;       // rows from this length on: several workgroups of k_hier_heavy (rows between: their wave)
constexpr int kHierHeavyGrid = 64, kHierHeavyChunks = 8;   // k_hier_heavy: rows side by side x workgroups along a row
constexpr int kHierStepGrid = 2048;         // k_hier_claim / k_hier_adopt: at most this many workgroups, each striding

struct HierCtl {                            // 64 bytes, zeroed before every run
    uint32_t n_heavy;                       // rows queued for k_hier_heavy (this level)
    uint32_t log_n;                         // hooked vertices so far
    uint32_t n_nodes;                       // nodes so far
    uint32_t n_roots;                       // tail: nodes without a parent
    int32_t  depth;                         // tail: most nodes on a path from a root down
    uint32_t pad[11];
};
static_assert(sizeof(HierCtl) == 64, "HierCtl layout");

struct HierNodes { int32_t *k, *rep, *par; uint32_t *size, *shell; };   // nodes in the order they were made / in final order

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

// off[k] = the first position of the sorted keys with a key >= k, for k = 0 .. levels (every word written exactly once)
__global__ void k_hier_offsets(uint32_t n, const uint32_t *__restrict__ keys, uint32_t levels, uint32_t *__restrict__ off)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    const uint32_t first = i > 0 ? keys[i - 1] + 1u : 0u;
    const uint32_t last = i < n ? keys[i] : levels;
    for (uint32_t k = first; k <= last && k <= levels; ++k) off[k] = i;
}

__device__ __forceinline__ void hier_log(HierCtl *ctl, int32_t *log, uint32_t cap, int32_t hooked)
{
    if (hooked < 0) return;
    const uint32_t slot = atomicAdd(&ctl->log_n, 1u);
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

// the queued rows: block (x, y) takes the rows x, x + gridDim.x, ... and of each the entries y * kBlock + lane, stepping gridDim.y * kBlock
__global__ void k_hier_heavy(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int32_t *__restrict__ core, int32_t k,
                             int32_t *parent, HierCtl *ctl, const int32_t *__restrict__ heavy, uint32_t heavy_cap, int32_t *log, uint32_t cap)
{
    uint32_t n = ctl->n_heavy;
    if (n > heavy_cap) n = heavy_cap;
    const uint32_t t = blockIdx.y * kBlock + threadIdx.x, stride = gridDim.y * kBlock;
    for (uint32_t h = blockIdx.x; h < n; h += gridDim.x) {
        const int32_t v = heavy[h];
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

// arr[key] += the lanes of the wave that hold key, one atomic per distinct key; every lane of the wave calls it, key < 0 takes no part
__device__ __forceinline__ void hier_wave_add(uint32_t *arr, int32_t key)
{
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = key >= 0;
    unsigned long long m = __ballot(act);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        const int32_t lead = __shfl(key, src);
        const unsigned long long same = __ballot(act && key == lead);
        if (lane == src) atomicAdd(arr + lead, (uint32_t)__popcll(same));
        m &= ~same;
    }
}

// the node (k, r) of root r, made by the first lane that asks for it at this level (levels descend: the atomicMin tells it)
__device__ __forceinline__ void hier_claim(int32_t r, int32_t k, HierCtl *ctl, int32_t *claimk, int32_t *cur, const HierNodes &t, uint32_t cap)
{
    if (pload(claimk + r) <= k) return;      // (the word only falls: a stale read costs the atomic, no more)
    if (atomicMin(claimk + r, k) <= k) return;
    const uint32_t id = atomicAdd(&ctl->n_nodes, 1u);
    if (id >= cap) return;                   // (cannot happen: every node has a hooked or isolated vertex of its own; the host checks n_nodes)
    t.k[id] = k; t.rep[id] = r; t.par[id] = -1; t.size[id] = 0u; t.shell[id] = 0u;
    const int32_t prev = cur[r];             // cur[r] belongs to this lane: r is a root, and only its claimer touches it in this launch
    if (prev >= 0) t.par[prev] = (int32_t)id;    // the same root stood for a component of a higher level: now a child
    cur[r] = (int32_t)id;
}

// CLAIM (after the level's LINK launches; hooks nothing: a vertex read as a root is one.  Its walks still split the paths they pass --
// parent[] is no output here, and ADOPT's read-only walks are then a step or two).  seg[li] .. log_n is the level's segment of the log.
__global__ void k_hier_claim(int32_t k, uint32_t li, bool isolated, const uint32_t *__restrict__ vord, uint32_t sh_b, uint32_t sh_n,
                             int32_t *parent, const int32_t *__restrict__ log, uint32_t *seg, HierCtl *ctl,
                             int32_t *claimk, int32_t *cur, uint32_t *cnt, HierNodes t, uint32_t cap)
{
    const uint32_t lb = seg[li];
    uint32_t le = ctl->log_n;
    if (le > cap) le = cap;
    const uint32_t gt = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    if (gt == 0) { seg[li + 1] = le; ctl->n_heavy = 0u; }       // (read by later launches only)
    const int lane = threadIdx.x & (kWave - 1);
    for (uint32_t base = lb + blockIdx.x * kBlock; base < le; base += stride) {  // (uniform per workgroup: the ballots see whole waves)
        const uint32_t i = base + threadIdx.x;
        int32_t r = -1;
        if (i < le) {
            const int32_t x = log[i];
            r = comp_find(parent, x);
            const uint32_t c = cnt[x];       // x is no root any more: nobody adds to cnt[x] now
            if (c) atomicAdd(cnt + r, c);
        }
        unsigned long long m = __ballot(r >= 0);                                 // one lane per distinct root of the wave asks for its node
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            const int32_t lead = __shfl(r, src);
            const unsigned long long same = __ballot(r == lead);
            if (lane == src) hier_claim(lead, k, ctl, claimk, cur, t, cap);
            m &= ~same;
        }
    }
    for (uint32_t base = blockIdx.x * kBlock; base < sh_n; base += stride) {
        const uint32_t j = base + threadIdx.x;
        int32_t r = -1;
        if (j < sh_n) {
            r = comp_find(parent, (int32_t)vord[sh_b + j]);
            if (isolated) hier_claim(r, k, ctl, claimk, cur, t, cap);            // core kind, k = 0: nothing was linked, every vertex is its own root
        }
        hier_wave_add(cnt, r);
    }
}

// ADOPT (after CLAIM: cur[] of this level's roots is settled)
__global__ void k_hier_adopt(uint32_t li, const uint32_t *__restrict__ vord, uint32_t sh_b, uint32_t sh_n, const int32_t *parent,
                             const int32_t *__restrict__ log, const uint32_t *__restrict__ seg, const int32_t *__restrict__ cur,
                             const uint32_t *__restrict__ cnt, HierNodes t, int32_t *__restrict__ vnode)
{
    const uint32_t lb = seg[li], le = seg[li + 1];
    const uint32_t gt = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    for (uint32_t i = lb + gt; i < le; i += stride) {
        const int32_t x = log[i];
        const int32_t r = comp_find_ro(parent, x);
        const int32_t nr = cur[r], nx = cur[x];
        if (nr < 0) continue;
        if (nx >= 0) t.par[nx] = nr;         // x was the root of a component of a higher level
        t.size[nr] = cnt[r];                 // (every writer stores the same word)
    }
    for (uint32_t base = blockIdx.x * kBlock; base < sh_n; base += stride) {
        const uint32_t j = base + threadIdx.x;
        int32_t nr = -1;
        if (j < sh_n) {
            const int32_t v = (int32_t)vord[sh_b + j];
            const int32_t r = comp_find_ro(parent, v);
            nr = cur[r];
            vnode[v] = nr;
            if (nr >= 0) t.size[nr] = cnt[r];
        }
        hier_wave_add(t.shell, nr);
    }
}

// ---- the tail: nodes into (k, rep) order
__global__ void k_hier_node_keys(uint32_t n, HierNodes t, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((uint64_t)(uint32_t)t.k[i] << 32) | (uint32_t)t.rep[i];
    vals[i] = i;
}

__global__ void k_hier_ranks(uint32_t n, const uint32_t *__restrict__ order, int32_t *__restrict__ rank)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) rank[order[j]] = (int32_t)j;
}

__global__ void k_hier_nodes_out(uint32_t n, const uint32_t *__restrict__ order, const int32_t *__restrict__ rank, HierNodes t, HierNodes out, HierCtl *ctl)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool root = false;
    if (j < n) {
        const uint32_t i = order[j];
        const int32_t p = t.par[i];
        out.k[j] = t.k[i]; out.rep[j] = t.rep[i]; out.par[j] = p >= 0 ? rank[p] : -1;
        out.size[j] = t.size[i]; out.shell[j] = t.shell[i];
        root = p < 0;
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(&ctl->n_roots, (uint32_t)__popcll(m));
}

__global__ void k_hier_vertices_out(uint32_t nv, const int32_t *__restrict__ vnode, const int32_t *__restrict__ rank, int32_t *__restrict__ out)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int32_t i = vnode[v];
    out[v] = i >= 0 ? rank[i] : -1;
}

// the most nodes on a path from a root down (parents have smaller numbers: every walk ends)
__global__ void k_hier_depth(uint32_t n, const int32_t *__restrict__ par, HierCtl *ctl)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    int32_t d = 0;
    if (j < n) {
        d = 1;
        for (int32_t c = (int32_t)j, a = par[j]; a >= 0 && a < c; c = a, a = par[a]) ++d;
    }
    for (int o = kWave / 2; o > 0; o >>= 1) { const int32_t other = __shfl_xor(d, o); d = other > d ? other : d; }
    if ((threadIdx.x & (kWave - 1)) == 0 && d) atomicMax(&ctl->depth, d);
}

inline int hier_grid(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }
inline int hier_bits(uint32_t levels) { int b = 1; while (b < 32 && (1u << b) < levels) ++b; return b; }

} // namespace

// kind and the state it needs are checked by the caller (api.cpp)
int hierarchy_run(komb_ctx *ctx, int32_t kind)
{
    const int64_t nv = ctx->nv;
    hipStream_t s = ctx->stream;
    const bool truss = kind == KOMB_COMP_TRUSS;
    ctx->hier_done = false;
    const size_t cap = (size_t)(nv > 0 ? nv : 1);            // nodes <= vertices (header comment)
    if (!ctx->d_hier_nodes) {
        KOMB_HIP(ctx, dev_malloc(ctx, (void **)&ctx->d_hier_nodes, 5 * cap * sizeof(int32_t)));
        KOMB_HIP(ctx, dev_malloc(ctx, (void **)&ctx->d_hier_vnode, cap * sizeof(int32_t)));
    }
    ctx->hier_kind = kind; ctx->hier_nodes = ctx->hier_roots = 0; ctx->hier_depth = 0; ctx->hier_ms = 0.0;
    ctx->hier_kmax = truss ? 2 : 0;
    if (nv == 0) { ctx->hier_done = true; return KOMB_OK; }

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
    HierNodes t{};
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

    const int grid = hier_grid(nv);
    const int bits = hier_bits(levels);
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(HierCtl), s));
    KOMB_HIP(ctx, hipMemsetAsync(d_tab, 0, tab_words * sizeof(uint32_t), s));
    k_hier_init<<<grid, kBlock, 0, s>>>((uint32_t)nv, parent, cur, claimk, cnt, vnode, lvl);
    uint32_t *vord = nullptr, *eord = nullptr, *sorted_keys = nullptr;
    if (truss) {
        if (m > 0) k_hier_keys_edges<<<hier_grid(m), kBlock, 0, s>>>((uint32_t)m, ctx->d_t_eu, ctx->d_t_ev, ctx->d_t_truss, levels, ekeys, evals, lvl);
        KOMB_TRY(prim_sort_pairs_u32_u32(ctx, ekeys, ekeys2, evals, evals2, m, bits, &sorted_keys, &eord));
        k_hier_offsets<<<hier_grid(m + 1), kBlock, 0, s>>>((uint32_t)m, sorted_keys, levels, d_second);
        k_hier_keys_lvl<<<grid, kBlock, 0, s>>>((uint32_t)nv, lvl, vkeys, vvals);
    } else {
        k_hier_keys_core<<<grid, kBlock, 0, s>>>((uint32_t)nv, ctx->d_core, ctx->d_o_rowptr, levels, vkeys, vvals, d_second);
    }
    KOMB_TRY(prim_sort_pairs_u32_u32(ctx, vkeys, vkeys2, vvals, vvals2, nv, bits, &sorted_keys, &vord));
    k_hier_offsets<<<hier_grid(nv + 1), kBlock, 0, s>>>((uint32_t)nv, sorted_keys, levels, d_voff);
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

    int32_t k_top = k_min;
    uint32_t li = 0;
    for (int32_t k = (int32_t)levels - 1; k >= k_min; --k) {  // no read and no wait in this loop
        const uint32_t sh_b = voff[k], sh_n = level_vertices(k);
        const uint32_t e_n = truss ? level_edges(k) : 0u;
        if (!(truss ? e_n : sh_n)) continue;
        if (li == 0) k_top = k;
        uint64_t hooks;                                      // at most this many hooks at this level
        if (truss) {
            k_hier_edges<<<hier_grid(e_n), kBlock, 0, s>>>(ctx->d_t_eu, ctx->d_t_ev, eord, second[k], e_n, parent, d_ctl, log, (uint32_t)nv);
            hooks = e_n < (uint64_t)nv ? e_n : (uint64_t)nv;
        } else {
            if (k > 0) {                                     // (coreness 0: no row has an entry)
                k_hier_rows<<<hier_grid(sh_n), kBlock, 0, s>>>(ctx->d_o_rowptr, ctx->d_o_col, ctx->d_core, k, vord, sh_b, sh_n, parent, d_ctl,
                                                               d_heavy, heavy_cap, log, (uint32_t)nv);
                if (second[k])
                    k_hier_heavy<<<dim3(second[k] < (uint32_t)kHierHeavyGrid ? second[k] : kHierHeavyGrid, kHierHeavyChunks), kBlock, 0, s>>>(
                        ctx->d_o_rowptr, ctx->d_o_col, ctx->d_core, k, parent, d_ctl, d_heavy, heavy_cap, log, (uint32_t)nv);
            }
            hooks = (uint64_t)nv - voff[k];                  // the vertices of coreness >= k
        }
        const uint64_t work = hooks > sh_n ? hooks : sh_n;
        const int g = (int)((work + kBlock - 1) / kBlock < (uint64_t)kHierStepGrid ? (work + kBlock - 1) / kBlock : (uint64_t)kHierStepGrid);
        k_hier_claim<<<g > 0 ? g : 1, kBlock, 0, s>>>(k, li, !truss && k == 0, vord, sh_b, sh_n, parent, log, seg, d_ctl, claimk, cur, cnt, t, (uint32_t)nv);
        k_hier_adopt<<<g > 0 ? g : 1, kBlock, 0, s>>>(li, vord, sh_b, sh_n, parent, log, seg, cur, cnt, t, vnode);
        ++li;
    }
    KOMB_HIP(ctx, hipGetLastError());
    HierCtl h;
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(HierCtl)));     // the number of nodes sizes the tail
    if (h.n_nodes > (uint64_t)nv || h.log_n > (uint64_t)nv)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_hierarchy_run: inconsistent state (%u nodes, %u hooks, %lld vertices)", h.n_nodes, h.log_n, (long long)nv);
    const uint32_t n = h.n_nodes;

    HierNodes out{ctx->d_hier_nodes, ctx->d_hier_nodes + cap, ctx->d_hier_nodes + 2 * cap,
                  (uint32_t *)ctx->d_hier_nodes + 3 * cap, (uint32_t *)ctx->d_hier_nodes + 4 * cap};
    int32_t *rank = cur;                                      // (cur[] has served; n <= nv)
    if (n > 0) {
        uint64_t *nkeys = nullptr, *nkeys2 = nullptr, *nsorted = nullptr;
        uint32_t *order = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&nkeys, (size_t)n));
        KOMB_HIP(ctx, bufs.alloc(&nkeys2, (size_t)n));
        k_hier_node_keys<<<hier_grid(n), kBlock, 0, s>>>(n, t, nkeys, vvals);
        KOMB_TRY(prim_sort_pairs_u64_u32(ctx, nkeys, nkeys2, vvals, vvals2, n, 32 + bits, &nsorted, &order));
        k_hier_ranks<<<hier_grid(n), kBlock, 0, s>>>(n, order, rank);
        k_hier_nodes_out<<<hier_grid(n), kBlock, 0, s>>>(n, order, rank, t, out, d_ctl);
        k_hier_depth<<<hier_grid(n), kBlock, 0, s>>>(n, out.par, d_ctl);
    }
    k_hier_vertices_out<<<grid, kBlock, 0, s>>>((uint32_t)nv, vnode, rank, ctx->d_hier_vnode);
    const double ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(HierCtl)));
    ctx->hier_nodes = (int64_t)n; ctx->hier_roots = (int64_t)h.n_roots; ctx->hier_depth = h.depth;
    ctx->hier_kmax = n > 0 ? k_top : k_min;
    ctx->hier_ms = ms;
    ctx->hier_done = true;
    return KOMB_OK;
}

} // namespace komb
