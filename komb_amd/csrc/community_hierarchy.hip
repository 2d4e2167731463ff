// community_hierarchy.hip -- the nesting forest of the k-truss communities over all k (komb_community_hierarchy_run): which
// community of C_k lies inside which community of C_(k-1).  DESIGN.md section 4.6e; the definition is in include/komb_accel.h.
//
// communities.hip's member list (the edges of trussness >= 3 compacted in canonical order, an oriented CSR of its own) and its
// triangle search (oriented_search_dev.h: walk the shorter side, bisect the longer; the same three length classes) joined to
// the forest builder (forest.hip; its header comment has CLAIM, ADOPT, the tail and why they are right).  This file's: the ITEMS are the
// member edges, by position in the member list (kept[] is monotone, so kept[root] is the smallest canonical index), bucketed
// by their own trussness; the LINKS are triangle records (j, x) and (j, y) of weight w = the smallest trussness of the
// triangle's three edges -- the level at which the triangle starts to bind.  The triangles are enumerated ONCE into a record
// stream (a counting launch of the same search sizes it: 2 T records), the stream is sorted by w, and the boundaries of the
// buckets are read by the host once: they size every launch of the loop, which reads nothing back and waits for nothing.
// Nothing is linked during the enumeration -- a union made at the wrong level cannot be undone.  LINK (k_ch_link) is one lane
// per record of the level; the hooks go to the log, slots taken per WAVE.
//
// Why every node has a hooked member: a member of trussness k lies in a triangle of the k-truss, so it has a record of weight
// exactly k; it was alone before, so the tree it ends the level in holds a member hooked at this level.
#include "forest_dev.h"
#include "oriented_search_dev.h"

namespace komb {

namespace {

constexpr uint32_t kChShort = 16;           // shorter side up to this long: the edge's own lane (communities.hip's classes)
constexpr uint32_t kChHeavy = 2048;         // from this length on: several workgroups of k_ch_heavy (between: the edge's wave)
constexpr int kChHeavyGrid = 256, kChHeavyChunks = 8;
constexpr uint64_t kChMaxRecords = 0x7FFFFFFFull;   // the record stream is indexed with 32 bits

struct ChCtl {                              // 64 bytes, zeroed before every run
    ForestCtl f;
    uint32_t n_heavy;                       // members queued for k_ch_heavy
    uint32_t n_members;
    uint32_t rec_n;                         // records written so far
    uint32_t pad0;
    unsigned long long n_tri;               // the counting launch: triangles
    uint32_t pad[6];
};
static_assert(sizeof(ChCtl) == 64 && offsetof(ChCtl, f) == 0, "ChCtl layout");

// ---- members: the edges of trussness >= 3 in canonical order

// the member list; every member a class of its own that stands for no node yet
__global__ void k_ch_compact(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ truss,
                             uint32_t m, uint32_t levels, const uint32_t *__restrict__ pos, int32_t *__restrict__ kept,
                             int32_t *__restrict__ mu, int32_t *__restrict__ mv, int32_t *__restrict__ mt, uint32_t *__restrict__ mkeys,
                             uint32_t *__restrict__ mvals, int32_t *__restrict__ parent, uint32_t *__restrict__ cnt,
                             int32_t *__restrict__ cur, int32_t *__restrict__ claimk)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || truss[i] < 3) return;
    const uint32_t j = pos[i];
    const int32_t t = (uint32_t)truss[i] < levels ? truss[i] : (int32_t)levels - 1;     // (levels > the largest trussness)
    kept[j] = (int32_t)i; mu[j] = eu[i]; mv[j] = ev[i]; mt[j] = t;
    mkeys[j] = (uint32_t)t; mvals[j] = j;
    parent[j] = (int32_t)j; cnt[j] = 0u;
    cur[j] = -1;                             // the node this member stands for as a root (the latest)
    claimk[j] = 0x7FFFFFFF;                  // the level that node was made at
}

// ---- the triangle search, counting or writing records

// entry x of the walked side against the searched one [lo, end): the position of the common third vertex there, or false
__device__ __forceinline__ bool ch_search(const int32_t *__restrict__ mv, uint32_t x, uint32_t lo, uint32_t end, uint32_t *y)
{
    const int32_t c = mv[x];
    lo = row_lower(mv, c, lo, end);
    if (lo >= end || mv[lo] != c) return false;
    *y = lo;
    return true;
}

struct ChStream { uint32_t *keys; unsigned long long *vals; uint32_t cap; };   // the records: weight | (j << 32) | other member

// the hits of a wave: two records each, (j, x) and (j, y) of weight min(mt); the slots are taken once per wave.  Every lane
// of the wave calls it.
__device__ __forceinline__ void ch_emit(bool hit, uint32_t j, uint32_t x, uint32_t y, const int32_t *__restrict__ mt, ChCtl *ctl, const ChStream &st)
{
    const uint32_t slot = wave_append(hit, &ctl->rec_n, 2u);
    if (!hit || slot >= st.cap || st.cap - slot < 2u) return;       // (cannot happen: the counting launch found every hit; the host checks rec_n)
    const int32_t tj = mt[j], tx = mt[x], ty = mt[y];
    const int32_t w = tj < tx ? (tj < ty ? tj : ty) : (tx < ty ? tx : ty);
    st.keys[slot] = (uint32_t)w;     st.vals[slot] = ((unsigned long long)j << 32) | x;
    st.keys[slot + 1] = (uint32_t)w; st.vals[slot + 1] = ((unsigned long long)j << 32) | y;
}

// entry x of member j's walked side, for the lane with valid set; called by whole waves
template <bool kEmit>
__device__ __forceinline__ void ch_entry(bool valid, uint32_t j, uint32_t x, uint32_t lo, uint32_t hi, const int32_t *__restrict__ mv,
                                         const int32_t *__restrict__ mt, ChCtl *ctl, const ChStream &st, uint32_t &found)
{
    uint32_t y = 0;
    const bool hit = valid && ch_search(mv, x, lo, hi, &y);
    if (kEmit) ch_emit(hit, j, x, y, mt, ctl, st);
    else found += hit ? 1u : 0u;
}

// the triangle pass: one lane per member.  A short walked side stays with its lane, longer ones are walked by the whole wave
// one after the other, the longest are queued for k_ch_heavy (by the counting launch; the writing launch finds the queue).
template <bool kEmit>
__global__ void k_ch_tri(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, const int32_t *__restrict__ mt,
                         const uint32_t *__restrict__ rs, const uint32_t *__restrict__ re, const uint32_t *__restrict__ n_mem, ChCtl *ctl,
                         int32_t *__restrict__ heavy, uint32_t heavy_cap, uint32_t n_short, uint32_t n_heavy, ChStream st)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    EdgeSides s{0, 0, 0, 0, true};
    if (j < *n_mem) s = edge_sides(mu, mv, rs, re, j);
    bool act = s.n > 0;
    if (act && s.n >= n_heavy) {
        if (!kEmit) {
            const uint32_t slot = atomicAdd(&ctl->n_heavy, 1u);
            if (slot < heavy_cap) heavy[slot] = (int32_t)j;      // (cannot overflow: heavy_cap is the number of edges)
        }
        act = false;
    }
    const bool mid = act && s.n > n_short;
    uint32_t found = 0;
    const uint32_t own = act && !mid ? s.n : 0u;
    const uint32_t top = wave_max(own);
    for (uint32_t i = 0; i < top; ++i) ch_entry<kEmit>(i < own, j, s.it + i, s.lo, s.hi, mv, mt, ctl, st, found);
    wave_turns(mid, [&](int src) {
        const uint32_t rj = from_lane(j, src);
        const EdgeSides r = from_lane(s, src);
        wave_walk_all(r.it, r.n, lane, [&](uint32_t x, bool in) { ch_entry<kEmit>(in, rj, x, r.lo, r.hi, mv, mt, ctl, st, found); });
    });
    if (!kEmit) {
        found = wave_sum(found);
        if (lane == 0 && found) atomicAdd(&ctl->n_tri, (unsigned long long)found);
        if (j == 0) ctl->n_members = *n_mem;
    }
}

// the queued members: block (x, y) takes the members x, x + gridDim.x, ... and of each the entries y * kBlock + lane, stepping gridDim.y * kBlock
template <bool kEmit>
__global__ void k_ch_heavy(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, const int32_t *__restrict__ mt,
                           const uint32_t *__restrict__ rs, const uint32_t *__restrict__ re, ChCtl *ctl, const int32_t *__restrict__ heavy,
                           uint32_t heavy_cap, ChStream st)
{
    uint32_t n = ctl->n_heavy;
    if (n > heavy_cap) n = heavy_cap;
    const uint32_t t = blockIdx.y * kBlock + threadIdx.x, stride = gridDim.y * kBlock;
    uint32_t found = 0;
    for (uint32_t h = blockIdx.x; h < n; h += gridDim.x) {
        const uint32_t j = (uint32_t)heavy[h];
        const EdgeSides s = edge_sides(mu, mv, rs, re, j);
        for (uint32_t base = 0; base < s.n; base += stride)      // (uniform per workgroup)
            ch_entry<kEmit>(base + t < s.n, j, s.it + base + t, s.lo, s.hi, mv, mt, ctl, st, found);
    }
    if (!kEmit) {
        found = wave_sum(found);
        if ((threadIdx.x & (kWave - 1)) == 0 && found) atomicAdd(&ctl->n_tri, (unsigned long long)found);
    }
}

// ---- the levels

// LINK: one lane per record of the level (recs[r_b .. r_b + r_n)); the hooked roots go to the log, a wave's slots at once
__global__ void k_ch_link(const unsigned long long *__restrict__ recs, uint32_t r_b, uint32_t r_n, uint32_t n_mem, int32_t *parent,
                          ChCtl *ctl, int32_t *__restrict__ log, uint32_t cap)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    int32_t hooked = -1;
    if (i < r_n) {
        const unsigned long long r = recs[r_b + i];
        const uint32_t j = (uint32_t)(r >> 32), x = (uint32_t)r;
        if (j < n_mem && x < n_mem) hooked = comp_link_hooked(parent, (int32_t)j, (int32_t)x);
    }
    forest_log_wave(hooked, &ctl->f, log, cap);
}

// node[] in canonical order; mnode == nullptr: no members
__global__ void k_ch_edges_out(uint32_t m, const int32_t *__restrict__ truss, const uint32_t *__restrict__ pos, const int32_t *__restrict__ mnode,
                               const int32_t *__restrict__ rank, uint32_t n, int32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    int32_t nd = -1;
    if (mnode && truss[i] >= 3) {
        const int32_t made = mnode[pos[i]];
        if (made >= 0 && (uint32_t)made < n) nd = rank[made];
    }
    out[i] = nd;
}

// komb_community_hierarchy_labels: from node[i] up while the parent's level is still >= k; k == 2: an edge without a node is
// a community of its own
__global__ void k_ch_labels(uint32_t m, int32_t k, const int32_t *__restrict__ enode, uint32_t n, const int32_t *__restrict__ nk,
                            const int32_t *__restrict__ rep, const int32_t *__restrict__ par, const int32_t *__restrict__ size,
                            int32_t *__restrict__ label, int32_t *__restrict__ lsize)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    int32_t lab = -1, sz = 0;
    int32_t c = enode[i];
    if (c < 0 || (uint32_t)c >= n) {
        if (k <= 2) { lab = (int32_t)i; sz = 1; }
    } else if (nk[c] >= k) {
        c = forest_walk_up(c, k, nk, par);
        lab = rep[c]; sz = size[c];
    }
    label[i] = lab; lsize[i] = sz;
}

} // namespace

// the state it needs is checked by the caller (api.cpp).  The result is built in blocks of its own and replaces the
// previous one only when the run has succeeded.
int community_hierarchy_run(komb_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));             // (a whole-graph result whose endpoints no fetch has asked for yet)

    Range r_all("komb_community_hierarchy_run");
    komb_ctx::CommunityHierarchy res;                            // the new result: goes back to the pool unless it is installed
    size_t cap_nodes = 1;
    KOMB_HIP(ctx, ctx->pool.get((void **)res.enode.slot(&ctx->pool), (size_t)(m > 0 ? m : 1) * sizeof(int32_t)));

    if (m > 0) {
        DevBufs bufs(ctx);
        const int32_t top = ctx->stats.max_trussness > 2 ? ctx->stats.max_trussness : 2;
        const uint32_t levels = (uint32_t)top + 1u;              // level numbers 0 .. levels - 1
        const int bits = forest_bits(levels);
        const uint32_t heavy_cap = (uint32_t)m;                  // every member could be queued
        const uint32_t n_short = ctx_opt_u32(ctx, "COMM_SHORT", kChShort);      // (tests: every edge through the wave / the queued path)
        uint32_t n_heavy = ctx_opt_u32(ctx, "COMM_HEAVY", kChHeavy);
        if (n_heavy <= n_short) n_heavy = n_short + 1;

        ChCtl *d_ctl = nullptr;
        uint32_t *d_flag = nullptr, *d_pos = nullptr, *d_rs = nullptr, *d_re = nullptr, *mkeys = nullptr, *mkeys2 = nullptr, *mvals = nullptr, *mvals2 = nullptr;
        int32_t *kept = nullptr, *mu = nullptr, *mv = nullptr, *mt = nullptr, *parent = nullptr, *cur = nullptr, *claimk = nullptr, *d_heavy = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)m + 1));       // membership for the scan; then cnt[] (edges per root)
        KOMB_HIP(ctx, bufs.alloc(&d_pos, (size_t)m + 1));
        KOMB_HIP(ctx, bufs.alloc(&kept, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mu, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mv, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mt, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mkeys, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mkeys2, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mvals, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&mvals2, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&parent, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&cur, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&claimk, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&d_heavy, (size_t)heavy_cap));

        const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *truss = ctx->d_t_truss;
        const uint32_t *d_nm = d_pos + m;                        // the number of members, on the device
        uint32_t *cnt = d_flag;
        const int grid = tiles_of(m);
        ctx->timer.start(s);
        KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(ChCtl), s));
        KOMB_TRY(prim_flag_ge_scan(ctx, truss, m, 3, d_flag, d_pos));
        k_ch_compact<<<grid, kBlock, 0, s>>>(eu, ev, truss, (uint32_t)m, levels, d_pos, kept, mu, mv, mt, mkeys, mvals, parent, cnt, cur, claimk);
        KOMB_TRY(oriented_rows(ctx, bufs, mu, m, d_nm, &d_rs, &d_re));
        // the counting launch: the triangles of the result (an edge of a triangle has trussness >= 3: all of them are found here)
        const ChStream none{nullptr, nullptr, 0u};
        k_ch_tri<false><<<grid, kBlock, 0, s>>>(mu, mv, mt, d_rs, d_re, d_nm, d_ctl, d_heavy, heavy_cap, n_short, n_heavy, none);
        k_ch_heavy<false><<<dim3(kChHeavyGrid, kChHeavyChunks), kBlock, 0, s>>>(mu, mv, mt, d_rs, d_re, d_ctl, d_heavy, heavy_cap, none);
        KOMB_HIP(ctx, hipGetLastError());
        ChCtl h;
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(ChCtl)));       // members and triangles size everything behind
        const uint32_t nm = h.n_members;
        if ((int64_t)nm > m || h.n_heavy > heavy_cap)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_community_hierarchy_run: inconsistent state (%u members, %u queued, %lld edges)", nm, h.n_heavy, (long long)m);
        if (h.n_tri > kChMaxRecords / 2)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_community_hierarchy_run: %llu triangles: two link records each do not fit 32-bit indexing", h.n_tri);
        const uint32_t n_rec = 2u * (uint32_t)h.n_tri;
        uint32_t n = 0;
        int32_t *mnode = nullptr, *rank = cur;                   // (cur[] has served when the ranks are made; nodes <= members)

        if (nm > 0) {
            ChStream st{nullptr, nullptr, n_rec};
            uint32_t *rkeys2 = nullptr, *d_tab = nullptr, *seg = nullptr;
            unsigned long long *rvals2 = nullptr;
            int32_t *log = nullptr;
            ForestNodes t{};
            KOMB_HIP(ctx, bufs.alloc(&st.keys, (size_t)n_rec));
            KOMB_HIP(ctx, bufs.alloc(&rkeys2, (size_t)n_rec));
            KOMB_HIP(ctx, bufs.alloc(&st.vals, (size_t)n_rec));
            KOMB_HIP(ctx, bufs.alloc(&rvals2, (size_t)n_rec));
            KOMB_HIP(ctx, bufs.alloc(&mnode, (size_t)nm));
            KOMB_HIP(ctx, bufs.alloc(&log, (size_t)nm));
            KOMB_HIP(ctx, bufs.alloc(&t.k, (size_t)nm));
            KOMB_HIP(ctx, bufs.alloc(&t.rep, (size_t)nm));
            KOMB_HIP(ctx, bufs.alloc(&t.par, (size_t)nm));
            KOMB_HIP(ctx, bufs.alloc(&t.size, (size_t)nm));
            KOMB_HIP(ctx, bufs.alloc(&t.shell, (size_t)nm));
            // the level table the host reads once: moff[levels + 1] (members by trussness) | roff[levels + 1] (records by weight)
            const size_t tab_words = 2 * ((size_t)levels + 1);
            KOMB_HIP(ctx, bufs.alloc(&d_tab, tab_words));
            uint32_t *d_moff = d_tab, *d_roff = d_tab + levels + 1;
            KOMB_HIP(ctx, hipMemsetAsync(d_tab, 0, tab_words * sizeof(uint32_t), s));

            const int mgrid = tiles_of(nm);
            k_ch_tri<true><<<mgrid, kBlock, 0, s>>>(mu, mv, mt, d_rs, d_re, d_nm, d_ctl, d_heavy, heavy_cap, n_short, n_heavy, st);
            if (h.n_heavy)
                k_ch_heavy<true><<<dim3(kChHeavyGrid, kChHeavyChunks), kBlock, 0, s>>>(mu, mv, mt, d_rs, d_re, d_ctl, d_heavy, heavy_cap, st);
            uint32_t *rsorted = nullptr, *msorted = nullptr, *mord = nullptr;
            unsigned long long *recs = nullptr;
            KOMB_TRY(prim_sort_pairs_u32_u64(ctx, st.keys, rkeys2, st.vals, rvals2, n_rec, 0, bits, &rsorted, &recs));
            forest_offsets(ctx, n_rec, rsorted, levels, d_roff);
            KOMB_TRY(prim_sort_pairs_u32_u32(ctx, mkeys, mkeys2, mvals, mvals2, nm, bits, &msorted, &mord));
            forest_offsets(ctx, nm, msorted, levels, d_moff);
            KOMB_HIP(ctx, hipGetLastError());
            std::vector<uint32_t> tab(tab_words);
            KOMB_HIP(ctx, d2h(ctx, tab.data(), d_tab, tab_words * sizeof(uint32_t)));     // the one read before the loop
            const uint32_t *moff = tab.data(), *roff = tab.data() + levels + 1;
            if (moff[levels] != nm || roff[levels] != n_rec)
                KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_community_hierarchy_run: inconsistent level table (%u of %u members, %u of %u records)",
                          moff[levels], nm, roff[levels], n_rec);

            uint32_t n_levels = 0;
            for (int32_t k = (int32_t)levels - 1; k >= 3; --k) n_levels += moff[k + 1] - moff[k] ? 1u : 0u;
            KOMB_HIP(ctx, bufs.alloc(&seg, (size_t)n_levels + 1));                      // seg[i]: where the i-th populated level's hooks start in the log
            KOMB_HIP(ctx, hipMemsetAsync(seg, 0, ((size_t)n_levels + 1) * sizeof(uint32_t), s));

            const ForestState f{parent, log, claimk, cur, cnt, seg, mnode, t, &d_ctl->f, nm};
            uint32_t li = 0;
            for (int32_t k = (int32_t)levels - 1; k >= 3; --k) {                        // no read and no wait in this loop
                const uint32_t sh_b = moff[k], sh_n = moff[k + 1] - moff[k];
                const uint32_t r_b = roff[k], r_n = roff[k + 1] - roff[k];
                if (!sh_n) continue;                                                    // (a record of weight k has an edge of trussness k)
                if (li == 0) res.kmax = k;
                if (r_n) k_ch_link<<<tiles_of(r_n), kBlock, 0, s>>>(recs, r_b, r_n, nm, parent, d_ctl, log, nm);
                forest_level(ctx, f, k, li, false, mord, sh_b, sh_n, r_n < nm ? r_n : nm);      // at most this many hooks at this level
                ++li;
            }
            KOMB_HIP(ctx, hipGetLastError());
            KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(ChCtl)));                          // the number of nodes sizes the tail
            if (h.f.n_nodes > nm || h.f.log_n > nm || h.rec_n != n_rec)
                KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_community_hierarchy_run: inconsistent state (%u nodes, %u hooks, %u members, %u of %u records)",
                          h.f.n_nodes, h.f.log_n, nm, h.rec_n, n_rec);
            n = h.f.n_nodes;
            if (n > 0) {
                cap_nodes = n;
                KOMB_HIP(ctx, ctx->pool.get((void **)res.nodes.slot(&ctx->pool), 5 * cap_nodes * sizeof(int32_t)));
                ForestNodes out{res.nodes, res.nodes + cap_nodes, res.nodes + 2 * cap_nodes,
                                (uint32_t *)res.nodes.get() + 3 * cap_nodes, (uint32_t *)res.nodes.get() + 4 * cap_nodes};
                KOMB_TRY(forest_tail(ctx, bufs, f, n, bits, out, rank, kept, mvals, mvals2));    // (the members' sort has served: n <= nm)
            }
            k_ch_edges_out<<<grid, kBlock, 0, s>>>((uint32_t)m, truss, d_pos, mnode, rank, n, res.enode);
        } else {
            k_ch_edges_out<<<grid, kBlock, 0, s>>>((uint32_t)m, truss, d_pos, nullptr, nullptr, 0u, res.enode);
        }
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(ChCtl)));
        res.n_nodes = (int64_t)n; res.n_roots = (int64_t)h.f.n_roots; res.depth = h.f.depth; res.members = (int64_t)nm;
        if (n == 0) res.kmax = 2;
    }
    if (!res.nodes) KOMB_HIP(ctx, ctx->pool.get((void **)res.nodes.slot(&ctx->pool), 5 * cap_nodes * sizeof(int32_t)));

    res.cap = (int64_t)cap_nodes;
    res.done = true;
    ctx->ch = std::move(res);
    return KOMB_OK;
}

// k is checked and resolved by the caller (api.cpp): >= 2.  One walk per canonical edge over the stored forest.
int community_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label, int32_t *size)
{
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0;
    if (m == 0 || (!label && !size)) return KOMB_OK;
    hipStream_t s = ctx->stream;
    DevBufs bufs(ctx);
    int32_t *d_label = nullptr, *d_size = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_label, (size_t)m));
    KOMB_HIP(ctx, bufs.alloc(&d_size, (size_t)m));
    const int32_t *nodes = ctx->ch.nodes;
    const size_t c = (size_t)ctx->ch.cap;
    k_ch_labels<<<tiles_of(m), kBlock, 0, s>>>((uint32_t)m, k, ctx->ch.enode, (uint32_t)ctx->ch.n_nodes, nodes, nodes + c, nodes + 2 * c,
                                              nodes + 3 * c, d_label, d_size);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, hipStreamSynchronize(s));
    if (label) KOMB_HIP(ctx, staged_copy(ctx, label, d_label, (size_t)m * sizeof(int32_t), false));
    if (size) KOMB_HIP(ctx, staged_copy(ctx, size, d_size, (size_t)m * sizeof(int32_t), false));
    return KOMB_OK;
}

} // namespace komb
