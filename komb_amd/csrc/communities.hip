// communities.hip -- k-truss communities (komb_truss_communities_run): the classes of the k-truss' edges under triangle
// connectivity (Huang, Cheng, Qin, Tian, Yu, SIGMOD 2014).  DESIGN.md section 4.6c.
//
// Input: the last k-truss result in canonical order, eu[i] < ev[i], sorted by (eu, ev), original vertex ids -- whole-graph
// and vmask runs alike.  The MEMBER edges (trussness >= k) are compacted in that order: member j is canonical edge
// kept[j], with endpoints (mu[j], mv[j]).  The compacted list is itself an oriented CSR of the k-truss: row a = the
// members with mu == a, [rs[a], re[a]), their mv ascending.  A triangle a < b < c of three members is found exactly
// once, from its edge (a, b) = member j: c is in the part of row a behind j and in row b.  The search is
// oriented_search_dev.h's: the lane walks the SHORTER of the two and bisects the longer (sum over the edges of
// min(d(a), d(b)) <= 2 x arboricity x |E|: no orientation by degree is needed for the bound), and a hit gives the three
// member ids as positions, without any lookup: link(j, x), link(j, y) with x the position of (a, c) and y that of (b, c).
//
// The union-find is components.hip's (unionfind_dev.h) over member ids: hooks hang the larger root under the smaller,
// walks go through strictly decreasing ids, and the root of a finished class is its smallest member id -- kept[] is
// monotone, so kept[root] is the smallest canonical index of the community, the label the interface promises.  What
// that file's header says about stale reads holds word for word for this parent[].  As there, a compressing flatten
// launch is followed by a read-only labelling launch.  No workgroup waits for another; a call is a constant number of
// launches; the one queue (edges whose shorter side is long) has room for every member edge.
#include "oriented_search_dev.h"
#include "unionfind_dev.h"

namespace komb {

namespace {

constexpr uint32_t kCommShort = 16;         // shorter side up to this long: the edge's own lane
constexpr uint32_t kCommHeavy = 2048;       // from this length on: several workgroups of k_comm_heavy (between: the edge's wave)
constexpr int kCommHeavyGrid = 256, kCommHeavyChunks = 8;   // k_comm_heavy: edges side by side x workgroups along one

struct CommCtl {                            // 64 bytes, zeroed before every run
    uint32_t n_heavy;                       // edges queued for k_comm_heavy
    uint32_t n_members, n_communities, largest;
    uint32_t n_multi;                       // vertices in more than one community (the vertex pass)
    uint32_t pad[11];
};
static_assert(sizeof(CommCtl) == 64, "CommCtl layout");

// the member list in canonical order; every member a class of its own
__global__ void k_comm_compact(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ truss,
                               uint32_t m, int32_t k, const uint32_t *__restrict__ pos, int32_t *__restrict__ kept,
                               int32_t *__restrict__ mu, int32_t *__restrict__ mv, int32_t *__restrict__ parent, uint32_t *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || truss[i] < k) return;
    const uint32_t j = pos[i];
    kept[j] = (int32_t)i; mu[j] = eu[i]; mv[j] = ev[i];
    parent[j] = (int32_t)j; cnt[j] = 0u;
}

// entry x of the walked side against the searched one [lo, end): a common third vertex closes a triangle of three members
__device__ __forceinline__ void comm_entry(const int32_t *__restrict__ mv, int32_t *parent, uint32_t j, uint32_t x, uint32_t lo, uint32_t end)
{
    const int32_t c = mv[x];
    lo = row_lower(mv, c, lo, end);
    if (lo >= end || mv[lo] != c) return;
    comp_link(parent, (int32_t)j, (int32_t)x);       // (both positions are behind j: the edges (a, c) and (b, c))
    comp_link(parent, (int32_t)j, (int32_t)lo);
}

// the triangle pass: one lane per member edge.  A short walked side stays with its lane, longer ones are walked by the
// whole wave one after the other, the longest are queued for k_comm_heavy.
__global__ void k_comm_tri(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, const uint32_t *__restrict__ rs,
                           const uint32_t *__restrict__ re, const uint32_t *__restrict__ n_mem, int32_t *parent, CommCtl *ctl,
                           int32_t *__restrict__ heavy, uint32_t heavy_cap, uint32_t n_short, uint32_t n_heavy)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    EdgeSides s{0, 0, 0, 0, true};
    if (j < *n_mem) s = edge_sides(mu, mv, rs, re, j);
    bool act = s.n > 0;
    if (act && s.n >= n_heavy) {
        const uint32_t slot = atomicAdd(&ctl->n_heavy, 1u);
        if (slot < heavy_cap) heavy[slot] = (int32_t)j;      // (cannot overflow: heavy_cap is the number of edges)
        act = false;
    }
    const bool mid = act && s.n > n_short;
    if (act && !mid)
        for (uint32_t x = s.it; x < s.it + s.n; ++x) comm_entry(mv, parent, j, x, s.lo, s.hi);
    wave_turns(mid, [&](int src) {
        const uint32_t rj = from_lane(j, src);
        const EdgeSides r = from_lane(s, src);
        wave_walk(r.it, r.n, lane, [&](uint32_t x) { comm_entry(mv, parent, rj, x, r.lo, r.hi); });
    });
}

// the queued edges: block (x, y) takes the edges x, x + gridDim.x, ... and of each the entries y * kBlock + lane, stepping gridDim.y * kBlock
__global__ void k_comm_heavy(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, const uint32_t *__restrict__ rs,
                             const uint32_t *__restrict__ re, int32_t *parent, const CommCtl *ctl, const int32_t *__restrict__ heavy, uint32_t heavy_cap)
{
    uint32_t n = ctl->n_heavy;
    if (n > heavy_cap) n = heavy_cap;
    const uint32_t t = blockIdx.y * kBlock + threadIdx.x, stride = gridDim.y * kBlock;
    for (uint32_t h = blockIdx.x; h < n; h += gridDim.x) {
        const uint32_t j = (uint32_t)heavy[h];
        const EdgeSides s = edge_sides(mu, mv, rs, re, j);
        for (uint32_t x = s.it + t; x < s.it + s.n; x += stride) comm_entry(mv, parent, j, x, s.lo, s.hi);
    }
}

// !kFinal: every member points itself at the root it finds, its walk splitting the paths it passes (a hint: it may be
// overwritten by another walk's compression).  kFinal: parent[j] = root of j; read-only walks.
template <bool kFinal>
__global__ void k_comm_flatten(const uint32_t *__restrict__ n_mem, int32_t *parent)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= *n_mem) return;
    comp_flatten<kFinal>(parent, j);
}

// canonical order again: label[i] = kept[root], size[i] = cnt[root] (-1 / 0 for a non-member); members, communities
// (root == own position) and the largest size summed up per workgroup
__global__ void k_comm_finish(uint32_t m, const int32_t *__restrict__ truss, int32_t k, const uint32_t *__restrict__ pos,
                              const int32_t *__restrict__ root, const int32_t *__restrict__ kept, const uint32_t *__restrict__ cnt,
                              int32_t *__restrict__ label, int32_t *__restrict__ size, CommCtl *ctl)
{
    uint32_t n_mem = 0, n_root = 0, mx = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
        int32_t lab = -1; uint32_t sz = 0u;
        if (truss[i] >= k) {
            const uint32_t j = pos[i];
            const int32_t r = root[j];
            lab = kept[r]; sz = cnt[r];
            ++n_mem;
            if (r == (int32_t)j) { ++n_root; mx = sz > mx ? sz : mx; }
        }
        label[i] = lab; size[i] = (int32_t)sz;
    }
    class_totals(n_mem, n_root, mx, &ctl->n_members, &ctl->n_communities, &ctl->largest);
}

// ---- the vertex pass: n_comm[v] = distinct labels among the member edges at v

__global__ void k_comm_vflag(const int32_t *__restrict__ label, uint32_t m, uint32_t *__restrict__ flag)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > m) return;
    flag[i] = i < m && label[i] >= 0 ? 1u : 0u;
}

// two keys per member edge: (endpoint << 32) | label
__global__ void k_comm_keys(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ label,
                            uint32_t m, const uint32_t *__restrict__ pos, uint64_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int32_t lab = label[i];
    if (lab < 0) return;
    const uint64_t j = pos[i];
    keys[2 * j] = ((uint64_t)(uint32_t)eu[i] << 32) | (uint32_t)lab;
    keys[2 * j + 1] = ((uint64_t)(uint32_t)ev[i] << 32) | (uint32_t)lab;
}

// the sorted distinct keys: the first key of a vertex finds the end of its run by bisection and writes the run's length
// (n_comm zeroed before); vertices with more than one community are counted per workgroup
__global__ void k_comm_runs(const uint64_t *__restrict__ uk, uint32_t n, int32_t *__restrict__ n_comm, CommCtl *ctl)
{
    __shared__ uint32_t s_multi;
    if (threadIdx.x == 0) s_multi = 0u;
    __syncthreads();
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    bool multi = false;
    if (t < n) {
        const uint32_t v = (uint32_t)(uk[t] >> 32);
        if (t == 0 || (uint32_t)(uk[t - 1] >> 32) != v) {
            uint32_t lo = t + 1, hi = n;
            while (lo < hi) {                 // first position behind t whose vertex is not v
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if ((uint32_t)(uk[mid] >> 32) == v) lo = mid + 1; else hi = mid;
            }
            n_comm[v] = (int32_t)(lo - t);
            multi = lo - t > 1;
        }
    }
    const unsigned long long b = __ballot(multi);
    if ((threadIdx.x & (kWave - 1)) == 0 && b) atomicAdd(&s_multi, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && s_multi) atomicAdd(&ctl->n_multi, s_multi);
}

} // namespace

// k is checked and resolved by the caller (api.cpp): >= 2
int communities_run(komb_ctx *ctx, int32_t k)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne;
    ctx->comm = {};                                  // a run that fails leaves no result (include/komb_accel.h)
    komb_ctx::Communities res;                       // goes back to the pool unless it is installed
    res.k = k;
    if (m <= 0) { res.done = true; ctx->comm = std::move(res); return KOMB_OK; }
    KOMB_TRY(truss_edges_canonical(ctx));            // (a whole-graph result whose endpoints no fetch has asked for yet)

    Range r_all("komb_truss_communities_run");
    KOMB_HIP(ctx, ctx->pool.get((void **)res.label.slot(&ctx->pool), (size_t)m * sizeof(int32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.size.slot(&ctx->pool), (size_t)m * sizeof(int32_t)));
    DevBufs bufs(ctx);
    CommCtl *d_ctl = nullptr;
    uint32_t *d_flag = nullptr, *d_pos = nullptr, *d_rs = nullptr, *d_re = nullptr;
    int32_t *d_kept = nullptr, *d_mu = nullptr, *d_mv = nullptr, *d_parent = nullptr, *d_heavy = nullptr;
    const uint32_t heavy_cap = (uint32_t)m;          // every member edge could be queued
    KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
    KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)m + 1));      // membership for the scan; then cnt[] (members per root)
    KOMB_HIP(ctx, bufs.alloc(&d_pos, (size_t)m + 1));
    KOMB_HIP(ctx, bufs.alloc(&d_kept, (size_t)m));
    KOMB_HIP(ctx, bufs.alloc(&d_mu, (size_t)m));
    KOMB_HIP(ctx, bufs.alloc(&d_mv, (size_t)m));
    KOMB_HIP(ctx, bufs.alloc(&d_parent, (size_t)m));
    KOMB_HIP(ctx, bufs.alloc(&d_heavy, (size_t)heavy_cap));
    const uint32_t n_short = ctx_opt_u32(ctx, "COMM_SHORT", kCommShort);    // (tests: every edge through the wave / the queued path)
    uint32_t n_heavy = ctx_opt_u32(ctx, "COMM_HEAVY", kCommHeavy);
    if (n_heavy <= n_short) n_heavy = n_short + 1;

    const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *truss = ctx->d_t_truss;
    const uint32_t *d_nm = d_pos + m;                // the number of members, on the device
    uint32_t *d_cnt = d_flag;
    const int grid = tiles_of(m);
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(CommCtl), s));
    KOMB_TRY(prim_flag_ge_scan(ctx, truss, m, k, d_flag, d_pos));
    k_comm_compact<<<grid, kBlock, 0, s>>>(eu, ev, truss, (uint32_t)m, k, d_pos, d_kept, d_mu, d_mv, d_parent, d_cnt);
    KOMB_TRY(oriented_rows(ctx, bufs, d_mu, m, d_nm, &d_rs, &d_re));
    k_comm_tri<<<grid, kBlock, 0, s>>>(d_mu, d_mv, d_rs, d_re, d_nm, d_parent, d_ctl, d_heavy, heavy_cap, n_short, n_heavy);
    k_comm_heavy<<<dim3(kCommHeavyGrid, kCommHeavyChunks), kBlock, 0, s>>>(d_mu, d_mv, d_rs, d_re, d_parent, d_ctl, d_heavy, heavy_cap);
    // two passes: the first compresses, the second labels -- read-only walks of a step or two
    k_comm_flatten<false><<<grid, kBlock, 0, s>>>(d_nm, d_parent);
    k_comm_flatten<true><<<grid, kBlock, 0, s>>>(d_nm, d_parent);
    class_count(ctx, m, d_nm, d_parent, d_cnt);
    k_comm_finish<<<class_tail_grid(m), kBlock, 0, s>>>((uint32_t)m, truss, k, d_pos, d_parent, d_kept, d_cnt, res.label, res.size, d_ctl);
    const double ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    CommCtl h;
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(CommCtl)));
    res.members = (int64_t)h.n_members; res.count = (int64_t)h.n_communities; res.largest = (int64_t)h.largest;
    res.ms = ms;
    res.done = true;
    ctx->comm = std::move(res);
    return KOMB_OK;
}

// n_comm[nv] and the number of vertices in more than one community, made by the first fetch_vertices / info after a run
int communities_vertices(komb_ctx *ctx)
{
    if (ctx->comm.v_ready) return KOMB_OK;
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne, nv = ctx->nv, nm = ctx->comm.members;
    if (!ctx->comm.ncomm) KOMB_HIP(ctx, ctx->pool.get((void **)ctx->comm.ncomm.slot(&ctx->pool), (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t)));
    ctx->comm.multi = 0;
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(ctx->comm.ncomm, 0, (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t), s));
    if (nm > 0) {
        Range r_all("komb_truss_communities: vertices");
        DevBufs bufs(ctx);
        CommCtl *d_ctl = nullptr;
        uint32_t *d_flag = nullptr, *d_pos = nullptr;
        uint64_t *d_keys = nullptr, *d_tmp = nullptr, *sorted = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)m + 1));
        KOMB_HIP(ctx, bufs.alloc(&d_pos, (size_t)m + 1));
        KOMB_HIP(ctx, bufs.alloc(&d_keys, 2 * (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&d_tmp, 2 * (size_t)nm));
        KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(CommCtl), s));
        k_comm_vflag<<<tiles_of(m + 1), kBlock, 0, s>>>(ctx->comm.label, (uint32_t)m, d_flag);
        KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_pos, m + 1));
        k_comm_keys<<<tiles_of(m), kBlock, 0, s>>>(ctx->d_t_eu, ctx->d_t_ev, ctx->comm.label, (uint32_t)m, d_pos, d_keys);
        int vb = 1;
        while (vb < 31 && (1ll << vb) < nv) ++vb;
        KOMB_TRY(prim_sort_u64(ctx, d_keys, d_tmp, 2 * nm, 32 + vb, &sorted));
        uint64_t *uniq = sorted == d_keys ? d_tmp : d_keys;
        int64_t n_u = 0;
        KOMB_TRY(prim_unique_u64(ctx, sorted, uniq, 2 * nm, &n_u));
        k_comm_runs<<<tiles_of(n_u), kBlock, 0, s>>>(uniq, (uint32_t)n_u, ctx->comm.ncomm, d_ctl);
        KOMB_HIP(ctx, hipGetLastError());
        CommCtl h;
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(CommCtl)));
        ctx->comm.multi = (int64_t)h.n_multi;
    }
    ctx->comm.ms_vertices = ctx->timer.stop(s);
    ctx->comm.v_ready = true;
    return KOMB_OK;
}

} // namespace komb
