// nucleus_hierarchy.hip -- the (3,4)-nuclei as connected classes and their nesting forest over all k
// (komb_nucleus_hierarchy_run): which k-nucleus lies inside which (k-1)-nucleus.  DESIGN.md section 4.6i; the definition is
// in include/komb_accel.h.
//
// The forest builder (forest.hip; its header comment has CLAIM, ADOPT, the tail and why they are right) one rung above
// community_hierarchy.hip.  What is this file's: the ITEMS are the triangles of the stored nucleus result (ids in ascending
// (a, b, c) order: the root of a tree is its rep), bucketed by their own theta; the LINKS are 4-clique records of weight
// w = the smallest theta of the clique's four triangles -- the level at which the clique starts to bind.  komb_nucleus_run
// drops its clique records with its scratch, so the cliques are enumerated ONCE more here, by nucleus.hip's search
// (oriented_search_dev.h: the shortest of three tails walked, the other two bisected, the ids of the other three triangles by
// bisection in c[] through a rebuilt tri_ptr), into a record stream whose length the stored result gives exactly
// (n_cliques4): there is no counting pass, a wave takes its slots with one returning atomic, and a cursor that does not end
// on n_cliques4 fails the run.  The stream is sorted by w (a sort of (w, slot) pairs; LINK reads its records through the
// sorted slots), the bucket boundaries are read by the host once, and the loop behind them reads nothing back.  LINK
// (k_nh_link) is one lane per record of the level: (t0, t1), (t0, t2), (t0, t3); the hooks go to the log, slots taken per WAVE.
//
// Why every node has a hooked triangle: a triangle of theta = k lies in at least k cliques whose other triangles all have
// theta >= k, records of weight exactly k; it was alone before, so the tree it ends the level in holds a triangle hooked at
// this level.  The levels run from theta_max down to 1.
// Every device loop runs over a row part or a length fixed before its launch; the labels are read by a later store-free launch
// (the header comment of components.hip says why).
#include "forest_dev.h"
#include "oriented_search_dev.h"

namespace komb {

namespace {

constexpr uint32_t kNhShort = 16;           // walked tail up to this long: the triangle's own lane (option NUC_SHORT, as in nucleus.hip)

struct NhCtl {                              // 64 bytes, zeroed before every run
    ForestCtl f;
    uint32_t rec_n;                         // clique records written so far
    uint32_t n_members;                     // triangles with theta >= 1
    uint32_t bad;                           // a position or a triangle id that a bisection did not find (cannot happen; checked)
    uint32_t pad[9];
};
static_assert(sizeof(NhCtl) == 64 && offsetof(NhCtl, f) == 0, "NhCtl layout");

struct NhStream { uint32_t *keys, *idx; uint4 *recs; uint32_t cap; };  // record slot q: weight | q | the four triangle ids

// ---- the search structures of nucleus.hip, rebuilt from the stored a, b, c and the canonical edge list

// per triangle: the positions of its edges (three bisections), its membership flag for the scan (flag[n_tri] = 0), and its
// union-find words -- a class of its own that stands for no node yet.  A triangle whose edges are not found takes no part
// in the search (j = kNucNone) and fails the run.
__global__ void k_nh_tri(uint32_t n_tri, uint32_t nv, NucTri o, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                         const uint32_t *__restrict__ re, const int32_t *__restrict__ theta, uint32_t *__restrict__ flag,
                         int32_t *__restrict__ parent, uint32_t *__restrict__ cnt, int32_t *__restrict__ cur, int32_t *__restrict__ claimk, NhCtl *ctl)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t > n_tri) return;
    if (t == n_tri) { flag[t] = 0u; return; }
    const int32_t a = o.a[t], b = o.b[t], c = o.c[t];
    uint32_t j = kNucNone, pac = kNucNone, pbc = kNucNone;
    if ((uint32_t)a < nv && (uint32_t)b < nv && (uint32_t)c < nv) {
        j = nuc_find(ev, b, rs[a], re[a]);
        if (j != kNucNone) pac = nuc_find(ev, c, j + 1, re[a]);
        pbc = nuc_find(ev, c, rs[b], re[b]);
    }
    if (j == kNucNone || pac == kNucNone || pbc == kNucNone) { j = pac = pbc = kNucNone; ctl->bad = 1u; }
    o.j[t] = j; o.pac[t] = pac; o.pbc[t] = pbc;
    flag[t] = theta[t] >= 1 ? 1u : 0u;
    parent[t] = (int32_t)t; cnt[t] = 0u;
    cur[t] = -1;                             // the node this triangle stands for as a root (the latest)
    claimk[t] = 0x7FFFFFFF;                  // the level that node was made at
}

// tri_ptr[e] = the first triangle whose edge (a, b) is at position >= e, for e = 0 .. m: triangle order is (position of
// (a, b), c) order, so the triangles of edge e are [tri_ptr[e], tri_ptr[e + 1]), their c ascending
__global__ void k_nh_tri_ptr(uint32_t m, uint32_t n_tri, const uint32_t *__restrict__ tj, uint32_t *__restrict__ tri_ptr)
{
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e > m) return;
    uint32_t lo = 0, hi = n_tri;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tj[mid] < e) lo = mid + 1; else hi = mid;
    }
    tri_ptr[e] = lo;
}

// the hits of a wave: one record each, triangle t and the three triangles its vertices make with d = ev[x], of weight
// min(theta); the slots are taken once per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void nh_emit(bool hit, uint32_t t, uint32_t x, const int32_t *__restrict__ ev, const NucTri &o,
                                        const uint32_t *__restrict__ tri_ptr, const int32_t *__restrict__ theta, NhCtl *ctl, const NhStream &st)
{
    const unsigned long long m = __ballot(hit);
    if (!m) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int lead = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(&ctl->rec_n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int32_t)base, lead);
    if (!hit) return;
    const uint32_t slot = base + (uint32_t)__popcll(m & nuc_below(lane));
    if (slot >= st.cap) return;              // (cannot happen: the stored result counted every clique; the host checks rec_n)
    const int32_t d = ev[x];
    uint4 r;
    r.x = t;
    r.y = tri_id(tri_ptr, o.c, o.j[t], d, t, &ctl->bad);        // (a, b, d)
    r.z = tri_id(tri_ptr, o.c, o.pac[t], d, t, &ctl->bad);      // (a, c, d)
    r.w = tri_id(tri_ptr, o.c, o.pbc[t], d, t, &ctl->bad);      // (b, c, d)
    const int32_t w0 = theta[r.x], w1 = theta[r.y], w2 = theta[r.z], w3 = theta[r.w];
    const int32_t wa = w0 < w1 ? w0 : w1, wb = w2 < w3 ? w2 : w3;
    st.keys[slot] = (uint32_t)(wa < wb ? wa : wb);           // (a weight outside 1 .. theta_max shows in the level table; the host checks it)
    st.idx[slot] = slot;
    st.recs[slot] = r;
}

// The 4-clique pass of nucleus.hip writing records: one lane per triangle; a walked tail above n_short goes through the
// triangle's wave.  The own-lane walk runs to the longest tail of the wave, so that nh_emit's ballots see every lane.
__global__ void k_nh_clq(const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs, const uint32_t *__restrict__ re, NucTri o,
                         uint32_t n_tri, const uint32_t *__restrict__ tri_ptr, const int32_t *__restrict__ theta,
                         const uint32_t *__restrict__ n_mem, NhCtl *ctl, uint32_t n_short, NhStream st)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    NucTails s{0, 0, 0, 0, 0, 0};
    if (t < n_tri && o.j[t] != kNucNone) s = nuc_tails(o, rs, re, t);
    const bool act = s.n > 0, mid = act && s.n > n_short;
    const uint32_t own = act && !mid ? s.n : 0u;
    const uint32_t top = wave_max(own);
    for (uint32_t i = 0; i < top; ++i) {
        const bool hit = i < own && nuc_clq_entry(ev, s, s.it + i);
        nh_emit(hit, t, s.it + i, ev, o, tri_ptr, theta, ctl, st);
    }
    wave_turns(mid, [&](int src) {
        const uint32_t rt = from_lane(t, src);
        const NucTails r = from_lane(s, src);
        wave_walk_all(r.it, r.n, lane, [&](uint32_t x, bool in) { nh_emit(in && nuc_clq_entry(ev, r, x), rt, x, ev, o, tri_ptr, theta, ctl, st); });
    });
    if (t == 0) ctl->n_members = *n_mem;
}

// ---- members: the triangles with theta >= 1, for the sort by theta
__global__ void k_nh_compact(uint32_t n_tri, const int32_t *__restrict__ theta, uint32_t levels, const uint32_t *__restrict__ pos,
                             uint32_t cap, uint32_t *__restrict__ mkeys, uint32_t *__restrict__ mvals)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri || theta[t] < 1) return;
    const uint32_t j = pos[t];
    if (j >= cap) return;                    // (cannot happen: cap is the scan's total)
    mkeys[j] = (uint32_t)theta[t] < levels ? (uint32_t)theta[t] : levels - 1u;       // (levels > the largest theta)
    mvals[j] = t;
}

// ---- the levels: LINK

// LINK: one lane per record of the level (the slots order[r_b .. r_b + r_n)); three links, each hook logged
__global__ void k_nh_link(const uint4 *__restrict__ recs, const uint32_t *__restrict__ order, uint32_t r_b, uint32_t r_n, uint32_t n_rec,
                          uint32_t n_tri, int32_t *parent, NhCtl *ctl, int32_t *__restrict__ log, uint32_t cap)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    int32_t h0 = -1, h1 = -1, h2 = -1;
    if (i < r_n) {
        const uint32_t q = order[r_b + i];
        if (q < n_rec) {
            const uint4 r = recs[q];
            if (r.x < n_tri && r.y < n_tri && r.z < n_tri && r.w < n_tri) {
                h0 = comp_link_hooked(parent, (int32_t)r.x, (int32_t)r.y);
                h1 = comp_link_hooked(parent, (int32_t)r.x, (int32_t)r.z);
                h2 = comp_link_hooked(parent, (int32_t)r.x, (int32_t)r.w);
            }
        }
    }
    forest_log_wave(h0, &ctl->f, log, cap); forest_log_wave(h1, &ctl->f, log, cap); forest_log_wave(h2, &ctl->f, log, cap);
}

// node[] in triangle order
__global__ void k_nh_tri_out(uint32_t n_tri, const int32_t *__restrict__ theta, const int32_t *__restrict__ mnode,
                             const int32_t *__restrict__ rank, uint32_t n, int32_t *__restrict__ out)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri) return;
    int32_t nd = -1;
    if (theta[t] >= 1) {
        const int32_t made = mnode[t];
        if (made >= 0 && (uint32_t)made < n) nd = rank[made];
    }
    out[t] = nd;
}

// ---- readers of the stored forest

// komb_nucleus_hierarchy_labels: from node[t] up while the parent's level is still >= k
__global__ void k_nh_labels(uint32_t n_tri, int32_t k, const int32_t *__restrict__ tnode, uint32_t n, const int32_t *__restrict__ nk,
                            const int32_t *__restrict__ rep, const int32_t *__restrict__ par, const int32_t *__restrict__ size,
                            int32_t *__restrict__ label, int32_t *__restrict__ lsize)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri) return;
    int32_t lab = -1, sz = 0;
    int32_t c = tnode[t];
    if (c >= 0 && (uint32_t)c < n && nk[c] >= k) {
        c = forest_walk_up(c, k, nk, par);
        lab = rep[c]; sz = size[c];
    }
    label[t] = lab; lsize[t] = sz;
}

// flag[t] = triangle t is the rep of its k-nucleus (flag[n_tri] = 0: the scan's last entry is the number of nuclei)
__global__ void k_nh_rep_flag(uint32_t n_tri, const int32_t *__restrict__ label, uint32_t *__restrict__ flag)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t > n_tri) return;
    flag[t] = t < n_tri && label[t] == (int32_t)t ? 1u : 0u;
}

// the position of (u, v) in the canonical edge list (sorted by (eu, ev))
__device__ __forceinline__ uint32_t nh_edge_pos(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, uint32_t m, int32_t u, int32_t v)
{
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const int32_t mu = eu[mid];
        if (mu < u || (mu == u && ev[mid] < v)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// (label << 32 | vertex) and (label << 32 | edge position) of a member triangle's three vertices and three edges; all ones
// for a triangle outside every k-nucleus (sorted behind every real key)
__global__ void k_nh_keys(uint32_t n_tri, const int32_t *__restrict__ label, const int32_t *__restrict__ ta, const int32_t *__restrict__ tb,
                          const int32_t *__restrict__ tc, const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, uint32_t m,
                          uint64_t *__restrict__ vkeys, uint64_t *__restrict__ ekeys)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri) return;
    const size_t at = 3 * (size_t)t;
    const int32_t lab = label[t];
    if (lab < 0) {
        for (int i = 0; i < 3; ++i) { vkeys[at + i] = ~0ull; ekeys[at + i] = ~0ull; }
        return;
    }
    const uint64_t hi = (uint64_t)(uint32_t)lab << 32;
    const int32_t a = ta[t], b = tb[t], c = tc[t];
    vkeys[at] = hi | (uint32_t)a; vkeys[at + 1] = hi | (uint32_t)b; vkeys[at + 2] = hi | (uint32_t)c;
    ekeys[at] = hi | nh_edge_pos(eu, ev, m, a, b); ekeys[at + 1] = hi | nh_edge_pos(eu, ev, m, a, c); ekeys[at + 2] = hi | nh_edge_pos(eu, ev, m, b, c);
}

// the distinct keys of [lo, hi) in a sorted list of distinct keys: two bisections
__device__ __forceinline__ uint32_t nh_range(const uint64_t *__restrict__ keys, uint32_t n, uint64_t lo_key, uint64_t hi_key)
{
    uint32_t b[2];
    const uint64_t want[2] = {lo_key, hi_key};
    for (int i = 0; i < 2; ++i) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < want[i]) lo = mid + 1; else hi = mid;
        }
        b[i] = lo;
    }
    return b[1] - b[0];
}

// one row per k-nucleus, in ascending rep order (the scan's order): rep, triangles, distinct edges, distinct vertices
__global__ void k_nh_nuclei_out(uint32_t n_tri, const int32_t *__restrict__ label, const int32_t *__restrict__ lsize, const uint32_t *__restrict__ pos,
                                uint32_t n_nuc, const uint64_t *__restrict__ vuniq, uint32_t n_v, const uint64_t *__restrict__ euniq, uint32_t n_e,
                                int32_t *__restrict__ rep, int32_t *__restrict__ ntri, int32_t *__restrict__ nedge, int32_t *__restrict__ nvert)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri || label[t] != (int32_t)t) return;
    const uint32_t i = pos[t];
    if (i >= n_nuc) return;                  // (cannot happen: n_nuc is the scan's total)
    const uint64_t lo = (uint64_t)t << 32, hi = ((uint64_t)t + 1) << 32;
    rep[i] = (int32_t)t; ntri[i] = lsize[t];
    nvert[i] = (int32_t)nh_range(vuniq, n_v, lo, hi);
    nedge[i] = (int32_t)nh_range(euniq, n_e, lo, hi);
}

// label[] / size[] of threshold k on the device (k resolved by the caller: >= 1)
int nh_labels_dev(komb_ctx *ctx, int32_t k, int32_t *d_label, int32_t *d_size)
{
    const int64_t T = ctx->nuc.n_tri;
    const int32_t *nodes = ctx->nh.nodes;
    const size_t c = (size_t)ctx->nh.cap;
    k_nh_labels<<<tiles_of(T), kBlock, 0, ctx->stream>>>((uint32_t)T, k, ctx->nh.tnode, (uint32_t)ctx->nh.n_nodes, nodes, nodes + c, nodes + 2 * c,
                                                        nodes + 3 * c, d_label, d_size);
    KOMB_HIP(ctx, hipGetLastError());
    return KOMB_OK;
}

} // namespace

// the nucleus result it needs is checked by the caller (api.cpp).  The result is built in blocks of its own and replaces the
// previous one only when the run has succeeded.
int nucleus_hierarchy_run(komb_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    const int64_t T = ctx->nuc.n_tri, Q = ctx->nuc.n_clq;

    Range r_all("komb_nucleus_hierarchy_run");
    komb_ctx::NucleusHierarchy res;                              // the new result: goes back to the pool unless it is installed
    res.theta_max = ctx->nuc.theta_max;
    size_t cap_nodes = 1;
    KOMB_HIP(ctx, ctx->pool.get((void **)res.tnode.slot(&ctx->pool), (size_t)(T > 0 ? T : 1) * sizeof(int32_t)));

    ctx->timer.start(s);
    if (Q > 0) {
        if (T < 1 || m < 1 || res.theta_max < 1)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_run: inconsistent nucleus result (%lld cliques, %lld triangles, %lld edges, theta_max %d)",
                      (long long)Q, (long long)T, (long long)m, res.theta_max);
        DevBufs bufs(ctx);
        const uint32_t um = (uint32_t)m, uT = (uint32_t)T, uQ = (uint32_t)Q;
        const uint32_t levels = (uint32_t)res.theta_max + 1u;    // level numbers 0 .. levels - 1
        const int bits = forest_bits(levels);
        const uint32_t n_short = ctx_opt_u32(ctx, "NUC_SHORT", kNhShort);      // (tests: every triangle through the wave / its lane)
        const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *theta = ctx->nuc.theta;

        NhCtl *d_ctl = nullptr;
        uint32_t *d_rs = nullptr, *d_re = nullptr, *tri_ptr = nullptr, *d_flag = nullptr, *d_pos = nullptr, *cnt = nullptr, *rkeys2 = nullptr, *ridx2 = nullptr;
        int32_t *parent = nullptr, *cur = nullptr, *claimk = nullptr, *mnode = nullptr;
        NucTri o{ctx->nuc.a, ctx->nuc.b, ctx->nuc.c, nullptr, nullptr, nullptr};
        NhStream st{nullptr, nullptr, nullptr, uQ};
        KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&tri_ptr, (size_t)m + 1));
        KOMB_HIP(ctx, bufs.alloc(&o.j, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&o.pac, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&o.pbc, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)T + 1));
        KOMB_HIP(ctx, bufs.alloc(&d_pos, (size_t)T + 1));
        KOMB_HIP(ctx, bufs.alloc(&cnt, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&parent, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&cur, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&claimk, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&mnode, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&st.keys, (size_t)Q));
        KOMB_HIP(ctx, bufs.alloc(&rkeys2, (size_t)Q));
        KOMB_HIP(ctx, bufs.alloc(&st.idx, (size_t)Q));
        KOMB_HIP(ctx, bufs.alloc(&ridx2, (size_t)Q));
        KOMB_HIP(ctx, bufs.alloc(&st.recs, (size_t)Q));

        // ---- the search structures, the members' flags, and the one clique enumeration
        const uint32_t *d_nm = d_pos + T;                        // the number of members, on the device
        KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(NhCtl), s));
        KOMB_TRY(oriented_rows(ctx, bufs, eu, m, nullptr, &d_rs, &d_re));
        k_nh_tri<<<tiles_of(T + 1), kBlock, 0, s>>>(uT, (uint32_t)nv, o, ev, d_rs, d_re, theta, d_flag, parent, cnt, cur, claimk, d_ctl);
        k_nh_tri_ptr<<<tiles_of(m + 1), kBlock, 0, s>>>(um, uT, o.j, tri_ptr);
        KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_pos, T + 1));
        k_nh_clq<<<tiles_of(T), kBlock, 0, s>>>(ev, d_rs, d_re, o, uT, tri_ptr, theta, d_nm, d_ctl, n_short, st);
        KOMB_HIP(ctx, hipGetLastError());
        NhCtl h;
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NhCtl)));       // the cursor, read once: it ends on the stored count or the run fails
        const uint32_t nm = h.n_members;
        if (h.bad || h.rec_n != uQ || nm < 1 || (int64_t)nm > T)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_run: the clique pass is inconsistent (%u of %u records, %u members of %lld triangles, bad %u)",
                      h.rec_n, uQ, nm, (long long)T, h.bad);

        // ---- buckets: records by weight, members by theta; one table for the host
        uint32_t *mkeys = nullptr, *mkeys2 = nullptr, *mvals = nullptr, *mvals2 = nullptr, *d_tab = nullptr, *seg = nullptr;
        int32_t *log = nullptr;
        ForestNodes t{};
        KOMB_HIP(ctx, bufs.alloc(&mkeys, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&mkeys2, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&mvals, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&mvals2, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&log, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&t.k, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&t.rep, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&t.par, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&t.size, (size_t)nm));
        KOMB_HIP(ctx, bufs.alloc(&t.shell, (size_t)nm));
        // the level table the host reads once: moff[levels + 1] (members by theta) | roff[levels + 1] (records by weight)
        const size_t tab_words = 2 * ((size_t)levels + 1);
        KOMB_HIP(ctx, bufs.alloc(&d_tab, tab_words));
        uint32_t *d_moff = d_tab, *d_roff = d_tab + levels + 1;
        KOMB_HIP(ctx, hipMemsetAsync(d_tab, 0, tab_words * sizeof(uint32_t), s));
        k_nh_compact<<<tiles_of(T), kBlock, 0, s>>>(uT, theta, levels, d_pos, nm, mkeys, mvals);
        uint32_t *rsorted = nullptr, *order = nullptr, *msorted = nullptr, *mord = nullptr;
        KOMB_TRY(prim_sort_pairs_u32_u32(ctx, st.keys, rkeys2, st.idx, ridx2, Q, bits, &rsorted, &order));
        forest_offsets(ctx, uQ, rsorted, levels, d_roff);
        KOMB_TRY(prim_sort_pairs_u32_u32(ctx, mkeys, mkeys2, mvals, mvals2, nm, bits, &msorted, &mord));
        forest_offsets(ctx, nm, msorted, levels, d_moff);
        KOMB_HIP(ctx, hipGetLastError());
        std::vector<uint32_t> tab(tab_words);
        KOMB_HIP(ctx, d2h(ctx, tab.data(), d_tab, tab_words * sizeof(uint32_t)));     // the one read before the loop
        const uint32_t *moff = tab.data(), *roff = tab.data() + levels + 1;
        bool ascending = true;                                                      // (they size the loop's launches)
        for (uint32_t k = 0; k < levels; ++k) ascending = ascending && moff[k] <= moff[k + 1] && roff[k] <= roff[k + 1];
        if (!ascending || moff[levels] != nm || roff[levels] != uQ || moff[1] != 0u || roff[1] != 0u)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_run: inconsistent level table (%u of %u members, %u of %u records, %u / %u below level 1)",
                      moff[levels], nm, roff[levels], uQ, moff[1], roff[1]);

        uint32_t n_levels = 0;
        for (int32_t k = (int32_t)levels - 1; k >= 1; --k) n_levels += moff[k + 1] - moff[k] ? 1u : 0u;
        KOMB_HIP(ctx, bufs.alloc(&seg, (size_t)n_levels + 1));                      // seg[i]: where the i-th populated level's hooks start in the log
        KOMB_HIP(ctx, hipMemsetAsync(seg, 0, ((size_t)n_levels + 1) * sizeof(uint32_t), s));

        // ---- the levels, from theta_max down
        const ForestState f{parent, log, claimk, cur, cnt, seg, mnode, t, &d_ctl->f, nm};
        uint32_t li = 0;
        for (int32_t k = (int32_t)levels - 1; k >= 1; --k) {                        // no read and no wait in this loop
            const uint32_t sh_b = moff[k], sh_n = moff[k + 1] - moff[k];
            const uint32_t r_b = roff[k], r_n = roff[k + 1] - roff[k];
            if (!sh_n) continue;                                                    // (a record of weight k has a triangle of theta k)
            if (r_n) k_nh_link<<<tiles_of(r_n), kBlock, 0, s>>>(st.recs, order, r_b, r_n, uQ, uT, parent, d_ctl, log, nm);
            forest_level(ctx, f, k, li, false, mord, sh_b, sh_n, 3ull * r_n < nm ? 3ull * r_n : nm);      // at most this many hooks at this level
            ++li;
        }
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NhCtl)));                          // the number of nodes sizes the tail
        if (h.f.n_nodes < 1 || h.f.n_nodes > nm || h.f.log_n > nm || h.bad)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_run: inconsistent state (%u nodes, %u hooks, %u members, bad %u)",
                      h.f.n_nodes, h.f.log_n, nm, h.bad);

        // ---- the tail
        const uint32_t n = h.f.n_nodes;
        int32_t *rank = cur;                                     // (cur[] has served when the ranks are made; nodes <= members <= triangles)
        cap_nodes = n;
        KOMB_HIP(ctx, ctx->pool.get((void **)res.nodes.slot(&ctx->pool), 5 * cap_nodes * sizeof(int32_t)));
        ForestNodes out{res.nodes, res.nodes + cap_nodes, res.nodes + 2 * cap_nodes,
                        (uint32_t *)res.nodes.get() + 3 * cap_nodes, (uint32_t *)res.nodes.get() + 4 * cap_nodes};
        KOMB_TRY(forest_tail(ctx, bufs, f, n, bits, out, rank, nullptr, mvals, mvals2));   // (the members' sort has served: n <= nm)
        k_nh_tri_out<<<tiles_of(T), kBlock, 0, s>>>(uT, theta, mnode, rank, n, res.tnode);
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NhCtl)));
        res.n_nodes = (int64_t)n; res.n_roots = (int64_t)h.f.n_roots; res.depth = h.f.depth; res.n_members = (int64_t)nm;
    } else {
        if (T > 0) KOMB_HIP(ctx, hipMemsetAsync(res.tnode, 0xFF, (size_t)T * sizeof(int32_t), s));   // no clique: no nucleus
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
    }
    if (!res.nodes) KOMB_HIP(ctx, ctx->pool.get((void **)res.nodes.slot(&ctx->pool), 5 * cap_nodes * sizeof(int32_t)));
    res.cap = (int64_t)cap_nodes;

    res.done = true;
    ctx->nh = std::move(res);
    return KOMB_OK;
}

// k is checked and resolved by the caller (api.cpp): >= 1.  One walk per triangle over the stored forest.
int nucleus_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label, int32_t *size)
{
    const int64_t T = ctx->nuc.n_tri;
    if (T == 0 || (!label && !size)) return KOMB_OK;
    DevBufs bufs(ctx);
    int32_t *d_label = nullptr, *d_size = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_label, (size_t)T));
    KOMB_HIP(ctx, bufs.alloc(&d_size, (size_t)T));
    KOMB_TRY(nh_labels_dev(ctx, k, d_label, d_size));
    KOMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (label) KOMB_HIP(ctx, staged_copy(ctx, label, d_label, (size_t)T * sizeof(int32_t), false));
    if (size) KOMB_HIP(ctx, staged_copy(ctx, size, d_size, (size_t)T * sizeof(int32_t), false));
    return KOMB_OK;
}

// k is checked and resolved by the caller (api.cpp): >= 1.  The k-nuclei as subgraphs: per nucleus, in ascending rep order,
// its triangles, its distinct canonical edges and its distinct vertices (the distinct (label, vertex) and (label, edge
// position) keys, counted between the boundaries of each label).
int nucleus_hierarchy_nuclei(komb_ctx *ctx, int32_t k, int64_t cap, int64_t *n_nuclei, int32_t *rep, int32_t *n_triangles,
                             int32_t *n_edges, int32_t *n_vertices)
{
    hipStream_t s = ctx->stream;
    const int64_t T = ctx->nuc.n_tri, m = ctx->t_ne > 0 ? ctx->t_ne : 0;
    const bool want = rep || n_triangles || n_edges || n_vertices;
    int64_t n_nuc = 0;
    DevBufs bufs(ctx);
    int32_t *d_label = nullptr, *d_size = nullptr;
    uint32_t *d_flag = nullptr, *d_pos = nullptr;
    if (T > 0 && ctx->nh.n_nodes > 0) {
        KOMB_HIP(ctx, bufs.alloc(&d_label, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&d_size, (size_t)T));
        KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)T + 1));
        KOMB_HIP(ctx, bufs.alloc(&d_pos, (size_t)T + 1));
        KOMB_TRY(nh_labels_dev(ctx, k, d_label, d_size));
        k_nh_rep_flag<<<tiles_of(T + 1), kBlock, 0, s>>>((uint32_t)T, d_label, d_flag);
        KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_pos, T + 1));
        KOMB_HIP(ctx, hipGetLastError());
        uint32_t total = 0;
        KOMB_HIP(ctx, d2h(ctx, &total, d_pos + T, sizeof(uint32_t)));
        n_nuc = (int64_t)total;
    }
    if (want && cap < n_nuc)
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_nucleus_hierarchy_nuclei: room for %lld nuclei, the level has %lld", (long long)cap, (long long)n_nuc);
    if (want && n_nuc > 0) {
        const size_t n_keys = 3 * (size_t)T;
        if (n_keys > 0xFFFFFFFFull)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_nucleus_hierarchy_nuclei: %lld triangles: three keys each do not fit 32-bit indexing", (long long)T);
        uint64_t *vkeys = nullptr, *ekeys = nullptr, *tmp = nullptr, *vuniq = nullptr, *euniq = nullptr, *sorted = nullptr;
        int32_t *d_out = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&vkeys, n_keys));
        KOMB_HIP(ctx, bufs.alloc(&ekeys, n_keys));
        KOMB_HIP(ctx, bufs.alloc(&tmp, n_keys));
        KOMB_HIP(ctx, bufs.alloc(&vuniq, n_keys));
        KOMB_HIP(ctx, bufs.alloc(&euniq, n_keys));
        KOMB_HIP(ctx, bufs.alloc(&d_out, 4 * (size_t)n_nuc));
        k_nh_keys<<<tiles_of(T), kBlock, 0, s>>>((uint32_t)T, d_label, ctx->nuc.a, ctx->nuc.b, ctx->nuc.c, ctx->d_t_eu, ctx->d_t_ev,
                                                (uint32_t)m, vkeys, ekeys);
        KOMB_HIP(ctx, hipGetLastError());
        int64_t n_v = 0, n_e = 0;
        KOMB_TRY(prim_sort_u64(ctx, vkeys, tmp, (int64_t)n_keys, 64, &sorted));
        KOMB_TRY(prim_unique_u64(ctx, sorted, vuniq, (int64_t)n_keys, &n_v));
        KOMB_TRY(prim_sort_u64(ctx, ekeys, tmp, (int64_t)n_keys, 64, &sorted));
        KOMB_TRY(prim_unique_u64(ctx, sorted, euniq, (int64_t)n_keys, &n_e));
        if (n_v < 0 || n_e < 0 || (size_t)n_v > n_keys || (size_t)n_e > n_keys)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_nuclei: inconsistent key counts (%lld vertices, %lld edges of %zu keys)",
                      (long long)n_v, (long long)n_e, n_keys);
        int32_t *o_rep = d_out, *o_tri = d_out + n_nuc, *o_edge = d_out + 2 * n_nuc, *o_vert = d_out + 3 * n_nuc;
        k_nh_nuclei_out<<<tiles_of(T), kBlock, 0, s>>>((uint32_t)T, d_label, d_size, d_pos, (uint32_t)n_nuc, vuniq, (uint32_t)n_v, euniq, (uint32_t)n_e,
                                                      o_rep, o_tri, o_edge, o_vert);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, hipStreamSynchronize(s));
        const size_t bytes = (size_t)n_nuc * sizeof(int32_t);
        if (rep) KOMB_HIP(ctx, staged_copy(ctx, rep, o_rep, bytes, false));
        if (n_triangles) KOMB_HIP(ctx, staged_copy(ctx, n_triangles, o_tri, bytes, false));
        if (n_edges) KOMB_HIP(ctx, staged_copy(ctx, n_edges, o_edge, bytes, false));
        if (n_vertices) KOMB_HIP(ctx, staged_copy(ctx, n_vertices, o_vert, bytes, false));
    }
    if (n_nuclei) *n_nuclei = n_nuc;
    return KOMB_OK;
}

} // namespace komb
