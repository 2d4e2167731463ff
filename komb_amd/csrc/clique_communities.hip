// clique_communities.hip -- k-clique communities (komb_clique_communities_run): clique percolation over the held list of maximal
// cliques.  The MEMBER cliques are those of at least k vertices, two are ADJACENT when they share at least k - 1 vertices, a
// community is the union of the vertex sets of one connected class.  DESIGN.md section 4.6m.
//
// Adjacent pairs are found without testing all pairs.  A clique j adjacent to a clique i of s vertices misses at most s - k + 1 of
// i's vertices, so it contains at least one of ANY s - k + 2 of them: the PIVOTS of i, its s - k + 2 vertices of smallest
// (load(v), v), load(v) = the member cliques through v.  Every adjacent pair is found from both sides, so only the candidates
// j > i of a pivot's row of the incidence are examined.  pair_tests = the sum over member cliques and their pivots of the row
// entries above the clique: k_pc_pivots computes it, and the start of every pivot's walk, before anything is linked.
// The launches of a run: k_pc_flag, a scan; k_pc_keys (vertex << 32 | clique), the sort, k_pc_rows; k_pc_pivots; k_pc_link;
// k_pc_label (store-free on parent[]), k_pc_sizes, a scan, k_pc_reps; k_pc_ckeys (community << 32 | vertex), the sort, the unique,
// k_pc_comm, k_pc_vfix.  No workgroup waits for another.
//
// k_pc_link: one wavefront per member clique i, handed out in chunks of 64 from one cursor.  The clique's ascending vertices and
// the starts of its pivots' walks are staged in LDS.  A pivot's row above i is walked 64 candidates per trip: one lane per
// candidate reads both roots (comp_find) and drops the candidate when they are equal -- classes only ever merge, so what was one
// class stays one -- the survivors are compacted into LDS by ballot, and groups of g lanes intersect one survivor each with the
// staged clique: the candidate's vertices are loaded g at a time, every lane bisects its vertex in the LDS copy, the hits are
// counted by ballot and popcount, until k - 1 is reached or can no longer be reached.  parent[] is touched by agent-scope atomics
// only (unionfind_dev.h).
#include "common.h"
#include "unionfind_dev.h"

#include <algorithm>

namespace komb {

namespace {

constexpr int kPcGrid = 1024;                         // wavefronts (workgroups of one) of a launch
constexpr long long kPcDefaultBudget = 1ll << 32;     // pair tests
constexpr long long kPcMaxWords = 1ll << 24;          // the list's words at most (MAXIMAL_LIST's limit)
constexpr uint32_t kPcMaxSize = 4098;                 // vertices of a clique at most: a root edge and its 4096 candidates
constexpr uint32_t kPcNone = 0xFFFFFFFFu;             // pstart[] of a vertex that is no pivot

struct PcCtl {                                        // 32 bytes, zeroed before every run
    unsigned long long pair_tests;
    unsigned long long links;                         // pairs found adjacent (PERC_DEBUG; depends on scheduling)
    uint32_t cursor;                                  // next chunk of 64 cliques (zeroed before every launch)
    uint32_t bad;                                     // an inconsistency (cannot happen; checked)
    uint32_t pad[2];
};
static_assert(sizeof(PcCtl) == 32, "PcCtl layout");

struct PcArgs {
    const uint32_t *off;                              // [nc + 1] the list's offsets
    const int32_t *verts;                             // [words]
    const uint32_t *msize;                            // [nc] the vertices of a member clique, 0 for any other
    const uint32_t *rs, *re;                          // [nv] the rows of the incidence
    const int32_t *row;                               // [entries] member cliques through a vertex, ascending
    uint32_t *pstart;                                 // [words] per vertex of a member clique: where its row's walk starts, or kPcNone
    int32_t *parent;                                  // [nc]
    PcCtl *ctl;
    uint32_t nc, n_chunks, k, smax, group;
};

// the clique that holds word w: the largest i with off[i] <= w
__device__ __forceinline__ uint32_t pc_owner(const uint32_t *__restrict__ off, uint32_t nc, uint32_t w)
{
    uint32_t lo = 0, hi = nc;                         // off[lo] <= w < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void k_pc_flag(const uint32_t *__restrict__ off, uint32_t nc, uint32_t k, uint32_t *__restrict__ msize, int32_t *__restrict__ parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc) return;
    const uint32_t s = off[i + 1] - off[i];
    msize[i] = s >= k ? s : 0u;
    parent[i] = (int32_t)i;
}

__global__ void k_pc_keys(const uint32_t *__restrict__ off, const int32_t *__restrict__ verts, const uint32_t *__restrict__ msize,
                          const uint32_t *__restrict__ mpos, uint32_t nc, uint32_t words, uint32_t nv, uint64_t *__restrict__ keys, PcCtl *ctl)
{
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w >= words) return;
    const uint32_t i = pc_owner(off, nc, w);
    if (!msize[i]) return;
    uint32_t v = (uint32_t)verts[w];
    if (v >= nv) { ctl->bad = 1u; v = 0u; }
    keys[mpos[i] + (w - off[i])] = ((uint64_t)v << 32) | i;
}

__global__ void k_pc_rows(const uint64_t *__restrict__ keys, uint32_t n, uint32_t nv, uint32_t nc, int32_t *__restrict__ row, uint32_t *__restrict__ rs,
                          uint32_t *__restrict__ re, PcCtl *ctl)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t v = (uint32_t)(keys[p] >> 32), i = (uint32_t)keys[p];
    if (v >= nv || i >= nc) { ctl->bad = 1u; row[p] = 0; return; }
    row[p] = (int32_t)i;
    if (p == 0 || (uint32_t)(keys[p - 1] >> 32) != v) rs[v] = p;
    if (p + 1 == n || (uint32_t)(keys[p + 1] >> 32) != v) re[v] = p + 1;
}

// The pivots of every member clique and pair_tests.  One wavefront per clique; its keys (load << 32 | vertex) in LDS, the rank of
// each by counting the smaller ones (they are distinct).
__global__ __launch_bounds__(kWave) void k_pc_pivots(PcArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long skey[];
    const int lane = threadIdx.x;
    unsigned long long tests = 0ull;
    for (;;) {
        uint32_t chunk = 0;
        if (lane == 0) chunk = atomicAdd(&A.ctl->cursor, 1u);
        chunk = (uint32_t)__shfl((int32_t)chunk, 0);
        if (chunk >= A.n_chunks) break;
        const uint32_t c = chunk * kWave + (uint32_t)lane;
        unsigned long long todo = __ballot(c < A.nc && A.msize[c] != 0u);
        while (todo) {
            const uint32_t i = chunk * kWave + (uint32_t)(__ffsll((long long)todo) - 1);
            todo &= todo - 1;
            const uint32_t o = A.off[i], s = A.off[i + 1] - o;
            if (s > A.smax) { if (lane == 0) A.ctl->bad = 1u; continue; }
            for (uint32_t t = (uint32_t)lane; t < s; t += kWave) {
                const uint32_t v = (uint32_t)A.verts[o + t];
                skey[t] = ((unsigned long long)(A.re[v] - A.rs[v]) << 32) | v;
            }
            __syncthreads();
            const uint32_t np = s - A.k + 2u;
            for (uint32_t t = (uint32_t)lane; t < s; t += kWave) {
                const unsigned long long mine = skey[t];
                uint32_t rank = 0;
                for (uint32_t x = 0; x < s; ++x) rank += skey[x] < mine ? 1u : 0u;
                uint32_t start = kPcNone;
                if (rank < np) {                        // a pivot: its row holds i; the walk starts behind it
                    const uint32_t v = (uint32_t)mine, end = A.re[v];
                    uint32_t lo = A.rs[v], hi = end;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if ((uint32_t)A.row[mid] < i) lo = mid + 1; else hi = mid;
                    }
                    if (lo >= end || (uint32_t)A.row[lo] != i) { A.ctl->bad = 1u; start = end; }
                    else start = lo + 1u;
                    tests += end - start;
                }
                A.pstart[o + t] = start;
            }
            __syncthreads();                             // (the next clique writes skey again)
        }
    }
    if (tests) atomicAdd(&A.ctl->pair_tests, tests);
}

// One member clique i against the candidates above it in its pivots' rows.  Every branch around a ballot or a barrier is uniform
// over the wave.
__device__ void pc_clique(const PcArgs &A, uint32_t i, int32_t *sv, uint32_t *sp, int32_t *cand, uint32_t &links, int lane)
{
    const uint32_t o = A.off[i], s = A.off[i + 1] - o;
    if (s > A.smax) { if (lane == 0) A.ctl->bad = 1u; return; }
    for (uint32_t t = (uint32_t)lane; t < s; t += kWave) { sv[t] = A.verts[o + t]; sp[t] = A.pstart[o + t]; }
    __syncthreads();
    // a candidate that is adjacent has at least k - 1 vertices, and the cliques around one clique are about its size
    const uint32_t g = A.group ? A.group : (s <= 8u ? 4u : (s <= 32u ? 16u : 64u));
    const uint32_t ng = kWave / g, q = (uint32_t)lane / g, gl = (uint32_t)lane % g;
    const unsigned long long gmask = g == 64u ? ~0ull : (1ull << g) - 1ull;
    const uint32_t need = A.k - 1u;
    for (uint32_t t = 0; t < s; ++t) {
        const uint32_t p0 = sp[t];
        if (p0 == kPcNone) continue;
        const uint32_t end = A.re[(uint32_t)sv[t]];
        for (uint32_t base = p0; base < end; base += kWave) {
            const uint32_t p = base + (uint32_t)lane;
            int32_t j = -1;
            bool live = false;
            if (p < end) {
                j = A.row[p];
                live = comp_find(A.parent, (int32_t)i) != comp_find(A.parent, j);
            }
            const unsigned long long mask = __ballot(live);
            if (!mask) continue;
            const uint32_t n_live = (uint32_t)__popcll(mask);
            if (live) cand[__popcll(mask & ((1ull << lane) - 1ull))] = j;
            __syncthreads();
            for (uint32_t b = 0; b < n_live; b += ng) {
                const bool has = b + q < n_live;
                const int32_t j2 = has ? cand[b + q] : 0;
                const uint32_t oj = has ? A.off[j2] : 0u, sj = has ? A.off[j2 + 1] - oj : 0u;
                uint32_t cnt = 0, done = 0;              // (the same in every lane of a group)
                for (;;) {
                    const bool act = has && cnt < need && cnt + (sj - done) >= need;
                    if (!__ballot(act)) break;
                    bool hit = false;
                    if (act && done + gl < sj) {
                        const int32_t x = A.verts[oj + done + gl];
                        uint32_t lo = 0, hi = s;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (sv[mid] < x) lo = mid + 1; else hi = mid;
                        }
                        hit = lo < s && sv[lo] == x;
                    }
                    const unsigned long long hm = __ballot(hit);
                    if (act) {
                        cnt += (uint32_t)__popcll((hm >> (q * g)) & gmask);
                        done = done + g < sj ? done + g : sj;
                    }
                }
                if (has && gl == 0 && cnt >= need) { comp_link(A.parent, (int32_t)i, j2); ++links; }
            }
            __syncthreads();                             // (the next trip writes cand again)
        }
    }
    __syncthreads();                                     // (the next clique writes sv and sp again)
}

__global__ __launch_bounds__(kWave) void k_pc_link(PcArgs A)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    int32_t *sv = lds;
    uint32_t *sp = (uint32_t *)(lds + A.smax);
    int32_t *cand = lds + 2 * (size_t)A.smax;
    const int lane = threadIdx.x;
    uint32_t links = 0;
    for (;;) {
        uint32_t chunk = 0;
        if (lane == 0) chunk = atomicAdd(&A.ctl->cursor, 1u);
        chunk = (uint32_t)__shfl((int32_t)chunk, 0);
        if (chunk >= A.n_chunks) break;
        const uint32_t c = chunk * kWave + (uint32_t)lane;
        unsigned long long todo = __ballot(c < A.nc && A.msize[c] != 0u);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            pc_clique(A, chunk * kWave + (uint32_t)src, sv, sp, cand, links, lane);
        }
    }
    if (links) atomicAdd(&A.ctl->links, (unsigned long long)links);
}

// ---- the outputs.  k_pc_label is a launch of its own: it reads parent[] and stores nothing there.
__global__ void k_pc_label(const int32_t *parent, const uint32_t *__restrict__ msize, uint32_t nc, int32_t *__restrict__ label, uint32_t *__restrict__ csize)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc) return;
    int32_t l = -1;
    if (msize[i]) { l = comp_find_ro(parent, (int32_t)i); atomicAdd(csize + l, 1u); }
    label[i] = l;
}

__global__ void k_pc_sizes(const int32_t *__restrict__ label, const uint32_t *__restrict__ csize, uint32_t nc, int32_t *__restrict__ size, uint32_t *__restrict__ flag)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc) return;
    const int32_t l = label[i];
    size[i] = l >= 0 ? (int32_t)csize[l] : 0;
    flag[i] = l == (int32_t)i ? 1u : 0u;
}

__global__ void k_pc_reps(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ cnum, const uint32_t *__restrict__ csize, uint32_t nc,
                          int32_t *__restrict__ rep, int32_t *__restrict__ ncl)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc || !flag[i]) return;
    rep[cnum[i]] = (int32_t)i;
    ncl[cnum[i]] = (int32_t)csize[i];
}

__global__ void k_pc_ckeys(const uint32_t *__restrict__ off, const int32_t *__restrict__ verts, const uint32_t *__restrict__ msize,
                           const uint32_t *__restrict__ mpos, const int32_t *__restrict__ label, const uint32_t *__restrict__ cnum, uint32_t nc,
                           uint32_t words, uint64_t *__restrict__ keys)
{
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w >= words) return;
    const uint32_t i = pc_owner(off, nc, w);
    if (!msize[i]) return;
    keys[mpos[i] + (w - off[i])] = ((uint64_t)cnum[label[i]] << 32) | (uint32_t)verts[w];
}

// the distinct (community, vertex) pairs, sorted: the communities' vertex lists as they stand
__global__ void k_pc_comm(const uint64_t *__restrict__ keys, uint32_t n, uint32_t n_comm, uint32_t nv, uint32_t *__restrict__ coff, int32_t *__restrict__ cverts,
                          int32_t *__restrict__ v_comm, int32_t *__restrict__ v_first, PcCtl *ctl)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t c = (uint32_t)(keys[p] >> 32), v = (uint32_t)keys[p];
    if (c >= n_comm || v >= nv) { ctl->bad = 1u; cverts[p] = 0; return; }
    cverts[p] = (int32_t)v;
    if (p == 0 || (uint32_t)(keys[p - 1] >> 32) != c) coff[c] = p;
    atomicAdd(v_comm + v, 1);
    atomicMin(v_first + v, (int32_t)c);
}

__global__ void k_pc_vfix(const int32_t *__restrict__ v_comm, int32_t *__restrict__ v_first, uint32_t nv)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v < nv && v_comm[v] == 0) v_first[v] = -1;
}

} // namespace

// the held list (listed, k_min <= k), 2 <= k and the budget's sign are checked by the caller (api.cpp).  The result is built on the
// side and replaces the previous one only when the run has succeeded.
int clique_communities_run(komb_ctx *ctx, int32_t k, int64_t budget)
{
    hipStream_t s = ctx->stream;
    const komb_ctx::MaximalCliques &mx = ctx->mx;
    const int64_t nc = mx.n_cliques, words = (int64_t)mx.verts.size(), nv = ctx->nv > 0 ? ctx->nv : 0;
    if ((int64_t)mx.offset.size() != nc + 1 || mx.offset[(size_t)nc] != words || words > kPcMaxWords)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_communities_run: the held list of %lld cliques and %lld words is inconsistent", (long long)nc, (long long)words);
    Range r_all("komb_clique_communities_run");
    const unsigned long long limit = budget == 0 ? (unsigned long long)kPcDefaultBudget : (unsigned long long)budget;
    komb_ctx::CliqueCommunities res;
    res.k = k; res.k_min = mx.k_min;
    res.label.assign((size_t)nc, -1);
    res.size.assign((size_t)nc, 0);
    res.offset.assign(1, 0);
    res.v_comm.assign((size_t)nv, 0);
    res.v_first.assign((size_t)nv, -1);
    // ---- the offsets as 32-bit words, the member cliques, their entries and the largest of them
    std::vector<uint32_t> off32((size_t)nc + 1);
    int64_t entries = 0;
    uint32_t smax = 0;
    for (int64_t i = 0; i <= nc; ++i) off32[(size_t)i] = (uint32_t)mx.offset[(size_t)i];
    for (int64_t i = 0; i < nc; ++i) {
        const uint32_t sz = off32[(size_t)i + 1] - off32[(size_t)i];
        if (sz >= (uint32_t)k) { ++res.n_member; entries += sz; smax = std::max(smax, sz); }
    }
    if (smax > kPcMaxSize)
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_communities_run: a clique of %u vertices; the limit is %u", smax, kPcMaxSize);
    DevBufs bufs(ctx);
    PcCtl h{};
    unsigned group = 0;
    if (const char *e = ctx_opt(ctx, "PERC_GROUP")) {
        group = (unsigned)strtoul(e, nullptr, 10);
        if (group != 4 && group != 16 && group != 64) group = 0;
    }
    uint32_t links_seen = 0;
    ctx->timer.start(s);
    if (res.n_member > 0) {
        const uint32_t unc = (uint32_t)nc, uw = (uint32_t)words, ue = (uint32_t)entries, unv = (uint32_t)nv;
        PcArgs A{};
        uint32_t *d_off = nullptr, *d_msize = nullptr, *d_mpos = nullptr, *d_rs = nullptr, *d_re = nullptr, *d_pstart = nullptr, *d_csize = nullptr,
                 *d_flag = nullptr, *d_cnum = nullptr, *d_coff = nullptr;
        int32_t *d_verts = nullptr, *d_row = nullptr, *d_parent = nullptr, *d_label = nullptr, *d_size = nullptr, *d_rep = nullptr, *d_ncl = nullptr,
                *d_cverts = nullptr, *d_vc = nullptr;
        uint64_t *d_keys = nullptr, *d_keys_alt = nullptr, *d_sorted = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&A.ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&d_off, (size_t)nc + 1));
        KOMB_HIP(ctx, bufs.alloc(&d_verts, (size_t)words));
        KOMB_HIP(ctx, bufs.alloc(&d_msize, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_mpos, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_parent, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_rs, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_re, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_row, (size_t)entries));
        KOMB_HIP(ctx, bufs.alloc(&d_pstart, (size_t)words));
        KOMB_HIP(ctx, bufs.alloc(&d_keys, (size_t)entries));
        KOMB_HIP(ctx, bufs.alloc(&d_keys_alt, (size_t)entries));
        KOMB_HIP(ctx, hipMemsetAsync(A.ctl, 0, sizeof(PcCtl), s));
        KOMB_HIP(ctx, staged_copy(ctx, d_off, off32.data(), off32.size() * sizeof(uint32_t), true));
        KOMB_HIP(ctx, staged_copy(ctx, d_verts, mx.verts.data(), (size_t)words * sizeof(int32_t), true));
        for (uint32_t *p : {d_rs, d_re}) KOMB_HIP(ctx, hipMemsetAsync(p, 0, (size_t)nv * sizeof(uint32_t), s));
        // ---- the incidence: keys (vertex, clique) of the member cliques, sorted; a vertex' row is its member cliques, ascending
        k_pc_flag<<<tiles_of(nc), kBlock, 0, s>>>(d_off, unc, (uint32_t)k, d_msize, d_parent);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_TRY(prim_exclusive_sum_u32(ctx, d_msize, d_mpos, nc));
        k_pc_keys<<<tiles_of(words), kBlock, 0, s>>>(d_off, d_verts, d_msize, d_mpos, unc, uw, unv, d_keys, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_TRY(prim_sort_u64(ctx, d_keys, d_keys_alt, entries, 32 + key_bits(nv), &d_sorted));
        k_pc_rows<<<tiles_of(entries), kBlock, 0, s>>>(d_sorted, ue, unv, unc, d_row, d_rs, d_re, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        // ---- the pivots and pair_tests, before anything is linked
        A.off = d_off; A.verts = d_verts; A.msize = d_msize; A.rs = d_rs; A.re = d_re; A.row = d_row; A.pstart = d_pstart; A.parent = d_parent;
        A.nc = unc; A.n_chunks = (unc + kWave - 1) / kWave; A.k = (uint32_t)k; A.smax = smax; A.group = group;
        const int grid = (int)std::min<uint32_t>(A.n_chunks, (uint32_t)kPcGrid);
        k_pc_pivots<<<grid, kWave, (size_t)smax * sizeof(unsigned long long), s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(PcCtl)));
        if (h.bad)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_communities_run: the incidence of %lld member cliques is inconsistent (%lld entries)",
                      (long long)res.n_member, (long long)entries);
        if (h.pair_tests > limit)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_communities_run: %llu pair tests at k %d exceed the budget of %llu (%lld member cliques)", h.pair_tests,
                      (int)k, limit, (long long)res.n_member);
        res.pair_tests = (int64_t)h.pair_tests;
        // ---- the links
        KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->cursor, 0, sizeof(uint32_t), s));
        k_pc_link<<<grid, kWave, ((size_t)2 * smax + kWave) * sizeof(int32_t), s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        // ---- labels, sizes, reps, community numbers
        KOMB_HIP(ctx, bufs.alloc(&d_label, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_size, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_csize, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)nc));
        KOMB_HIP(ctx, bufs.alloc(&d_cnum, (size_t)nc));
        KOMB_HIP(ctx, hipMemsetAsync(d_csize, 0, (size_t)nc * sizeof(uint32_t), s));
        k_pc_label<<<tiles_of(nc), kBlock, 0, s>>>(d_parent, d_msize, unc, d_label, d_csize);
        KOMB_HIP(ctx, hipGetLastError());
        k_pc_sizes<<<tiles_of(nc), kBlock, 0, s>>>(d_label, d_csize, unc, d_size, d_flag);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_cnum, nc));
        uint32_t tail[2] = {0u, 0u};
        KOMB_HIP(ctx, d2h(ctx, &tail[0], d_cnum + (nc - 1), sizeof(uint32_t)));
        KOMB_HIP(ctx, d2h(ctx, &tail[1], d_flag + (nc - 1), sizeof(uint32_t)));
        const int64_t n_comm = (int64_t)tail[0] + tail[1];
        if (n_comm < 1 || n_comm > res.n_member)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_communities_run: %lld communities of %lld member cliques", (long long)n_comm, (long long)res.n_member);
        KOMB_HIP(ctx, bufs.alloc(&d_rep, (size_t)n_comm));
        KOMB_HIP(ctx, bufs.alloc(&d_ncl, (size_t)n_comm));
        KOMB_HIP(ctx, bufs.alloc(&d_coff, (size_t)n_comm));
        KOMB_HIP(ctx, bufs.alloc(&d_cverts, (size_t)entries));
        KOMB_HIP(ctx, bufs.alloc(&d_vc, (size_t)std::max<int64_t>(2 * nv, 1)));   // v_comm[nv] | v_first[nv]
        k_pc_reps<<<tiles_of(nc), kBlock, 0, s>>>(d_flag, d_cnum, d_csize, unc, d_rep, d_ncl);
        KOMB_HIP(ctx, hipGetLastError());
        // ---- the communities' vertices: keys (community, vertex) of every member clique's vertices, sorted, distinct
        k_pc_ckeys<<<tiles_of(words), kBlock, 0, s>>>(d_off, d_verts, d_msize, d_mpos, d_label, d_cnum, unc, uw, d_keys);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_TRY(prim_sort_u64(ctx, d_keys, d_keys_alt, entries, 32 + key_bits(n_comm), &d_sorted));
        uint64_t *d_uniq = d_sorted == d_keys ? d_keys_alt : d_keys;
        int64_t n_uniq = 0;
        KOMB_TRY(prim_unique_u64(ctx, d_sorted, d_uniq, entries, &n_uniq));
        if (n_uniq < n_comm || n_uniq > entries)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_communities_run: %lld distinct vertices in %lld communities", (long long)n_uniq, (long long)n_comm);
        KOMB_HIP(ctx, hipMemsetAsync(d_coff, 0, (size_t)n_comm * sizeof(uint32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(d_vc, 0, (size_t)nv * sizeof(int32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(d_vc + nv, 0x7F, (size_t)nv * sizeof(int32_t), s));
        k_pc_comm<<<tiles_of(n_uniq), kBlock, 0, s>>>(d_uniq, (uint32_t)n_uniq, (uint32_t)n_comm, unv, d_coff, d_cverts, d_vc, d_vc + nv, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        k_pc_vfix<<<tiles_of(nv), kBlock, 0, s>>>(d_vc, d_vc + nv, unv);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(PcCtl)));
        if (h.bad)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_communities_run: the links are inconsistent (k %d, %lld member cliques, %lld communities)", (int)k,
                      (long long)res.n_member, (long long)n_comm);
        links_seen = (uint32_t)std::min<unsigned long long>(h.links, 0xFFFFFFFFull);
        // ---- to the host
        res.n_comm = n_comm;
        res.rep.resize((size_t)n_comm);
        res.n_cliques.resize((size_t)n_comm);
        res.verts.resize((size_t)n_uniq);
        std::vector<uint32_t> coff((size_t)n_comm);
        KOMB_HIP(ctx, staged_copy(ctx, res.label.data(), d_label, (size_t)nc * sizeof(int32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, res.size.data(), d_size, (size_t)nc * sizeof(int32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, res.rep.data(), d_rep, (size_t)n_comm * sizeof(int32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, res.n_cliques.data(), d_ncl, (size_t)n_comm * sizeof(int32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, coff.data(), d_coff, (size_t)n_comm * sizeof(uint32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, res.verts.data(), d_cverts, (size_t)n_uniq * sizeof(int32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, res.v_comm.data(), d_vc, (size_t)nv * sizeof(int32_t), false));
        KOMB_HIP(ctx, staged_copy(ctx, res.v_first.data(), d_vc + nv, (size_t)nv * sizeof(int32_t), false));
        res.offset.assign((size_t)n_comm + 1, 0);
        for (int64_t c = 0; c < n_comm; ++c) res.offset[(size_t)c] = (int64_t)coff[(size_t)c];
        res.offset[(size_t)n_comm] = n_uniq;
        for (int64_t c = 0; c < n_comm; ++c) {
            const int64_t len = res.offset[(size_t)c + 1] - res.offset[(size_t)c];
            if (len < k) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_clique_communities_run: community %lld has %lld vertices at k %d", (long long)c, (long long)len, (int)k);
            res.largest = std::max(res.largest, len);
        }
        for (int64_t v = 0; v < nv; ++v) {
            res.n_covered += res.v_comm[(size_t)v] >= 1;
            res.n_overlap += res.v_comm[(size_t)v] >= 2;
        }
    }
    res.ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    if (ctx_flag(ctx, "PERC_DEBUG"))
        fprintf(stderr, "komb clique communities: k %d (list k_min %d), %lld cliques, %lld members of at most %u vertices, %lld entries, group %u, "
                "%lld pair tests of %llu, %u links, %lld communities, largest %lld, covered %lld, overlap %lld, run %.3f ms\n", (int)k, (int)res.k_min,
                (long long)nc, (long long)res.n_member, smax, (long long)entries, group, (long long)res.pair_tests, limit, links_seen, (long long)res.n_comm,
                (long long)res.largest, (long long)res.n_covered, (long long)res.n_overlap, res.ms);
    res.done = true;
    ctx->pc = std::move(res);
    return KOMB_OK;
}

} // namespace komb
