// graphlets.hip -- the graphlet census (komb_graphlets_run): per vertex the fifteen orbits of the induced 3- and 4-vertex
// subgraphs (Przulj, "Biological network comparison using graphlet degree distribution", Bioinformatics 2007; the counting
// scheme is that of ORCA, Hocevar and Demsar 2014, and PGD, Ahmed et al. 2015: count the few patterns that need a search,
// derive the rest), per canonical edge its 4-cycles and 4-cliques, on the last complete k-truss result.  DESIGN.md section 4.6o.
//
// Input: the canonical edges (eu[i] < ev[i], sorted by (eu, ev), original ids) of that result and the supports sup[i] the
// peel started from (the triangles through the edge).  Three passes:
//
//   1. 4-cycles per edge, THE HOT PASS, degree ordered.  The vertices are ranked by (d, id) and the result is rebuilt as a
//      symmetric CSR in RANKS, every row ascending, with the canonical edge id beside every entry (k_gl_adj_keys, one radix
//      sort of the 2 |E| (row, neighbour) keys, k_gl_split): the neighbours of u below a rank r are a PREFIX of u's row, found
//      once per entry by a bisection (k_gl_plen: plen[i] for the entry i = (r, u) with u below r; their sum is the root's number of
//      walked entries, items[r]).  Root r walks every u in its own prefix and every w in u's prefix below r: cnt[w] += 1.  The
//      same walk a second time adds cnt[w] - 1 to edge (u, w), one 64-bit atomic per walked entry, and their sum over w to edge
//      (r, u), one atomic per (root, u).  Every 4-cycle is found once, from its highest-ranked vertex.
//      cnt lives where the root's size puts it (k_gl_classify queues the roots by tier):
//        wave    items <= GRAPHLET_SHORT: one wavefront, an open-addressing table of kGlWaveSlots words in LDS (k_gl_cyc_wave)
//        lds     items <= GRAPHLET_LDS:   one workgroup, a table of kGlLdsSlots words in LDS, 64 KiB (k_gl_cyc_lds)
//        heavy   the rest: one of kGlSlots dense tables of nv words in global memory, kGlParts workgroups per root, three
//                launches per batch of kGlSlots roots -- count, add, and a third walk that puts the zeros back (k_gl_cyc_heavy)
//      A table holds at most as many keys as the root walks entries, and the thresholds are clamped to half the slots, so a
//      probe sequence always ends.
//   2. triangles (k_gl_tri): every triangle a < b < c once, from its edge (a, b) over the oriented canonical rows, the shorter
//      side walked and the longer one bisected (oriented_search_dev.h: edge_sides, nuc_find).  Per triangle
//      D2[x] += sup(opposite edge) - 1 for its three vertices, and the 4-cliques with a fourth vertex above c (nuc_tails,
//      nuc_clq_entry): each adds 1 to its six edges directly -- the three of the triangle summed up first -- so no triangle
//      is stored and there is no triangle or clique limit (the nucleus decomposition numbers both and has one).
//   3. vertices: two sweeps over the edges that sum per-edge terms onto both ends (k_gl_edge1, k_gl_edge2: the eu end by a
//      segmented sum inside the wave, the ev end by one atomic per edge and term), then the fifteen closed forms and the sums
//      of the nine totals (k_gl_vertex).
//
// Which word is written when: cycles4[] only by pass 1's atomics, cliques4[] and D2[] only by pass 2's, the sums of pass 3 by
// its two sweeps, each read only by later launches.  All arithmetic is unsigned 64-bit; with every degree below 2^20 no
// exact value reaches 2^63 (DESIGN.md has the derivation), so the wrap-around of an intermediate difference cancels.
#include "oriented_search_dev.h"

namespace komb {

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr uint32_t kGlMaxDeg = 1u << 20;    // a result with a vertex of this degree or more is refused (KOMB_ERR_LIMIT)
constexpr int kGlWaveBits = 8, kGlWaveSlots = 1 << kGlWaveBits, kGlWaveMax = kGlWaveSlots / 2;
constexpr int kGlLdsBits = 13, kGlLdsSlots = 1 << kGlLdsBits, kGlLdsMax = kGlLdsSlots / 2;   // 2 x 32 KiB: two workgroups share a CU's 160 KiB
constexpr int kGlSlots = 8, kGlParts = 64;  // heavy roots side by side x workgroups per root
constexpr int kGlWaveGrid = 2048, kGlLdsGrid = 1024;    // queue kernels: at most this many workgroups, each striding
constexpr uint32_t kGlEmpty = 0xFFFFFFFFu;
constexpr uint32_t kGlTriShort = 16;        // triangle pass: a walked side up to this long stays with the edge's lane
constexpr int kGlSums = 7, kGlSums2 = 2;    // planes of the two edge sweeps

struct GlCtl {                              // zeroed before every run
    uint32_t max_deg, n_wave, n_lds, n_heavy;
    u64 items;                              // walked entries of pass 1
    u64 lo[KOMB_GRAPHLET_TYPES], hi[KOMB_GRAPHLET_TYPES];   // the orbit sums behind the totals, low and high 32 bits summed apart
};

struct GlCsr { const uint32_t *rowptr, *col, *plen, *eid; };   // the result in ranks (see above)

inline int gl_grid(int64_t n) { const int64_t g = (n + kBlock - 1) / kBlock; return (int)(g < 1 ? 1 : g); }

__device__ __forceinline__ u64 wave_sum64(u64 v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The lanes of a wave hold consecutive canonical edges, u = eu of the lane's edge (-1 past the end): inclusive sums of v over
// the lanes with equal u (one run: eu ascends).  The LAST lane of a run (gl_run_last) holds the run's total.  Every lane calls both.
__device__ __forceinline__ u64 seg_sum(int32_t u, u64 v, int lane)
{
    for (int o = 1; o < kWave; o <<= 1) {
        const u64 ov = __shfl_up(v, o);
        const int32_t ou = __shfl_up(u, o);
        if (lane >= o && ou == u) v += ov;
    }
    return v;
}
__device__ __forceinline__ bool gl_run_last(int32_t u, int lane)
{
    const int32_t nu = __shfl_down(u, 1);
    return lane == kWave - 1 || nu != u;
}

// ---- degrees, ranks, the CSR in ranks

__global__ void k_gl_deg_init(uint32_t nv, const uint32_t *__restrict__ rowptr, uint32_t *__restrict__ deg)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) deg[v] = rowptr ? rowptr[v + 1] - rowptr[v] : 0u;
}

// d(v) of a vmask result: the result edges at v
__global__ void k_gl_deg_count(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, uint32_t m, uint32_t *deg)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = i < m;
    const int32_t u = act ? eu[i] : -1;
    const u64 n = seg_sum(u, 1ull, lane);
    const bool last = gl_run_last(u, lane);
    if (act && last) atomicAdd(deg + u, (uint32_t)n);
    if (act) atomicAdd(deg + ev[i], 1u);
}

__global__ void k_gl_key(uint32_t nv, const uint32_t *__restrict__ deg, uint64_t *__restrict__ key, GlCtl *ctl)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t d = v < nv ? deg[v] : 0u;
    if (v < nv) key[v] = ((uint64_t)d << 32) | v;
    const uint32_t mx = wave_max(d);
    if ((threadIdx.x & (kWave - 1)) == 0 && mx) atomicMax(&ctl->max_deg, mx);
}

// order[i] = (d, v) of the vertex of rank i: rank[v] = i, rdeg[i] = d, rdeg[nv] = 0 (the scan's last entry)
__global__ void k_gl_rank(uint32_t nv, const uint64_t *__restrict__ order, uint32_t *__restrict__ rank, uint32_t *__restrict__ rdeg)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > nv) return;
    if (i == nv) { rdeg[i] = 0u; return; }
    const uint64_t k = order[i];
    rank[(uint32_t)k] = i;
    rdeg[i] = (uint32_t)(k >> 32);
}

// both directions of every edge as (row rank, neighbour rank) keys with the canonical edge id as the value
__global__ void k_gl_adj_keys(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, uint32_t m, const uint32_t *__restrict__ rank,
                              uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= m) return;
    const uint32_t ru = rank[eu[e]], rv = rank[ev[e]];
    key[2 * (size_t)e] = ((uint64_t)ru << 32) | rv;
    key[2 * (size_t)e + 1] = ((uint64_t)rv << 32) | ru;
    val[2 * (size_t)e] = e;
    val[2 * (size_t)e + 1] = e;
}

__global__ void k_gl_split(const uint64_t *__restrict__ skey, uint32_t n2, uint32_t *__restrict__ col)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n2) col[i] = (uint32_t)skey[i];
}

// entry i = (r, u): with u below r, plen[i] = the entries of row u below r, added to items[r]; else 0
__global__ void k_gl_plen(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ col, const uint32_t *__restrict__ rowptr, uint32_t n2,
                          uint32_t *__restrict__ plen, u64 *items)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n2) return;
    const uint32_t r = (uint32_t)(skey[i] >> 32), u = col[i];
    uint32_t p = 0;
    if (u < r) { const uint32_t b = rowptr[u]; p = row_lower(col, r, b, rowptr[u + 1]) - b; }
    plen[i] = p;
    if (p) atomicAdd(items + r, (u64)p);
}

// the roots with something to walk into the queue of their tier (the order inside a queue is whatever the atomics give)
__global__ void k_gl_classify(uint32_t nv, const u64 *__restrict__ items, uint32_t n_short, uint32_t n_lds, GlCtl *ctl,
                              uint32_t *__restrict__ q_wave, uint32_t *__restrict__ q_lds, uint32_t *__restrict__ q_heavy)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    const u64 it = r < nv ? items[r] : 0ull;
    if (it) {
        if (it <= n_short) q_wave[atomicAdd(&ctl->n_wave, 1u)] = r;
        else if (it <= n_lds) q_lds[atomicAdd(&ctl->n_lds, 1u)] = r;
        else q_heavy[atomicAdd(&ctl->n_heavy, 1u)] = r;
    }
    const u64 sum = wave_sum64(it);
    if ((threadIdx.x & (kWave - 1)) == 0 && sum) atomicAdd(&ctl->items, sum);
}

// ---- pass 1: the tables and the walks

template <int kBits> struct GlHash {        // open addressing in LDS: key[] = kGlEmpty, cnt[] = 0 between roots
    uint32_t *key, *cnt;
    static __device__ __forceinline__ uint32_t home(uint32_t w) { return (w * 2654435761u) >> (32 - kBits); }
    __device__ __forceinline__ void add(uint32_t w) const
    {
        uint32_t h = home(w);
        for (;;) {
            const uint32_t prev = atomicCAS(key + h, kGlEmpty, w);
            if (prev == kGlEmpty || prev == w) { atomicAdd(cnt + h, 1u); return; }
            h = (h + 1) & ((1u << kBits) - 1u);
        }
    }
    __device__ __forceinline__ uint32_t get(uint32_t w) const       // (w was added: the probe ends at it)
    {
        uint32_t h = home(w);
        while (key[h] != w) h = (h + 1) & ((1u << kBits) - 1u);
        return cnt[h];
    }
    __device__ __forceinline__ void clean(uint32_t) const {}
    __device__ __forceinline__ void wipe(int tid, int n) const      // by the n threads that share the table
    {
        for (int k = tid; k < (1 << kBits); k += n) { key[k] = kGlEmpty; cnt[k] = 0u; }
    }
};

struct GlDense {                            // nv words of global memory, zero between roots
    uint32_t *cnt;
    __device__ __forceinline__ void add(uint32_t w) const { atomicAdd(cnt + w, 1u); }
    __device__ __forceinline__ uint32_t get(uint32_t w) const { return cnt[w]; }
    __device__ __forceinline__ void clean(uint32_t w) const { cnt[w] = 0u; }
};

// phase 0: cnt[w] += 1; phase 1: the edges' shares; phase 2: cnt[w] = 0
template <int kPhase, class Tab>
__device__ __forceinline__ u64 gl_entry(const GlCsr &g, uint32_t x, const Tab &tab, u64 *cyc)
{
    const uint32_t w = g.col[x];
    if (kPhase == 0) tab.add(w);
    if (kPhase == 2) tab.clean(w);
    if (kPhase != 1) return 0ull;
    const u64 c = (u64)(tab.get(w) - 1u);
    if (c) atomicAdd(cyc + g.eid[x], c);
    return c;
}

// the root's prefix [row, row + pre), one LANE per u, its prefix entry by entry (roots of the wave tier: a few entries each)
template <int kPhase, class Tab>
__device__ __forceinline__ void gl_walk_lanes(const GlCsr &g, uint32_t row, uint32_t pre, int lane, const Tab &tab, u64 *cyc)
{
    for (uint32_t i = row + (uint32_t)lane; i < row + pre; i += kWave) {
        const uint32_t b = g.rowptr[g.col[i]], n = g.plen[i];
        u64 acc = 0;
        for (uint32_t x = b; x < b + n; ++x) acc += gl_entry<kPhase>(g, x, tab, cyc);
        if (kPhase == 1 && acc) atomicAdd(cyc + g.eid[i], acc);
    }
}

// ... one WAVE per u, wave `wid` of `nw`, the lanes side by side over u's prefix.  Every lane of the wave calls it.
template <int kPhase, class Tab>
__device__ __forceinline__ void gl_walk_waves(const GlCsr &g, uint32_t row, uint32_t pre, uint32_t wid, uint32_t nw, int lane, const Tab &tab, u64 *cyc)
{
    for (uint32_t i = row + wid; i < row + pre; i += nw) {                  // (uniform per wave)
        const uint32_t b = g.rowptr[g.col[i]], n = g.plen[i];
        u64 acc = 0;
        for (uint32_t x = b + (uint32_t)lane; x < b + n; x += kWave) acc += gl_entry<kPhase>(g, x, tab, cyc);
        if (kPhase == 1) {
            acc = wave_sum64(acc);
            if (lane == 0 && acc) atomicAdd(cyc + g.eid[i], acc);
        }
    }
}

// what one wave wrote to its LDS table is there for all its lanes (LDS serves a wave's accesses in order; the compiler keeps them so)
__device__ __forceinline__ void gl_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(kBlock) k_gl_cyc_wave(GlCsr g, const uint32_t *__restrict__ queue, uint32_t nq, u64 *cyc)
{
    __shared__ uint32_t s_key[kBlock / kWave][kGlWaveSlots], s_cnt[kBlock / kWave][kGlWaveSlots];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const GlHash<kGlWaveBits> tab{s_key[wave], s_cnt[wave]};
    tab.wipe(lane, kWave);
    gl_wave_sync();
    const uint32_t nw = gridDim.x * (kBlock / kWave);
    for (uint32_t i = blockIdx.x * (kBlock / kWave) + (uint32_t)wave; i < nq; i += nw) {   // (uniform per wave)
        const uint32_t r = queue[i], row = g.rowptr[r];
        const uint32_t pre = row_lower(g.col, r, row, g.rowptr[r + 1]) - row;
        gl_walk_lanes<0>(g, row, pre, lane, tab, cyc);
        gl_wave_sync();
        gl_walk_lanes<1>(g, row, pre, lane, tab, cyc);
        gl_wave_sync();
        tab.wipe(lane, kWave);
        gl_wave_sync();
    }
}

__global__ void __launch_bounds__(kBlock) k_gl_cyc_lds(GlCsr g, const uint32_t *__restrict__ queue, uint32_t nq, u64 *cyc)
{
    __shared__ uint32_t s_key[kGlLdsSlots], s_cnt[kGlLdsSlots];
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = threadIdx.x / kWave;
    const GlHash<kGlLdsBits> tab{s_key, s_cnt};
    tab.wipe((int)threadIdx.x, kBlock);
    __syncthreads();
    for (uint32_t i = blockIdx.x; i < nq; i += gridDim.x) {                 // (uniform per workgroup)
        const uint32_t r = queue[i], row = g.rowptr[r];
        const uint32_t pre = row_lower(g.col, r, row, g.rowptr[r + 1]) - row;
        gl_walk_waves<0>(g, row, pre, wave, kBlock / kWave, lane, tab, cyc);
        __syncthreads();
        gl_walk_waves<1>(g, row, pre, wave, kBlock / kWave, lane, tab, cyc);
        __syncthreads();
        tab.wipe((int)threadIdx.x, kBlock);
        __syncthreads();
    }
}

// block (x, y): the x-th of gridDim.x parts of the root queue[first + y], on the y-th dense table
template <int kPhase>
__global__ void __launch_bounds__(kBlock) k_gl_cyc_heavy(GlCsr g, const uint32_t *__restrict__ queue, uint32_t first, uint32_t nq, uint32_t *dense,
                                                         uint32_t nv, u64 *cyc)
{
    const uint32_t i = first + blockIdx.y;
    if (i >= nq) return;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t r = queue[i], row = g.rowptr[r];
    const uint32_t pre = row_lower(g.col, r, row, g.rowptr[r + 1]) - row;
    const GlDense tab{dense + (size_t)blockIdx.y * nv};
    gl_walk_waves<kPhase>(g, row, pre, blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave, gridDim.x * (kBlock / kWave), lane, tab, cyc);
}

// ---- pass 2: triangles and the 4-cliques above them

// triangle a < b < c with (a, b) at j, (a, c) at pac, (b, c) at pbc
__device__ __forceinline__ void gl_triangle(const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs, const uint32_t *__restrict__ re,
                                            const int32_t *__restrict__ sup, int32_t a, int32_t b, int32_t c, uint32_t j, uint32_t pac,
                                            uint32_t pbc, u64 *d2, u64 *clq)
{
    const u64 ta = (u64)(sup[pbc] - 1), tb = (u64)(sup[pac] - 1), tc = (u64)(sup[j] - 1);   // (each edge is in this triangle: sup >= 1)
    if (ta) atomicAdd(d2 + a, ta);
    if (tb) atomicAdd(d2 + b, tb);
    if (tc) atomicAdd(d2 + c, tc);
    const NucTails s = nuc_tails(a, b, c, pac, pbc, rs, re);
    u64 mine = 0;
    for (uint32_t x = s.it; x < s.it + s.n; ++x) {
        uint32_t p1, p2;
        if (!nuc_clq_entry(ev, s, x, &p1, &p2)) continue;
        atomicAdd(clq + x, 1ull); atomicAdd(clq + p1, 1ull); atomicAdd(clq + p2, 1ull);   // (a, d), (b, d), (c, d) in some order
        ++mine;
    }
    if (mine) { atomicAdd(clq + j, mine); atomicAdd(clq + pac, mine); atomicAdd(clq + pbc, mine); }
}

// one lane per edge j = (a, b): c is in row a behind j and in row b; the shorter side is walked, the longer one bisected.  A
// side above n_short goes through the edge's wave, every lane taking the triangles it finds.
__global__ void k_gl_tri(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                         const uint32_t *__restrict__ re, const int32_t *__restrict__ sup, uint32_t m, uint32_t n_short, u64 *d2, u64 *clq)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    EdgeSides s{0, 0, 0, 0, true};
    int32_t a = 0, b = 0;
    if (j < m && sup[j] > 0) { a = eu[j]; b = ev[j]; s = edge_sides(eu, ev, rs, re, j); }
    // entry x of edge ej = (ea, eb) with the sides e
    const auto entry = [&](uint32_t ej, int32_t ea, int32_t eb, const EdgeSides &e, uint32_t x) {
        const int32_t c = ev[x];
        const uint32_t hit = nuc_find(ev, c, e.lo, e.hi);
        if (hit != kNucNone) gl_triangle(ev, rs, re, sup, ea, eb, c, ej, e.walk_a ? x : hit, e.walk_a ? hit : x, d2, clq);
    };
    const bool mid = s.n > n_short;
    if (!mid)
        for (uint32_t x = s.it; x < s.it + s.n; ++x) entry(j, a, b, s, x);
    wave_turns(mid, [&](int src) {
        const uint32_t rj = from_lane(j, src);
        const int32_t ra = __shfl(a, src), rb = __shfl(b, src);
        const EdgeSides r = from_lane(s, src);
        wave_walk(r.it, r.n, lane, [&](uint32_t x) { entry(rj, ra, rb, r, x); });
    });
}

// ---- pass 3: the per-vertex sums and the closed forms

// `val` of the lane's edge onto both ends in plane p: the eu end by runs, the ev end by an atomic.  Every lane calls it.
__device__ __forceinline__ void gl_add(u64 *plane, int32_t u, int32_t v, bool act, bool last, u64 to_u, u64 to_v, int lane)
{
    const u64 s = seg_sum(u, to_u, lane);
    if (act && last && s) atomicAdd(plane + u, s);
    if (act && to_v) atomicAdd(plane + v, to_v);
}

// planes of acc[kGlSums * nv]: 0 sum t_e | 1 sum cliques4 | 2 sum cycles4 | 3 sum C(t_e, 2) | 4 sum t_e (d(other) - 2) |
// 5 S = sum (d(other) - 1) | 6 sum C(d(other) - 1, 2)
__global__ void k_gl_edge1(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ sup,
                           const u64 *__restrict__ cyc, const u64 *__restrict__ clq, uint32_t m, const uint32_t *__restrict__ deg, u64 *acc, size_t nv)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = i < m;
    int32_t u = -1, v = -1;
    u64 t = 0, k = 0, c = 0, du = 0, dv = 0;
    if (act) { u = eu[i]; v = ev[i]; t = (u64)sup[i]; k = clq[i]; c = cyc[i]; du = deg[u]; dv = deg[v]; }
    const bool last = gl_run_last(u, lane);
    gl_add(acc, u, v, act, last, t, t, lane);
    gl_add(acc + nv, u, v, act, last, k, k, lane);
    gl_add(acc + 2 * nv, u, v, act, last, c, c, lane);
    const u64 t2 = t * (t - 1) / 2;                                         // (t = 0: 0)
    gl_add(acc + 3 * nv, u, v, act, last, t2, t2, lane);
    gl_add(acc + 4 * nv, u, v, act, last, t * (dv - 2), t * (du - 2), lane);               // (t > 0: both ends have degree >= 2)
    gl_add(acc + 5 * nv, u, v, act, last, act ? dv - 1 : 0ull, act ? du - 1 : 0ull, lane);
    gl_add(acc + 6 * nv, u, v, act, last, act ? (dv - 1) * (dv - 2) / 2 : 0ull, act ? (du - 1) * (du - 2) / 2 : 0ull, lane);   // (d = 1: 0 x anything)
}

// planes of acc2[kGlSums2 * nv]: 0 sum (t(other) - t_e) | 1 sum S(other)
__global__ void k_gl_edge2(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ sup, uint32_t m,
                           const u64 *__restrict__ acc, u64 *acc2, size_t nv)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = i < m;
    int32_t u = -1, v = -1;
    u64 nu = 0, nw = 0, su = 0, sv = 0;
    if (act) {
        u = eu[i]; v = ev[i];
        const u64 t = (u64)sup[i];
        nu = acc[v] / 2 - t; nw = acc[u] / 2 - t;                           // (the triangles at a vertex include those of its edge)
        su = acc[5 * nv + v]; sv = acc[5 * nv + u];
    }
    const bool last = gl_run_last(u, lane);
    gl_add(acc2, u, v, act, last, nu, nw, lane);
    gl_add(acc2 + nv, u, v, act, last, su, sv, lane);
}

__global__ void k_gl_vertex(uint32_t n, const uint32_t *__restrict__ deg, const u64 *__restrict__ acc, const u64 *__restrict__ acc2,
                            const u64 *__restrict__ d2, u64 *__restrict__ orbit, GlCtl *ctl)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const size_t nv = n;
    u64 o[KOMB_GRAPHLET_ORBITS];
    for (int i = 0; i < KOMB_GRAPHLET_ORBITS; ++i) o[i] = 0;
    if (v < n) {
        const u64 d = deg[v], t = acc[v] / 2, k3 = acc[nv + v], k4 = k3 / 3, c4 = acc[2 * nv + v] / 2, d3 = acc[3 * nv + v];
        const u64 w10 = acc[4 * nv + v], S = acc[5 * nv + v], b6 = acc[6 * nv + v], n9 = acc2[v], ss = acc2[nv + v], D2 = d2[v];
        o[0] = d;
        o[3] = t;
        o[2] = d * (d - 1) / 2 - t;
        o[1] = S - 2 * t;
        o[14] = k4;
        o[13] = d3 - k3;
        o[12] = D2 - k3;
        o[8] = c4 - o[12] - o[13] - k3;
        o[11] = t * (d - 2) - 2 * o[13] - k3;
        o[10] = w10 - 2 * o[13] - 2 * o[12] - 2 * k3;
        o[9] = n9 - 2 * o[12] - k3;
        o[7] = d * (d - 1) * (d - 2) / 6 - o[11] - o[13] - k4;
        o[6] = b6 - o[9] - o[10] - o[13] - 2 * o[12] - k3;
        o[4] = ss - d * (d - 1) - 2 * t - 2 * o[8] - 2 * o[9] - o[10] - 2 * o[13] - 4 * o[12] - 2 * k3;
        o[5] = (d - 1) * S - 2 * t - 2 * o[8] - o[10] - 2 * o[11] - 4 * o[13] - 2 * o[12] - 2 * k3;
        for (int i = 0; i < KOMB_GRAPHLET_ORBITS; ++i) orbit[(size_t)i * nv + v] = o[i];
    }
    const int which[KOMB_GRAPHLET_TYPES] = {0, 2, 3, 5, 7, 8, 11, 13, 14};
    for (int i = 0; i < KOMB_GRAPHLET_TYPES; ++i) {
        const u64 x = o[which[i]];
        const u64 lo = wave_sum64(x & 0xFFFFFFFFull), hi = wave_sum64(x >> 32);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            if (lo) atomicAdd(&ctl->lo[i], lo);
            if (hi) atomicAdd(&ctl->hi[i], hi);
        }
    }
}

inline uint32_t gl_opt_u32(const komb_ctx *ctx, const char *name, uint32_t dflt, uint32_t cap)
{
    const char *e = ctx_opt(ctx, name);
    if (!e) return dflt;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v > cap ? cap : (uint32_t)v;
}

} // namespace

// the k-truss result it needs is checked by the caller (api.cpp).  The result is built in blocks of its own and replaces the
// previous one only when the run has succeeded: a run that fails (KOMB_ERR_NOMEM, KOMB_ERR_LIMIT) leaves the previous one.
int graphlets_run(komb_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    if (m > 0) {
        KOMB_TRY(truss_edges_canonical(ctx));           // (a whole-graph result whose endpoints no fetch has asked for yet)
        KOMB_TRY(truss_support_canonical(ctx));         // (... whose supports no fetch has put in canonical order yet)
    }
    Range r_all("komb_graphlets_run");
    komb_ctx::Graphlets res;                             // goes back to the pool unless it is installed
    const uint32_t n_lds = gl_opt_u32(ctx, "GRAPHLET_LDS", kGlLdsMax, kGlLdsMax);
    uint32_t n_short = gl_opt_u32(ctx, "GRAPHLET_SHORT", kGlWaveMax, kGlWaveMax);
    if (n_short > n_lds) n_short = n_lds;                // (GRAPHLET_LDS=0: every root on a dense table)
    if (nv > 0) {
        const uint32_t un = (uint32_t)nv, um = (uint32_t)m, n2 = 2u * um;
        const int gv = gl_grid(nv), ge = gl_grid(m), g2 = gl_grid(2 * m);
        DevBufs bufs(ctx);
        EventSet evs;
        hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
        KOMB_HIP(ctx, evs.make(&e0)); KOMB_HIP(ctx, evs.make(&e1)); KOMB_HIP(ctx, evs.make(&e2));
        GlCtl *d_ctl = nullptr;
        uint32_t *d_deg = nullptr;
        uint64_t *d_key = nullptr, *d_key_alt = nullptr, *order = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&d_deg, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_key, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_key_alt, (size_t)nv));
        const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *sup = ctx->d_t_sup;
        const bool whole = !ctx->t_own_edges;            // d(v) is the resident row length; a vmask result counts its endpoints

        ctx->timer.start(s);
        KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(GlCtl), s));
        k_gl_deg_init<<<gv, kBlock, 0, s>>>(un, whole && m > 0 ? ctx->d_o_rowptr : nullptr, d_deg);
        if (m > 0 && !whole) k_gl_deg_count<<<ge, kBlock, 0, s>>>(eu, ev, um, d_deg);
        k_gl_key<<<gv, kBlock, 0, s>>>(un, d_deg, d_key, d_ctl);
        KOMB_HIP(ctx, hipGetLastError());
        GlCtl h;
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(GlCtl)));
        if (h.max_deg >= kGlMaxDeg)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_graphlets_run: a vertex of degree %u; the exact 64-bit orbit counts need every degree below 2^20", h.max_deg);
        res.max_degree = (int32_t)h.max_deg;

        KOMB_HIP(ctx, ctx->pool.get((void **)res.orbit.slot(&ctx->pool), (size_t)KOMB_GRAPHLET_ORBITS * nv * sizeof(u64)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.cycles4.slot(&ctx->pool), (size_t)m * sizeof(u64)));
        KOMB_HIP(ctx, ctx->pool.get((void **)res.cliques4.slot(&ctx->pool), (size_t)m * sizeof(u64)));
        if (m == 0) {
            KOMB_HIP(ctx, hipMemsetAsync(res.orbit, 0, (size_t)KOMB_GRAPHLET_ORBITS * nv * sizeof(u64), s));
        } else {
            KOMB_HIP(ctx, hipMemsetAsync(res.cycles4, 0, (size_t)m * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(res.cliques4, 0, (size_t)m * sizeof(u64), s));

            // ---- the result in ranks
            uint32_t *d_rank = nullptr, *d_rowptr = nullptr, *d_val = nullptr, *d_val_alt = nullptr, *d_col = nullptr, *d_plen = nullptr, *eid = nullptr;
            uint32_t *q_wave = nullptr, *q_lds = nullptr, *q_heavy = nullptr;
            uint64_t *d_akey = nullptr, *d_akey_alt = nullptr, *skey = nullptr;
            u64 *d_items = nullptr;
            KOMB_TRY(prim_sort_u64(ctx, d_key, d_key_alt, nv, 32 + key_bits((int64_t)h.max_deg + 1), &order));
            KOMB_HIP(ctx, bufs.alloc(&d_rank, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&d_rowptr, (size_t)nv + 1));
            KOMB_HIP(ctx, bufs.alloc(&d_akey, (size_t)n2));
            KOMB_HIP(ctx, bufs.alloc(&d_akey_alt, (size_t)n2));
            KOMB_HIP(ctx, bufs.alloc(&d_val, (size_t)n2));
            KOMB_HIP(ctx, bufs.alloc(&d_val_alt, (size_t)n2));
            KOMB_HIP(ctx, bufs.alloc(&d_col, (size_t)n2));
            KOMB_HIP(ctx, bufs.alloc(&d_plen, (size_t)n2));
            KOMB_HIP(ctx, bufs.alloc(&d_items, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&q_wave, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&q_lds, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&q_heavy, (size_t)nv));
            (void)hipEventRecord(e0, s);
            k_gl_rank<<<gl_grid(nv + 1), kBlock, 0, s>>>(un, order, d_rank, d_rowptr);
            KOMB_TRY(prim_exclusive_sum_u32(ctx, d_rowptr, d_rowptr, nv + 1));
            k_gl_adj_keys<<<ge, kBlock, 0, s>>>(eu, ev, um, d_rank, d_akey, d_val);
            KOMB_TRY(prim_sort_pairs_u64_u32(ctx, d_akey, d_akey_alt, d_val, d_val_alt, 2 * m, 32 + key_bits(nv), &skey, &eid));
            KOMB_HIP(ctx, hipMemsetAsync(d_items, 0, (size_t)nv * sizeof(u64), s));
            k_gl_split<<<g2, kBlock, 0, s>>>(skey, n2, d_col);
            k_gl_plen<<<g2, kBlock, 0, s>>>(skey, d_col, d_rowptr, n2, d_plen, d_items);
            k_gl_classify<<<gv, kBlock, 0, s>>>(un, d_items, n_short, n_lds, d_ctl, q_wave, q_lds, q_heavy);
            KOMB_HIP(ctx, hipGetLastError());
            KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(GlCtl)));
            bufs.release(d_akey == skey ? d_akey_alt : d_akey);              // (the sort's other buffer has served)

            // ---- pass 1: 4-cycles per edge
            const GlCsr g{d_rowptr, d_col, d_plen, eid};
            const uint32_t nw = h.n_wave < un ? h.n_wave : un, nl = h.n_lds < un ? h.n_lds : un, nh = h.n_heavy < un ? h.n_heavy : un;
            if (nw) {
                const int64_t gw = ((int64_t)nw + kBlock / kWave - 1) / (kBlock / kWave);
                k_gl_cyc_wave<<<(int)(gw < kGlWaveGrid ? gw : kGlWaveGrid), kBlock, 0, s>>>(g, q_wave, nw, res.cycles4);
            }
            if (nl) k_gl_cyc_lds<<<(int)(nl < (uint32_t)kGlLdsGrid ? nl : (uint32_t)kGlLdsGrid), kBlock, 0, s>>>(g, q_lds, nl, res.cycles4);
            if (nh) {
                uint32_t *d_dense = nullptr;
                KOMB_HIP(ctx, bufs.alloc(&d_dense, (size_t)kGlSlots * nv));
                KOMB_HIP(ctx, hipMemsetAsync(d_dense, 0, (size_t)kGlSlots * nv * sizeof(uint32_t), s));
                for (uint32_t first = 0; first < nh; first += kGlSlots) {
                    const dim3 grid(kGlParts, nh - first < (uint32_t)kGlSlots ? nh - first : (uint32_t)kGlSlots);
                    k_gl_cyc_heavy<0><<<grid, kBlock, 0, s>>>(g, q_heavy, first, nh, d_dense, un, res.cycles4);
                    k_gl_cyc_heavy<1><<<grid, kBlock, 0, s>>>(g, q_heavy, first, nh, d_dense, un, res.cycles4);
                    k_gl_cyc_heavy<2><<<grid, kBlock, 0, s>>>(g, q_heavy, first, nh, d_dense, un, res.cycles4);
                }
            }
            KOMB_HIP(ctx, hipGetLastError());
            (void)hipEventRecord(e1, s);

            // ---- pass 2: triangles, 4-cliques per edge, D2
            uint32_t *d_rs = nullptr, *d_re = nullptr;
            u64 *d_d2 = nullptr, *d_acc = nullptr, *d_acc2 = nullptr;
            KOMB_HIP(ctx, bufs.alloc(&d_d2, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&d_acc, (size_t)kGlSums * nv));
            KOMB_HIP(ctx, bufs.alloc(&d_acc2, (size_t)kGlSums2 * nv));
            KOMB_HIP(ctx, hipMemsetAsync(d_d2, 0, (size_t)nv * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(d_acc, 0, (size_t)kGlSums * nv * sizeof(u64), s));
            KOMB_HIP(ctx, hipMemsetAsync(d_acc2, 0, (size_t)kGlSums2 * nv * sizeof(u64), s));
            KOMB_TRY(oriented_rows(ctx, bufs, eu, m, nullptr, &d_rs, &d_re));
            k_gl_tri<<<ge, kBlock, 0, s>>>(eu, ev, d_rs, d_re, sup, um, kGlTriShort, d_d2, res.cliques4);
            KOMB_HIP(ctx, hipGetLastError());
            (void)hipEventRecord(e2, s);

            // ---- pass 3: the sums over the edges at a vertex, the orbits, the totals
            k_gl_edge1<<<ge, kBlock, 0, s>>>(eu, ev, sup, res.cycles4, res.cliques4, um, d_deg, d_acc, (size_t)nv);
            k_gl_edge2<<<ge, kBlock, 0, s>>>(eu, ev, sup, um, d_acc, d_acc2, (size_t)nv);
            k_gl_vertex<<<gv, kBlock, 0, s>>>(un, d_deg, d_acc, d_acc2, d_d2, res.orbit, d_ctl);
            KOMB_HIP(ctx, hipGetLastError());
        }
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
        if (m > 0) {
            KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(GlCtl)));
            float f = 0.f;
            if (hipEventElapsedTime(&f, e0, e1) == hipSuccess) res.ms_cycles = (double)f;
            if (hipEventElapsedTime(&f, e1, e2) == hipSuccess) res.ms_tri = (double)f;
            if (hipEventElapsedTime(&f, e2, ctx->timer.b) == hipSuccess) res.ms_vertex = (double)f;
            const unsigned div[KOMB_GRAPHLET_TYPES] = {2, 1, 3, 2, 1, 4, 1, 2, 4};
            for (int i = 0; i < KOMB_GRAPHLET_TYPES; ++i) {
                const u128 t = ((u128)h.lo[i] + ((u128)h.hi[i] << 32)) / div[i];
                const bool sat = t > (u128)0xFFFFFFFFFFFFFFFFull;
                res.total[i] = sat ? 0xFFFFFFFFFFFFFFFFull : (uint64_t)t;
                if (sat) res.flags |= KOMB_GRAPHLET_SATURATED;
            }
            const uint64_t i64max = 0x7FFFFFFFFFFFFFFFull;
            res.cycle_items = (int64_t)(h.items < i64max ? h.items : i64max);
            res.n_triangles = (int64_t)(res.total[2] < i64max ? res.total[2] : i64max);
            res.n_cliques4 = (int64_t)(res.total[8] < i64max ? res.total[8] : i64max);
            res.n_wave = h.n_wave; res.n_lds = h.n_lds; res.n_heavy = h.n_heavy;
        }
    }
    if (ctx_flag(ctx, "GRAPHLET_DEBUG"))
        fprintf(stderr, "komb graphlets: %lld vertices, %lld edges, max degree %d, %lld walked entries, roots %lld wave / %lld lds / %lld heavy, "
                "run %.3f ms, 4-cycle pass %.3f ms, triangle pass %.3f ms, vertex pass %.3f ms\n", (long long)nv, (long long)m, res.max_degree,
                (long long)res.cycle_items, (long long)res.n_wave, (long long)res.n_lds, (long long)res.n_heavy, res.ms, res.ms_cycles,
                res.ms_tri, res.ms_vertex);
    res.done = true;
    ctx->gl = std::move(res);
    return KOMB_OK;
}

} // namespace komb
