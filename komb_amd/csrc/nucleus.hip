// nucleus.hip -- the (3,4)-nucleus decomposition (komb_nucleus_run): triangles peeled by the 4-cliques they lie in, the
// third rung of the nucleus ladder of Sariyuce, Seshadhri, Pinar, Catalyurek ("Finding the hierarchy of dense subgraphs
// using nucleus decompositions", WWW 2015) after k-core (1,2) and k-truss (2,3).  DESIGN.md section 4.6h.
//
// Input: the canonical edges (eu[i] < ev[i], sorted by (eu, ev), original ids) of the last complete k-truss result, whole
// graph and vmask runs alike.  As in communities.hip the list is an oriented CSR: row a = the positions [rs[a], re[a]) with
// eu == a, their ev ascending; the search over it (sides, tails, bisection, lane and wave tiers) is oriented_search_dev.h's.
//
// The launches of a run:
//   k_rows                        row bounds
//   k_nuc_tri<count>, <fill>      triangles a < b < c from edge j = (a, b): c is in row a behind j and in row b; the shorter
//                                 side is walked, the longer one bisected.  A short side stays with the edge's lane, a medium
//                                 one is walked by its wave, a long one is queued for k_nuc_tri_heavy (several workgroups,
//                                 each a contiguous part of the side).  Counts -> exclusive sum -> tri_ptr[m + 1]; the fill
//                                 writes the third vertices ASCENDING within an edge, so id(a, b, c) = tri_ptr[pos(a, b)] +
//                                 rank of c: triangle order is (a, b, c) order, and an id is one bisection away.
//   k_nuc_clq<count>, <fill>      THE HOT PASS.  4-cliques a < b < c < d from triangle t = (a, b, c): d is behind c in rows
//                                 a and b and anywhere in row c (all of row c is above c).  The shortest of the three tails
//                                 is walked, the other two bisected; a d found in all three closes a clique, and three
//                                 bisections in tc[], on the triangle's own edges (a, b), (a, c), (b, c), give the ids of
//                                 (a, b, d), (a, c, d), (b, c, d).  One 16-byte record of four triangle ids per clique; key0
//                                 by atomicAdd.  Storage is reserved from the COUNT.
//   k_nuc_inc                     the per-triangle incidence lists (inc_ptr = exclusive sum of key0; clique ids)
//   the peel (below)              level-synchronous over the triangles with a live key
//   k_nuc_out                     edge_theta / vertex_theta by atomicMax, skipped when a relaxed read shows it cannot land
//
// The peel.  theta[t] < 0 marks a live triangle; key[t] is its number of live cliques.  A level k starts from
// k_nuc_min (k = the smallest live key) and k_nuc_collect (the live triangles with key <= k: the first frontier).  A
// sub-round is two launches: k_nuc_stamp writes theta = k on its frontier, and only then k_nuc_walk goes through the
// frontier's incidence lists -- so the walk reads stamps a PREVIOUS launch wrote and needs no hand-off inside a launch.
// A clique is retired once, by whoever wins the atomicExch on its word; its members that are still live take an atomicSub,
// and the one decrement that lands a key on exactly k appends the triangle to the next sub-round's queue (later decrements
// take it below k; it is stamped k all the same).  The host reads the 64-byte control block once per sub-round and
// launches the next, or the next level when the queue is empty.  No workgroup waits for another.  Bounds: every sub-round
// that is launched retires at least one triangle, so there are at most n_triangles of them; a triangle enters a queue
// once, so a queue of n_triangles words cannot overflow (appends are guarded all the same); the device loops run over row
// parts, incidence lists and queue lengths that are fixed before the launch.
#include "oriented_search_dev.h"

namespace komb {

namespace {

constexpr uint32_t kNucShort = 16;          // walked side up to this long: the unit's own lane
constexpr uint32_t kNucHeavy = 2048;        // triangle pass: from this length on several workgroups of k_nuc_tri_heavy (between: the wave)
constexpr int kNucHeavyGrid = 256, kNucHeavyChunks = 8;     // k_nuc_tri_heavy: edges side by side x parts of one side
constexpr int kNucSweepGrid = 2048;         // sweeps over all triangles and frontiers of unknown length: workgroups, each over several tiles
constexpr int64_t kNucMaxTri = 0x7FFFFFFFll, kNucMaxClq = 0x3FFFFFFFll;

struct NucCtl {                             // 64 bytes, zeroed before every run
    unsigned long long n_tri, n_clq;        // counted by the two count passes
    uint32_t n_heavy;                       // edges for k_nuc_tri_heavy: counted by the count pass, which sizes their queue ...
    uint32_t n_queued;                      // ... and the cursor k_nuc_queue fills it with
    uint32_t bad;                           // a triangle id that a bisection did not find (cannot happen; checked)
    int32_t kmin;                           // the level: smallest live key (k_nuc_min)
    uint32_t n_q[2];                        // entries of the two frontier queues
    uint32_t pad[6];
};
static_assert(sizeof(NucCtl) == 64, "NucCtl layout");

inline int nuc_sweep(int64_t n) { const int g = tiles_of(n); return g < 1 ? 1 : (g < kNucSweepGrid ? g : kNucSweepGrid); }

__device__ __forceinline__ void nuc_emit(const NucTri &o, uint32_t t, uint32_t j, int32_t a, int32_t b, int32_t c, uint32_t x, uint32_t hit, bool walk_a)
{
    o.a[t] = a; o.b[t] = b; o.c[t] = c;
    o.j[t] = j; o.pac[t] = walk_a ? x : hit; o.pbc[t] = walk_a ? hit : x;
}

// The triangle pass: one lane per edge.  !kFill: cnt[j] = the triangles of edge j found here (an edge with a long side: 0,
// it is counted in ctl->n_heavy and the heavy kernel adds its own), cnt[m] = 0, the total into ctl.  kFill: triangle tri_ptr[j] + r for the r-th hit, the walked side
// ascending.
template <bool kFill>
__global__ void k_nuc_tri(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                          const uint32_t *__restrict__ re, uint32_t m, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ tri_ptr,
                          NucCtl *ctl, uint32_t n_short, uint32_t n_heavy, NucTri o)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    EdgeSides s{0, 0, 0, 0, true};
    if (j < m) s = edge_sides(eu, ev, rs, re, j);
    bool act = s.n > 0;
    if (act && s.n >= n_heavy) {
        if (!kFill) atomicAdd(&ctl->n_heavy, 1u);
        act = false;
    }
    const bool mid = act && s.n > n_short;
    uint32_t mine = 0;
    if (act && !mid) {
        const int32_t a = eu[j], b = ev[j];
        const uint32_t base = kFill ? tri_ptr[j] : 0u;
        for (uint32_t x = s.it; x < s.it + s.n; ++x) {
            const int32_t c = ev[x];
            const uint32_t hit = nuc_find(ev, c, s.lo, s.hi);
            if (hit == kNucNone) continue;
            if (kFill) nuc_emit(o, base + mine, j, a, b, c, x, hit, s.walk_a);
            ++mine;
        }
    }
    wave_turns(mid, [&](int src) {
        const uint32_t rj = from_lane(j, src);
        const EdgeSides r = from_lane(s, src);
        const int32_t a = eu[rj], b = ev[rj];
        const uint32_t base = kFill ? tri_ptr[rj] : 0u;
        uint32_t run = 0;
        wave_walk_all(r.it, r.n, lane, [&](uint32_t x, bool in) {
            int32_t c = 0;
            uint32_t hit = kNucNone;
            if (in) { c = ev[x]; hit = nuc_find(ev, c, r.lo, r.hi); }
            const unsigned long long hits = __ballot(hit != kNucNone);
            if (kFill && hit != kNucNone) nuc_emit(o, base + run + (uint32_t)__popcll(hits & nuc_below(lane)), rj, a, b, c, x, hit, r.walk_a);
            run += (uint32_t)__popcll(hits);
        });
        if (lane == src) mine = run;
    });
    if (!kFill) {
        if (j <= m) cnt[j] = j < m ? mine : 0u;
        unsigned long long sum = mine;
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0 && sum) atomicAdd(&ctl->n_tri, sum);
    }
}

// the queue of the edges with a long side, sized from the count pass's n_heavy (cap); its order is whatever the atomics give
// and stays as it is for both heavy launches
__global__ void k_nuc_queue(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                            const uint32_t *__restrict__ re, uint32_t m, uint32_t n_heavy, NucCtl *ctl, uint32_t *__restrict__ heavy, uint32_t cap)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m || edge_sides(eu, ev, rs, re, j).n < n_heavy) return;
    const uint32_t slot = atomicAdd(&ctl->n_queued, 1u);
    if (slot < cap) heavy[slot] = j;                     // (the same edges the count pass counted: slot < cap)
}

// The queued edges: block (x, y) takes the edges x, x + gridDim.x, ... of the queue and of each the y-th of gridDim.y
// contiguous parts of its walked side, 256 entries at a time in ascending order.  !kFill: part[h * gridDim.y + y] = the
// hits of the part, added to cnt[j] and to the total.  kFill: the part starts behind the hits of the parts before it.
template <bool kFill>
__global__ void k_nuc_tri_heavy(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                                const uint32_t *__restrict__ re, uint32_t *cnt, const uint32_t *__restrict__ tri_ptr, NucCtl *ctl,
                                const uint32_t *__restrict__ heavy, uint32_t n_queued, uint32_t *__restrict__ part, NucTri o)
{
    __shared__ uint32_t s_w[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (uint32_t h = blockIdx.x; h < n_queued; h += gridDim.x) {
        const uint32_t j = heavy[h];
        const EdgeSides s = edge_sides(eu, ev, rs, re, j);
        const uint32_t end = s.it + s.n, seg = (s.n + gridDim.y - 1) / gridDim.y;
        uint32_t x0 = s.it + blockIdx.y * seg, x1 = x0 + seg;
        if (x0 > end) x0 = end;
        if (x1 > end) x1 = end;
        const int32_t a = eu[j], b = ev[j];
        uint32_t run = 0;
        if (kFill) {
            run = tri_ptr[j];
            for (uint32_t y = 0; y < blockIdx.y; ++y) run += part[(size_t)h * gridDim.y + y];
        }
        for (uint32_t xb = x0; xb < x1; xb += kBlock) {                    // (uniform per workgroup)
            const uint32_t x = xb + threadIdx.x;
            int32_t c = 0;
            uint32_t hit = kNucNone;
            if (x < x1) { c = ev[x]; hit = nuc_find(ev, c, s.lo, s.hi); }
            const unsigned long long hits = __ballot(hit != kNucNone);
            if (lane == 0) s_w[wave] = (uint32_t)__popcll(hits);
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (int w = 0; w < kBlock / kWave; ++w) { before += w < wave ? s_w[w] : 0u; all += s_w[w]; }
            if (kFill && hit != kNucNone) nuc_emit(o, run + before + (uint32_t)__popcll(hits & nuc_below(lane)), j, a, b, c, x, hit, s.walk_a);
            run += all;
            __syncthreads();
        }
        if (!kFill && threadIdx.x == 0) {
            part[(size_t)h * gridDim.y + blockIdx.y] = run;
            if (run) { atomicAdd(cnt + j, run); atomicAdd(&ctl->n_tri, (unsigned long long)run); }
        }
    }
}

// record q: triangle t and the three triangles its vertices make with d = ev[x].  They hang on t's own edges (a, b), (a, c),
// (b, c), so the positions of (a, d), (b, d), (c, d) the searches found are not needed again.
__device__ __forceinline__ void nuc_clq_write(const int32_t *__restrict__ ev, const NucTri &o, const uint32_t *__restrict__ tri_ptr,
                                              uint32_t t, uint32_t x, uint32_t q, uint4 *__restrict__ clq, uint32_t *key0, NucCtl *ctl)
{
    const int32_t d = ev[x];
    uint4 r;
    r.x = t;
    r.y = tri_id(tri_ptr, o.c, o.j[t], d, t, &ctl->bad);       // (a, b, d)
    r.z = tri_id(tri_ptr, o.c, o.pac[t], d, t, &ctl->bad);     // (a, c, d)
    r.w = tri_id(tri_ptr, o.c, o.pbc[t], d, t, &ctl->bad);     // (b, c, d)
    clq[q] = r;
    atomicAdd(key0 + r.y, 1u); atomicAdd(key0 + r.z, 1u); atomicAdd(key0 + r.w, 1u);
}

// The 4-clique pass: one lane per triangle; a walked tail above n_short goes through the triangle's wave.  !kFill:
// qcnt[t] = the cliques whose smallest triangle is t, qcnt[n_tri] = 0, the total into ctl.  kFill: the records at
// q_ptr[t] + r, key0 of the other three triangles by atomics, of t itself by one add of its count.
template <bool kFill>
__global__ void k_nuc_clq(const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs, const uint32_t *__restrict__ re, NucTri o,
                          uint32_t n_tri, const uint32_t *__restrict__ tri_ptr, uint32_t *__restrict__ qcnt, const uint32_t *__restrict__ q_ptr,
                          uint4 *__restrict__ clq, uint32_t *key0, NucCtl *ctl, uint32_t n_short)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    NucTails s{0, 0, 0, 0, 0, 0};
    if (t < n_tri) s = nuc_tails(o, rs, re, t);
    const bool act = s.n > 0, mid = act && s.n > n_short;
    uint32_t mine = 0;
    if (act && !mid) {
        const uint32_t base = kFill ? q_ptr[t] : 0u;
        for (uint32_t x = s.it; x < s.it + s.n; ++x) {
            if (!nuc_clq_entry(ev, s, x)) continue;
            if (kFill) nuc_clq_write(ev, o, tri_ptr, t, x, base + mine, clq, key0, ctl);
            ++mine;
        }
    }
    wave_turns(mid, [&](int src) {
        const uint32_t rt = from_lane(t, src);
        const NucTails r = from_lane(s, src);
        const uint32_t base = kFill ? q_ptr[rt] : 0u;
        uint32_t run = 0;
        wave_walk_all(r.it, r.n, lane, [&](uint32_t x, bool in) {
            const bool hit = in && nuc_clq_entry(ev, r, x);
            const unsigned long long hits = __ballot(hit);
            if (kFill && hit) nuc_clq_write(ev, o, tri_ptr, rt, x, base + run + (uint32_t)__popcll(hits & nuc_below(lane)), clq, key0, ctl);
            run += (uint32_t)__popcll(hits);
        });
        if (lane == src) mine = run;
    });
    if (kFill) {
        if (mine) atomicAdd(key0 + t, mine);
    } else {
        if (t <= n_tri) qcnt[t] = t < n_tri ? mine : 0u;
        unsigned long long sum = mine;
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0 && sum) atomicAdd(&ctl->n_clq, sum);
    }
}

// the incidence lists: clique q into the list of each of its four triangles (cur zeroed before; the order inside a list is
// whatever the atomics give -- nothing reads it as an order)
__global__ void k_nuc_inc(const uint4 *__restrict__ clq, uint32_t n_clq, const uint32_t *__restrict__ inc_ptr, uint32_t *cur, uint32_t *__restrict__ inc)
{
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n_clq) return;
    const uint4 r = clq[q];
    inc[inc_ptr[r.x] + atomicAdd(cur + r.x, 1u)] = q;
    inc[inc_ptr[r.y] + atomicAdd(cur + r.y, 1u)] = q;
    inc[inc_ptr[r.z] + atomicAdd(cur + r.z, 1u)] = q;
    inc[inc_ptr[r.w] + atomicAdd(cur + r.w, 1u)] = q;
}

// ---- the peel

__global__ void k_nuc_level_begin(NucCtl *ctl)
{
    ctl->kmin = 0x7FFFFFFF; ctl->n_q[0] = 0u; ctl->n_q[1] = 0u;
}

// kmin = the smallest key of a live triangle
__global__ void k_nuc_min(uint32_t n_tri, const int32_t *__restrict__ theta, const int32_t *__restrict__ key, NucCtl *ctl)
{
    int32_t lo = 0x7FFFFFFF;
    for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < n_tri; t += gridDim.x * kBlock)
        if (theta[t] < 0) { const int32_t k = key[t]; lo = k < lo ? k : lo; }
    for (int off = kWave / 2; off > 0; off >>= 1) { const int32_t other = __shfl_xor(lo, off); lo = other < lo ? other : lo; }
    if ((threadIdx.x & (kWave - 1)) == 0 && lo != 0x7FFFFFFF) atomicMin(&ctl->kmin, lo);
}

// the first frontier of level kmin: every live triangle whose key is not above it, one append per wave
__global__ void k_nuc_collect(uint32_t n_tri, const int32_t *__restrict__ theta, const int32_t *__restrict__ key, NucCtl *ctl, uint32_t *__restrict__ queue)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t k = ctl->kmin;
    for (uint32_t base = blockIdx.x * kBlock; base < n_tri; base += gridDim.x * kBlock) {   // (uniform per workgroup)
        const uint32_t t = base + threadIdx.x;
        const bool in = t < n_tri && theta[t] < 0 && key[t] <= k;
        const unsigned long long b = __ballot(in);
        if (!b) continue;
        uint32_t slot = 0;
        if (lane == __ffsll((long long)b) - 1) slot = atomicAdd(&ctl->n_q[0], (uint32_t)__popcll(b));
        slot = (uint32_t)__shfl((int32_t)slot, __ffsll((long long)b) - 1) + (uint32_t)__popcll(b & nuc_below(lane));
        if (in && slot < n_tri) queue[slot] = t;
    }
}

// the frontier's stamp, in a launch of its own: theta = k, no longer alive.  It also empties the queue the walk appends to.
__global__ void k_nuc_stamp(NucCtl *ctl, int sel, const uint32_t *__restrict__ queue, uint32_t n_tri, int32_t *__restrict__ theta)
{
    uint32_t n = ctl->n_q[sel];
    if (n > n_tri) n = n_tri;
    const int32_t k = ctl->kmin;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) theta[queue[i]] = k;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->n_q[sel ^ 1] = 0u;
}

// clique q seen from frontier triangle t: the first visitor retires it
__device__ __forceinline__ void nuc_retire(uint32_t q, uint32_t t, int32_t k, const uint4 *__restrict__ clq, uint32_t *dead,
                                           const int32_t *__restrict__ theta, int32_t *key, NucCtl *ctl, int nsel, uint32_t *__restrict__ next, uint32_t cap)
{
    if (atomicExch(dead + q, 1u) != 0u) return;
    const uint4 r = clq[q];
    const uint32_t u[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (u[i] == t || theta[u[i]] >= 0) continue;     // (stamped by an earlier launch: this frontier or an earlier one)
        if (atomicSub(key + u[i], 1) - 1 == k) {
            const uint32_t slot = atomicAdd(&ctl->n_q[nsel], 1u);
            if (slot < cap) next[slot] = u[i];
        }
    }
}

// the walk of a sub-round: one lane per frontier triangle; an incidence list above n_short goes through the wave
__global__ void k_nuc_walk(NucCtl *ctl, int sel, const uint32_t *__restrict__ queue, uint32_t *__restrict__ next, uint32_t n_tri,
                           const uint32_t *__restrict__ inc_ptr, const uint32_t *__restrict__ inc, const uint4 *__restrict__ clq, uint32_t *dead,
                           const int32_t *__restrict__ theta, int32_t *key, uint32_t n_short)
{
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t n = ctl->n_q[sel];
    if (n > n_tri) n = n_tri;
    const int32_t k = ctl->kmin;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {        // (uniform per workgroup: wave_turns)
        const uint32_t i = base + threadIdx.x;
        uint32_t t = 0, lo = 0, hi = 0;
        if (i < n) { t = queue[i]; lo = inc_ptr[t]; hi = inc_ptr[t + 1]; }
        const bool mid = hi - lo > n_short;
        if (!mid)
            for (uint32_t x = lo; x < hi; ++x) nuc_retire(inc[x], t, k, clq, dead, theta, key, ctl, sel ^ 1, next, n_tri);
        wave_turns(mid, [&](int src) {
            const uint32_t rt = from_lane(t, src), rlo = from_lane(lo, src), rhi = from_lane(hi, src);
            wave_walk(rlo, rhi - rlo, lane, [&](uint32_t x) { nuc_retire(inc[x], rt, k, clq, dead, theta, key, ctl, sel ^ 1, next, n_tri); });
        });
    }
}

// ---- outputs

__device__ __forceinline__ void nuc_max(int32_t *p, int32_t x)
{
    if (x > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, x);
}

__global__ void k_nuc_out(uint32_t n_tri, NucTri o, const int32_t *__restrict__ theta, int32_t *edge_theta, int32_t *vertex_theta)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri) return;
    const int32_t th = theta[t];
    nuc_max(edge_theta + o.j[t], th); nuc_max(edge_theta + o.pac[t], th); nuc_max(edge_theta + o.pbc[t], th);
    nuc_max(vertex_theta + o.a[t], th); nuc_max(vertex_theta + o.b[t], th); nuc_max(vertex_theta + o.c[t], th);
}

} // namespace

// the k-truss result it needs is checked by the caller (api.cpp).  The result is built in blocks of its own and replaces the
// previous one only when the run has succeeded.
int nucleus_run(komb_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));     // (a whole-graph result whose endpoints no fetch has asked for yet)
    Range r_all("komb_nucleus_run");
    komb_ctx::Nucleus res;                               // goes back to the pool unless it is installed
    const uint32_t n_short = ctx_opt_u32(ctx, "NUC_SHORT", kNucShort);       // (tests: every unit through the wave / the queued path)
    uint32_t n_heavy = ctx_opt_u32(ctx, "NUC_HEAVY", kNucHeavy);
    if (n_heavy <= n_short) n_heavy = n_short + 1;
    int64_t cap = kNucMaxClq;                                                // NUC_CAP (tests): a smaller clique limit
    if (const char *e = ctx_opt(ctx, "NUC_CAP")) { const long long v = strtoll(e, nullptr, 10); if (v >= 0 && v < cap) cap = v; }

    const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev;
    const uint32_t um = (uint32_t)m;
    KOMB_HIP(ctx, ctx->pool.get((void **)res.edge.slot(&ctx->pool), (size_t)m * sizeof(int32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.vertex.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
    DevBufs bufs(ctx);
    EventSet evs;
    hipEvent_t e_t0 = nullptr, e_t1 = nullptr, e_q0 = nullptr, e_q1 = nullptr, e_p1 = nullptr;
    KOMB_HIP(ctx, evs.make(&e_t0)); KOMB_HIP(ctx, evs.make(&e_t1));
    KOMB_HIP(ctx, evs.make(&e_q0)); KOMB_HIP(ctx, evs.make(&e_q1)); KOMB_HIP(ctx, evs.make(&e_p1));
    NucCtl *d_ctl = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
    NucCtl h;
    int64_t T = 0, Q = 0;
    bool timed_clq = false;

    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(NucCtl), s));
    if (m > 0) KOMB_HIP(ctx, hipMemsetAsync(res.edge, 0xFF, (size_t)m * sizeof(int32_t), s));
    if (nv > 0) KOMB_HIP(ctx, hipMemsetAsync(res.vertex, 0xFF, (size_t)nv * sizeof(int32_t), s));
    (void)hipEventRecord(e_t0, s);
    if (m > 0) {
        // ---- triangles
        uint32_t *d_rs = nullptr, *d_re = nullptr, *d_cnt = nullptr, *d_heavy = nullptr, *d_part = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&d_cnt, (size_t)m + 1));        // counts, then tri_ptr
        const NucTri none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        KOMB_TRY(oriented_rows(ctx, bufs, eu, m, nullptr, &d_rs, &d_re));
        k_nuc_tri<false><<<tiles_of(m + 1), kBlock, 0, s>>>(eu, ev, d_rs, d_re, um, d_cnt, nullptr, d_ctl, n_short, n_heavy, none);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NucCtl)));
        const uint32_t n_queued = h.n_heavy < um ? h.n_heavy : um;
        const dim3 hgrid(n_queued < (uint32_t)kNucHeavyGrid ? (n_queued ? n_queued : 1u) : (uint32_t)kNucHeavyGrid, kNucHeavyChunks);
        if (n_queued) {
            KOMB_HIP(ctx, bufs.alloc(&d_heavy, (size_t)n_queued));          // (sized from the count, as the clique storage is)
            KOMB_HIP(ctx, bufs.alloc(&d_part, (size_t)n_queued * kNucHeavyChunks));
            k_nuc_queue<<<tiles_of(m), kBlock, 0, s>>>(eu, ev, d_rs, d_re, um, n_heavy, d_ctl, d_heavy, n_queued);
            k_nuc_tri_heavy<false><<<hgrid, kBlock, 0, s>>>(eu, ev, d_rs, d_re, d_cnt, nullptr, d_ctl, d_heavy, n_queued, d_part, none);
            KOMB_HIP(ctx, hipGetLastError());
            KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NucCtl)));
        }
        if (h.n_tri > (unsigned long long)kNucMaxTri)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_nucleus_run: %llu triangles; triangle ids are limited to 2^31 - 1", h.n_tri);
        T = (int64_t)h.n_tri;
        const uint32_t uT = (uint32_t)T;
        if (T > 0) {
            uint32_t *tri_ptr = d_cnt;
            KOMB_TRY(prim_exclusive_sum_u32(ctx, d_cnt, tri_ptr, m + 1));
            NucTri o;
            KOMB_HIP(ctx, ctx->pool.get((void **)res.a.slot(&ctx->pool), (size_t)T * sizeof(int32_t)));
            KOMB_HIP(ctx, ctx->pool.get((void **)res.b.slot(&ctx->pool), (size_t)T * sizeof(int32_t)));
            KOMB_HIP(ctx, ctx->pool.get((void **)res.c.slot(&ctx->pool), (size_t)T * sizeof(int32_t)));
            KOMB_HIP(ctx, ctx->pool.get((void **)res.key0.slot(&ctx->pool), ((size_t)T + 1) * sizeof(int32_t)));   // (+ 1: the scan's last entry)
            KOMB_HIP(ctx, ctx->pool.get((void **)res.theta.slot(&ctx->pool), (size_t)T * sizeof(int32_t)));
            o.a = res.a; o.b = res.b; o.c = res.c;
            KOMB_HIP(ctx, bufs.alloc(&o.j, (size_t)T));
            KOMB_HIP(ctx, bufs.alloc(&o.pac, (size_t)T));
            KOMB_HIP(ctx, bufs.alloc(&o.pbc, (size_t)T));
            k_nuc_tri<true><<<tiles_of(m), kBlock, 0, s>>>(eu, ev, d_rs, d_re, um, nullptr, tri_ptr, d_ctl, n_short, n_heavy, o);
            if (n_queued) k_nuc_tri_heavy<true><<<hgrid, kBlock, 0, s>>>(eu, ev, d_rs, d_re, nullptr, tri_ptr, d_ctl, d_heavy, n_queued, d_part, o);
            KOMB_HIP(ctx, hipGetLastError());
            (void)hipEventRecord(e_t1, s);

            // ---- 4-cliques: count, reserve, fill, incidence lists
            uint32_t *d_qcnt = nullptr, *d_inc_ptr = nullptr, *d_cur = nullptr, *d_inc = nullptr, *d_dead = nullptr, *d_queue = nullptr;
            int32_t *d_key = nullptr;
            uint4 *d_clq = nullptr;
            uint32_t *key0 = (uint32_t *)res.key0.get();
            KOMB_HIP(ctx, bufs.alloc(&d_qcnt, (size_t)T + 1));   // counts, then q_ptr
            (void)hipEventRecord(e_q0, s);
            k_nuc_clq<false><<<tiles_of(T + 1), kBlock, 0, s>>>(ev, d_rs, d_re, o, uT, tri_ptr, d_qcnt, nullptr, nullptr, nullptr, d_ctl, n_short);
            KOMB_HIP(ctx, hipGetLastError());
            KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NucCtl)));
            if (h.n_clq > (unsigned long long)cap)
                KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_nucleus_run: %llu 4-cliques on %lld triangles; the limit is %lld (clique ids are 32-bit, four incidences each)",
                          h.n_clq, (long long)T, (long long)cap);
            Q = (int64_t)h.n_clq;
            const uint32_t uQ = (uint32_t)Q;
            KOMB_TRY(prim_exclusive_sum_u32(ctx, d_qcnt, d_qcnt, T + 1));
            KOMB_HIP(ctx, bufs.alloc(&d_clq, (size_t)Q));
            KOMB_HIP(ctx, bufs.alloc(&d_inc_ptr, (size_t)T + 1));
            KOMB_HIP(ctx, bufs.alloc(&d_cur, (size_t)T));
            KOMB_HIP(ctx, bufs.alloc(&d_inc, 4 * (size_t)Q));
            KOMB_HIP(ctx, bufs.alloc(&d_dead, (size_t)Q));
            KOMB_HIP(ctx, bufs.alloc(&d_key, (size_t)T));
            KOMB_HIP(ctx, bufs.alloc(&d_queue, 2 * (size_t)T));
            KOMB_HIP(ctx, hipMemsetAsync(key0, 0, ((size_t)T + 1) * sizeof(uint32_t), s));
            KOMB_HIP(ctx, hipMemsetAsync(d_cur, 0, (size_t)T * sizeof(uint32_t), s));
            if (Q > 0) {
                KOMB_HIP(ctx, hipMemsetAsync(d_dead, 0, (size_t)Q * sizeof(uint32_t), s));
                k_nuc_clq<true><<<tiles_of(T), kBlock, 0, s>>>(ev, d_rs, d_re, o, uT, tri_ptr, nullptr, d_qcnt, d_clq, key0, d_ctl, n_short);
            }
            KOMB_TRY(prim_exclusive_sum_u32(ctx, key0, d_inc_ptr, T + 1));
            if (Q > 0) k_nuc_inc<<<tiles_of(Q), kBlock, 0, s>>>(d_clq, uQ, d_inc_ptr, d_cur, d_inc);
            KOMB_HIP(ctx, hipGetLastError());
            (void)hipEventRecord(e_q1, s);
            timed_clq = true;

            // ---- the peel
            KOMB_HIP(ctx, hipMemcpyAsync(d_key, key0, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            KOMB_HIP(ctx, hipMemsetAsync(res.theta, 0xFF, (size_t)T * sizeof(int32_t), s));
            uint32_t *queue[2] = {d_queue, d_queue + T};
            const int sweep = nuc_sweep(T);
            int64_t remaining = T;
            while (remaining > 0) {
                k_nuc_level_begin<<<1, 1, 0, s>>>(d_ctl);
                k_nuc_min<<<sweep, kBlock, 0, s>>>(uT, res.theta, d_key, d_ctl);
                k_nuc_collect<<<sweep, kBlock, 0, s>>>(uT, res.theta, d_key, d_ctl, queue[0]);
                int sel = 0, grid = sweep;                       // (the first frontier's length is on the device only)
                bool first = true;
                for (;;) {
                    k_nuc_stamp<<<grid, kBlock, 0, s>>>(d_ctl, sel, queue[sel], uT, res.theta);
                    k_nuc_walk<<<grid, kBlock, 0, s>>>(d_ctl, sel, queue[sel], queue[sel ^ 1], uT, d_inc_ptr, d_inc, d_clq, d_dead, res.theta, d_key, n_short);
                    KOMB_HIP(ctx, hipGetLastError());
                    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NucCtl)));      // the one host read of the sub-round
                    const int64_t done = h.n_q[sel], next = h.n_q[sel ^ 1];
                    if (h.bad || done < 1 || done + next > remaining)
                        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_run: the peel is inconsistent at level %d (frontier %lld, next %lld, left %lld, bad %u)",
                                  h.kmin, (long long)done, (long long)next, (long long)remaining, h.bad);
                    remaining -= done;
                    ++res.n_subrounds;
                    if (first) { ++res.n_levels; res.theta_max = h.kmin; first = false; }
                    if (next == 0) break;
                    sel ^= 1;
                    grid = nuc_sweep(next);
                }
            }
            (void)hipEventRecord(e_p1, s);
            k_nuc_out<<<tiles_of(T), kBlock, 0, s>>>(uT, o, res.theta, res.edge, res.vertex);
            KOMB_HIP(ctx, hipGetLastError());
        }
    }
    res.ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    res.n_tri = T; res.n_clq = Q;
    if (T == 0) res.theta_max = -1;
    if (timed_clq) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, e_t0, e_t1) == hipSuccess) res.ms_tri = (double)f;
        if (hipEventElapsedTime(&f, e_q0, e_q1) == hipSuccess) res.ms_clq = (double)f;
        if (hipEventElapsedTime(&f, e_q1, e_p1) == hipSuccess) res.ms_peel = (double)f;
    }
    if (ctx_flag(ctx, "NUC_DEBUG"))
        fprintf(stderr, "komb nucleus: %lld edges, %lld triangles, %lld cliques, theta_max %d, %d levels, %lld sub-rounds, run %.3f ms, "
                "triangle pass %.3f ms, clique pass %.3f ms, peel %.3f ms\n", (long long)m, (long long)T, (long long)Q, res.theta_max,
                res.n_levels, (long long)res.n_subrounds, res.ms, res.ms_tri, res.ms_clq, res.ms_peel);
    ctx->nh = {};                            // (the nuclei and their forest index the triangles of the result that goes)
    res.done = true;
    ctx->nuc = std::move(res);
    return KOMB_OK;
}

} // namespace komb
