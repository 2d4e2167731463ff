// nucleus_hierarchy.hip -- the (3,4)-nuclei as connected classes and their nesting forest over all k
// (komb_nucleus_hierarchy_run): which k-nucleus lies inside which (k-1)-nucleus.  DESIGN.md section 4.6i; the definition is
// in include/komb_accel.h.
//
// community_hierarchy.hip's level-descending LINK / CLAIM / ADOPT one rung up: the ITEMS are the triangles of the stored
// nucleus result (ids in ascending (a, b, c) order), bucketed by their own theta; the LINKS are 4-clique records of weight
// w = the smallest theta of the clique's four triangles -- the level at which the clique starts to bind.  komb_nucleus_run
// drops its clique records with its scratch, so the cliques are enumerated ONCE more here, by nucleus.hip's search
// (nucleus_search_dev.h: the shortest of three tails walked, the other two bisected, the ids of the other three triangles by
// bisection in c[] through a rebuilt tri_ptr), into a record stream whose length the stored result gives exactly
// (n_cliques4): there is no counting pass, a wave takes its slots with one returning atomic, and a cursor that does not end
// on n_cliques4 fails the run.  The stream is sorted by w (a sort of (w, slot) pairs; LINK reads its records through the
// sorted slots), the bucket boundaries are read by the host once, and the loop behind them reads nothing back.
//
// One union-find over triangle ids (unionfind_dev.h: a root is the smallest id of its tree, so it is the rep) takes the levels
// from theta_max down to 1: after the records of weight >= k are linked its trees are the k-nuclei.  A triangle of theta = k
// lies in at least k cliques whose other triangles all have theta >= k, records of weight exactly k; it was alone before, so
// the tree it ends the level in holds a triangle hooked at this level.  Hence the roots of the hooked triangles are this
// level's nodes, every node owns a hooked triangle, there are at most n_members nodes, and nothing is counted first.
//
// Per populated level three launches, a kernel boundary between them (the names and the LDS sums are community_hierarchy.hip's):
//   LINK   one lane per record of the level: (t0, t1), (t0, t2), (t0, t3); the hooks go to the log, slots taken per WAVE
//   CLAIM  for every hooked x: cnt[root] += cnt[x]; one lane per root makes the node (k, root); for every triangle of the
//          level: cnt[root] += 1.  What goes to the root the workgroup's first entry has is summed in LDS first
//   ADOPT  parents of the nodes the hooked triangles stood for; node and shell of the level's triangles; a node's size
// The tail: nodes sorted by (k, rep), ranks, parents, roots and a guarded depth walk.
// Every ballot sits in a loop whose bounds are uniform over its wave; every device loop runs over a row part or a length
// fixed before its launch; every access to parent[] is a relaxed agent-scope atomic, and the labels are read by a later
// store-free launch (the header comment of components.hip says why).
#include "common.h"
#include "nucleus_search_dev.h"
#include "unionfind_dev.h"

namespace komb {

namespace {

constexpr uint32_t kNhShort = 16;           // walked tail up to this long: the triangle's own lane (option NUC_SHORT, as in nucleus.hip)
constexpr int kNhStepGrid = 2048;           // k_nh_claim / k_nh_adopt: at most this many workgroups, each striding

struct NhCtl {                              // 64 bytes, zeroed before every run
    uint32_t rec_n;                         // clique records written so far
    uint32_t n_members;                     // triangles with theta >= 1
    uint32_t log_n;                         // hooked triangles so far
    uint32_t n_nodes;                       // nodes so far
    uint32_t n_roots;                       // tail: nodes without a parent
    int32_t  depth;                         // tail: most nodes on a path from a root down
    uint32_t bad;                           // a position or a triangle id that a bisection did not find (cannot happen; checked)
    uint32_t pad[9];
};
static_assert(sizeof(NhCtl) == 64, "NhCtl layout");

struct NhNodes { int32_t *k, *rep, *par; uint32_t *size, *shell; };   // nodes in the order they were made / in final order

struct NhStream { uint32_t *keys, *idx; uint4 *recs; uint32_t cap; };  // record slot q: weight | q | the four triangle ids

inline int nh_grid(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }
inline int nh_bits(uint32_t levels) { int b = 1; while (b < 32 && (1u << b) < levels) ++b; return b; }

__device__ __forceinline__ uint32_t nh_wave_sum(uint32_t v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int32_t)v, o);
    return v;
}
__device__ __forceinline__ uint32_t nh_wave_max(uint32_t v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int32_t)v, o); v = other > v ? other : v; }
    return v;
}

// ---- the search structures of nucleus.hip, rebuilt from the stored a, b, c and the canonical edge list

// row bounds per original vertex (rs / re zeroed before: a vertex without a row has an empty one)
__global__ void k_nh_rows(const int32_t *__restrict__ eu, uint32_t m, uint32_t *__restrict__ rs, uint32_t *__restrict__ re)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const int32_t u = eu[j];
    if (j == 0 || eu[j - 1] != u) rs[u] = j;
    if (j + 1 == m || eu[j + 1] != u) re[u] = j + 1;
}

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

// the id of the triangle of the edge at position e whose third vertex is d: a bisection in e's ascending part of tc[]
__device__ __forceinline__ uint32_t nh_tri_id(const uint32_t *__restrict__ tri_ptr, const int32_t *__restrict__ tc, uint32_t e, int32_t d,
                                              uint32_t fallback, NhCtl *ctl)
{
    uint32_t lo = tri_ptr[e];
    const uint32_t end = tri_ptr[e + 1];
    uint32_t hi = end;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tc[mid] < d) lo = mid + 1; else hi = mid;
    }
    if (lo < end && tc[lo] == d) return lo;
    ctl->bad = 1u;                                       // (three edges of the result that close a triangle the result does not hold)
    return fallback;
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
    r.y = nh_tri_id(tri_ptr, o.c, o.j[t], d, t, ctl);        // (a, b, d)
    r.z = nh_tri_id(tri_ptr, o.c, o.pac[t], d, t, ctl);      // (a, c, d)
    r.w = nh_tri_id(tri_ptr, o.c, o.pbc[t], d, t, ctl);      // (b, c, d)
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
    const uint32_t top = nh_wave_max(own);                               // (uniform per wave)
    for (uint32_t i = 0; i < top; ++i) {
        const bool hit = i < own && nuc_clq_entry(ev, s, s.it + i);
        nh_emit(hit, t, s.it + i, ev, o, tri_ptr, theta, ctl, st);
    }
    unsigned long long todo = __ballot(mid);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t rt = (uint32_t)__shfl((int32_t)t, src);
        NucTails r;
        r.it = (uint32_t)__shfl((int32_t)s.it, src); r.n = (uint32_t)__shfl((int32_t)s.n, src);
        r.lo1 = (uint32_t)__shfl((int32_t)s.lo1, src); r.hi1 = (uint32_t)__shfl((int32_t)s.hi1, src);
        r.lo2 = (uint32_t)__shfl((int32_t)s.lo2, src); r.hi2 = (uint32_t)__shfl((int32_t)s.hi2, src);
        for (uint32_t x0 = r.it; x0 < r.it + r.n; x0 += kWave) {         // (uniform per wave)
            const uint32_t x = x0 + (uint32_t)lane;
            const bool hit = x < r.it + r.n && nuc_clq_entry(ev, r, x);
            nh_emit(hit, rt, x, ev, o, tri_ptr, theta, ctl, st);
        }
    }
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

// off[k] = the first position of the sorted keys with a key >= k, for k = 0 .. levels (every word written exactly once)
__global__ void k_nh_offsets(uint32_t n, const uint32_t *__restrict__ keys, uint32_t levels, uint32_t *__restrict__ off)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    const uint32_t first = i > 0 ? keys[i - 1] + 1u : 0u;
    const uint32_t last = i < n ? keys[i] : levels;
    for (uint32_t k = first; k <= last && k <= levels; ++k) off[k] = i;
}

// ---- the levels

// a wave's hooks into the log, its slots taken at once.  Every lane of the wave calls it.
__device__ __forceinline__ void nh_log(int32_t hooked, NhCtl *ctl, int32_t *__restrict__ log, uint32_t cap)
{
    const unsigned long long m = __ballot(hooked >= 0);
    if (!m) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int lead = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(&ctl->log_n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int32_t)base, lead);
    if (hooked < 0) return;
    const uint32_t slot = base + (uint32_t)__popcll(m & nuc_below(lane));
    if (slot < cap) log[slot] = hooked;      // (cannot overflow: a triangle is hooked once, and only members are linked)
}

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
    nh_log(h0, ctl, log, cap); nh_log(h1, ctl, log, cap); nh_log(h2, ctl, log, cap);
}

// arr[key] += 1 for every lane with key >= 0: the lanes of a wave that share a key add once, and what goes to `first` is
// summed in *s_sum (LDS) for the workgroup's one global atomic.  Every lane of the wave calls it.
__device__ __forceinline__ void nh_group_add(uint32_t *arr, int32_t key, int32_t first, uint32_t *s_sum)
{
    const int lane = threadIdx.x & (kWave - 1);
    const bool act = key >= 0;
    unsigned long long m = __ballot(act);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        const int32_t lead = __shfl(key, src);
        const unsigned long long same = __ballot(act && key == lead);
        if (lane == src) {
            if (lead == first) atomicAdd(s_sum, (uint32_t)__popcll(same));
            else atomicAdd(arr + lead, (uint32_t)__popcll(same));
        }
        m &= ~same;
    }
}

// the node (k, r) of root r, made by the first lane that asks for it at this level (levels descend: the atomicMin tells it)
__device__ __forceinline__ void nh_claim(int32_t r, int32_t k, NhCtl *ctl, int32_t *claimk, int32_t *cur, const NhNodes &t, uint32_t cap)
{
    if (pload(claimk + r) <= k) return;      // (the word only falls: a stale read costs the atomic, no more)
    if (atomicMin(claimk + r, k) <= k) return;
    const uint32_t id = atomicAdd(&ctl->n_nodes, 1u);
    if (id >= cap) return;                   // (cannot happen: every node has a hooked triangle of its own; the host checks n_nodes)
    t.k[id] = k; t.rep[id] = r; t.par[id] = -1; t.size[id] = 0u; t.shell[id] = 0u;
    const int32_t prev = cur[r];             // cur[r] belongs to this lane: r is a root, and only its claimer touches it in this launch
    if (prev >= 0) t.par[prev] = (int32_t)id;    // the same root stood for a nucleus of a higher level: now a child
    cur[r] = (int32_t)id;
}

// CLAIM (after the level's LINK; hooks nothing: a triangle read as a root is one.  Its walks still split the paths they pass).
// seg[li] .. log_n is the level's segment of the log; mord[sh_b .. sh_b + sh_n) are the level's triangles.
__global__ void k_nh_claim(int32_t k, uint32_t li, const uint32_t *__restrict__ mord, uint32_t sh_b, uint32_t sh_n, int32_t *parent,
                           const int32_t *__restrict__ log, uint32_t *seg, NhCtl *ctl, int32_t *claimk, int32_t *cur, uint32_t *cnt,
                           NhNodes t, uint32_t cap)
{
    __shared__ int32_t s_first;
    __shared__ uint32_t s_sum;
    const uint32_t lb = seg[li];
    uint32_t le = ctl->log_n;
    if (le > cap) le = cap;
    const uint32_t b0 = blockIdx.x * kBlock, stride = gridDim.x * kBlock;
    if (b0 + threadIdx.x == 0) seg[li + 1] = le;                 // (read by later launches only)
    const int lane = threadIdx.x & (kWave - 1);
    if (threadIdx.x == 0) {                                      // the root this workgroup's first entry has
        s_first = lb + b0 < le ? comp_find(parent, log[lb + b0]) : (b0 < sh_n ? comp_find(parent, (int32_t)mord[sh_b + b0]) : -1);
        s_sum = 0u;
    }
    __syncthreads();
    const int32_t first = s_first;
    for (uint32_t base = lb + b0; base < le; base += stride) {   // (uniform per workgroup: the ballots see whole waves)
        const uint32_t i = base + threadIdx.x;
        int32_t r = -1;
        uint32_t mine = 0;
        if (i < le) {
            const int32_t x = log[i];
            r = comp_find(parent, x);
            const uint32_t c = cnt[x];       // x is no root any more: nobody adds to cnt[x] now
            if (r == first) mine = c;
            else if (c) atomicAdd(cnt + r, c);
        }
        mine = nh_wave_sum(mine);
        if (lane == 0 && mine) atomicAdd(&s_sum, mine);
        unsigned long long m = __ballot(r >= 0);                 // one lane per distinct root of the wave asks for its node
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            const int32_t lead = __shfl(r, src);
            const unsigned long long same = __ballot(r == lead);
            if (lane == src) nh_claim(lead, k, ctl, claimk, cur, t, cap);
            m &= ~same;
        }
    }
    for (uint32_t base = b0; base < sh_n; base += stride) {
        const uint32_t j = base + threadIdx.x;
        const int32_t r = j < sh_n ? comp_find(parent, (int32_t)mord[sh_b + j]) : -1;
        nh_group_add(cnt, r, first, &s_sum);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(cnt + first, s_sum);
}

// ADOPT (after CLAIM: cur[] of this level's roots is settled)
__global__ void k_nh_adopt(uint32_t li, const uint32_t *__restrict__ mord, uint32_t sh_b, uint32_t sh_n, const int32_t *parent,
                           const int32_t *__restrict__ log, const uint32_t *__restrict__ seg, const int32_t *__restrict__ cur,
                           const uint32_t *__restrict__ cnt, NhNodes t, int32_t *__restrict__ mnode)
{
    __shared__ int32_t s_first;
    __shared__ uint32_t s_sum;
    const uint32_t lb = seg[li], le = seg[li + 1];
    const uint32_t b0 = blockIdx.x * kBlock, stride = gridDim.x * kBlock;
    if (threadIdx.x == 0) {                                      // the node this workgroup's first triangle goes to
        s_first = b0 < sh_n ? cur[comp_find_ro(parent, (int32_t)mord[sh_b + b0])] : -1;
        s_sum = 0u;
    }
    __syncthreads();
    const int32_t first = s_first;
    for (uint32_t i = lb + b0 + threadIdx.x; i < le; i += stride) {
        const int32_t x = log[i];
        const int32_t r = comp_find_ro(parent, x);
        const int32_t nr = cur[r], nx = cur[x];
        if (nr < 0) continue;
        if (nx >= 0) t.par[nx] = nr;         // x was the root of a nucleus of a higher level
        t.size[nr] = cnt[r];                 // (every writer stores the same word)
    }
    for (uint32_t base = b0; base < sh_n; base += stride) {      // (uniform per workgroup)
        const uint32_t j = base + threadIdx.x;
        int32_t nr = -1;
        if (j < sh_n) {
            const int32_t e = (int32_t)mord[sh_b + j];
            const int32_t r = comp_find_ro(parent, e);
            nr = cur[r];
            mnode[e] = nr;
            if (nr >= 0) t.size[nr] = cnt[r];
        }
        nh_group_add(t.shell, nr, first, &s_sum);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum && first >= 0) atomicAdd(t.shell + first, s_sum);
}

// ---- the tail: nodes into (k, rep) order
__global__ void k_nh_node_keys(uint32_t n, NhNodes t, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((uint64_t)(uint32_t)t.k[i] << 32) | (uint32_t)t.rep[i];
    vals[i] = i;
}

__global__ void k_nh_ranks(uint32_t n, const uint32_t *__restrict__ order, int32_t *__restrict__ rank)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) rank[order[j]] = (int32_t)j;
}

__global__ void k_nh_nodes_out(uint32_t n, const uint32_t *__restrict__ order, const int32_t *__restrict__ rank, NhNodes t, NhNodes out, NhCtl *ctl)
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

// the most nodes on a path from a root down (parents have smaller numbers: every walk ends)
__global__ void k_nh_depth(uint32_t n, const int32_t *__restrict__ par, NhCtl *ctl)
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

// ---- readers of the stored forest

// komb_nucleus_hierarchy_labels: from node[t] up while the parent's level is still >= k (parents have smaller numbers:
// every walk ends)
__global__ void k_nh_labels(uint32_t n_tri, int32_t k, const int32_t *__restrict__ tnode, uint32_t n, const int32_t *__restrict__ nk,
                            const int32_t *__restrict__ rep, const int32_t *__restrict__ par, const int32_t *__restrict__ size,
                            int32_t *__restrict__ label, int32_t *__restrict__ lsize)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri) return;
    int32_t lab = -1, sz = 0;
    int32_t c = tnode[t];
    if (c >= 0 && (uint32_t)c < n && nk[c] >= k) {
        for (int32_t a = par[c]; a >= 0 && a < c && nk[a] >= k; a = par[a]) c = a;
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

inline uint32_t nh_opt_u32(const komb_ctx *ctx, const char *name, uint32_t dflt)
{
    const char *e = ctx_opt(ctx, name);
    if (!e) return dflt;
    const unsigned long v = strtoul(e, nullptr, 10);
    return v < 1 ? 1u : (v > 0x7FFFFFFFul ? 0x7FFFFFFFu : (uint32_t)v);
}

// label[] / size[] of threshold k on the device (k resolved by the caller: >= 1)
int nh_labels_dev(komb_ctx *ctx, int32_t k, int32_t *d_label, int32_t *d_size)
{
    const int64_t T = ctx->nuc.n_tri;
    const int32_t *nodes = ctx->d_nh_nodes;
    const size_t c = (size_t)ctx->nh.cap;
    k_nh_labels<<<nh_grid(T), kBlock, 0, ctx->stream>>>((uint32_t)T, k, ctx->d_nh_tnode, (uint32_t)ctx->nh.n_nodes, nodes, nodes + c, nodes + 2 * c,
                                                        nodes + 3 * c, d_label, d_size);
    KOMB_HIP(ctx, hipGetLastError());
    return KOMB_OK;
}

} // namespace

void nucleus_hierarchy_drop(komb_ctx *ctx)
{
    ctx->pool.put(ctx->d_nh_nodes); ctx->pool.put(ctx->d_nh_tnode);
    ctx->d_nh_nodes = ctx->d_nh_tnode = nullptr;
    ctx->nh_done = false;
}

// the nucleus result it needs is checked by the caller (api.cpp).  The result is built in blocks of its own and replaces the
// previous one only when the run has succeeded.
int nucleus_hierarchy_run(komb_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    const int64_t T = ctx->nuc.n_tri, Q = ctx->nuc.n_clq;

    Range r_all("komb_nucleus_hierarchy_run");
    struct Fresh {                                               // the new result: goes back to the pool unless it is installed
        komb_ctx *c; int32_t *nodes = nullptr, *tnode = nullptr;
        ~Fresh() { c->pool.put(nodes); c->pool.put(tnode); }
    } fresh{ctx};
    komb_ctx::NucleusHierarchy res;
    res.theta_max = ctx->nuc.theta_max;
    size_t cap_nodes = 1;
    KOMB_HIP(ctx, ctx->pool.get((void **)&fresh.tnode, (size_t)(T > 0 ? T : 1) * sizeof(int32_t)));

    ctx->timer.start(s);
    if (Q > 0) {
        if (T < 1 || m < 1 || res.theta_max < 1)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_run: inconsistent nucleus result (%lld cliques, %lld triangles, %lld edges, theta_max %d)",
                      (long long)Q, (long long)T, (long long)m, res.theta_max);
        DevBufs bufs(ctx);
        const uint32_t um = (uint32_t)m, uT = (uint32_t)T, uQ = (uint32_t)Q;
        const uint32_t levels = (uint32_t)res.theta_max + 1u;    // level numbers 0 .. levels - 1
        const int bits = nh_bits(levels);
        const uint32_t n_short = nh_opt_u32(ctx, "NUC_SHORT", kNhShort);      // (tests: every triangle through the wave / its lane)
        const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *theta = ctx->d_nuc_theta;

        NhCtl *d_ctl = nullptr;
        uint32_t *d_rs = nullptr, *d_re = nullptr, *tri_ptr = nullptr, *d_flag = nullptr, *d_pos = nullptr, *cnt = nullptr, *rkeys2 = nullptr, *ridx2 = nullptr;
        int32_t *parent = nullptr, *cur = nullptr, *claimk = nullptr, *mnode = nullptr;
        NucTri o{ctx->d_nuc_a, ctx->d_nuc_b, ctx->d_nuc_c, nullptr, nullptr, nullptr};
        NhStream st{nullptr, nullptr, nullptr, uQ};
        KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
        KOMB_HIP(ctx, bufs.alloc(&d_rs, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_re, (size_t)nv));
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
        KOMB_HIP(ctx, hipMemsetAsync(d_rs, 0, (size_t)nv * sizeof(uint32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(d_re, 0, (size_t)nv * sizeof(uint32_t), s));
        k_nh_rows<<<nh_grid(m), kBlock, 0, s>>>(eu, um, d_rs, d_re);
        k_nh_tri<<<nh_grid(T + 1), kBlock, 0, s>>>(uT, (uint32_t)nv, o, ev, d_rs, d_re, theta, d_flag, parent, cnt, cur, claimk, d_ctl);
        k_nh_tri_ptr<<<nh_grid(m + 1), kBlock, 0, s>>>(um, uT, o.j, tri_ptr);
        KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_pos, T + 1));
        k_nh_clq<<<nh_grid(T), kBlock, 0, s>>>(ev, d_rs, d_re, o, uT, tri_ptr, theta, d_nm, d_ctl, n_short, st);
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
        NhNodes t{};
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
        k_nh_compact<<<nh_grid(T), kBlock, 0, s>>>(uT, theta, levels, d_pos, nm, mkeys, mvals);
        uint32_t *rsorted = nullptr, *order = nullptr, *msorted = nullptr, *mord = nullptr;
        KOMB_TRY(prim_sort_pairs_u32_u32(ctx, st.keys, rkeys2, st.idx, ridx2, Q, bits, &rsorted, &order));
        k_nh_offsets<<<nh_grid(Q + 1), kBlock, 0, s>>>(uQ, rsorted, levels, d_roff);
        KOMB_TRY(prim_sort_pairs_u32_u32(ctx, mkeys, mkeys2, mvals, mvals2, nm, bits, &msorted, &mord));
        k_nh_offsets<<<nh_grid((int64_t)nm + 1), kBlock, 0, s>>>(nm, msorted, levels, d_moff);
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
        uint32_t li = 0;
        for (int32_t k = (int32_t)levels - 1; k >= 1; --k) {                        // no read and no wait in this loop
            const uint32_t sh_b = moff[k], sh_n = moff[k + 1] - moff[k];
            const uint32_t r_b = roff[k], r_n = roff[k + 1] - roff[k];
            if (!sh_n) continue;                                                    // (a record of weight k has a triangle of theta k)
            if (r_n) k_nh_link<<<nh_grid(r_n), kBlock, 0, s>>>(st.recs, order, r_b, r_n, uQ, uT, parent, d_ctl, log, nm);
            const uint64_t hooks = 3ull * r_n < nm ? 3ull * r_n : nm;               // at most this many hooks at this level
            const uint64_t work = hooks > sh_n ? hooks : sh_n;
            const int g = (int)((work + kBlock - 1) / kBlock < (uint64_t)kNhStepGrid ? (work + kBlock - 1) / kBlock : (uint64_t)kNhStepGrid);
            k_nh_claim<<<g > 0 ? g : 1, kBlock, 0, s>>>(k, li, mord, sh_b, sh_n, parent, log, seg, d_ctl, claimk, cur, cnt, t, nm);
            k_nh_adopt<<<g > 0 ? g : 1, kBlock, 0, s>>>(li, mord, sh_b, sh_n, parent, log, seg, cur, cnt, t, mnode);
            ++li;
        }
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NhCtl)));                          // the number of nodes sizes the tail
        if (h.n_nodes < 1 || h.n_nodes > nm || h.log_n > nm || h.bad)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_nucleus_hierarchy_run: inconsistent state (%u nodes, %u hooks, %u members, bad %u)",
                      h.n_nodes, h.log_n, nm, h.bad);

        // ---- the tail
        const uint32_t n = h.n_nodes;
        int32_t *rank = cur;                                     // (cur[] has served when the ranks are made; nodes <= members <= triangles)
        cap_nodes = n;
        KOMB_HIP(ctx, ctx->pool.get((void **)&fresh.nodes, 5 * cap_nodes * sizeof(int32_t)));
        NhNodes out{fresh.nodes, fresh.nodes + cap_nodes, fresh.nodes + 2 * cap_nodes,
                    (uint32_t *)fresh.nodes + 3 * cap_nodes, (uint32_t *)fresh.nodes + 4 * cap_nodes};
        uint64_t *nkeys = nullptr, *nkeys2 = nullptr, *nsorted = nullptr;
        uint32_t *norder = nullptr;
        KOMB_HIP(ctx, bufs.alloc(&nkeys, (size_t)n));
        KOMB_HIP(ctx, bufs.alloc(&nkeys2, (size_t)n));
        k_nh_node_keys<<<nh_grid(n), kBlock, 0, s>>>(n, t, nkeys, mvals);           // (the members' sort has served: n <= nm)
        KOMB_TRY(prim_sort_pairs_u64_u32(ctx, nkeys, nkeys2, mvals, mvals2, n, 32 + bits, &nsorted, &norder));
        k_nh_ranks<<<nh_grid(n), kBlock, 0, s>>>(n, norder, rank);
        k_nh_nodes_out<<<nh_grid(n), kBlock, 0, s>>>(n, norder, rank, t, out, d_ctl);
        k_nh_depth<<<nh_grid(n), kBlock, 0, s>>>(n, out.par, d_ctl);
        k_nh_tri_out<<<nh_grid(T), kBlock, 0, s>>>(uT, theta, mnode, rank, n, fresh.tnode);
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(NhCtl)));
        res.n_nodes = (int64_t)n; res.n_roots = (int64_t)h.n_roots; res.depth = h.depth; res.n_members = (int64_t)nm;
    } else {
        if (T > 0) KOMB_HIP(ctx, hipMemsetAsync(fresh.tnode, 0xFF, (size_t)T * sizeof(int32_t), s));   // no clique: no nucleus
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
    }
    if (!fresh.nodes) KOMB_HIP(ctx, ctx->pool.get((void **)&fresh.nodes, 5 * cap_nodes * sizeof(int32_t)));
    res.cap = (int64_t)cap_nodes;

    nucleus_hierarchy_drop(ctx);
    ctx->d_nh_nodes = fresh.nodes; ctx->d_nh_tnode = fresh.tnode;
    fresh.nodes = fresh.tnode = nullptr;
    ctx->nh = res;
    ctx->nh_done = true;
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
        k_nh_rep_flag<<<nh_grid(T + 1), kBlock, 0, s>>>((uint32_t)T, d_label, d_flag);
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
        k_nh_keys<<<nh_grid(T), kBlock, 0, s>>>((uint32_t)T, d_label, ctx->d_nuc_a, ctx->d_nuc_b, ctx->d_nuc_c, ctx->d_t_eu, ctx->d_t_ev,
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
        k_nh_nuclei_out<<<nh_grid(T), kBlock, 0, s>>>((uint32_t)T, d_label, d_size, d_pos, (uint32_t)n_nuc, vuniq, (uint32_t)n_v, euniq, (uint32_t)n_e,
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
