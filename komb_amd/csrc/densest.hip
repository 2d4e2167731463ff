// densest.hip -- densest-subgraph search with a certified upper bound (komb_densest_subgraph_run): the core density
// profile, the prune to the ceil(m*/n*)-core, integer Frank-Wolfe rounds on the pruned edge list and the best prefix of the
// load order.  DESIGN.md section 4.6f; the definition is in include/komb_accel.h.  Everything is integer arithmetic, every
// comparison of two densities a 64-bit cross-multiplication (edge and vertex counts are below 2^31), and every step's result
// is a sum, a maximum or a sort of distinct keys: nothing depends on the schedule.
//
// The launches of a run:
//   PROFILE  k_den_rows<DenHist> (+ k_den_heavy): vertices by coreness, upper-half slots by min(coreness), histogrammed in
//            LDS per workgroup and flushed once (global atomics when k_max + 1 bins do not fit); k_den_profile: suffix sums,
//            the arg-max with the exact comparator, c = ceil(m*/n*).
//   PRUNE    k_den_mark + scan: dense ids of P; k_den_rows<DenCount>: upper-half member entries per row and the largest degree
//            inside P; scan; k_den_total.  The host reads the sizes here, once (they size the edge list and the load table,
//            select the path of the rounds and answer KOMB_ERR_LIMIT before a round is queued);  k_den_rows<DenFill>: (u', v').
//   ROUNDS   grid path: k_den_round (four consecutive pairs per lane, two gathers and one atomic on the delta table per
//            pair) + k_den_fold per round, queued back to back; local path: k_den_local, one workgroup, all rounds, loads and
//            deltas in LDS.
//   EXTRACT  k_den_keys (and the largest load), prim_sort_u64, k_den_ranks, k_den_rank_hist, a 64-bit scan, k_den_prefix_part,
//            k_den_decide (prefix against best core), k_den_out (member / load in original ids, into the result's own arrays).
// The rows of the three row passes are walked in the classes of components.hip: short rows by their lane, longer ones by
// their wave, the longest queued for several workgroups.
#include "common.h"

namespace komb {

namespace {

constexpr uint32_t kDenShort = 16;          // rows up to this long: the row's own lane
constexpr uint32_t kDenHeavy = 2048;        // rows from this length on: several workgroups of k_den_heavy (rows between: their wave)
constexpr int kDenHeavyGrid = 64, kDenHeavyChunks = 8;   // k_den_heavy: rows side by side x workgroups along a row
constexpr int kDenGrid = 2048;              // row passes, reductions: at most this many workgroups, each striding
constexpr uint32_t kDenLdsBins = 4096;      // PROFILE: two histograms of up to this many bins live in LDS (32 KB)
constexpr int kDenLocalBlock = 1024;        // k_den_local: lanes of its one workgroup
constexpr int kDenPairs = 4;                // k_den_round: consecutive pairs per lane (two 16-byte loads)
// Local path, automatic choice: pruned edge lists up to this long (and loads + deltas in LDS) run all rounds in one launch.
// Measured on the MI355X (profiles/densest_paths.txt): a round of the one workgroup costs 0.29 us
// per 1000 pairs, a round of the grid path 6.3 us of launches up to 10^5 pairs; they cross near 21 000 pairs.
constexpr uint64_t kDenLocalAutoPairs = 20000;

struct DenCtl {                             // 128 bytes, zeroed before every run
    uint32_t n_heavy;                       // rows queued for k_den_heavy (reset between the passes)
    int32_t  k_best, k_prune;               // best core k*, c = ceil(m*/n*)
    uint32_t n_p;                           // |P|
    uint32_t max_deg_p;                     // largest degree inside P
    uint32_t load_max;
    int32_t  source;                        // 0: best core, 1: best prefix
    uint32_t best_i;                        // length of the best prefix
    unsigned long long m_best, n_best;      // edges, vertices of the best core
    unsigned long long m_p;                 // |E_P|
    unsigned long long best_m;              // edges of the best prefix
    unsigned long long n_sub, m_sub;
    uint32_t pad[12];
};
static_assert(sizeof(DenCtl) == 128, "DenCtl layout");

// m1 / n1 > m2 / n2, exactly (n1, n2 >= 1; all four below 2^32)
__device__ __forceinline__ bool den_denser(unsigned long long m1, unsigned long long n1, unsigned long long m2, unsigned long long n2)
{
    return m1 * n2 > m2 * n1;
}
__device__ __forceinline__ bool den_equal(unsigned long long m1, unsigned long long n1, unsigned long long m2, unsigned long long n2)
{
    return m1 * n2 == m2 * n1;
}

// ---- the three row passes: what they do with a row.  lane_row: the whole row by one lane.  row_begin / wave_part / row_end:
// a row walked by a wave (every lane of the wave calls them, i < re says whether the lane holds an entry); kHeavy: several
// waves of several workgroups share the row.

// PROFILE: hist[0 .. K) vertices by coreness, hist[K .. 2K) upper-half slots by min(coreness)
template <bool kLds>
struct DenHist {
    const int32_t *core; uint32_t K; uint32_t *g_hist;
    __device__ __forceinline__ uint32_t bin(int32_t c) const { return c < 0 ? 0u : ((uint32_t)c < K ? (uint32_t)c : K - 1u); }
    __device__ __forceinline__ void add(uint32_t *s, uint32_t idx) const { atomicAdd((kLds ? s : g_hist) + idx, 1u); }
    __device__ void begin(uint32_t *s) const
    {
        if (!kLds) return;
        for (uint32_t j = threadIdx.x; j < 2 * K; j += blockDim.x) s[j] = 0u;
        __syncthreads();
    }
    __device__ void end(uint32_t *s, DenCtl *) const
    {
        if (!kLds) return;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < 2 * K; j += blockDim.x) { const uint32_t c = s[j]; if (c) atomicAdd(g_hist + j, c); }
    }
    __device__ __forceinline__ bool member(const DenCtl *, uint32_t) const { return true; }
    __device__ __forceinline__ void vertex(uint32_t *s, const DenCtl *, uint32_t v) const { add(s, bin(core[v])); }
    __device__ __forceinline__ void on_heavy(uint32_t) const {}
    __device__ __forceinline__ void entry(uint32_t *s, int32_t cv, uint32_t v, int32_t w) const
    {
        if ((uint32_t)w <= v) return;
        const int32_t cw = core[w];
        add(s, K + bin(cw < cv ? cw : cv));
    }
    __device__ void lane_row(uint32_t *s, const DenCtl *, const int32_t *col, uint32_t v, uint32_t b, uint32_t e) const
    {
        const int32_t cv = core[v];
        for (uint32_t i = b; i < e; ++i) entry(s, cv, v, col[i]);
    }
    __device__ __forceinline__ void row_begin() const {}
    template <bool kHeavy>
    __device__ __forceinline__ void wave_part(uint32_t *s, const DenCtl *, const int32_t *col, uint32_t v, uint32_t, uint64_t i, uint32_t re) const
    {
        if (i < re) entry(s, core[v], v, col[i]);
    }
    __device__ __forceinline__ void row_end(DenCtl *, uint32_t, int32_t) const {}
};

// PRUNE, first pass: cnt[v] = entries w > v of the row with coreness(w) >= c (0 for a non-member); the largest degree inside P
struct DenCount {
    const int32_t *core; uint32_t *cnt; uint32_t *hdeg;   // hdeg[h]: degree inside P of the h-th queued row (zeroed)
    uint32_t mx, acc_up, acc_all;
    __device__ void begin(uint32_t *) { mx = 0u; }
    __device__ void end(uint32_t *, DenCtl *ctl)
    {
        const uint32_t m = wave_max(mx);
        if ((threadIdx.x & (kWave - 1)) == 0 && m > ctl->max_deg_p) atomicMax(&ctl->max_deg_p, m);   // (the word only grows: a stale read costs the atomic)
    }
    __device__ __forceinline__ bool member(const DenCtl *ctl, uint32_t v) const { return core[v] >= ctl->k_prune; }
    __device__ __forceinline__ void vertex(uint32_t *, const DenCtl *ctl, uint32_t v) const { if (core[v] < ctl->k_prune) cnt[v] = 0u; }
    __device__ __forceinline__ void on_heavy(uint32_t v) const { cnt[v] = 0u; }      // (k_den_heavy adds to it, a launch later)
    __device__ void lane_row(uint32_t *, const DenCtl *ctl, const int32_t *col, uint32_t v, uint32_t b, uint32_t e)
    {
        const int32_t c = ctl->k_prune;
        uint32_t up = 0, all = 0;
        for (uint32_t i = b; i < e; ++i) {
            const int32_t w = col[i];
            if (core[w] < c) continue;
            ++all; up += (uint32_t)w > v ? 1u : 0u;
        }
        cnt[v] = up;
        mx = all > mx ? all : mx;
    }
    __device__ __forceinline__ void row_begin() { acc_up = 0u; acc_all = 0u; }
    template <bool kHeavy>
    __device__ __forceinline__ void wave_part(uint32_t *, const DenCtl *ctl, const int32_t *col, uint32_t v, uint32_t, uint64_t i, uint32_t re)
    {
        bool q = false, up = false;
        if (i < re) { const int32_t w = col[i]; q = core[w] >= ctl->k_prune; up = q && (uint32_t)w > v; }
        acc_all += (uint32_t)__popcll(__ballot(q));
        acc_up += (uint32_t)__popcll(__ballot(up));
    }
    __device__ __forceinline__ void row_end(DenCtl *, uint32_t v, int32_t h)
    {
        if ((threadIdx.x & (kWave - 1)) != 0) return;
        if (h < 0) { cnt[v] = acc_up; mx = acc_all > mx ? acc_all : mx; }
        else { if (acc_up) atomicAdd(cnt + v, acc_up); if (acc_all) atomicAdd(hdeg + h, acc_all); }
    }
};

// PRUNE, second pass: the pairs (pid[v], pid[w]) of the entries counted above, row v's from off[v] on
struct DenFill {
    const int32_t *core; const uint32_t *pid; const uint32_t *off; uint2 *pairs; uint32_t *hcur; uint64_t m_p;   // hcur[h]: append cursor of the h-th queued row (zeroed)
    uint32_t acc;
    __device__ void begin(uint32_t *) const {}
    __device__ void end(uint32_t *, DenCtl *) const {}
    __device__ __forceinline__ bool member(const DenCtl *ctl, uint32_t v) const { return core[v] >= ctl->k_prune; }
    __device__ __forceinline__ void vertex(uint32_t *, const DenCtl *, uint32_t) const {}
    __device__ __forceinline__ void on_heavy(uint32_t) const {}
    __device__ void lane_row(uint32_t *, const DenCtl *ctl, const int32_t *col, uint32_t v, uint32_t b, uint32_t e) const
    {
        const int32_t c = ctl->k_prune;
        uint64_t pos = off[v];
        const uint32_t pu = pid[v];
        for (uint32_t i = b; i < e; ++i) {
            const int32_t w = col[i];
            if ((uint32_t)w <= v || core[w] < c) continue;
            if (pos < m_p) pairs[pos] = make_uint2(pu, pid[w]);
            ++pos;
        }
    }
    __device__ __forceinline__ void row_begin() { acc = 0u; }
    template <bool kHeavy>
    __device__ __forceinline__ void wave_part(uint32_t *, const DenCtl *ctl, const int32_t *col, uint32_t v, uint32_t h, uint64_t i, uint32_t re)
    {
        const int lane = threadIdx.x & (kWave - 1);
        bool q = false; int32_t w = 0;
        if (i < re) { w = col[i]; q = (uint32_t)w > v && core[w] >= ctl->k_prune; }
        const unsigned long long mask = __ballot(q);
        if (!mask) return;                                   // (uniform per wave)
        const uint32_t n = (uint32_t)__popcll(mask);
        uint32_t base;
        if (kHeavy) {
            uint32_t got = 0;
            if (lane == __ffsll((long long)mask) - 1) got = atomicAdd(hcur + h, n);
            base = (uint32_t)__shfl((int32_t)got, __ffsll((long long)mask) - 1);
        } else {
            base = acc; acc += n;
        }
        if (q) {
            const uint64_t pos = (uint64_t)off[v] + base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (pos < m_p) pairs[pos] = make_uint2(pid[v], pid[w]);
        }
    }
    __device__ __forceinline__ void row_end(DenCtl *, uint32_t, int32_t) const {}
};

// one lane per vertex, a workgroup over several tiles (uniform per workgroup: the ballots see whole waves)
template <class Op>
__global__ void __launch_bounds__(kBlock) k_den_rows(Op op, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, uint32_t nv,
                                                     DenCtl *ctl, int32_t *__restrict__ heavy, uint32_t heavy_cap)
{
    extern __shared__ uint32_t s_den[];
    op.begin(s_den);
    const int lane = threadIdx.x & (kWave - 1);
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < nv; base += (uint64_t)gridDim.x * kBlock) {
        const uint32_t v = (uint32_t)base + threadIdx.x;
        bool act = false;
        if (v < nv) { op.vertex(s_den, ctl, v); act = op.member(ctl, v); }
        uint32_t b = 0, e = 0;
        if (act) { b = rowptr[v]; e = rowptr[v + 1]; }
        const uint32_t deg = e - b;
        if (act && deg >= kDenHeavy) {
            const uint32_t slot = atomicAdd(&ctl->n_heavy, 1u);
            if (slot < heavy_cap) heavy[slot] = (int32_t)v;  // (cannot overflow: heavy_cap counts every row this long)
            op.on_heavy(v);
            act = false;
        }
        const bool mid = act && deg > kDenShort;
        if (act && !mid) op.lane_row(s_den, ctl, col, v, b, e);
        unsigned long long m = __ballot(mid);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t rv = (uint32_t)__shfl((int32_t)v, src);
            const uint32_t rb = (uint32_t)__shfl((int32_t)b, src), re = (uint32_t)__shfl((int32_t)e, src);
            op.row_begin();
            for (uint64_t i0 = rb; i0 < re; i0 += kWave) op.template wave_part<false>(s_den, ctl, col, rv, 0u, i0 + (uint32_t)lane, re);
            op.row_end(ctl, rv, -1);
        }
    }
    op.end(s_den, ctl);
}

// the queued rows: block (x, y) takes the rows x, x + gridDim.x, ... and of each the entries y * kBlock + lane, stepping gridDim.y * kBlock
template <class Op>
__global__ void __launch_bounds__(kBlock) k_den_heavy(Op op, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col, DenCtl *ctl,
                                                      const int32_t *__restrict__ heavy, uint32_t heavy_cap)
{
    extern __shared__ uint32_t s_den[];
    op.begin(s_den);
    uint32_t n = ctl->n_heavy;
    if (n > heavy_cap) n = heavy_cap;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave_off = threadIdx.x & ~(uint32_t)(kWave - 1);
    const uint64_t stride = (uint64_t)gridDim.y * kBlock;
    for (uint32_t h = blockIdx.x; h < n; h += gridDim.x) {
        const uint32_t v = (uint32_t)heavy[h];
        const uint32_t b = rowptr[v], e = rowptr[v + 1];
        op.row_begin();
        for (uint64_t i0 = (uint64_t)b + blockIdx.y * kBlock + wave_off; i0 < e; i0 += stride)
            op.template wave_part<true>(s_den, ctl, col, v, h, i0 + (uint32_t)lane, e);
        op.row_end(ctl, v, (int32_t)h);
    }
    op.end(s_den, ctl);
}

// n_k[k], m_k[k] = the suffix sums of the two histograms; the best core by the exact comparator (ties: the larger k); c.  One workgroup.
__global__ void __launch_bounds__(kBlock) k_den_profile(uint32_t K, const uint32_t *__restrict__ hist, long long *__restrict__ n_k, long long *__restrict__ m_k, DenCtl *ctl)
{
    __shared__ unsigned long long s_v[kBlock], s_e[kBlock], s_bm[kBlock], s_bn[kBlock];
    __shared__ int32_t s_bk[kBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t ch = (K + kBlock - 1) / kBlock;
    const uint32_t lo = t * ch < K ? t * ch : K, hi = lo + ch < K ? lo + ch : K;
    unsigned long long sv = 0, se = 0;
    for (uint32_t k = lo; k < hi; ++k) { sv += hist[k]; se += hist[K + k]; }
    s_v[t] = sv; s_e[t] = se;
    __syncthreads();
    unsigned long long av = 0, ae = 0;
    for (uint32_t j = t + 1; j < kBlock; ++j) { av += s_v[j]; ae += s_e[j]; }
    unsigned long long bm = 0, bn = 1; int32_t bk = -1;
    for (uint32_t k = hi; k > lo; --k) {                     // (descending: of equal densities the first seen has the larger k)
        av += hist[k - 1]; ae += hist[K + k - 1];
        n_k[k - 1] = (long long)av; m_k[k - 1] = (long long)ae;
        if (av && (bk < 0 || den_denser(ae, av, bm, bn))) { bm = ae; bn = av; bk = (int32_t)(k - 1); }
    }
    s_bm[t] = bm; s_bn[t] = bn; s_bk[t] = bk;
    __syncthreads();
    if (t != 0) return;
    bm = 0; bn = 1; bk = -1;
    for (int j = kBlock - 1; j >= 0; --j) {                  // (chunks descending as well)
        if (s_bk[j] < 0) continue;
        if (bk < 0 || den_denser(s_bm[j], s_bn[j], bm, bn)) { bm = s_bm[j]; bn = s_bn[j]; bk = s_bk[j]; }
    }
    if (bk < 0) { bk = 0; bm = 0; bn = 0; }
    ctl->k_best = bk; ctl->m_best = bm; ctl->n_best = bn;
    ctl->k_prune = bn ? (int32_t)((bm + bn - 1) / bn) : 0;
}

__global__ void k_den_mark(uint32_t nv, const int32_t *__restrict__ core, const DenCtl *ctl, uint32_t *__restrict__ flag)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) flag[v] = core[v] >= ctl->k_prune ? 1u : 0u;
}

// |P|, |E_P| and the queued rows' degrees inside P.  One workgroup.
__global__ void __launch_bounds__(kBlock) k_den_total(uint32_t nv, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pid,
                                                      const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                      const uint32_t *__restrict__ hdeg, uint32_t heavy_cap, DenCtl *ctl)
{
    uint32_t n = ctl->n_heavy;
    if (n > heavy_cap) n = heavy_cap;
    uint32_t mx = 0;
    for (uint32_t h = threadIdx.x; h < n; h += kBlock) { const uint32_t d = hdeg[h]; mx = d > mx ? d : mx; }
    mx = wave_max(mx);
    if ((threadIdx.x & (kWave - 1)) == 0 && mx) atomicMax(&ctl->max_deg_p, mx);
    if (threadIdx.x == 0) {
        ctl->n_p = pid[nv - 1] + flag[nv - 1];
        ctl->m_p = (unsigned long long)off[nv - 1] + cnt[nv - 1];
    }
}

__global__ void k_den_zero2(uint32_t n, uint32_t *__restrict__ a, uint32_t *__restrict__ b)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) { a[i] = 0u; b[i] = 0u; }
}

// the endpoint a pair's unit goes to: the smaller load; on equal loads u in even rounds, v in odd ones
__device__ __forceinline__ uint32_t den_pick(uint2 p, uint32_t lu, uint32_t lv, bool odd)
{
    return (lu < lv || (lu == lv && !odd)) ? p.x : p.y;
}

// one Frank-Wolfe round, grid path: every read of the round sees load[] (L_t); the units go to delta[]
// (an endpoint is below n whenever count and fill agree; the test keeps a disagreement from becoming a wild access)
__device__ __forceinline__ void den_unit(uint2 p, uint32_t n, const uint32_t *__restrict__ load, uint32_t *delta, bool odd)
{
    if (p.x >= n || p.y >= n) return;
    atomicAdd(delta + den_pick(p, load[p.x], load[p.y], odd), 1u);
}

__global__ void __launch_bounds__(kBlock) k_den_round(const uint2 *__restrict__ pairs, uint64_t m, uint32_t n, const uint32_t *__restrict__ load,
                                                      uint32_t *delta, int odd)
{
    const uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kDenPairs;
    if (i >= m) return;
    if (i + kDenPairs <= m) {
        const uint4 a = *(const uint4 *)(pairs + i), b = *(const uint4 *)(pairs + i + 2);
        const uint2 p0 = make_uint2(a.x, a.y), p1 = make_uint2(a.z, a.w), p2 = make_uint2(b.x, b.y), p3 = make_uint2(b.z, b.w);
        den_unit(p0, n, load, delta, odd);                   // (the compiler issues the eight gathers before the first atomic)
        den_unit(p1, n, load, delta, odd);
        den_unit(p2, n, load, delta, odd);
        den_unit(p3, n, load, delta, odd);
    } else {
        for (uint64_t j = i; j < m; ++j) den_unit(pairs[j], n, load, delta, odd);
    }
}

// L_(t+1) = L_t + the round's units; the delta table is clear for the next round
__global__ void k_den_fold(uint32_t n, uint32_t *__restrict__ load, uint32_t *__restrict__ delta)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t d = delta[i];
    if (d) { load[i] += d; delta[i] = 0u; }
}

// all rounds in one launch, local path: one workgroup, loads and deltas in LDS, a workgroup barrier where the grid path has a launch
__global__ void __launch_bounds__(kDenLocalBlock) k_den_local(const uint2 *__restrict__ pairs, uint32_t m, uint32_t n, int32_t iters,
                                                              uint32_t *__restrict__ load_out)
{
    extern __shared__ uint32_t s_den[];
    uint32_t *s_load = s_den, *s_delta = s_den + n;
    for (uint32_t j = threadIdx.x; j < n; j += kDenLocalBlock) { s_load[j] = 0u; s_delta[j] = 0u; }
    __syncthreads();
    for (int32_t t = 0; t < iters; ++t) {
        const bool odd = (t & 1) != 0;
        for (uint32_t i = threadIdx.x; i < m; i += kDenLocalBlock) {
            const uint2 p = pairs[i];
            if (p.x >= n || p.y >= n) continue;
            atomicAdd(s_delta + den_pick(p, s_load[p.x], s_load[p.y], odd), 1u);
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < n; j += kDenLocalBlock) { s_load[j] += s_delta[j]; s_delta[j] = 0u; }
        __syncthreads();
    }
    for (uint32_t j = threadIdx.x; j < n; j += kDenLocalBlock) load_out[j] = s_load[j];
}

// EXTRACT: one key per member, (inverted load, dense id): ascending keys are (load descending, id ascending); the largest load
__global__ void __launch_bounds__(kBlock) k_den_keys(uint32_t n, const uint32_t *__restrict__ load, uint64_t *__restrict__ keys, DenCtl *ctl)
{
    uint32_t mx = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t l = load[i];
        keys[i] = ((uint64_t)(0xFFFFFFFFu - l) << 32) | (uint32_t)i;
        mx = l > mx ? l : mx;
    }
    mx = wave_max(mx);
    if ((threadIdx.x & (kWave - 1)) == 0 && mx > ctl->load_max) atomicMax(&ctl->load_max, mx);
}

__global__ void k_den_ranks(uint32_t n, const uint64_t *__restrict__ sorted, uint32_t *__restrict__ rank, uint32_t *__restrict__ hist)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t id = (uint32_t)(sorted[j] & 0xFFFFFFFFull);
    if (id < n) rank[id] = j;
    hist[j] = 0u;
}

// hist[max(rank u, rank v)] += 1: the prefix that first holds both ends of the pair
__global__ void k_den_rank_hist(const uint2 *__restrict__ pairs, uint64_t m, uint32_t n, const uint32_t *__restrict__ rank, uint32_t *hist)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint2 p = pairs[i];
    if (p.x >= n || p.y >= n) return;
    const uint32_t ru = rank[p.x], rv = rank[p.y];
    const uint32_t r = ru > rv ? ru : rv;
    if (r < n) atomicAdd(hist + r, 1u);
}

// every workgroup's best prefix (most edges per vertex, exactly; ties: the shorter): part[2 * block] = edges, [2 * block + 1] = length
__global__ void __launch_bounds__(kBlock) k_den_prefix_part(uint32_t n, const uint32_t *__restrict__ hist, const unsigned long long *__restrict__ excl,
                                                            unsigned long long *__restrict__ part)
{
    __shared__ unsigned long long s_m[kBlock], s_i[kBlock];
    unsigned long long bm = 0, bi = 0;                       // (bi == 0: none yet)
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {   // (ascending: of equal densities the first seen is the shorter)
        const unsigned long long mi = excl[j] + hist[j], len = j + 1;
        if (!bi || den_denser(mi, len, bm, bi)) { bm = mi; bi = len; }
    }
    s_m[threadIdx.x] = bm; s_i[threadIdx.x] = bi;
    __syncthreads();
    if (threadIdx.x != 0) return;
    bm = 0; bi = 0;
    for (int t = 0; t < kBlock; ++t) {
        const unsigned long long mi = s_m[t], len = s_i[t];
        if (!len) continue;
        if (!bi || den_denser(mi, len, bm, bi) || (den_equal(mi, len, bm, bi) && len < bi)) { bm = mi; bi = len; }
    }
    part[2 * blockIdx.x] = bm; part[2 * blockIdx.x + 1] = bi;
}

// the best prefix of all (n_part == 0: there is none), and whether it is strictly denser than the best core.  One lane.
__global__ void k_den_decide(uint32_t n_part, const unsigned long long *__restrict__ part, DenCtl *ctl)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    unsigned long long bm = 0, bi = 0;
    for (uint32_t t = 0; t < n_part; ++t) {
        const unsigned long long mi = part[2 * t], len = part[2 * t + 1];
        if (!len) continue;
        if (!bi || den_denser(mi, len, bm, bi) || (den_equal(mi, len, bm, bi) && len < bi)) { bm = mi; bi = len; }
    }
    const unsigned long long cm = ctl->m_best, cn = ctl->n_best;
    const bool prefix = bi && (cn == 0 || den_denser(bm, bi, cm, cn));
    ctl->best_m = bm; ctl->best_i = (uint32_t)bi;
    ctl->source = prefix ? 1 : 0;
    ctl->n_sub = prefix ? bi : cn;
    ctl->m_sub = prefix ? bm : cm;
}

// member[] and load[] in original ids (load / rank: null when no round ran)
__global__ void k_den_out(uint32_t nv, const int32_t *__restrict__ core, const uint32_t *__restrict__ pid, const uint32_t *__restrict__ load,
                          const uint32_t *__restrict__ rank, const DenCtl *ctl, int32_t *__restrict__ member, int32_t *__restrict__ load_out)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int32_t c = core[v];
    const bool in_p = c >= ctl->k_prune;
    const uint32_t i = in_p ? pid[v] : 0u;
    bool mem;
    if (ctl->source == 1 && rank) mem = in_p && rank[i] < ctl->best_i;
    else mem = c >= ctl->k_best;
    member[v] = mem ? 1 : 0;
    load_out[v] = in_p && load ? (int32_t)load[i] : 0;
}

inline int den_grid(uint64_t n) { return (int)((n + kBlock - 1) / kBlock); }
inline int den_grid_capped(uint64_t n) { const uint64_t g = (n + kBlock - 1) / kBlock; return (int)(g < 1 ? 1 : (g < (uint64_t)kDenGrid ? g : (uint64_t)kDenGrid)); }

template <class Op>
void den_row_pass(komb_ctx *ctx, Op op, size_t lds_bytes, DenCtl *d_ctl, int32_t *d_heavy, uint32_t heavy_cap)
{
    hipStream_t s = ctx->stream;
    (void)hipMemsetAsync(&d_ctl->n_heavy, 0, sizeof(uint32_t), s);
    k_den_rows<Op><<<den_grid_capped((uint64_t)ctx->nv), kBlock, lds_bytes, s>>>(op, ctx->d_o_rowptr, ctx->d_o_col, (uint32_t)ctx->nv, d_ctl, d_heavy, heavy_cap);
    k_den_heavy<Op><<<dim3(kDenHeavyGrid, kDenHeavyChunks), kBlock, lds_bytes, s>>>(op, ctx->d_o_rowptr, ctx->d_o_col, d_ctl, d_heavy, heavy_cap);
}

} // namespace

// the graph, iters >= 0 and the k-core result are checked by the caller (api.cpp)
int densest_run(komb_ctx *ctx, int32_t iters)
{
    const int64_t nv = ctx->nv;
    hipStream_t s = ctx->stream;
    if (!ctx->dens.member) {                                 // the result's own arrays: pool blocks, kept until the graph goes
        DevArr<int32_t> a, b;                                // (both or neither)
        KOMB_HIP(ctx, ctx->pool.get((void **)a.slot(&ctx->pool), (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t)));
        KOMB_HIP(ctx, ctx->pool.get((void **)b.slot(&ctx->pool), (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t)));
        ctx->dens.member = std::move(a); ctx->dens.load = std::move(b);
    }
    if (nv == 0) {
        komb_ctx::Densest r;                                 // an empty summary on the arrays the context holds
        r.member = std::move(ctx->dens.member); r.load = std::move(ctx->dens.load);
        r.iters = iters; r.profile.assign(2, 0); r.done = true;
        ctx->dens = std::move(r);
        return KOMB_OK;
    }

    Range r_all("komb_densest_subgraph_run");
    DevBufs bufs(ctx);
    const int32_t k_max = ctx->stats.max_coreness > 0 ? ctx->stats.max_coreness : 0;
    const uint32_t K = (uint32_t)k_max + 1u;
    const uint32_t heavy_cap = (uint32_t)((2 * ctx->ne) / kDenHeavy + 64);
    const int grid = den_grid((uint64_t)nv);

    DenCtl *d_ctl = nullptr; int32_t *d_heavy = nullptr;
    uint32_t *d_hist = nullptr, *d_flag = nullptr, *d_pid = nullptr, *d_cnt = nullptr, *d_off = nullptr, *d_hdeg = nullptr, *d_hcur = nullptr;
    long long *d_prof = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
    KOMB_HIP(ctx, bufs.alloc(&d_heavy, (size_t)heavy_cap));
    KOMB_HIP(ctx, bufs.alloc(&d_hdeg, (size_t)heavy_cap));
    KOMB_HIP(ctx, bufs.alloc(&d_hcur, (size_t)heavy_cap));
    KOMB_HIP(ctx, bufs.alloc(&d_hist, (size_t)2 * K));
    KOMB_HIP(ctx, bufs.alloc(&d_prof, (size_t)2 * K));
    KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&d_pid, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&d_cnt, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&d_off, (size_t)nv));

    // ---- PROFILE and the sizes of the prune
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(DenCtl), s));
    KOMB_HIP(ctx, hipMemsetAsync(d_hist, 0, (size_t)2 * K * sizeof(uint32_t), s));
    KOMB_HIP(ctx, hipMemsetAsync(d_hdeg, 0, (size_t)heavy_cap * sizeof(uint32_t), s));
    KOMB_HIP(ctx, hipMemsetAsync(d_hcur, 0, (size_t)heavy_cap * sizeof(uint32_t), s));
    if (K <= kDenLdsBins) den_row_pass(ctx, DenHist<true>{ctx->core.core, K, d_hist}, (size_t)2 * K * sizeof(uint32_t), d_ctl, d_heavy, heavy_cap);
    else den_row_pass(ctx, DenHist<false>{ctx->core.core, K, d_hist}, 0, d_ctl, d_heavy, heavy_cap);
    k_den_profile<<<1, kBlock, 0, s>>>(K, d_hist, d_prof, d_prof + K, d_ctl);
    k_den_mark<<<grid, kBlock, 0, s>>>((uint32_t)nv, ctx->core.core, d_ctl, d_flag);
    KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_pid, nv));
    den_row_pass(ctx, DenCount{ctx->core.core, d_cnt, d_hdeg, 0u, 0u, 0u}, 0, d_ctl, d_heavy, heavy_cap);
    KOMB_TRY(prim_exclusive_sum_u32(ctx, d_cnt, d_off, nv));
    k_den_total<<<1, kBlock, 0, s>>>((uint32_t)nv, d_flag, d_pid, d_cnt, d_off, d_hdeg, heavy_cap, d_ctl);
    double ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    DenCtl h;
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(DenCtl)));      // the sizes: the one read before the rounds
    std::vector<int64_t> profile((size_t)2 * K);
    KOMB_HIP(ctx, d2h(ctx, profile.data(), d_prof, profile.size() * sizeof(int64_t)));
    const uint64_t n_p = h.n_p, m_p = h.m_p;
    if (n_p > (uint64_t)nv || m_p > (uint64_t)ctx->ne)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_densest_subgraph_run: inconsistent state (%llu of %lld vertices, %llu of %lld edges)",
                  (unsigned long long)n_p, (long long)nv, (unsigned long long)m_p, (long long)ctx->ne);
    if ((uint64_t)iters * h.max_deg_p > (uint64_t)INT32_MAX)
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_densest_subgraph_run: %d rounds on a vertex of degree %u inside the pruned set overflow the 32-bit load word",
                  iters, h.max_deg_p);

    // ---- the pruned edge list, the rounds, the extraction
    const bool rounds = iters >= 1 && m_p > 0;               // (without an edge in P every load stays 0 and no prefix beats the best core)
    uint2 *d_pairs = nullptr; uint32_t *d_load = nullptr, *d_delta = nullptr, *d_rank = nullptr, *d_rhist = nullptr;
    uint64_t *d_keys = nullptr, *d_keys2 = nullptr;
    unsigned long long *d_excl = nullptr, *d_part = nullptr;
    const int part_grid = den_grid_capped(n_p);
    bool local = false;
    if (rounds) {
        KOMB_HIP(ctx, bufs.alloc(&d_pairs, (size_t)m_p + kDenPairs));
        KOMB_HIP(ctx, bufs.alloc(&d_load, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_delta, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_rank, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_rhist, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_keys, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_keys2, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_excl, (size_t)n_p));
        KOMB_HIP(ctx, bufs.alloc(&d_part, (size_t)2 * part_grid));
        // option DENSEST_LOCAL: 0 = never the local path, 1 = whenever loads + deltas fit in LDS, unset = automatic
        int lds_cap = 0;
        KOMB_HIP(ctx, hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
        const bool fits = n_p * 2 * sizeof(uint32_t) <= (uint64_t)(lds_cap > 0 ? lds_cap : 0) && m_p <= 0xFFFFFFFFull;
        const char *lo = ctx_opt(ctx, "DENSEST_LOCAL");
        local = fits && (lo ? strcmp(lo, "0") != 0 : m_p <= kDenLocalAutoPairs);
        if (local)
            KOMB_HIP(ctx, hipFuncSetAttribute((const void *)k_den_local, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(n_p * 2 * sizeof(uint32_t))));
    }
    ctx->timer.start(s);
    if (rounds) {
        den_row_pass(ctx, DenFill{ctx->core.core, d_pid, d_off, d_pairs, d_hcur, m_p, 0u}, 0, d_ctl, d_heavy, heavy_cap);
        if (local) {
            k_den_local<<<1, kDenLocalBlock, (size_t)n_p * 2 * sizeof(uint32_t), s>>>(d_pairs, (uint32_t)m_p, (uint32_t)n_p, iters, d_load);
        } else {
            const int rgrid = den_grid((m_p + kDenPairs - 1) / kDenPairs), ngrid = den_grid(n_p);
            k_den_zero2<<<ngrid, kBlock, 0, s>>>((uint32_t)n_p, d_load, d_delta);
            for (int32_t t = 0; t < iters; ++t) {            // queued back to back: no read and no wait in this loop
                k_den_round<<<rgrid, kBlock, 0, s>>>(d_pairs, m_p, (uint32_t)n_p, d_load, d_delta, t & 1);
                k_den_fold<<<ngrid, kBlock, 0, s>>>((uint32_t)n_p, d_load, d_delta);
            }
        }
        KOMB_HIP(ctx, hipGetLastError());
        k_den_keys<<<part_grid, kBlock, 0, s>>>((uint32_t)n_p, d_load, d_keys, d_ctl);
        uint64_t *sorted = nullptr;
        KOMB_TRY(prim_sort_u64(ctx, d_keys, d_keys2, (int64_t)n_p, 64, &sorted));
        k_den_ranks<<<den_grid(n_p), kBlock, 0, s>>>((uint32_t)n_p, sorted, d_rank, d_rhist);
        k_den_rank_hist<<<den_grid(m_p), kBlock, 0, s>>>(d_pairs, m_p, (uint32_t)n_p, d_rank, d_rhist);
        KOMB_TRY(prim_exclusive_sum_u32_u64(ctx, d_rhist, d_excl, (int64_t)n_p));
        k_den_prefix_part<<<part_grid, kBlock, 0, s>>>((uint32_t)n_p, d_rhist, d_excl, d_part);
    }
    k_den_decide<<<1, kWave, 0, s>>>(rounds ? (uint32_t)part_grid : 0u, d_part, d_ctl);
    KOMB_HIP(ctx, hipGetLastError());
    // from here on the previous result is overwritten
    k_den_out<<<grid, kBlock, 0, s>>>((uint32_t)nv, ctx->core.core, d_pid, d_load, d_rank, d_ctl, ctx->dens.member, ctx->dens.load);
    ms += ctx->timer.stop(s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = d2h(ctx, &h, d_ctl, sizeof(DenCtl));
    if (e != hipSuccess) { ctx->dens.done = false; KOMB_HIP(ctx, e); }
    komb_ctx::Densest &r = ctx->dens;
    r.source = h.source; r.k_best = h.k_best; r.k_prune = h.k_prune; r.iters = iters; r.k_max = k_max;
    r.n_pruned = (int64_t)n_p; r.m_pruned = (int64_t)m_p; r.n_sub = (int64_t)h.n_sub; r.m_sub = (int64_t)h.m_sub;
    r.load_max = (int64_t)h.load_max; r.ms = ms; r.local = local;
    r.profile.swap(profile);
    r.done = true;
    return KOMB_OK;
}

} // namespace komb
