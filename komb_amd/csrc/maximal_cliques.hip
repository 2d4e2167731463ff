// maximal_cliques.hip -- maximal-clique enumeration (komb_maximal_cliques_run): every clique of the last complete k-truss result
// that lies in no larger one and has at least k_min vertices, as a size histogram, per-vertex counts and a sorted list.
// DESIGN.md section 4.6l.
//
// Input and roots are those of max_clique.hip and clique_census.hip: the canonical edges of the result as an oriented CSR, every
// clique handled at the canonical edge (a, b) of its two smallest ids, its other vertices in P = {c > b : (a, c) and (b, c) in
// H, both of trussness >= k_min}.  Maximality also needs the EXCLUDED vertices X = {x < b, x != a : (x, a) and (x, b) in H, both
// of trussness >= k_min}: a clique through (a, b) that some x of X extends has a smaller root and is not maximal here.  The
// oriented list has no rows for them, so a run first makes the LOWER ROWS (the canonical edges sorted by (ev, eu): one key sort)
// and clq_cut_x (clique_root_dev.h) cuts X from them.  The cut by k_min is exact: a clique of >= k_min vertices and any vertex
// that extends it use only edges of trussness >= k_min, so maximal among those edges <=> maximal in H.
//
// The candidate list of a root is Q = X ++ P, ascending (X < b < P), its adjacency the bit matrix of clq_matrix, in LDS or in
// the workgroup's slot of global scratch.  One wavefront owns one root at a time and lane w owns word w of every set.  The walk
// is Bron-Kerbosch with pivoting (Tomita, Tanaka, Takahashi 2006).  A NODE is a pair (P, X) of masks over Q with the HELD
// vertices a, b and the path; the root's is (P, X) as cut.
//   * P empty: a LEAF.  The held set is reported iff X is empty and it has >= k_min vertices.
//   * |held| + |P| < k_min: nothing below reaches k_min.
//   * else a pivot u of P | X (the one with the most neighbours in P, the smallest such; or the first of P): for every v of
//     P \ row(u) in ascending order the child (P & row(v), X & row(v)), then v moves from P to X.
// The walk is iterative over an explicit stack: level d keeps its (P, X) as they stand, its pivot and the vertex the current
// child took.  The held vertices are a clique, so d + 2 <= t_max bounds the depth.
//   * A report: hist[size] in an array of the wave's own in LDS, flushed once with atomic adds; count[v] += 1 and
//     largest[v] = max(largest[v], size) by atomics; one add of size + 1 to the cursor of the word stream and (size, vertices)
//     written there -- or, past the stream's end, nothing but the overflow word.  All are read by the host after the launch.
//   * nodes: as in the search, batches of at most 256 per wave to one counter that every node reads; a wave that finds the budget
//     spent stops.  What was reported by then is a lower bound: every reported clique is maximal, none is reported twice.
// The launches of a run: k_clq_tmax; k_rows, k_mx_keys, the sort, k_mx_lower; k_mx_walk in count mode (the largest |Q| at need
// k_min, which sizes the scratch slots and the LDS; above 4096 the run is refused) and in run mode.  No workgroup waits for another.
#include "clique_root_dev.h"

#include <algorithm>
#include <numeric>

namespace komb {

namespace {

constexpr long long kMxListDefault = 65536;           // MAXIMAL_LIST
constexpr long long kMxListMax = 1ll << 24;           // its largest value, and the words of the stream at most

struct MxArgs {
    ClqGraph g;
    ClqLower low;
    uint32_t m, n_chunks;
    ClqCtl *ctl;
    bool count_only, pivot_max;
    uint32_t k_min, k_hi;
    unsigned long long budget;
    ClqLayout lay;                                    // the candidates are Q; LDS head: cur[levels], piv[levels] | hist[k_hi - k_min + 1]; two sets per stack level
    unsigned long long *hist;
    int32_t *count, *largest, *list;
    unsigned long long list_cap;                      // words of the stream
};

// ---- the lower rows: keys (ev, position) sorted, then one entry per key and the row bounds
__global__ void k_mx_keys(const int32_t *__restrict__ ev, uint32_t m, uint64_t *__restrict__ keys)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < m) keys[j] = ((uint64_t)(uint32_t)ev[j] << 32) | j;
}

__global__ void k_mx_lower(const uint64_t *__restrict__ keys, const int32_t *__restrict__ eu, uint32_t m, uint32_t nv, int32_t *__restrict__ lu,
                           uint32_t *__restrict__ lpos, uint32_t *__restrict__ ls, uint32_t *__restrict__ le, ClqCtl *ctl)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t b = (uint32_t)(keys[i] >> 32), p = (uint32_t)keys[i];
    if (b >= nv || p >= m) { ctl->bad = 1u; lu[i] = 0; lpos[i] = 0u; return; }
    lu[i] = eu[p];
    lpos[i] = p;
    if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != b) ls[b] = i;
    if (i + 1 == m || (uint32_t)(keys[i + 1] >> 32) != b) le[b] = i + 1;
}

// A maximal clique of d + 2 vertices: a, b and the d vertices of cur[].
__device__ __forceinline__ void mx_report(const MxArgs &A, unsigned long long *hist, int32_t a, int32_t b, const int32_t *Q, const volatile int32_t *cur,
                                          uint32_t d, int lane)
{
    const uint32_t s = d + 2u;
    if (s > A.k_hi) { if (lane == 0) A.ctl->bad = 1u; return; }   // (a clique of more than t_max vertices; s >= k_min: the caller checked)
    unsigned long long off = 0ull;
    if (lane == 0) {
        hist[s - A.k_min] += 1ull;
        off = atomicAdd(&A.ctl->list_words, (unsigned long long)(s + 1u));
    }
    off = clq_shfl64(off, 0);
    const bool keep = off + s + 1u <= A.list_cap;
    if (lane == 0) {
        if (keep) __hip_atomic_store(A.list + off, (int32_t)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else A.ctl->overflow = 1u;
    }
    for (uint32_t i = (uint32_t)lane; i < s; i += kWave) {
        const int32_t v = i == 0 ? a : (i == 1 ? b : Q[cur[i - 2]]);
        atomicAdd(A.count + v, 1);
        atomicMax(A.largest + v, (int32_t)s);
        if (keep) __hip_atomic_store(A.list + off + 1u + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One root: canonical edge rj = (a, b).  Every branch below is uniform over the wave.
__device__ void mx_root(const MxArgs &A, uint32_t rj, unsigned long long *smem, ClqWave &w, int lane)
{
    ClqCtl *ctl = A.ctl;
    const int32_t a = A.g.eu[rj], b = A.g.ev[rj];
    int32_t *Q = (int32_t *)clq_slot(A.lay);
    const bool fill = !A.count_only;
    const uint32_t cap_q = A.lay.cap;
    const uint32_t nx = clq_cut_x(A.g, A.low, rj, A.k_min, Q, cap_q, fill, lane);
    const uint32_t room = nx < cap_q ? cap_q - nx : 0u;
    const uint32_t np = clq_cut(A.g, rj, A.k_min, Q + (cap_q - room), room, fill, lane);
    const uint32_t n = nx + np;
    if (A.count_only) { w.max_cand = n > w.max_cand ? n : w.max_cand; return; }
    ++w.roots;
    if (n > cap_q || n > kClqMaxCand) { if (lane == 0) ctl->bad = 1u; return; }   // (the count launch saw every root at this need)
    volatile int32_t *cur = (int32_t *)smem, *piv = cur + A.lay.levels;   // (written by lane 0, read by every lane)
    unsigned long long *hist = smem + A.lay.lds_off_extra;
    if (np == 0 || np + 2u < A.k_min) {                  // the edge alone, or no clique of k_min vertices: one node, no matrix
        clq_count(ctl, w, lane);
        if (np == 0 && nx == 0 && A.k_min <= 2u) mx_report(A, hist, a, b, Q, cur, 0u, lane);
        return;
    }
    const uint32_t W = (n + 63u) >> 6;
    const ClqPlace at = clq_place(A.lay, smem, n);
    unsigned long long *mat = at.mat, *stk = at.stk;
    clq_matrix(A.g, A.k_min, Q, n, W, mat, lane);
    // ---- the walk: (P, X) is the node at level d, which holds d + 2 vertices
    const bool mine = (uint32_t)lane < W;
    const uint32_t base = (uint32_t)lane * 64u;
    unsigned long long X = mine ? clq_prefix(nx, base) : 0ull;
    unsigned long long P = mine ? clq_prefix(n, base) & ~X : 0ull;
    uint32_t d = 0;
    bool enter = true;
    for (;;) {
        uint32_t u = 0;
        if (enter) {                                     // a node
            if (!clq_node(ctl, w, A.budget, lane)) break;
            const uint32_t cnt = (uint32_t)clq_sum(__popcll(P));
            bool open = false;
            if (cnt == 0) {
                if (d + 2u >= A.k_min && !__ballot(X != 0ull)) mx_report(A, hist, a, b, Q, cur, d, lane);
            } else if (d + 2u + cnt >= A.k_min) {
                u = A.pivot_max ? clq_pivot(P, P | X, mat, W, lane) : clq_first(P);   // (of P | X; or the first of P)
                if (d + 1 >= at.levels || u >= n) { if (lane == 0) ctl->bad = 1u; break; }   // (a clique of more than t_max vertices)
                if (mine) {
                    stk[(size_t)(2 * d) * W + lane] = P;
                    stk[(size_t)(2 * d + 1) * W + lane] = X;
                }
                if (lane == 0) piv[d] = (int32_t)u;
                open = true;
            }
            if (!open) {
                if (d == 0) break;
                --d;
            }
            enter = open;
        }
        // ---- level d: its next vertex outside the pivot's row, if one is left
        if (!enter) {                                    // (back at the parent: its sets and its pivot)
            u = (uint32_t)piv[d];
            P = mine ? stk[(size_t)(2 * d) * W + lane] : 0ull;
            X = mine ? stk[(size_t)(2 * d + 1) * W + lane] : 0ull;
        }
        const unsigned long long T = mine ? P & ~mat[(size_t)u * W + lane] : 0ull;
        const uint32_t v = clq_first(T);
        if (v == kClqNone) {
            if (d == 0) break;
            --d;
            enter = false;
            continue;
        }
        if ((uint32_t)lane == (v >> 6)) { P &= ~(1ull << (v & 63u)); X |= 1ull << (v & 63u); }   // (v moves from P to X; row(v) holds no v, so the child loses it)
        if (mine) {
            stk[(size_t)(2 * d) * W + lane] = P;
            stk[(size_t)(2 * d + 1) * W + lane] = X;
            const unsigned long long row = mat[(size_t)v * W + lane];
            P &= row;
            X &= row;
        }
        if (lane == 0) cur[d] = (int32_t)v;
        ++d;
        enter = true;
    }
    __syncthreads();                                     // (the next root writes Q, mat and the stack again)
}

__global__ __launch_bounds__(kWave) void k_mx_walk(MxArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const int lane = threadIdx.x;
    ClqCtl *ctl = A.ctl;
    ClqWave w{0u, 0u, 0u, false};
    unsigned long long *hist = smem + A.lay.lds_off_extra;
    const uint32_t n_k = A.k_hi - A.k_min + 1u;
    if (!A.count_only) {                                 // (a count launch has no LDS)
        for (uint32_t i = (uint32_t)lane; i < n_k; i += kWave) hist[i] = 0ull;
        __syncthreads();
    }
    uint32_t chunk, tj;
    while (!w.stop && clq_next_chunk(ctl, A.g.tr, A.m, A.n_chunks, chunk, tj, lane)) {
        unsigned long long todo = __ballot(tj >= A.k_min);
        while (todo && !w.stop) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            if (!A.count_only && clq_nodes(ctl) >= A.budget) { w.stop = true; break; }
            mx_root(A, chunk * kWave + (uint32_t)src, smem, w, lane);
        }
    }
    if (!A.count_only) {
        __syncthreads();
        for (uint32_t i = (uint32_t)lane; i < n_k; i += kWave)
            if (hist[i]) atomicAdd(A.hist + i, hist[i]);
    }
    clq_finish(ctl, w, lane);
}

// The stream (size, vertices ...)* of n cliques as the sorted list: ascending tuples in lexicographic order, CSR style.
bool mx_sort_list(const std::vector<int32_t> &raw, size_t n, std::vector<int64_t> &offset, std::vector<int32_t> &verts)
{
    std::vector<size_t> at;
    at.reserve(n);
    std::vector<int32_t> sorted(raw);
    for (size_t p = 0; p < raw.size();) {
        const int32_t s = raw[p];
        if (s < 2 || p + 1 + (size_t)s > raw.size()) return false;
        std::sort(sorted.begin() + p + 1, sorted.begin() + p + 1 + s);
        at.push_back(p);
        p += 1 + (size_t)s;
    }
    if (at.size() != n) return false;
    std::sort(at.begin(), at.end(), [&](size_t x, size_t y) {
        return std::lexicographical_compare(sorted.begin() + x + 1, sorted.begin() + x + 1 + sorted[x], sorted.begin() + y + 1, sorted.begin() + y + 1 + sorted[y]);
    });
    offset.assign(n + 1, 0);
    verts.clear();
    verts.reserve(raw.size() - n);
    for (size_t i = 0; i < n; ++i) {
        verts.insert(verts.end(), sorted.begin() + at[i] + 1, sorted.begin() + at[i] + 1 + sorted[at[i]]);
        offset[i + 1] = (int64_t)verts.size();
    }
    return true;
}

} // namespace

// the k-truss result it needs, the budget's sign and 2 <= k_min are checked by the caller (api.cpp).  The result is built on the
// side and replaces the previous one only when the run has succeeded.
int maximal_cliques_run(komb_ctx *ctx, int32_t k_min, int64_t budget)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));     // (a whole-graph result whose endpoints no fetch has asked for yet)
    Range r_all("komb_maximal_cliques_run");
    komb_ctx::MaximalCliques res;                        // goes back to the pool unless it is installed
    const long long limit = budget == 0 ? kClqDefaultBudget : std::min<long long>(budget, kClqMaxBudget);
    const long long list_cap = clq_opt(ctx, "MAXIMAL_LIST", kMxListDefault, 0, kMxListMax);
    DevBufs bufs(ctx);
    ClqCtl h{};
    MxArgs A{};
    KOMB_HIP(ctx, bufs.alloc(&A.ctl, 1));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.count.slot(&ctx->pool), (size_t)std::max<int64_t>(2 * nv, 1) * sizeof(int32_t)));   // count[nv] | largest[nv]

    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(A.ctl, 0, sizeof(ClqCtl), s));
    if (nv > 0) KOMB_HIP(ctx, hipMemsetAsync(res.count, 0, (size_t)(2 * nv) * sizeof(int32_t), s));
    const uint32_t um = (uint32_t)m;
    if (m > 0) KOMB_TRY(clq_tmax(ctx, "komb_maximal_cliques_run", A.ctl, 0u, &h));
    const int32_t t_max = (int32_t)h.t_max;
    const int32_t k_hi = std::max(t_max, k_min);         // no clique has more than t_max vertices (and the fetch has at least one entry)
    const uint32_t n_k = (uint32_t)(k_hi - k_min + 1);
    res.k_min = k_min; res.k_hi = k_hi; res.t_max = t_max;
    res.hist.assign(n_k, 0);
    res.offset.assign(1, 0);
    res.flags = KOMB_MAXIMAL_COMPLETE | KOMB_MAXIMAL_LISTED;
    if (m > 0 && k_min <= t_max) {                       // (above t_max there is nothing to report)
        const int g = (int)((m + kBlock - 1) / kBlock);
        uint32_t *d_ls = nullptr, *d_le = nullptr, *d_lpos = nullptr;
        int32_t *d_lu = nullptr;
        uint64_t *d_keys = nullptr, *d_keys_alt = nullptr, *d_sorted = nullptr;
        KOMB_TRY(clq_rows(ctx, bufs, &A.g));
        KOMB_HIP(ctx, bufs.alloc(&d_ls, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_le, (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&d_lu, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&d_lpos, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&d_keys, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&d_keys_alt, (size_t)m));
        KOMB_HIP(ctx, bufs.alloc(&A.hist, (size_t)n_k));
        for (uint32_t *p : {d_ls, d_le}) KOMB_HIP(ctx, hipMemsetAsync(p, 0, (size_t)nv * sizeof(uint32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(A.hist, 0, (size_t)n_k * sizeof(unsigned long long), s));
        // ---- the lower rows: the canonical edges by (ev, eu); positions ascend with eu inside one ev, so (ev, position) sorts them
        k_mx_keys<<<g, kBlock, 0, s>>>(ctx->d_t_ev, um, d_keys);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_TRY(prim_sort_u64(ctx, d_keys, d_keys_alt, m, 32 + key_bits(nv), &d_sorted));
        k_mx_lower<<<g, kBlock, 0, s>>>(d_sorted, ctx->d_t_eu, um, (uint32_t)nv, d_lu, d_lpos, d_ls, d_le, A.ctl);
        KOMB_HIP(ctx, hipGetLastError());
        bufs.release(d_sorted == d_keys ? d_keys_alt : d_keys);
        A.low = ClqLower{d_lu, d_lpos, d_ls, d_le};
        A.m = um; A.n_chunks = (um + kWave - 1) / kWave;
        A.k_min = (uint32_t)k_min; A.k_hi = (uint32_t)k_hi;
        const char *pv = ctx_opt(ctx, "MAXIMAL_PIVOT");
        A.pivot_max = !(pv && strcmp(pv, "first") == 0);
        A.budget = (unsigned long long)limit;
        A.count = res.count; A.largest = res.count + nv;
        // ---- the largest |X| + |P| at need k_min
        A.count_only = true;
        const int count_grid = (int)std::min<uint32_t>(A.n_chunks, (uint32_t)kClqGrid);
        k_mx_walk<<<count_grid, kWave, 0, s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(ClqCtl)));
        if (h.bad) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_maximal_cliques_run: the lower rows are inconsistent (%lld edges)", (long long)m);
        const uint32_t max_q = h.max_cand;
        if (max_q > kClqMaxCand)
            KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_maximal_cliques_run: a root edge has %u candidates and excluded vertices of trussness >= %d; the limit is %u "
                      "(one 64-bit word per lane)", max_q, (int)k_min, kClqMaxCand);
        // ---- the slots and the LDS, sized from it
        const ClqLaunch L = clq_layout(A.lay, max_q, (uint32_t)t_max, 2, n_k, 2, (uint32_t)clq_opt(ctx, "MAXIMAL_LDS", kClqLdsCand, 0, kClqLdsCand),
                                       A.n_chunks, kClqGrid);
        if (!L.fits) KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_maximal_cliques_run: %u sizes at t_max %d do not fit the LDS of a wavefront", n_k, (int)t_max);
        KOMB_HIP(ctx, bufs.alloc(&A.lay.scratch, (size_t)L.grid * A.lay.slot_bytes));
        // the stream: a clique of s vertices takes s + 1 words, MAXIMAL_LIST cliques of t_max vertices fit unless that is more than 2^24 words
        A.list_cap = (unsigned long long)std::min<long long>(list_cap * ((long long)t_max + 1), kMxListMax);
        KOMB_HIP(ctx, bufs.alloc(&A.list, (size_t)A.list_cap));
        A.count_only = false;
        KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->cursor, 0, sizeof(uint32_t), s));
        k_mx_walk<<<L.grid, kWave, L.lds_bytes, s>>>(A);
        KOMB_HIP(ctx, hipGetLastError());
        KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(ClqCtl)));
        if (h.bad)
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_maximal_cliques_run: the walk is inconsistent (k_min %d, t_max %d, largest candidate list %u)", (int)k_min,
                      (int)t_max, max_q);
        std::vector<unsigned long long> hist(n_k);
        KOMB_HIP(ctx, staged_copy(ctx, hist.data(), A.hist, (size_t)n_k * sizeof(unsigned long long), false));
        for (uint32_t i = 0; i < n_k; ++i) res.hist[i] = (int64_t)hist[i];
        res.n_cliques = std::accumulate(res.hist.begin(), res.hist.end(), (int64_t)0);
        res.flags = h.stopped ? 0 : KOMB_MAXIMAL_COMPLETE;
        if (!h.stopped && !h.overflow && h.list_words <= A.list_cap && res.n_cliques <= list_cap) {
            std::vector<int32_t> raw((size_t)h.list_words);
            if (!raw.empty()) KOMB_HIP(ctx, staged_copy(ctx, raw.data(), A.list, raw.size() * sizeof(int32_t), false));
            if (!mx_sort_list(raw, (size_t)res.n_cliques, res.offset, res.verts))
                KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_maximal_cliques_run: the stream of %llu words does not hold %lld cliques", h.list_words, (long long)res.n_cliques);
            res.flags |= KOMB_MAXIMAL_LISTED;
        }
        res.max_q = (int32_t)max_q;
        res.n_roots = (int64_t)h.n_roots;
        res.nodes = (int64_t)h.nodes;
    }
    res.ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    for (uint32_t i = 0; i < n_k; ++i)
        if (res.hist[i]) res.omega = k_min + (int32_t)i;
    if (ctx_flag(ctx, "MAXIMAL_DEBUG"))
        fprintf(stderr, "komb maximal cliques: %lld edges, t_max %d, k_min %d, omega %d, flags %d, %lld cliques, largest candidate list %d, %lld roots, "
                "%lld nodes of %lld, run %.3f ms\n", (long long)m, res.t_max, res.k_min, res.omega, res.flags, (long long)res.n_cliques, res.max_q,
                (long long)res.n_roots, (long long)res.nodes, limit, res.ms);
    ctx->pc = {};                            // (the k-clique communities describe the list that goes)
    res.done = true;
    ctx->mx = std::move(res);
    return KOMB_OK;
}

} // namespace komb
