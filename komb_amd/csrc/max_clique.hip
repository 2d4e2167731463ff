// max_clique.hip -- maximum-clique search with a certified bound (komb_max_clique_run): omega, one witness, and -- budget
// permitting -- every maximum clique of the last complete k-truss result.  DESIGN.md section 4.6j.
//
// Input: the canonical edges (eu[i] < ev[i], sorted by (eu, ev), original ids) of that result with their trussness t[i]; their
// graph is H.  As in nucleus.hip the list is an oriented CSR: row a = the positions [rs[a], re[a]) with eu == a, ev ascending.
// K_n has trussness n on every edge, so a clique of s vertices uses only edges of trussness >= s, and omega <= t_max.
//
// A clique is searched from its ROOT, the canonical edge (a, b) of its two smallest ids: its other vertices are in
// P = {c > b : (a, c) and (b, c) in H, both of trussness >= need}, where need is the size a clique must have to matter (the
// search: best + 1; the enumeration: omega).  One wavefront owns one root at a time:
//   (P and the matrix are made by clique_root_dev.h, which the clique census shares.)
//   * P is cut from the tail of row a behind (a, b) and row b: the shorter is walked 64 entries at a time, the other bisected.
//   * The |P| x |P| adjacency (edges of trussness >= need only) becomes a bit matrix, rows of W = ceil(|P| / 64) 64-bit words,
//     in LDS up to MAXCLQ_LDS candidates and in the workgroup's slot of global scratch above.  Lane w owns word w of every row
//     and of every candidate set: |P| <= 4096 is the design limit (KOMB_ERR_LIMIT above it, checked by a count launch first).
//   * An iterative depth-first search over an explicit stack of candidate sets.  Level d holds the candidates that are adjacent
//     to the d vertices chosen so far; a NODE is one evaluation of the top set R at clique size s = d + 2:
//       - R empty: a leaf (the search: raise best; the enumeration: s == omega is a maximum clique); pop.
//       - k_need = the colours R must need for a clique through it to matter (search: best - s + 1; enumeration: omega - s).
//         |R| < k_need: pop.  Else k_need - 1 independent sets are taken off R greedily (Tomita-Seki colouring, sequential:
//         first vertex of the rest, minus its row, and again).  Nothing left: R is (k_need - 1)-colourable, pop.
//       - else the first vertex v that is left is the branch: it leaves R (the level is evaluated again when the search comes
//         back to it, as a node of its own), and R & row(v) is pushed.
//     Every subset of P that is a clique is reached at most once (with v | without v), so the enumeration counts each maximum
//     clique exactly once, at its root.
//   * best is one word: read at every node with an agent-scope atomic load, raised with atomicMax.  The wave that raises it to
//     s owns row s of the witness table if it wins the compare-and-swap on that row's owner word: one writer per row, read by the
//     host after the launch.  A stale best only costs nodes.
//   * nodes: every wave adds its nodes to one counter in batches of at most 256 and reads the counter at every node; once it has
//     reached the budget the wave stops.  The overshoot is at most 256 per wave (KOMB_MAXCLQ_OVERSHOOT in all).
// The launches of a run: k_rows, k_clq_tmax; then per phase (seed, search, enumeration) k_mc_search in count mode (the
// largest |P|, which sizes the scratch slots and the LDS) and in the phase's mode; k_mc_verify on the witness; k_mc_mark when
// the counts are the witness' own.  No workgroup waits for another; every loop runs over a row part, a candidate set or a
// stack that is bounded before it starts, and the node counter bounds the search as a whole.
#include "clique_root_dev.h"

#include <algorithm>

namespace komb {

namespace {

constexpr int kMcSeedWaves = 64;                      // greedy dives of the seed
constexpr long long kMcListDefault = 65536;

enum McMode : int { MC_COUNT = 0, MC_SEED = 1, MC_SEARCH = 2, MC_ENUM = 3 };

struct McArgs {
    ClqGraph g;
    uint32_t m, n_chunks;
    ClqCtl *ctl;
    int mode;
    uint32_t need;                                    // count / seed / enumeration: the threshold of roots and edges (the search reads best)
    unsigned long long budget;
    ClqLayout lay;                                    // the candidates are P; LDS head: cur[levels]; one set per stack level
    int32_t *wit;                                     // witness table: row s = a clique of s vertices
    uint32_t *wit_owner, wit_stride;
    int32_t *count, *list;                            // enumeration
    unsigned long long list_cap;
    uint32_t omega;
};

__device__ __forceinline__ uint32_t mc_best(ClqCtl *ctl) { return __hip_atomic_load(&ctl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One root: canonical edge rj = (a, b).  Every branch below is uniform over the wave.
__device__ void mc_root(const McArgs &A, uint32_t rj, uint32_t need, unsigned long long *smem, ClqWave &w, int lane)
{
    ClqCtl *ctl = A.ctl;
    const int32_t a = A.g.eu[rj], b = A.g.ev[rj];
    int32_t *P = (int32_t *)clq_slot(A.lay);
    const bool fill = A.mode != MC_COUNT;
    const uint32_t n = clq_cut(A.g, rj, need, P, A.lay.cap, fill, lane);
    if (!fill) { w.max_cand = n > w.max_cand ? n : w.max_cand; return; }
    ++w.roots;
    if (n > A.lay.cap || n > kClqMaxCand) { if (lane == 0) ctl->bad = 1u; return; }   // (the count launch saw every root with a need not above this one)
    if (n + 2u < (A.mode == MC_ENUM ? A.omega : mc_best(ctl) + 1u)) {            // too few candidates: closed at once, one node, no matrix
        clq_count(ctl, w, lane);
        return;
    }
    const uint32_t W = (n + 63u) >> 6;
    int32_t *cur = (int32_t *)smem;
    const ClqPlace at = clq_place(A.lay, smem, n);
    unsigned long long *mat = at.mat, *stk = at.stk;
    clq_matrix(A.g, need, P, n, W, mat, lane);
    // ---- the search
    const bool mine = (uint32_t)lane < W;
    if (mine) stk[lane] = clq_prefix(n, (uint32_t)lane * 64u);
    uint32_t d = 0;
    for (;;) {
        if (!clq_node(ctl, w, A.budget, lane)) break;
        unsigned long long R = mine ? stk[(size_t)d * W + lane] : 0ull;
        const int cnt = clq_sum(__popcll(R));
        const int s = (int)d + 2;
        const uint32_t best = mc_best(ctl);
        bool pop = false;
        unsigned long long U = R;
        if (cnt == 0) {
            pop = true;
            if (A.mode == MC_ENUM) {
                if ((uint32_t)s == A.omega) {                        // a maximum clique: a, b and the d chosen candidates
                    unsigned long long idx = 0;
                    if (lane == 0) idx = atomicAdd(&ctl->n_cliques, 1ull);
                    idx = clq_shfl64(idx, 0);
                    const bool keep = idx < A.list_cap;
                    for (int i = lane; i < s; i += kWave) {
                        const int32_t v = i == 0 ? a : (i == 1 ? b : P[cur[i - 2]]);
                        atomicAdd(A.count + v, 1);
                        if (keep) A.list[idx * A.omega + (uint32_t)i] = v;
                    }
                } else if ((uint32_t)s > A.omega && lane == 0) ctl->bad = 1u;
            } else if ((uint32_t)s > best) {
                uint32_t won = 0;
                if (lane == 0 && atomicMax(&ctl->best, (uint32_t)s) < (uint32_t)s && (uint32_t)s < A.wit_stride + 1u)
                    won = atomicCAS(A.wit_owner + s, 0u, 1u) == 0u ? 1u : 0u;
                if (__shfl((int32_t)won, 0))
                    for (int i = lane; i < s; i += kWave)
                        A.wit[(size_t)s * A.wit_stride + (uint32_t)i] = i == 0 ? a : (i == 1 ? b : P[cur[i - 2]]);
            }
        } else {
            const int k_need = A.mode == MC_ENUM ? (int)A.omega - s : (int)best - s + 1;
            if (cnt < k_need) pop = true;
            for (int k = 1; k < k_need && !pop; ++k) {               // one independent set off U per round
                unsigned long long Q = U;
                for (uint32_t v = clq_first(Q); v != kClqNone; v = clq_first(Q)) {
                    if (mine) Q &= ~mat[(size_t)v * W + lane];
                    if ((uint32_t)lane == (v >> 6)) { Q &= ~(1ull << (v & 63u)); U &= ~(1ull << (v & 63u)); }
                }
                if (!__ballot(U != 0ull)) pop = true;
            }
        }
        if (!pop) {
            const uint32_t v = clq_first(U);                         // (not empty: cnt > 0, or the colouring left something)
            if (d + 1 >= at.levels) { if (lane == 0) ctl->bad = 1u; break; }   // (a clique of more than t_max vertices)
            if (mine) {
                const unsigned long long child = R & mat[(size_t)v * W + lane];
                if ((uint32_t)lane == (v >> 6)) R &= ~(1ull << (v & 63u));
                stk[(size_t)d * W + lane] = R;
                stk[(size_t)(d + 1) * W + lane] = child;
            }
            if (lane == 0) cur[d] = (int32_t)v;
            ++d;
            continue;
        }
        if (A.mode == MC_SEED || d == 0) break;                      // (the seed is one greedy dive)
        --d;
    }
    __syncthreads();                                     // (the next root writes P, mat and the stack again)
}

__global__ __launch_bounds__(kWave) void k_mc_search(McArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const int lane = threadIdx.x;
    ClqCtl *ctl = A.ctl;
    ClqWave w{0u, 0u, 0u, false};
    bool done = false;                                   // the seed: one root per wave
    uint32_t chunk, tj;
    while (!w.stop && !done && clq_next_chunk(ctl, A.g.tr, A.m, A.n_chunks, chunk, tj, lane)) {
        unsigned long long todo = __ballot(tj >= (A.mode == MC_SEARCH ? mc_best(ctl) + 1u : A.need));
        while (todo && !w.stop && !done) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            uint32_t need = A.need;
            if (A.mode == MC_SEARCH) {                               // (best may have risen since the chunk was read)
                need = mc_best(ctl) + 1u;
                if ((uint32_t)__shfl((int32_t)tj, src) < need) continue;
            }
            if (A.mode != MC_COUNT && clq_nodes(ctl) >= A.budget) { w.stop = true; break; }
            mc_root(A, chunk * kWave + (uint32_t)src, need, smem, w, lane);
            done = A.mode == MC_SEED;
        }
    }
    clq_finish(ctl, w, lane);
}

// every pair of the witness is an edge of H (and its vertices are distinct)
__global__ void k_mc_verify(const int32_t *__restrict__ wit, uint32_t omega, const int32_t *__restrict__ ev, const uint32_t *__restrict__ rs,
                            const uint32_t *__restrict__ re, ClqCtl *ctl)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= omega * omega) return;
    const uint32_t i = id / omega, j = id % omega;
    if (i >= j) return;
    const int32_t u = wit[i] < wit[j] ? wit[i] : wit[j], v = wit[i] < wit[j] ? wit[j] : wit[i];
    if (u == v || nuc_find(ev, v, rs[u], re[u]) == kNucNone) ctl->bad = 1u;
}

__global__ void k_mc_mark(const int32_t *__restrict__ wit, uint32_t omega, int32_t *__restrict__ count)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < omega) count[wit[i]] = 1;
}

struct McRun {                                          // what the phases of one run share
    komb_ctx *ctx;
    McArgs A;
    ClqCtl h;
    uint32_t t_max, lds_opt;
    int launch(int mode, uint32_t need, int grid_cap);
};

// One phase: a count launch for the largest |P| at this need, then the launch itself with the slots and the LDS sized from it.
int McRun::launch(int mode, uint32_t need, int grid_cap)
{
    hipStream_t s = ctx->stream;
    A.need = need;
    A.mode = MC_COUNT;
    A.lay = ClqLayout{};
    const int count_grid = (int)std::min<uint32_t>(A.n_chunks, (uint32_t)kClqGrid);
    KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->cursor, 0, sizeof(uint32_t), s));
    KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->max_cand, 0, sizeof(uint32_t), s));
    k_mc_search<<<count_grid, kWave, 0, s>>>(A);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(ClqCtl)));
    const uint32_t max_p = h.max_cand;
    if (max_p > kClqMaxCand)
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_max_clique_run: a root edge has %u candidates of trussness >= %u; the limit is %u (one 64-bit word per lane)",
                  max_p, need, kClqMaxCand);
    const ClqLaunch L = clq_layout(A.lay, max_p, t_max, 1, 0, 1, lds_opt, A.n_chunks, grid_cap);
    if (!L.fits) KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_max_clique_run: t_max %u does not fit the LDS of a wavefront", t_max);
    DevBufs bufs(ctx);
    KOMB_HIP(ctx, bufs.alloc(&A.lay.scratch, (size_t)L.grid * A.lay.slot_bytes));
    A.mode = mode;
    KOMB_HIP(ctx, hipMemsetAsync(&A.ctl->cursor, 0, sizeof(uint32_t), s));
    k_mc_search<<<L.grid, kWave, L.lds_bytes, s>>>(A);
    KOMB_HIP(ctx, hipGetLastError());
    KOMB_HIP(ctx, d2h(ctx, &h, A.ctl, sizeof(ClqCtl)));
    if (h.bad) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_max_clique_run: the search is inconsistent (mode %d, need %u, largest candidate set %u)", mode, need, max_p);
    return KOMB_OK;
}

} // namespace

// the k-truss result it needs and the budget's sign are checked by the caller (api.cpp).  The result is built on the side and
// replaces the previous one only when the run has succeeded.
int max_clique_run(komb_ctx *ctx, int64_t budget)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv > 0 ? ctx->nv : 0;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));     // (a whole-graph result whose endpoints no fetch has asked for yet)
    Range r_all("komb_max_clique_run");
    komb_ctx::MaxClique res;                             // goes back to the pool unless it is installed
    const long long limit = budget == 0 ? kClqDefaultBudget : std::min<long long>(budget, kClqMaxBudget);
    const bool seed = !ctx_opt(ctx, "MAXCLQ_SEED") || ctx_flag(ctx, "MAXCLQ_SEED");
    const long long list_cap = clq_opt(ctx, "MAXCLQ_LIST", kMcListDefault, 0, 1ll << 24);
    KOMB_HIP(ctx, ctx->pool.get((void **)res.count.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
    DevBufs bufs(ctx);
    EventSet evs;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
    KOMB_HIP(ctx, evs.make(&e0)); KOMB_HIP(ctx, evs.make(&e1)); KOMB_HIP(ctx, evs.make(&e2)); KOMB_HIP(ctx, evs.make(&e3));
    uint64_t nodes_seed = 0, nodes_search = 0;
    bool timed = false;

    ctx->timer.start(s);
    if (nv > 0) KOMB_HIP(ctx, hipMemsetAsync(res.count, 0, (size_t)nv * sizeof(int32_t), s));
    if (m == 0) {                                        // no edge: omega = 0, nothing to list, all of it proven
        res.flags = KOMB_MAXCLQ_EXACT | KOMB_MAXCLQ_ENUMERATED | KOMB_MAXCLQ_LISTED;
        res.n_max = 0;
    } else {
        McRun run{};
        run.ctx = ctx;
        McArgs &A = run.A;
        KOMB_HIP(ctx, bufs.alloc(&A.ctl, 1));
        KOMB_HIP(ctx, hipMemsetAsync(A.ctl, 0, sizeof(ClqCtl), s));
        KOMB_TRY(clq_rows(ctx, bufs, &A.g));
        KOMB_TRY(clq_tmax(ctx, "komb_max_clique_run", A.ctl, 1u, &run.h));
        const uint32_t t_max = run.t_max = run.h.t_max, um = (uint32_t)m;
        run.lds_opt = (uint32_t)clq_opt(ctx, "MAXCLQ_LDS", kClqLdsCand, 0, kClqLdsCand);
        A.m = um; A.n_chunks = (um + kWave - 1) / kWave;
        A.budget = (unsigned long long)limit;
        A.wit_stride = t_max;
        KOMB_HIP(ctx, bufs.alloc(&A.wit, ((size_t)t_max + 1) * t_max));
        KOMB_HIP(ctx, bufs.alloc(&A.wit_owner, (size_t)t_max + 1));
        KOMB_HIP(ctx, hipMemsetAsync(A.wit_owner, 0, ((size_t)t_max + 1) * sizeof(uint32_t), s));
        res.t_max = (int32_t)t_max;

        // ---- seed: greedy dives from edges of the largest trussness
        (void)hipEventRecord(e0, s);
        if (seed) KOMB_TRY(run.launch(MC_SEED, t_max, kMcSeedWaves));
        nodes_seed = run.h.nodes;
        (void)hipEventRecord(e1, s);
        // ---- search: omega
        if (!run.h.stopped && run.h.best < t_max) KOMB_TRY(run.launch(MC_SEARCH, run.h.best + 1, kClqGrid));
        nodes_search = run.h.nodes - nodes_seed;
        (void)hipEventRecord(e2, s);
        uint32_t omega = run.h.best;
        const bool exact = !run.h.stopped || omega == t_max;
        const int32_t *d_wit = A.wit + (size_t)omega * A.wit_stride;
        std::vector<int32_t> &wit = res.witness;
        if (omega < 2) {                                 // (the budget ran out before the first leaf: an edge is a clique)
            omega = 2;
            wit.resize(2);
            KOMB_HIP(ctx, d2h(ctx, &wit[0], ctx->d_t_eu, sizeof(int32_t)));
            KOMB_HIP(ctx, d2h(ctx, &wit[1], ctx->d_t_ev, sizeof(int32_t)));
            KOMB_HIP(ctx, hipMemcpyAsync(A.wit, wit.data(), 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            KOMB_HIP(ctx, hipStreamSynchronize(s));
            d_wit = A.wit;
        } else {
            k_mc_verify<<<(int)(((size_t)omega * omega + kBlock - 1) / kBlock), kBlock, 0, s>>>(d_wit, omega, A.g.ev, A.g.rs, A.g.re, A.ctl);
            KOMB_HIP(ctx, hipGetLastError());
            wit.resize(omega);
            KOMB_HIP(ctx, staged_copy(ctx, wit.data(), d_wit, (size_t)omega * sizeof(int32_t), false));
            KOMB_HIP(ctx, d2h(ctx, &run.h, A.ctl, sizeof(ClqCtl)));
            if (run.h.bad) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_max_clique_run: the clique of %u vertices the search holds is not one", omega);
            std::sort(wit.begin(), wit.end());
        }
        res.omega = (int32_t)omega;
        res.flags = exact ? KOMB_MAXCLQ_EXACT : 0;
        res.upper = exact ? (int32_t)omega : (int32_t)t_max;
        // ---- enumeration: every maximum clique, each at its root
        bool enumerated = false;
        if (exact && !run.h.stopped) {
            A.omega = omega;
            A.count = res.count;
            A.list_cap = (unsigned long long)list_cap;
            KOMB_HIP(ctx, bufs.alloc(&A.list, (size_t)list_cap * omega));
            KOMB_TRY(run.launch(MC_ENUM, omega, kClqGrid));
            enumerated = !run.h.stopped;
            if (enumerated && run.h.n_cliques < 1)
                KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_max_clique_run: the enumeration found no clique of %u vertices", omega);
        }
        if (enumerated) {
            res.flags |= KOMB_MAXCLQ_ENUMERATED;
            res.n_max = (int64_t)run.h.n_cliques;
            if (run.h.n_cliques <= (unsigned long long)list_cap) {
                res.flags |= KOMB_MAXCLQ_LISTED;
                const size_t n = (size_t)run.h.n_cliques;
                std::vector<int32_t> raw(n * omega);
                KOMB_HIP(ctx, staged_copy(ctx, raw.data(), A.list, raw.size() * sizeof(int32_t), false));
                std::vector<size_t> order(n);
                for (size_t i = 0; i < n; ++i) { order[i] = i; std::sort(raw.begin() + i * omega, raw.begin() + (i + 1) * omega); }
                std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
                    return std::lexicographical_compare(raw.begin() + x * omega, raw.begin() + (x + 1) * omega, raw.begin() + y * omega, raw.begin() + (y + 1) * omega);
                });
                res.list.resize(n * omega);
                for (size_t i = 0; i < n; ++i) std::copy(raw.begin() + order[i] * omega, raw.begin() + (order[i] + 1) * omega, res.list.begin() + i * omega);
                wit.assign(res.list.begin(), res.list.begin() + omega);
            }
        } else {                                         // the counts are the witness' own
            res.n_max = -1;
            KOMB_HIP(ctx, hipMemsetAsync(res.count, 0, (size_t)nv * sizeof(int32_t), s));
            k_mc_mark<<<(int)((omega + kBlock - 1) / kBlock), kBlock, 0, s>>>(d_wit, omega, res.count);
            KOMB_HIP(ctx, hipGetLastError());
        }
        (void)hipEventRecord(e3, s);
        timed = true;
        res.n_roots = (int64_t)run.h.n_roots;
        res.nodes = (int64_t)run.h.nodes;
    }
    res.ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    if (ctx_flag(ctx, "MAXCLQ_DEBUG")) {
        float f[3] = {0.f, 0.f, 0.f};
        if (timed) { (void)hipEventElapsedTime(&f[0], e0, e1); (void)hipEventElapsedTime(&f[1], e1, e2); (void)hipEventElapsedTime(&f[2], e2, e3); }
        fprintf(stderr, "komb max clique: %lld edges, t_max %d, omega %d, upper %d, flags %d, %lld maximum cliques, %lld roots, nodes %llu seed + %llu search + "
                "%llu enumeration of %lld, run %.3f ms, seed %.3f ms, search %.3f ms, verify + enumeration %.3f ms\n", (long long)m, res.t_max, res.omega,
                res.upper, res.flags, (long long)res.n_max, (long long)res.n_roots, (unsigned long long)nodes_seed, (unsigned long long)nodes_search,
                (unsigned long long)((uint64_t)res.nodes - nodes_seed - nodes_search), limit, res.ms, f[0], f[1], f[2]);
    }
    res.done = true;
    ctx->mc = std::move(res);
    return KOMB_OK;
}

} // namespace komb
