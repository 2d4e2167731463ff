// onion.hip -- onion decomposition (Hebert-Dufresne, Grochow & Allard 2016): per vertex, the synchronous layer inside its
// k-shell in which it is peeled; what networkx.onion_layers returns (include/komb_accel.h has the definition).
//
// The k-core peel engine of peel_dev.h already runs level-synchronous sub-rounds: SCAN puts every live vertex of live
// degree <= k into a frontier, PROCESS walks the frontier's rows and the decrement that lands a neighbour exactly on k
// puts it into the next sub-round's frontier.  One sub-round is one onion layer, so the layer of a vertex is the number
// of the sub-round that peels it, stamped when the vertex enters a frontier (SCAN, or the trigger).  What k-core does
// on top of that and the onion cannot:
//   - in-wave chaining (CoreProblem::kChain): a triggered vertex would be peeled in its trigger's sub-round -- off here;
//   - the local finish (local_dev.h): an h-index fixed point has no removal order -- never used here;
//   - the LDS tail (core_tail.h) keeps sub-rounds exact; its kLayers variant stamps each vertex with its sub-round.
// Small layers stay inside one workgroup through the engine's in-kernel step chaining (plan_step): the ~600 layers of
// fewer than 100 vertices of a 10M-vertex graph cost no launch each.  The sub-round counter (PeelCtrl::round) is the
// device-side layer counter: it advances once per PROCESS step, and every PROCESS step has a non-empty frontier.
// Isolated vertices are layer 1 when there are any; the counter then starts at 2.
// Every array is the onion's own (results: resident, dev_malloc; scratch: the context's pool): a call changes no k-core,
// k-truss or CoreA result and no komb_stats field.
#include "peel_dev.h"
#include "core_tail.h"

namespace komb {

namespace {

// live degrees + liveness; isolated vertices are layer 1 (coreness 0).  init[0] counts them, init[1] receives the smallest
// positive degree (the first populated level), as k_core_init does for the engine's control block.
__global__ __launch_bounds__(kBlock) void k_onion_init(const uint32_t *__restrict__ rowptr, int64_t nv, int32_t *__restrict__ degw,
                                                       int32_t *__restrict__ core, int32_t *__restrict__ layer, uint32_t *__restrict__ init)
{
    uint32_t zeros = 0;
    int32_t lmin = 0x7FFFFFFF;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += (int64_t)gridDim.x * kBlock) {
        const int32_t d = (int32_t)(rowptr[v + 1] - rowptr[v]);
        degw[v] = d;
        if (d == 0) { core[v] = 0; layer[v] = 1; ++zeros; }
        else { core[v] = alive_marker((uint32_t)d); lmin = min(lmin, d); }
    }
    block_add_min(zeros, lmin, &init[0], (int32_t *)&init[1]);
}

// the first layer after the isolated vertices' is 2
__global__ void k_onion_round_base(PeelCtrl *ctrl, const uint32_t *grp_done)
{
    if (threadIdx.x == 0 && grp_done[kInitOff] != 0u) ctrl->round = 2;
}

// CoreProblem (kcore.hip) without chaining, stamping the layer with the coreness
struct OnionProblem {
    static constexpr bool kChain = false;      // a triggered vertex belongs to the NEXT layer
    static constexpr bool kSingleStep = false;
    uint32_t units;
    const uint32_t *rowptr;
    const int32_t *col;
    int32_t *degw;
    int32_t *core;
    int32_t *layer;

    __device__ __forceinline__ const int32_t *scan_marker() const { return core; }
    __device__ __forceinline__ const int32_t *scan_key() const { return degw; }
    __device__ __forceinline__ void mark_scanned(uint32_t v, const CtrlView &cv) const { core[v] = cv.level; layer[v] = cv.round; }
    __device__ __forceinline__ void slice(uint32_t v, uint32_t &b, uint32_t &len) const
    {
        b = rowptr[v];
        len = rowptr[v + 1] - b;
    }
    struct Loaded { int32_t u, c; };
    __device__ __forceinline__ Loaded item_load(int32_t, uint32_t pos, const CtrlView &) const
    {
        Loaded ld;
        ld.u = col[pos];
        ld.c = core[ld.u];
        return ld;
    }
    __device__ __forceinline__ void item_apply(const Loaded &ld, const CtrlView &cv, int32_t &t0, int32_t &, uint32_t &c0, uint32_t &) const
    {
        if (marker_alive(ld.c)) {                       // a stale "alive" only costs a no-op decrement (the landing on k is unique)
            if (atomicSub(&degw[ld.u], 1) == cv.level + 1) {
                core[ld.u] = cv.level; layer[ld.u] = cv.round + 1; t0 = ld.u; c0 = marker_chunks(ld.c);
            }
        }
    }
};

} // namespace

int onion_run(komb_ctx *ctx)
{
    if (ctx->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_onion_run: no graph loaded");
    const int64_t nv = ctx->nv;
    hipStream_t s = ctx->stream;
    ctx->onion.done = false;
    if (!ctx->onion.layer) {
        const size_t bytes = (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t);
        KOMB_HIP(ctx, dev_malloc_pair(ctx, ctx->onion.layer.slot(nullptr), bytes, ctx->onion.core.slot(nullptr), bytes));
    }
    if (nv == 0) {
        ctx->onion.n_layers = 0; ctx->onion.max_core = 0; ctx->onion.ms = 0.0;
        ctx->onion.done = true;
        return KOMB_OK;
    }

    Range r_all("komb_onion_run");
    DevBufs bufs(ctx);
    const size_t heavy_cap = (size_t)(2 * ctx->ne) / 32 + 64;    // as core_run: <= 3/128 of all items
    int32_t *d_degw = nullptr; PeelCtrl *d_ctrl = nullptr; uint32_t *d_grp = nullptr;
    CoreTailBufs T{};
    PeelQueues Q{nullptr, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, 0};
    KOMB_HIP(ctx, bufs.alloc(&d_degw, (size_t)nv));
    for (int i = 0; i < 2; ++i) {
        KOMB_HIP(ctx, bufs.alloc(&Q.light[i], (size_t)nv));
        KOMB_HIP(ctx, bufs.alloc(&Q.heavy[i], heavy_cap));
        KOMB_HIP(ctx, bufs.alloc(&Q.live[i], (size_t)nv / 2 + 64));
    }
    KOMB_HIP(ctx, bufs.alloc(&Q.code, (size_t)nv));
    KOMB_HIP(ctx, bufs.alloc(&d_ctrl, 1));
    KOMB_HIP(ctx, bufs.alloc(&d_grp, (size_t)kInitOff + 4));
    // the finish is the layer-keeping LDS tail unless FINISH=none (the local fixed point numbers no layers: "local" = "lds")
    uint32_t tail_limit = 0;
    const size_t live_words = ((size_t)nv + 63) / 64;
    if (finish_mode(ctx, FIN_LDS) != FIN_NONE) {
        tail_limit = kCoreTailV;
        if (const char *tl = ctx_opt(ctx, "CORE_TAIL")) tail_limit = (uint32_t)strtoul(tl, nullptr, 10);
        if (tail_limit > kCoreTailV) tail_limit = kCoreTailV;
        if (tail_limit) {
            KOMB_HIP(ctx, bufs.alloc(&T.livebits, live_words));
            KOMB_HIP(ctx, bufs.alloc(&T.vnum, (size_t)nv));
            KOMB_HIP(ctx, bufs.alloc(&T.cnt, 4));
            KOMB_HIP(ctx, bufs.alloc(&T.vlist, (size_t)kCoreTailV));
            KOMB_HIP(ctx, bufs.alloc(&T.rows, (size_t)kCoreTailV * kCoreTailWords));
        }
    }

    const int64_t g = (nv + kBlock - 1) / kBlock;
    const int grid_init = (int)(g > 1024 ? 1024 : g);
    const int grid = peel_grid(nv);
    OnionProblem P{(uint32_t)nv, ctx->d_o_rowptr, ctx->d_o_col, d_degw, ctx->onion.core, ctx->onion.layer};
    ctx->timer.start(s);
    peel_ctrl_pre(s, d_grp);
    k_onion_init<<<grid_init, kBlock, 0, s>>>(ctx->d_o_rowptr, nv, d_degw, ctx->onion.core, ctx->onion.layer, d_grp + kInitOff);
    peel_ctrl_init(s, d_ctrl, d_grp, (uint32_t)nv, tail_limit);
    k_onion_round_base<<<1, 64, 0, s>>>(d_ctrl, d_grp);
    // the live vertices are those of `list` (or all nv when list is null) whose coreness is still an alive marker
    auto run_tail = [&](const int32_t *list, uint32_t n_in) -> int {
        KOMB_HIP(ctx, hipMemsetAsync(T.livebits, 0, live_words * sizeof(unsigned long long), s));
        KOMB_HIP(ctx, hipMemsetAsync(T.cnt, 0, 4 * sizeof(uint32_t), s));
        KOMB_HIP(ctx, hipMemsetAsync(T.rows, 0, (size_t)kCoreTailV * kCoreTailWords * sizeof(unsigned long long), s));
        const int64_t gm = ((int64_t)n_in + kBlock - 1) / kBlock;
        k_ctail_mark<<<(int)(gm < 1 ? 1 : (gm > 1024 ? 1024 : gm)), kBlock, 0, s>>>(list, n_in, ctx->onion.core, T);
        k_ctail_rows<<<dim3(kCoreTailV, 8), kBlock, 0, s>>>(ctx->d_o_rowptr, ctx->d_o_col, T);
        k_core_tail<true><<<1, 1024, 0, s>>>(d_ctrl, T, d_degw, ctx->onion.core, ctx->onion.layer);
        KOMB_HIP(ctx, d2h(ctx, &ctx->h_ctrl[0], d_ctrl, sizeof(PeelCtrl)));
        return KOMB_OK;
    };
    int st = KOMB_OK;
    if (tail_limit && (uint64_t)nv <= tail_limit) {
        // small graph: the tail takes the whole peel (unless nothing is left to peel)
        st = d2h(ctx, &ctx->h_ctrl[0], d_ctrl, sizeof(PeelCtrl)) == hipSuccess ? KOMB_OK : KOMB_ERR_DEVICE;
        if (st == KOMB_OK && !ctx->h_ctrl[0].done) st = run_tail(nullptr, (uint32_t)nv);
    } else {
        ctx->h_ctrl[0].done = 0;
    }
    for (int guard = 0; st == KOMB_OK && ctx->h_ctrl[0].done != 1 && ctx->h_ctrl[0].done != 2 && guard < 64; ++guard) {
        if (ctx->h_ctrl[0].done == 3) {
            const PeelCtrl &c = ctx->h_ctrl[0];
            st = c.live_mode ? run_tail(Q.live[c.live_sel], c.live_count) : run_tail(nullptr, (uint32_t)nv);
            continue;
        }
        int batch = 0;
        st = drive_peel(ctx, d_ctrl, nv, [&](int32_t launch) {
            k_peel_step<OnionProblem><<<grid, kPeelBlock, 0, s>>>(d_ctrl, d_grp, Q, P, launch);
        }, &batch);
    }
    const double ms = ctx->timer.stop(s);
    KOMB_TRY(st);
    if (ctx->h_ctrl[0].done != 1) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "onion peel ended in an inconsistent state");
    ctx->onion.n_layers = (int64_t)ctx->h_ctrl[0].round - 1;       // the counter has moved past the last layer
    ctx->onion.max_core = ctx->h_ctrl[0].max_level;
    ctx->onion.ms = ms;
    ctx->onion.done = true;
    return KOMB_OK;
}

} // namespace komb
