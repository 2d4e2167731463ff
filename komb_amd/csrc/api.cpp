// api.cpp -- the extern "C" surface declared in include/komb_accel.h.
// Host-only glue: argument checks, device selection, copies in and out.  All
// arithmetic of the path runs in the HIP kernels of the sibling .hip files;
// there is no CPU fallback (a missing device is KOMB_ERR_DEVICE).
#include "common.h"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

using namespace komb;

namespace {

int require_device(komb_ctx *ctx)
{
    if (!ctx) return KOMB_ERR_ARG;
    if (!ctx->device_ok) {
        if (ctx->err.empty()) ctx->err = "no usable HIP device";
        return KOMB_ERR_DEVICE;
    }
    KOMB_HIP(ctx, hipSetDevice(ctx->device));
    ctx->err.clear();
    return KOMB_OK;
}

// what every analysis of a k-truss result asks first: a completed run that materialised all of its canonical edges
int require_full_truss(komb_ctx *ctx, const char *who)
{
    if (!ctx->truss_done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "%s: no completed k-truss result on this graph", who);
    if (ctx->t_ne > 0 && (ctx->t_k_lo != 0 || (int64_t)ctx->t_k_hi != ctx->t_ne))
        KOMB_FAIL(ctx, KOMB_ERR_STATE, "%s: the last k-truss run materialised only the canonical edges [%u, %u) of %lld", who,
                  ctx->t_k_lo, ctx->t_k_hi, (long long)ctx->t_ne);
    return KOMB_OK;
}

// the largest trussness of the result, 2 when it has no edge
int32_t truss_k_max(const komb_ctx *ctx) { return ctx->t_ne > 0 && ctx->stats.max_trussness > 2 ? ctx->stats.max_trussness : 2; }
// a k-truss threshold as the caller gave it (checked: >= K_MAX): K_MAX (KOMB_COMM_K_MAX, KOMB_BICONN_K_MAX: one value) is the
// largest trussness, anything below 2 runs as 2
int32_t resolve_truss_k(const komb_ctx *ctx, int32_t k)
{
    if (k == KOMB_COMM_K_MAX) k = truss_k_max(ctx);
    return k < 2 ? 2 : k;
}

// count elements of a device array into host memory; a null dst or no element is nothing to do
template <class T> int fetch(komb_ctx *ctx, T *dst, const void *src, size_t count)
{
    if (dst && count) KOMB_HIP(ctx, staged_copy(ctx, dst, src, count * sizeof(T), false));
    return KOMB_OK;
}

} // namespace

static_assert(KOMB_COMM_K_MAX == KOMB_BICONN_K_MAX, "resolve_truss_k serves both");

// The two openings of an entry point.  Most ask for the device first and then for the graph; the hierarchy-style ones ask for
// the graph first: a context without one says so whether or not it has a device.  The _DONE variants then ask for the result
// the entry reads: `done` is its record's flag, `missing` what the message says when it is not there (one text per result).
#define KOMB_DEV_ENTER(ctx, what)                                                          \
    do {                                                                                   \
        KOMB_TRY(require_device(ctx));                                                     \
        if ((ctx)->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, what ": no graph loaded");         \
    } while (0)
#define KOMB_HIER_ENTER(ctx, what)                                                         \
    do {                                                                                   \
        if (!(ctx)) return KOMB_ERR_ARG;                                                   \
        if ((ctx)->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, what ": no graph loaded");         \
        KOMB_TRY(require_device(ctx));                                                     \
    } while (0)
#define KOMB_DEV_ENTER_DONE(ctx, what, done, missing)                                      \
    do {                                                                                   \
        KOMB_DEV_ENTER(ctx, what);                                                         \
        if (!(done)) KOMB_FAIL(ctx, KOMB_ERR_STATE, what ": " missing);                    \
    } while (0)
#define KOMB_HIER_ENTER_DONE(ctx, what, done, missing)                                     \
    do {                                                                                   \
        KOMB_HIER_ENTER(ctx, what);                                                        \
        if (!(done)) KOMB_FAIL(ctx, KOMB_ERR_STATE, what ": " missing);                    \
    } while (0)
#define NO_ONION "komb_onion_run has not completed on this graph"
#define NO_COMP "komb_components_run has not completed on this graph"
#define NO_HIER "komb_hierarchy_run has not completed on this graph"
#define NO_COMM "no communities of the current k-truss result"
#define NO_BC "no blocks of the current k-truss result"
#define NO_DENS "komb_densest_subgraph_run has not completed on this graph"
#define NO_SC "no structural clustering of the current k-truss result"
#define NO_GL "no graphlet census of the current k-truss result"
#define NO_BTW "komb_betweenness_run has not completed on this graph"
#define NO_DIST "komb_distances_run has not completed on this graph"
#define NO_NUC "no nucleus decomposition of the current k-truss result"
#define NO_MC "no maximum-clique search of the current k-truss result"
#define NO_CC "no clique census of the current k-truss result"
#define NO_MX "no maximal cliques of the current k-truss result"
#define NO_PC "no k-clique communities of the current maximal cliques"
#define NO_NH "no nucleus hierarchy of the current nucleus decomposition"
#define NO_CH "no community hierarchy of the current k-truss result"

extern "C" {

int komb_abi_version(void) { return KOMB_ACCEL_ABI_VERSION; }

komb_ctx *komb_create(const komb_opts *opts)
{
    komb_ctx *ctx = new (std::nothrow) komb_ctx();
    if (!ctx) return nullptr;
    if (opts) ctx->opts = *opts;
    ctx->device = ctx->opts.device;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        ctx->err = std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        (void)hipGetLastError();
        return ctx;
    }
    if (ctx->device < 0 || ctx->device >= ndev) {
        ctx->err = "device ordinal out of range";
        return ctx;
    }
    e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_ctrl, 2 * sizeof(PeelCtrl), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_local, 2 * sizeof(LocalCtrl), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&ctx->h_stage, kStageBytes, hipHostMallocDefault);
    // Every context works on a stream of its own: a BLOCKING one (hipStreamCreate, not hipStreamNonBlocking), so that the
    // legacy default stream -- the synchronous hipMemcpy calls of the fetch entry points, a host that launches work of its own
    // there -- still orders with it, while two contexts (two host threads, or a host's RCCL stream beside the library) no
    // longer serialise on one queue.  (Round 2 tried a non-blocking stream before the peel's launches carried their sequence
    // word and saw stale control blocks with two processes on one GPU; with the sequence word the engine no longer depends
    // on launch-order visibility)  KOMB_CREATE_NULL_STREAM in komb_opts.reserved[0] puts the context
    // back on the default stream.
    ctx->stream = nullptr;
    if (e == hipSuccess && !(ctx->opts.reserved[0] & KOMB_CREATE_NULL_STREAM)) { e = hipStreamCreate(&ctx->stream); ctx->own_stream = e == hipSuccess; }
    if (e == hipSuccess && !ctx->timer.init()) e = hipErrorUnknown;
    if (e != hipSuccess) {
        ctx->err = std::string("device initialisation failed: ") + hipGetErrorString(e);
        return ctx;
    }
    ctx->device_ok = true;
    // One-time costs of a process' first use of the library -- loading its code object onto the device (the first kernel
    // launch) and, for a caller that asks (KOMB_CREATE_WARM_UPLOAD), the pinned staging buffers of the graph upload -- are
    // paid here, not by the first graph build: komb2 creates its context on a second thread beside the SAM parse, so they
    // leave its critical path (komb_amd/host/komb2.cpp).  KOMB_CREATE_NO_WARMUP skips it.
    if (!(ctx->opts.reserved[0] & KOMB_CREATE_NO_WARMUP)) warm_up(ctx);
    return ctx;
}

void komb_destroy(komb_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->device_ok) {
        (void)hipSetDevice(ctx->device);
        graph_free(ctx);
        stager_free(ctx);
        ctx->pool.clear();
        ctx->timer.destroy();
        if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
        if (ctx->h_ctrl) (void)hipHostFree(ctx->h_ctrl);
        if (ctx->h_local) (void)hipHostFree(ctx->h_local);
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    }
    delete ctx;
}

const char *komb_last_error(const komb_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int komb_graph_from_edges(komb_ctx *ctx, int64_t nv, int64_t n_raw, const int64_t *uv_pairs)
{
    KOMB_TRY(require_device(ctx));
    return graph_from_edges(ctx, nv, n_raw, uv_pairs);
}

int komb_graph_from_csr(komb_ctx *ctx, int64_t nv, const int64_t *rowptr, const int32_t *col)
{
    KOMB_TRY(require_device(ctx));
    return graph_from_csr(ctx, nv, rowptr, col);
}

int komb_graph_info(komb_ctx *ctx, int64_t *nv, int64_t *ne)
{
    if (!ctx) return KOMB_ERR_ARG;
    if (ctx->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_graph_info: no graph loaded");
    if (nv) *nv = ctx->nv;
    if (ne) *ne = ctx->ne;
    return KOMB_OK;
}

int komb_graph_get_csr(komb_ctx *ctx, int64_t *rowptr, int32_t *col)
{
    KOMB_TRY(require_device(ctx));
    if (ctx->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_graph_get_csr: no graph loaded");
    if (!rowptr || (ctx->ne > 0 && !col)) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_graph_get_csr: null output");
    std::vector<uint32_t> rp((size_t)ctx->nv + 1);
    KOMB_HIP(ctx, hipMemcpy(rp.data(), ctx->d_o_rowptr, rp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rp.size(); ++i) rowptr[i] = (int64_t)rp[i];
    if (ctx->ne > 0)
        KOMB_HIP(ctx, hipMemcpy(col, ctx->d_o_col, (size_t)(2 * ctx->ne) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return KOMB_OK;
}

int komb_core_run(komb_ctx *ctx)
{
    KOMB_TRY(require_device(ctx));
    return core_run(ctx);
}

int komb_core_run_sharded(komb_ctx *ctx, int32_t rank, int32_t world, komb_allreduce_fn allreduce, void *user)
{
    KOMB_TRY(require_device(ctx));
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !allreduce))
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_core_run_sharded: bad rank %d / world %d / callback", rank, world);
    return core_run(ctx, rank, world, allreduce, user, true);
}

int komb_set_shard_peel(komb_ctx *ctx, int32_t on)
{
    if (!ctx) return KOMB_ERR_ARG;
    ctx->shard_peel = on != 0;
    return KOMB_OK;
}

int komb_core_fetch(komb_ctx *ctx, int32_t *degree, int32_t *coreness)
{
    KOMB_TRY(require_device(ctx));
    if (!ctx->core.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_core_fetch: komb_core_run has not completed");
    KOMB_TRY(fetch(ctx, degree, ctx->core.deg, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, coreness, ctx->core.core, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_degree_coreness(komb_ctx *ctx, int32_t *degree, int32_t *coreness)
{
    KOMB_TRY(komb_core_run(ctx));
    return komb_core_fetch(ctx, degree, coreness);
}

int komb_onion_run(komb_ctx *ctx)
{
    KOMB_DEV_ENTER(ctx, "komb_onion_run");
    return onion_run(ctx);
}

int komb_onion_fetch(komb_ctx *ctx, int32_t *layer, int32_t *coreness)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_onion_fetch", ctx->onion.done, NO_ONION);
    KOMB_TRY(fetch(ctx, layer, ctx->onion.layer, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, coreness, ctx->onion.core, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_onion_info(komb_ctx *ctx, int64_t *n_layers, int32_t *max_coreness, double *ms)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_onion_info", ctx->onion.done, NO_ONION);
    if (n_layers) *n_layers = ctx->onion.n_layers;
    if (max_coreness) *max_coreness = ctx->onion.max_core;
    if (ms) *ms = ctx->onion.ms;
    return KOMB_OK;
}

int komb_components_run(komb_ctx *ctx, int32_t kind, int32_t k)
{
    KOMB_DEV_ENTER(ctx, "komb_components_run");
    if (kind != KOMB_COMP_CORE && kind != KOMB_COMP_TRUSS) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_components_run: unknown kind %d", kind);
    if (k < KOMB_COMP_K_MAX) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_components_run: bad threshold %d", k);
    if (kind == KOMB_COMP_CORE) {
        if (k != 0 && !ctx->core.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_components_run: komb_core_run has not completed on this graph");
        if (k == KOMB_COMP_K_MAX) k = ctx->nv > 0 ? ctx->stats.max_coreness : 0;
    } else {
        KOMB_TRY(require_full_truss(ctx, "komb_components_run"));
        if (k == KOMB_COMP_K_MAX) k = truss_k_max(ctx);      // (no clamp here: a threshold below 2 runs as given)
    }
    return components_run(ctx, kind, k);
}

int komb_components_fetch(komb_ctx *ctx, int32_t *label, int32_t *size)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_components_fetch", ctx->comp.done, NO_COMP);
    KOMB_TRY(fetch(ctx, label, ctx->comp.label, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, size, ctx->comp.size, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_components_info(komb_ctx *ctx, int32_t *kind, int32_t *k_used, int64_t *n_members, int64_t *n_components, int64_t *largest, double *ms)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_components_info", ctx->comp.done, NO_COMP);
    if (kind) *kind = ctx->comp.kind;
    if (k_used) *k_used = ctx->comp.k;
    if (n_members) *n_members = ctx->comp.members;
    if (n_components) *n_components = ctx->comp.count;
    if (largest) *largest = ctx->comp.largest;
    if (ms) *ms = ctx->comp.ms;
    return KOMB_OK;
}

int komb_hierarchy_run(komb_ctx *ctx, int32_t kind)
{
    KOMB_HIER_ENTER(ctx, "komb_hierarchy_run");
    if (kind != KOMB_COMP_CORE && kind != KOMB_COMP_TRUSS) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_hierarchy_run: unknown kind %d", kind);
    if (kind == KOMB_COMP_CORE) {
        if (!ctx->core.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_hierarchy_run: komb_core_run has not completed on this graph");
    } else {
        KOMB_TRY(require_full_truss(ctx, "komb_hierarchy_run"));
    }
    return hierarchy_run(ctx, kind);
}

int komb_hierarchy_count(komb_ctx *ctx, int64_t *n_nodes)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_hierarchy_count", ctx->hier.done, NO_HIER);
    if (n_nodes) *n_nodes = ctx->hier.n_nodes;
    return KOMB_OK;
}

int komb_hierarchy_fetch_nodes(komb_ctx *ctx, int32_t *k, int32_t *rep, int32_t *parent, int32_t *size, int32_t *shell)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_hierarchy_fetch_nodes", ctx->hier.done, NO_HIER);
    const size_t stride = (size_t)(ctx->nv > 0 ? ctx->nv : 1);
    int32_t *const out[5] = {k, rep, parent, size, shell};
    for (int i = 0; i < 5; ++i) KOMB_TRY(fetch(ctx, out[i], ctx->hier.nodes + i * stride, (size_t)ctx->hier.n_nodes));
    return KOMB_OK;
}

int komb_hierarchy_fetch_vertices(komb_ctx *ctx, int32_t *node)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_hierarchy_fetch_vertices", ctx->hier.done, NO_HIER);
    KOMB_TRY(fetch(ctx, node, ctx->hier.vnode, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_hierarchy_info(komb_ctx *ctx, int32_t *kind, int64_t *n_nodes, int64_t *n_roots, int32_t *k_max, int32_t *depth, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_hierarchy_info", ctx->hier.done, NO_HIER);
    if (kind) *kind = ctx->hier.kind;
    if (n_nodes) *n_nodes = ctx->hier.n_nodes;
    if (n_roots) *n_roots = ctx->hier.n_roots;
    if (k_max) *k_max = ctx->hier.kmax;
    if (depth) *depth = ctx->hier.depth;
    if (ms) *ms = ctx->hier.ms;
    return KOMB_OK;
}

int komb_truss_communities_run(komb_ctx *ctx, int32_t k)
{
    KOMB_DEV_ENTER(ctx, "komb_truss_communities_run");
    if (k < KOMB_COMM_K_MAX) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_truss_communities_run: bad threshold %d", k);
    KOMB_TRY(require_full_truss(ctx, "komb_truss_communities_run"));
    return communities_run(ctx, resolve_truss_k(ctx, k));
}

int komb_truss_communities_fetch(komb_ctx *ctx, int32_t *label, int32_t *size)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_truss_communities_fetch", ctx->comm.done, NO_COMM);
    const size_t m = (size_t)(ctx->t_ne > 0 ? ctx->t_ne : 0);
    KOMB_TRY(fetch(ctx, label, ctx->comm.label, m));
    KOMB_TRY(fetch(ctx, size, ctx->comm.size, m));
    return KOMB_OK;
}

int komb_truss_communities_fetch_vertices(komb_ctx *ctx, int32_t *n_comm)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_truss_communities_fetch_vertices", ctx->comm.done, NO_COMM);
    KOMB_TRY(communities_vertices(ctx));
    KOMB_TRY(fetch(ctx, n_comm, ctx->comm.ncomm, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_truss_communities_info(komb_ctx *ctx, int32_t *k_used, int64_t *n_member_edges, int64_t *n_communities,
                                int64_t *largest, int64_t *n_multi_vertices, double *ms)
{
    KOMB_DEV_ENTER_DONE(ctx, "komb_truss_communities_info", ctx->comm.done, NO_COMM);
    if (n_multi_vertices) {                              // (the vertex pass runs when somebody asks for what it makes)
        KOMB_TRY(communities_vertices(ctx));
        *n_multi_vertices = ctx->comm.multi;
    }
    if (k_used) *k_used = ctx->comm.k;
    if (n_member_edges) *n_member_edges = ctx->comm.members;
    if (n_communities) *n_communities = ctx->comm.count;
    if (largest) *largest = ctx->comm.largest;
    if (ms) *ms = ctx->comm.ms;
    return KOMB_OK;
}

int komb_biconnected_run(komb_ctx *ctx, int32_t k)
{
    KOMB_HIER_ENTER(ctx, "komb_biconnected_run");
    if (k < KOMB_BICONN_K_MAX) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_biconnected_run: bad threshold %d", k);
    KOMB_TRY(require_full_truss(ctx, "komb_biconnected_run"));
    return biconnected_run(ctx, resolve_truss_k(ctx, k));
}

int komb_biconnected_count(komb_ctx *ctx, int64_t *n_blocks)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_biconnected_count", ctx->bc.done, NO_BC);
    if (n_blocks) *n_blocks = ctx->bc.n_blocks;
    return KOMB_OK;
}

int komb_biconnected_fetch_edges(komb_ctx *ctx, int32_t *block, int32_t *size)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_biconnected_fetch_edges", ctx->bc.done, NO_BC);
    const size_t m = (size_t)(ctx->t_ne > 0 ? ctx->t_ne : 0);
    KOMB_TRY(fetch(ctx, block, ctx->bc.block, m));
    KOMB_TRY(fetch(ctx, size, ctx->bc.size, m));
    return KOMB_OK;
}

int komb_biconnected_fetch_vertices(komb_ctx *ctx, int32_t *n_blocks, int32_t *ecc_label, int32_t *ecc_size)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_biconnected_fetch_vertices", ctx->bc.done, NO_BC);
    const size_t nv = (size_t)ctx->nv;
    KOMB_TRY(fetch(ctx, n_blocks, ctx->bc.nblocks, nv));
    KOMB_TRY(fetch(ctx, ecc_label, ctx->bc.ecc_label, nv));
    KOMB_TRY(fetch(ctx, ecc_size, ctx->bc.ecc_size, nv));
    return KOMB_OK;
}

int komb_biconnected_fetch_blocks(komb_ctx *ctx, int32_t *rep, int32_t *n_edges, int32_t *n_verts)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_biconnected_fetch_blocks", ctx->bc.done, NO_BC);
    const size_t n = (size_t)ctx->bc.n_blocks;
    int32_t *const out[3] = {rep, n_edges, n_verts};
    for (int i = 0; i < 3; ++i) KOMB_TRY(fetch(ctx, out[i], ctx->bc.list + i * n, n));
    return KOMB_OK;
}

int komb_biconnected_info(komb_ctx *ctx, int32_t *k_used, int64_t *n_member_edges, int64_t *n_member_vertices, int64_t *n_blocks,
                          int64_t *n_bridges, int64_t *n_articulation, int64_t *largest_block, int64_t *n_ecc, int64_t *largest_ecc,
                          int32_t *depth, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_biconnected_info", ctx->bc.done, NO_BC);
    const komb_ctx::Biconnected &r = ctx->bc;
    if (k_used) *k_used = r.k;
    if (n_member_edges) *n_member_edges = r.n_member_edges;
    if (n_member_vertices) *n_member_vertices = r.n_member_vertices;
    if (n_blocks) *n_blocks = r.n_blocks;
    if (n_bridges) *n_bridges = r.n_bridges;
    if (n_articulation) *n_articulation = r.n_articulation;
    if (largest_block) *largest_block = r.largest_block;
    if (n_ecc) *n_ecc = r.n_ecc;
    if (largest_ecc) *largest_ecc = r.largest_ecc;
    if (depth) *depth = r.depth;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_densest_subgraph_run(komb_ctx *ctx, int32_t iters)
{
    KOMB_HIER_ENTER(ctx, "komb_densest_subgraph_run");
    if (iters < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_densest_subgraph_run: bad number of rounds %d", iters);
    if (!ctx->core.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_densest_subgraph_run: komb_core_run has not completed on this graph");
    return densest_run(ctx, iters);
}

int komb_densest_subgraph_fetch(komb_ctx *ctx, int32_t *member, int32_t *load)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_densest_subgraph_fetch", ctx->dens.done, NO_DENS);
    KOMB_TRY(fetch(ctx, member, ctx->dens.member, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, load, ctx->dens.load, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_densest_subgraph_profile(komb_ctx *ctx, int64_t *n_k, int64_t *m_k)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_densest_subgraph_profile", ctx->dens.done, NO_DENS);
    const size_t K = ctx->dens.profile.size() / 2;
    if (n_k) memcpy(n_k, ctx->dens.profile.data(), K * sizeof(int64_t));
    if (m_k) memcpy(m_k, ctx->dens.profile.data() + K, K * sizeof(int64_t));
    return KOMB_OK;
}

int komb_densest_subgraph_info(komb_ctx *ctx, int32_t *source, int32_t *k_best, int32_t *k_prune, int64_t *n_pruned, int64_t *m_pruned,
                               int64_t *n_sub, int64_t *m_sub, int64_t *load_max, int32_t *iters, int32_t *k_max, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_densest_subgraph_info", ctx->dens.done, NO_DENS);
    const komb_ctx::Densest &r = ctx->dens;
    if (source) *source = r.source;
    if (k_best) *k_best = r.k_best;
    if (k_prune) *k_prune = r.k_prune;
    if (n_pruned) *n_pruned = r.n_pruned;
    if (m_pruned) *m_pruned = r.m_pruned;
    if (n_sub) *n_sub = r.n_sub;
    if (m_sub) *m_sub = r.m_sub;
    if (load_max) *load_max = r.load_max;
    if (iters) *iters = r.iters;
    if (k_max) *k_max = r.k_max;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_structural_clusters_run(komb_ctx *ctx, int32_t eps_num, int32_t eps_den, int32_t mu)
{
    KOMB_HIER_ENTER(ctx, "komb_structural_clusters_run");
    if (eps_num < 1 || eps_num > eps_den || eps_den > 1000000)
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_structural_clusters_run: bad epsilon %d / %d (1 <= eps_num <= eps_den <= 1000000)", eps_num, eps_den);
    if (mu < 2) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_structural_clusters_run: bad mu %d (at least 2)", mu);
    KOMB_TRY(require_full_truss(ctx, "komb_structural_clusters_run"));
    return structural_run(ctx, eps_num, eps_den, mu);
}

int komb_structural_clusters_fetch(komb_ctx *ctx, int32_t *label, int32_t *size, int32_t *role, int32_t *sim_deg)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_structural_clusters_fetch", ctx->sc.done, NO_SC);
    const size_t nv = (size_t)ctx->nv;
    KOMB_TRY(fetch(ctx, label, ctx->sc.label, nv));
    KOMB_TRY(fetch(ctx, size, ctx->sc.size, nv));
    KOMB_TRY(fetch(ctx, role, ctx->sc.role, nv));
    KOMB_TRY(fetch(ctx, sim_deg, ctx->sc.simdeg, nv));
    return KOMB_OK;
}

int komb_structural_clusters_fetch_edges(komb_ctx *ctx, int32_t *similar)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_structural_clusters_fetch_edges", ctx->sc.done, NO_SC);
    return structural_fetch_edges(ctx, similar);
}

int komb_structural_clusters_info(komb_ctx *ctx, int32_t *eps_num, int32_t *eps_den, int32_t *mu, int64_t *n_similar_edges,
                                  int64_t *n_cores, int64_t *n_borders, int64_t *n_hubs, int64_t *n_outliers, int64_t *n_clusters,
                                  int64_t *largest, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_structural_clusters_info", ctx->sc.done, NO_SC);
    const komb_ctx::Structural &r = ctx->sc;
    if (eps_num) *eps_num = r.eps_num;
    if (eps_den) *eps_den = r.eps_den;
    if (mu) *mu = r.mu;
    if (n_similar_edges) *n_similar_edges = r.n_similar;
    if (n_cores) *n_cores = r.n_cores;
    if (n_borders) *n_borders = r.n_borders;
    if (n_hubs) *n_hubs = r.n_hubs;
    if (n_outliers) *n_outliers = r.n_outliers;
    if (n_clusters) *n_clusters = r.n_clusters;
    if (largest) *largest = r.largest;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_graphlets_run(komb_ctx *ctx)
{
    KOMB_HIER_ENTER(ctx, "komb_graphlets_run");
    KOMB_TRY(require_full_truss(ctx, "komb_graphlets_run"));
    return graphlets_run(ctx);
}

int komb_graphlets_fetch_vertices(komb_ctx *ctx, uint64_t *orbit)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_graphlets_fetch_vertices", ctx->gl.done, NO_GL);
    return fetch(ctx, orbit, ctx->gl.orbit, (size_t)KOMB_GRAPHLET_ORBITS * (size_t)ctx->nv);
}

int komb_graphlets_fetch_edges(komb_ctx *ctx, uint64_t *cycles4, uint64_t *cliques4)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_graphlets_fetch_edges", ctx->gl.done, NO_GL);
    const size_t m = ctx->t_ne > 0 && ctx->nv > 0 ? (size_t)ctx->t_ne : 0;
    KOMB_TRY(fetch(ctx, cycles4, ctx->gl.cycles4, m));
    KOMB_TRY(fetch(ctx, cliques4, ctx->gl.cliques4, m));
    return KOMB_OK;
}

int komb_graphlets_info(komb_ctx *ctx, uint64_t *total, int32_t *flags, int32_t *max_degree, int64_t *cycle_items,
                        int64_t *n_triangles, int64_t *n_cliques4, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_graphlets_info", ctx->gl.done, NO_GL);
    const komb_ctx::Graphlets &r = ctx->gl;
    if (total) memcpy(total, r.total, sizeof(r.total));
    if (flags) *flags = r.flags;
    if (max_degree) *max_degree = r.max_degree;
    if (cycle_items) *cycle_items = r.cycle_items;
    if (n_triangles) *n_triangles = r.n_triangles;
    if (n_cliques4) *n_cliques4 = r.n_cliques4;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_betweenness_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources)
{
    KOMB_HIER_ENTER(ctx, "komb_betweenness_run");
    return betweenness_run(ctx, n_sources, sources);
}

int komb_betweenness_fetch(komb_ctx *ctx, double *bc)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_betweenness_fetch", ctx->btw.done, NO_BTW);
    return fetch(ctx, bc, ctx->btw.bc, (size_t)ctx->nv);
}

int komb_betweenness_fetch_sources(komb_ctx *ctx, int32_t *source, int64_t *n_reached, int64_t *sum_dist, int32_t *ecc)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_betweenness_fetch_sources", ctx->btw.done, NO_BTW);
    const komb_ctx::Betweenness &r = ctx->btw;
    const size_t n = r.source.size();
    if (source && n) memcpy(source, r.source.data(), n * sizeof(int32_t));
    if (n_reached && n) memcpy(n_reached, r.n_reached.data(), n * sizeof(int64_t));
    if (sum_dist && n) memcpy(sum_dist, r.sum_dist.data(), n * sizeof(int64_t));
    if (ecc && n) memcpy(ecc, r.ecc.data(), n * sizeof(int32_t));
    return KOMB_OK;
}

int komb_betweenness_info(komb_ctx *ctx, int64_t *n_sources, int32_t *flags, int32_t *depth_max, int64_t *n_batches,
                          int64_t *n_level_steps, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_betweenness_info", ctx->btw.done, NO_BTW);
    const komb_ctx::Betweenness &r = ctx->btw;
    if (n_sources) *n_sources = (int64_t)r.source.size();
    if (flags) *flags = r.flags;
    if (depth_max) *depth_max = r.depth_max;
    if (n_batches) *n_batches = r.n_batches;
    if (n_level_steps) *n_level_steps = r.n_level_steps;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_distances_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources)
{
    KOMB_HIER_ENTER(ctx, "komb_distances_run");
    return distances_run(ctx, n_sources, sources);
}

int komb_distances_fetch(komb_ctx *ctx, int64_t *n_reached, int64_t *sum_dist, int32_t *ecc, double *harmonic)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_distances_fetch", ctx->dist.done, NO_DIST);
    const komb_ctx::Distances &r = ctx->dist;
    KOMB_TRY(fetch(ctx, n_reached, r.n_reached, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, sum_dist, r.sum_dist, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, ecc, r.ecc, (size_t)ctx->nv));
    return fetch(ctx, harmonic, r.harmonic, (size_t)ctx->nv);
}

int komb_distances_fetch_sources(komb_ctx *ctx, int32_t *source, int64_t *n_reached, int64_t *sum_dist, int32_t *ecc)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_distances_fetch_sources", ctx->dist.done, NO_DIST);
    const komb_ctx::Distances &r = ctx->dist;
    const size_t n = r.source.size();
    if (source && n) memcpy(source, r.source.data(), n * sizeof(int32_t));
    if (n_reached && n) memcpy(n_reached, r.s_reached.data(), n * sizeof(int64_t));
    if (sum_dist && n) memcpy(sum_dist, r.s_sum_dist.data(), n * sizeof(int64_t));
    if (ecc && n) memcpy(ecc, r.s_ecc.data(), n * sizeof(int32_t));
    return KOMB_OK;
}

int komb_distances_histogram(komb_ctx *ctx, int64_t *pairs, int64_t cap)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_distances_histogram", ctx->dist.done, NO_DIST);
    const komb_ctx::Distances &r = ctx->dist;
    if (cap < (int64_t)r.pairs.size())
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_distances_histogram: room for %lld distances, the run has %lld", (long long)cap,
                  (long long)r.pairs.size());
    if (pairs) memcpy(pairs, r.pairs.data(), r.pairs.size() * sizeof(int64_t));
    return KOMB_OK;
}

int komb_distances_info(komb_ctx *ctx, int64_t *n_sources, int32_t *flags, int32_t *depth_max, int32_t *depth_min, int64_t *n_pairs,
                        int64_t *sum_all, int64_t *n_batches, int64_t *n_level_steps, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_distances_info", ctx->dist.done, NO_DIST);
    const komb_ctx::Distances &r = ctx->dist;
    if (n_sources) *n_sources = (int64_t)r.source.size();
    if (flags) *flags = r.flags;
    if (depth_max) *depth_max = r.depth_max;
    if (depth_min) *depth_min = r.depth_min;
    if (n_pairs) *n_pairs = r.n_pairs;
    if (sum_all) *sum_all = r.sum_all;
    if (n_batches) *n_batches = r.n_batches;
    if (n_level_steps) *n_level_steps = r.n_level_steps;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_nucleus_run(komb_ctx *ctx)
{
    KOMB_HIER_ENTER(ctx, "komb_nucleus_run");
    KOMB_TRY(require_full_truss(ctx, "komb_nucleus_run"));
    return nucleus_run(ctx);
}

int komb_nucleus_count(komb_ctx *ctx, int64_t *n_triangles)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_count", ctx->nuc.done, NO_NUC);
    if (n_triangles) *n_triangles = ctx->nuc.n_tri;
    return KOMB_OK;
}

int komb_nucleus_fetch(komb_ctx *ctx, int32_t *a, int32_t *b, int32_t *c, int32_t *key0, int32_t *theta)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_fetch", ctx->nuc.done, NO_NUC);
    const komb_ctx::Nucleus &r = ctx->nuc;
    int32_t *const out[5] = {a, b, c, key0, theta};
    const int32_t *const src[5] = {r.a, r.b, r.c, r.key0, r.theta};
    for (int i = 0; i < 5; ++i) KOMB_TRY(fetch(ctx, out[i], src[i], (size_t)r.n_tri));
    return KOMB_OK;
}

int komb_nucleus_fetch_edges(komb_ctx *ctx, int32_t *edge_theta)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_fetch_edges", ctx->nuc.done, NO_NUC);
    KOMB_TRY(fetch(ctx, edge_theta, ctx->nuc.edge, (size_t)(ctx->t_ne > 0 ? ctx->t_ne : 0)));
    return KOMB_OK;
}

int komb_nucleus_fetch_vertices(komb_ctx *ctx, int32_t *vertex_theta)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_fetch_vertices", ctx->nuc.done, NO_NUC);
    KOMB_TRY(fetch(ctx, vertex_theta, ctx->nuc.vertex, (size_t)ctx->nv));
    return KOMB_OK;
}

int komb_nucleus_info(komb_ctx *ctx, int64_t *n_triangles, int64_t *n_cliques4, int32_t *theta_max, int32_t *n_levels, int64_t *n_subrounds, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_info", ctx->nuc.done, NO_NUC);
    const komb_ctx::Nucleus &r = ctx->nuc;
    if (n_triangles) *n_triangles = r.n_tri;
    if (n_cliques4) *n_cliques4 = r.n_clq;
    if (theta_max) *theta_max = r.theta_max;
    if (n_levels) *n_levels = r.n_levels;
    if (n_subrounds) *n_subrounds = r.n_subrounds;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_max_clique_run(komb_ctx *ctx, int64_t budget)
{
    KOMB_HIER_ENTER(ctx, "komb_max_clique_run");
    if (budget < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_max_clique_run: bad node budget %lld", (long long)budget);
    KOMB_TRY(require_full_truss(ctx, "komb_max_clique_run"));
    return max_clique_run(ctx, budget);
}

int komb_max_clique_fetch(komb_ctx *ctx, int32_t *count, int32_t *witness)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_max_clique_fetch", ctx->mc.done, NO_MC);
    KOMB_TRY(fetch(ctx, count, ctx->mc.count, (size_t)ctx->nv));
    if (witness && !ctx->mc.witness.empty()) memcpy(witness, ctx->mc.witness.data(), ctx->mc.witness.size() * sizeof(int32_t));
    return KOMB_OK;
}

int komb_max_clique_list(komb_ctx *ctx, int64_t cap, int64_t *n_cliques, int32_t *verts)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_max_clique_list", ctx->mc.done, NO_MC);
    const komb_ctx::MaxClique &r = ctx->mc;
    if (!(r.flags & KOMB_MAXCLQ_LISTED))
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_max_clique_list: the list was not kept (flags %d, %lld maximum cliques; option MAXCLQ_LIST, the node budget)",
                  r.flags, (long long)r.n_max);
    if (verts && cap < r.n_max) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_max_clique_list: room for %lld of %lld cliques", (long long)cap, (long long)r.n_max);
    if (n_cliques) *n_cliques = r.n_max;
    if (verts && !r.list.empty()) memcpy(verts, r.list.data(), r.list.size() * sizeof(int32_t));
    return KOMB_OK;
}

int komb_max_clique_info(komb_ctx *ctx, int32_t *omega, int32_t *upper, int32_t *flags, int32_t *t_max, int64_t *n_max_cliques,
                         int64_t *n_roots, int64_t *nodes, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_max_clique_info", ctx->mc.done, NO_MC);
    const komb_ctx::MaxClique &r = ctx->mc;
    if (omega) *omega = r.omega;
    if (upper) *upper = r.upper;
    if (flags) *flags = r.flags;
    if (t_max) *t_max = r.t_max;
    if (n_max_cliques) *n_max_cliques = r.n_max;
    if (n_roots) *n_roots = r.n_roots;
    if (nodes) *nodes = r.nodes;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_clique_census_run(komb_ctx *ctx, int32_t k_lo, int32_t k_hi, int32_t k_local, int64_t budget)
{
    KOMB_HIER_ENTER(ctx, "komb_clique_census_run");
    if (budget < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_clique_census_run: bad node budget %lld", (long long)budget);
    if (k_lo < 2 || (k_hi != -1 && k_hi < k_lo) || k_local < 0)
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_clique_census_run: bad window k_lo %d, k_hi %d, k_local %d", (int)k_lo, (int)k_hi, (int)k_local);
    KOMB_TRY(require_full_truss(ctx, "komb_clique_census_run"));
    return clique_census_run(ctx, k_lo, k_hi, k_local, budget);
}

int komb_clique_census_fetch(komb_ctx *ctx, uint64_t *total, uint64_t *local)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_census_fetch", ctx->cc.done, NO_CC);
    if (local && ctx->cc.k_local == 0) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_clique_census_fetch: the census ran without a k_local");
    KOMB_TRY(fetch(ctx, local, ctx->cc.local, (size_t)ctx->nv));
    if (total) memcpy(total, ctx->cc.total.data(), ctx->cc.total.size() * sizeof(uint64_t));
    return KOMB_OK;
}

int komb_clique_census_info(komb_ctx *ctx, int32_t *k_lo, int32_t *k_hi, int32_t *k_local, int32_t *t_max, int32_t *omega, int32_t *flags,
                            int32_t *max_candidates, int64_t *n_roots, int64_t *nodes, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_census_info", ctx->cc.done, NO_CC);
    const komb_ctx::CliqueCensus &r = ctx->cc;
    if (k_lo) *k_lo = r.k_lo;
    if (k_hi) *k_hi = r.k_hi;
    if (k_local) *k_local = r.k_local;
    if (t_max) *t_max = r.t_max;
    if (omega) *omega = r.omega;
    if (flags) *flags = r.flags;
    if (max_candidates) *max_candidates = r.max_p;
    if (n_roots) *n_roots = r.n_roots;
    if (nodes) *nodes = r.nodes;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_maximal_cliques_run(komb_ctx *ctx, int32_t k_min, int64_t budget)
{
    KOMB_HIER_ENTER(ctx, "komb_maximal_cliques_run");
    if (budget < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_maximal_cliques_run: bad node budget %lld", (long long)budget);
    if (k_min < 2) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_maximal_cliques_run: bad k_min %d", (int)k_min);
    KOMB_TRY(require_full_truss(ctx, "komb_maximal_cliques_run"));
    return maximal_cliques_run(ctx, k_min, budget);
}

int komb_maximal_cliques_fetch(komb_ctx *ctx, int64_t *hist, int32_t *count, int32_t *largest)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_maximal_cliques_fetch", ctx->mx.done, NO_MX);
    KOMB_TRY(fetch(ctx, count, ctx->mx.count, (size_t)ctx->nv));
    KOMB_TRY(fetch(ctx, largest, ctx->mx.count + ctx->nv, (size_t)ctx->nv));
    if (hist) memcpy(hist, ctx->mx.hist.data(), ctx->mx.hist.size() * sizeof(int64_t));
    return KOMB_OK;
}

int komb_maximal_cliques_list(komb_ctx *ctx, int64_t cap_cliques, int64_t cap_verts, int64_t *n_cliques, int64_t *n_verts, int64_t *offset, int32_t *verts)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_maximal_cliques_list", ctx->mx.done, NO_MX);
    const komb_ctx::MaximalCliques &r = ctx->mx;
    if (!(r.flags & KOMB_MAXIMAL_LISTED))
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_maximal_cliques_list: the list was not kept (flags %d, %lld cliques; option MAXIMAL_LIST, the node budget)",
                  r.flags, (long long)r.n_cliques);
    const int64_t nc = r.n_cliques, nw = (int64_t)r.verts.size();
    if ((offset && cap_cliques < nc) || (verts && cap_verts < nw))
        KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_maximal_cliques_list: room for %lld cliques and %lld vertices of %lld and %lld", (long long)cap_cliques,
                  (long long)cap_verts, (long long)nc, (long long)nw);
    if (n_cliques) *n_cliques = nc;
    if (n_verts) *n_verts = nw;
    if (offset) memcpy(offset, r.offset.data(), r.offset.size() * sizeof(int64_t));
    if (verts && nw) memcpy(verts, r.verts.data(), (size_t)nw * sizeof(int32_t));
    return KOMB_OK;
}

int komb_maximal_cliques_info(komb_ctx *ctx, int32_t *k_min, int32_t *k_hi, int32_t *t_max, int32_t *omega, int32_t *flags, int64_t *n_cliques,
                              int32_t *max_candidates, int64_t *n_roots, int64_t *nodes, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_maximal_cliques_info", ctx->mx.done, NO_MX);
    const komb_ctx::MaximalCliques &r = ctx->mx;
    if (k_min) *k_min = r.k_min;
    if (k_hi) *k_hi = r.k_hi;
    if (t_max) *t_max = r.t_max;
    if (omega) *omega = r.omega;
    if (flags) *flags = r.flags;
    if (n_cliques) *n_cliques = r.n_cliques;
    if (max_candidates) *max_candidates = r.max_q;
    if (n_roots) *n_roots = r.n_roots;
    if (nodes) *nodes = r.nodes;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_clique_communities_run(komb_ctx *ctx, int32_t k, int64_t budget)
{
    KOMB_HIER_ENTER(ctx, "komb_clique_communities_run");
    if (budget < 0) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_clique_communities_run: bad pair-test budget %lld", (long long)budget);
    if (k < 2) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_clique_communities_run: bad k %d", (int)k);
    if (!ctx->mx.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_clique_communities_run: " NO_MX);
    const komb_ctx::MaximalCliques &r = ctx->mx;
    if (r.k_min > k)
        KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_clique_communities_run: the held maximal cliques have k_min %d, above k %d: the list lacks member cliques",
                  (int)r.k_min, (int)k);
    if (!(r.flags & KOMB_MAXIMAL_LISTED))
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_clique_communities_run: the list was not kept (flags %d, %lld cliques; option MAXIMAL_LIST, the node budget)",
                  r.flags, (long long)r.n_cliques);
    return clique_communities_run(ctx, k, budget);
}

int komb_clique_communities_count(komb_ctx *ctx, int64_t *n_communities, int64_t *n_member_verts)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_communities_count", ctx->pc.done, NO_PC);
    if (n_communities) *n_communities = ctx->pc.n_comm;
    if (n_member_verts) *n_member_verts = (int64_t)ctx->pc.verts.size();
    return KOMB_OK;
}

int komb_clique_communities_fetch(komb_ctx *ctx, int32_t *label, int32_t *size)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_communities_fetch", ctx->pc.done, NO_PC);
    const komb_ctx::CliqueCommunities &r = ctx->pc;
    if (label && !r.label.empty()) memcpy(label, r.label.data(), r.label.size() * sizeof(int32_t));
    if (size && !r.size.empty()) memcpy(size, r.size.data(), r.size.size() * sizeof(int32_t));
    return KOMB_OK;
}

int komb_clique_communities_fetch_communities(komb_ctx *ctx, int32_t *rep, int32_t *n_cliques, int64_t *offset, int32_t *verts)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_communities_fetch_communities", ctx->pc.done, NO_PC);
    const komb_ctx::CliqueCommunities &r = ctx->pc;
    if (rep && !r.rep.empty()) memcpy(rep, r.rep.data(), r.rep.size() * sizeof(int32_t));
    if (n_cliques && !r.n_cliques.empty()) memcpy(n_cliques, r.n_cliques.data(), r.n_cliques.size() * sizeof(int32_t));
    if (offset) memcpy(offset, r.offset.data(), r.offset.size() * sizeof(int64_t));
    if (verts && !r.verts.empty()) memcpy(verts, r.verts.data(), r.verts.size() * sizeof(int32_t));
    return KOMB_OK;
}

int komb_clique_communities_fetch_vertices(komb_ctx *ctx, int32_t *n_comm, int32_t *first)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_communities_fetch_vertices", ctx->pc.done, NO_PC);
    const komb_ctx::CliqueCommunities &r = ctx->pc;
    if (n_comm && !r.v_comm.empty()) memcpy(n_comm, r.v_comm.data(), r.v_comm.size() * sizeof(int32_t));
    if (first && !r.v_first.empty()) memcpy(first, r.v_first.data(), r.v_first.size() * sizeof(int32_t));
    return KOMB_OK;
}

int komb_clique_communities_info(komb_ctx *ctx, int32_t *k, int32_t *k_min, int64_t *n_member_cliques, int64_t *n_communities, int64_t *largest,
                                 int64_t *n_covered, int64_t *n_overlap, int64_t *pair_tests, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_clique_communities_info", ctx->pc.done, NO_PC);
    const komb_ctx::CliqueCommunities &r = ctx->pc;
    if (k) *k = r.k;
    if (k_min) *k_min = r.k_min;
    if (n_member_cliques) *n_member_cliques = r.n_member;
    if (n_communities) *n_communities = r.n_comm;
    if (largest) *largest = r.largest;
    if (n_covered) *n_covered = r.n_covered;
    if (n_overlap) *n_overlap = r.n_overlap;
    if (pair_tests) *pair_tests = r.pair_tests;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_nucleus_hierarchy_run(komb_ctx *ctx)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_hierarchy_run", ctx->nuc.done, NO_NUC);
    return nucleus_hierarchy_run(ctx);
}

int komb_nucleus_hierarchy_count(komb_ctx *ctx, int64_t *n_nodes)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_hierarchy_count", ctx->nh.done, NO_NH);
    if (n_nodes) *n_nodes = ctx->nh.n_nodes;
    return KOMB_OK;
}

int komb_nucleus_hierarchy_fetch_nodes(komb_ctx *ctx, int32_t *k, int32_t *rep, int32_t *parent, int32_t *size, int32_t *shell)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_hierarchy_fetch_nodes", ctx->nh.done, NO_NH);
    const size_t stride = (size_t)ctx->nh.cap;
    int32_t *const out[5] = {k, rep, parent, size, shell};
    for (int i = 0; i < 5; ++i) KOMB_TRY(fetch(ctx, out[i], ctx->nh.nodes + i * stride, (size_t)ctx->nh.n_nodes));
    return KOMB_OK;
}

int komb_nucleus_hierarchy_fetch_triangles(komb_ctx *ctx, int32_t *node)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_hierarchy_fetch_triangles", ctx->nh.done, NO_NH);
    KOMB_TRY(fetch(ctx, node, ctx->nh.tnode, (size_t)ctx->nuc.n_tri));
    return KOMB_OK;
}

// k of _labels / _nuclei: KOMB_NUCLEUS_K_MAX is the largest theta, anything up to 1 runs as 1
static int32_t nucleus_hierarchy_k(const komb_ctx *ctx, int32_t k)
{
    if (k == KOMB_NUCLEUS_K_MAX) k = ctx->nh.theta_max;
    return k < 1 ? 1 : k;
}

int komb_nucleus_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label, int32_t *size)
{
    KOMB_HIER_ENTER(ctx, "komb_nucleus_hierarchy_labels");
    if (k < KOMB_NUCLEUS_K_MAX) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_nucleus_hierarchy_labels: bad threshold %d", k);
    if (!ctx->nh.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_nucleus_hierarchy_labels: " NO_NH);
    return nucleus_hierarchy_labels(ctx, nucleus_hierarchy_k(ctx, k), label, size);
}

int komb_nucleus_hierarchy_nuclei(komb_ctx *ctx, int32_t k, int64_t cap, int64_t *n_nuclei, int32_t *rep, int32_t *n_triangles,
                                  int32_t *n_edges, int32_t *n_vertices)
{
    KOMB_HIER_ENTER(ctx, "komb_nucleus_hierarchy_nuclei");
    if (k < KOMB_NUCLEUS_K_MAX) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_nucleus_hierarchy_nuclei: bad threshold %d", k);
    if (!ctx->nh.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_nucleus_hierarchy_nuclei: " NO_NH);
    return nucleus_hierarchy_nuclei(ctx, nucleus_hierarchy_k(ctx, k), cap, n_nuclei, rep, n_triangles, n_edges, n_vertices);
}

int komb_nucleus_hierarchy_info(komb_ctx *ctx, int64_t *n_nodes, int64_t *n_roots, int32_t *theta_max, int32_t *depth,
                                int64_t *n_member_triangles, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_nucleus_hierarchy_info", ctx->nh.done, NO_NH);
    const komb_ctx::NucleusHierarchy &r = ctx->nh;
    if (n_nodes) *n_nodes = r.n_nodes;
    if (n_roots) *n_roots = r.n_roots;
    if (theta_max) *theta_max = r.theta_max;
    if (depth) *depth = r.depth;
    if (n_member_triangles) *n_member_triangles = r.n_members;
    if (ms) *ms = r.ms;
    return KOMB_OK;
}

int komb_community_hierarchy_run(komb_ctx *ctx)
{
    KOMB_HIER_ENTER(ctx, "komb_community_hierarchy_run");
    KOMB_TRY(require_full_truss(ctx, "komb_community_hierarchy_run"));
    return community_hierarchy_run(ctx);
}

int komb_community_hierarchy_count(komb_ctx *ctx, int64_t *n_nodes)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_community_hierarchy_count", ctx->ch.done, NO_CH);
    if (n_nodes) *n_nodes = ctx->ch.n_nodes;
    return KOMB_OK;
}

int komb_community_hierarchy_fetch_nodes(komb_ctx *ctx, int32_t *k, int32_t *rep, int32_t *parent, int32_t *size, int32_t *shell)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_community_hierarchy_fetch_nodes", ctx->ch.done, NO_CH);
    const size_t stride = (size_t)ctx->ch.cap;
    int32_t *const out[5] = {k, rep, parent, size, shell};
    for (int i = 0; i < 5; ++i) KOMB_TRY(fetch(ctx, out[i], ctx->ch.nodes + i * stride, (size_t)ctx->ch.n_nodes));
    return KOMB_OK;
}

int komb_community_hierarchy_fetch_edges(komb_ctx *ctx, int32_t *node)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_community_hierarchy_fetch_edges", ctx->ch.done, NO_CH);
    KOMB_TRY(fetch(ctx, node, ctx->ch.enode, (size_t)(ctx->t_ne > 0 ? ctx->t_ne : 0)));
    return KOMB_OK;
}

int komb_community_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label, int32_t *size)
{
    KOMB_HIER_ENTER(ctx, "komb_community_hierarchy_labels");
    if (k < KOMB_COMM_K_MAX) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_community_hierarchy_labels: bad threshold %d", k);
    if (!ctx->ch.done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_community_hierarchy_labels: " NO_CH);
    return community_hierarchy_labels(ctx, resolve_truss_k(ctx, k), label, size);
}

int komb_community_hierarchy_info(komb_ctx *ctx, int64_t *n_nodes, int64_t *n_roots, int32_t *k_max, int32_t *depth,
                                  int64_t *n_member_edges, double *ms)
{
    KOMB_HIER_ENTER_DONE(ctx, "komb_community_hierarchy_info", ctx->ch.done, NO_CH);
    if (n_nodes) *n_nodes = ctx->ch.n_nodes;
    if (n_roots) *n_roots = ctx->ch.n_roots;
    if (k_max) *k_max = ctx->ch.kmax;
    if (depth) *depth = ctx->ch.depth;
    if (n_member_edges) *n_member_edges = ctx->ch.members;
    if (ms) *ms = ctx->ch.ms;
    return KOMB_OK;
}

int komb_set_option(komb_ctx *ctx, const char *name, const char *value)
{
    if (!ctx || !name || !*name) return KOMB_ERR_ARG;
    if (!strcmp(name, "POISON")) {                   // every device allocation is filled with this word first (common.h: Poison)
        Poison &p = ctx->pool.poison;
        if (!value) { p.on = false; p.word = 0; }
        else {
            char *end = nullptr;
            errno = 0;
            const unsigned long long w = strtoull(value, &end, 0);
            if (!*value || *end || errno || w > 0xFFFFFFFFull) KOMB_FAIL(ctx, KOMB_ERR_ARG, "option POISON=%s: expected a 32-bit word", value);
            p.on = true; p.word = (uint32_t)w; p.stream = ctx->stream;
        }
    }
    const bool fail_at = !strcmp(name, "ALLOC_FAIL_AT");
    if (fail_at || !strcmp(name, "ALLOC_TRIM_AT")) { // one-shot triggers on the count of device allocation requests (common.h: AllocHook)
        AllocHook &h = ctx->pool.hook;
        long long n = 0;
        if (value) {
            char *end = nullptr;
            errno = 0;
            n = strtoll(value, &end, 10);
            if (!*value || *end || errno || n < 0 || value[0] < '0' || value[0] > '9')
                KOMB_FAIL(ctx, KOMB_ERR_ARG, "option %s=%s: expected a request number (0: count only)", name, value);
        }
        if (fail_at) { h.fail_at = n; h.fired = 0; } else h.trim_at = n;
        if (value) h.requests = 0;                   // both count from the moment either was last set
        h.armed = ctx->options.count(fail_at ? "ALLOC_TRIM_AT" : "ALLOC_FAIL_AT") || value;
    }
    if (value) ctx->options[name] = value; else ctx->options.erase(name);
    return KOMB_OK;
}

int komb_alloc_info(komb_ctx *ctx, int64_t *requests, int32_t *fired, int64_t *pool_blocks_in_use, int64_t *pool_bytes_in_use,
                    int64_t *pool_blocks_cached, int64_t *trims)
{
    if (!ctx) return KOMB_ERR_ARG;                   // host state only: no device needed
    int64_t used = 0, used_bytes = 0, cached = 0;
    for (const auto &b : ctx->pool.blocks) {
        if (b.used) { ++used; used_bytes += (int64_t)b.bytes; } else ++cached;
    }
    if (requests) *requests = ctx->pool.hook.requests;
    if (fired) *fired = ctx->pool.hook.fired;
    if (pool_blocks_in_use) *pool_blocks_in_use = used;
    if (pool_bytes_in_use) *pool_bytes_in_use = used_bytes;
    if (pool_blocks_cached) *pool_blocks_cached = cached;
    if (trims) *trims = (int64_t)ctx->pool.n_trim;
    return KOMB_OK;
}

int komb_truss_prepare(komb_ctx *ctx)
{
    KOMB_TRY(require_device(ctx));
    if (ctx->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_truss_prepare: no graph loaded");
    if (ctx->prep.valid || ctx->nv == 0 || ctx->ne == 0) return KOMB_OK;
    KOMB_TRY(prep_ensure(ctx));
    ctx->stats.ms_prepare = ctx->prep.ms;
    ctx->stats.ms_prep_vertex = ctx->prep.ms_part[0]; ctx->stats.ms_prep_edges = ctx->prep.ms_part[1]; ctx->stats.ms_prep_rows = ctx->prep.ms_part[2];
    return KOMB_OK;
}

int komb_truss_unprepare(komb_ctx *ctx)
{
    KOMB_TRY(require_device(ctx));
    truss_free(ctx);
    prep_free(ctx, &ctx->prep);
    return KOMB_OK;
}

int komb_graph_moments(komb_ctx *ctx)
{
    KOMB_TRY(require_device(ctx));
    if (ctx->nv < 0) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_graph_moments: no graph loaded");
    int64_t mom[5] = {0, 0, 0, 0, 0};
    if (ctx->nv > 0 && ctx->ne > 0) KOMB_TRY(graph_moments(ctx, mom));
    ctx->stats.sum_deg_sq = mom[0]; ctx->stats.wedge_items = mom[1];
    ctx->stats.max_degree = (int32_t)mom[2]; ctx->stats.oriented_items = mom[4];
    return KOMB_OK;
}

int komb_truss_run(komb_ctx *ctx, const uint8_t *vmask)
{
    KOMB_TRY(require_device(ctx));
    return truss_run(ctx, vmask, 0, 1, nullptr, nullptr);
}

int komb_truss_run_sharded(komb_ctx *ctx, const uint8_t *vmask, int32_t rank, int32_t world,
                           komb_allreduce_fn allreduce, void *user)
{
    KOMB_TRY(require_device(ctx));
    return truss_run(ctx, vmask, rank, world, allreduce, user);
}

int komb_truss_run_slice(komb_ctx *ctx, const uint8_t *vmask, int32_t rank, int32_t world)
{
    KOMB_TRY(require_device(ctx));
    if (world < 1 || rank < 0 || rank >= world) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_truss_run_slice: bad rank %d / world %d", rank, world);
    ctx->slice_rank = rank; ctx->slice_world = world;
    const int rc = truss_run(ctx, vmask, 0, 1, nullptr, nullptr);
    ctx->slice_rank = 0; ctx->slice_world = 1;
    return rc;
}

int komb_truss_count(komb_ctx *ctx, int64_t *ne_sub)
{
    if (!ctx) return KOMB_ERR_ARG;
    if (!ctx->truss_done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_truss_count: komb_truss_run has not completed");
    if (ne_sub) *ne_sub = ctx->t_ne;
    return KOMB_OK;
}

int komb_truss_fetch(komb_ctx *ctx, int32_t *eu, int32_t *ev, int32_t *truss)
{
    KOMB_TRY(require_device(ctx));
    if (!ctx->truss_done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_truss_fetch: komb_truss_run has not completed");
    const size_t m = (size_t)ctx->t_ne;
    if (m == 0) return KOMB_OK;
    if (eu || ev) KOMB_TRY(truss_edges_canonical(ctx));  // (the endpoints: igraph_edge after igraph_trussness, src/graph.cpp:529-532 -- not part of the timed call)
    KOMB_TRY(fetch(ctx, eu, ctx->d_t_eu, m));
    KOMB_TRY(fetch(ctx, ev, ctx->d_t_ev, m));
    KOMB_TRY(fetch(ctx, truss, ctx->d_t_truss, m));
    return KOMB_OK;
}

int komb_truss_fetch_support(komb_ctx *ctx, int32_t *support)
{
    KOMB_TRY(require_device(ctx));
    if (!ctx->truss_done) KOMB_FAIL(ctx, KOMB_ERR_STATE, "komb_truss_fetch_support: komb_truss_run has not completed");
    KOMB_TRY(truss_support_canonical(ctx));              // (made on the first request: the timed step delivers trussness, as igraph_trussness does)
    KOMB_TRY(fetch(ctx, support, ctx->d_t_sup, (size_t)ctx->t_ne));
    return KOMB_OK;
}

int komb_trussness(komb_ctx *ctx, const uint8_t *vmask, int64_t *ne_out, int32_t *eu, int32_t *ev, int32_t *truss)
{
    KOMB_TRY(komb_truss_run(ctx, vmask));
    if (ne_out) *ne_out = ctx->t_ne;
    return komb_truss_fetch(ctx, eu, ev, truss);
}

int komb_corea_ranks(komb_ctx *ctx, const int32_t *degree, const int32_t *coreness, int64_t nv,
                     double *rank_degree, double *rank_key)
{
    KOMB_TRY(require_device(ctx));
    return corea_ranks(ctx, degree, coreness, nv, rank_degree, rank_key);
}

int komb_corea_scores(komb_ctx *ctx, const int32_t *degree, const int32_t *coreness, int64_t nv, double *score)
{
    KOMB_TRY(require_device(ctx));
    if (nv < 0 || (nv > 0 && !score)) KOMB_FAIL(ctx, KOMB_ERR_ARG, "komb_corea_scores: bad arguments");
    // (no std::vector: value-initialising 2 x 8 bytes x nv is 40 ms of page faults at nv = 10M before the first rank arrives)
    std::unique_ptr<double[]> rd(new (std::nothrow) double[(size_t)nv + 1]), rc(new (std::nothrow) double[(size_t)nv + 1]);
    if (!rd || !rc) KOMB_FAIL(ctx, KOMB_ERR_NOMEM, "komb_corea_scores: host allocation failed");
    KOMB_TRY(corea_ranks(ctx, degree, coreness, nv, rd.get(), rc.get()));
    // host libm on purpose: |ln r_deg - ln r_key| as src/CoreA.h:131, same "%f" text downstream (element-wise: the host's
    // threads share the loop, every element is the same libm call it would be on one)
    // (a GPU box shows every CPU of its host and grants a share of them: 16 threads at most)
#pragma omp parallel for schedule(static) num_threads(16) if (nv > 100000)
    for (int64_t i = 0; i < nv; ++i) score[i] = std::fabs(std::log(rd[(size_t)i]) - std::log(rc[(size_t)i]));
    return KOMB_OK;
}

int komb_densest_block(komb_ctx *ctx, const double *suspiciousness, int32_t *order, int32_t *side, int64_t *n_block, double *max_density)
{
    KOMB_TRY(require_device(ctx));
    return merge_run(ctx, suspiciousness, order, side, n_block, max_density);
}

int komb_get_stats(komb_ctx *ctx, komb_stats *out)
{
    if (!ctx || !out) return KOMB_ERR_ARG;
    *out = ctx->stats;
    return KOMB_OK;
}

} // extern "C"
