// biconnected.hip -- biconnected components (blocks), articulation points, bridges and 2-edge-connected components of the
// graph of the edges of trussness >= k of the last k-truss result (komb_biconnected_run): Tarjan & Vishkin (SIAM J. Comput.
// 1985) on a breadth-first spanning forest.  DESIGN.md section 4.6n.
//
// Input: the last k-truss result in canonical order, original vertex ids -- whole-graph and vmask runs alike.  The MEMBER
// edges (trussness >= k) are compacted in that order as communities.hip does (member j is canonical edge kept[j] =
// (mu[j], mv[j])), and a symmetric CSR over them is filled through per-vertex cursors (the order inside a row is the
// schedule's; no output depends on it).
//
// The forest.  The roots are the smallest member id of every connected component: the compaction pass links every member
// edge with the union-find of unionfind_dev.h, and after that launch a member is a root exactly when its word still holds
// its own id.  A level-synchronous top-down BFS starts from all roots at once: a vertex is claimed by one compare-and-swap
// on level[]; the winner writes parent[] and appends the vertex to order[], whose slices are the levels (the host reads
// the cursor once per level and keeps the offsets).  level[] is determined by the graph, parent[] is the schedule's.
// Three sweeps over the levels follow, one launch per level each: subtree sizes nd[] bottom-up, preorder numbers pre[]
// top-down (a child takes pre[p] + 1 + the sum of the subtrees of the siblings that came before it, whichever they are),
// and, after one flat pass over the member edges (k_bc_reach: the non-tree edges' ends, rule (i) below, and the vertex that
// names every edge's class), low[] / high[] -- the smallest / largest preorder number a non-tree edge out of the subtree
// reaches -- bottom-up.  A launch boundary is what makes one level's sums visible to the next
// across the eight L2s (the peel's argument).
//
// The blocks.  A tree edge is named by its child, so the union-find over the tree edges runs over vertex ids (roots of the
// forest stay alone and name nothing).  (i) a non-tree edge between unrelated vertices joins their two tree edges;
// (ii) the tree edge (v, w), v = parent[w] not a root, joins v's own tree edge when something in w's subtree reaches
// outside v's subtree: low[w] < pre[v] or high[w] >= pre[v] + nd[v]; (iii) a non-tree edge goes with the tree edge of its
// endpoint of larger preorder number.  Whatever forest the schedule chose, the classes are the biconnected components.
// The labels, the counts per class (edges, tree edges -- a block's tree edges are a subtree: its vertices are one more --
// and the smallest canonical index) and everything per vertex follow in a constant number of launches; the 2-edge-connected
// components are a second union-find over the vertices along the edges of blocks of more than one edge.
//
// Races.  Every word that a launch both reads and writes it touches with atomics only (level[] in the BFS, nd[], the sibling
// cursors, low[] / high[], the union-finds' parent[], the counters); every plain store is read by a LATER launch.  What
// components.hip's header says about stale reads in the hooking union-find holds word for word for the three parent[]
// arrays here, and as there a compressing flatten launch is followed by a store-free labelling launch.  A stale read of
// level[] in the BFS can only show an unclaimed vertex that is claimed by now: the compare-and-swap then fails.  No
// workgroup waits for another.  The number of launches is 4 per level of the forest plus a constant.
#include "unionfind_dev.h"   // the union-find and its class tail; wave_dev.h: wave_append, wave_by_key

namespace komb {

namespace {

constexpr uint32_t kBiconnHeavy = 32;       // BFS rows longer than this: the vertex' wave (option BICONN_HEAVY)
constexpr uint32_t kBiconnBlockRow = 2048;  // ... and from this length on: its workgroup

struct BiconnCtl {                          // 64 bytes, zeroed before every run
    uint32_t tail;                          // BFS: vertices appended to order[] so far
    uint32_t pre_next;                      // preorder: the first number of the next root's interval
    uint32_t n_member_edges, n_bridges, largest_block;
    uint32_t n_articulation, n_ecc, largest_ecc;
    uint32_t pad[8];
};
static_assert(sizeof(BiconnCtl) == 64, "BiconnCtl layout");

// per vertex: the three union-finds start as singletons, nobody has a level, every counter is empty (deg has nv + 1 entries)
__global__ void k_bc_vinit(uint32_t nv, uint32_t *__restrict__ deg, uint32_t *__restrict__ fill, int32_t *__restrict__ cpar,
                           int32_t *__restrict__ bpar, int32_t *__restrict__ epar, int32_t *__restrict__ level, uint32_t *__restrict__ nd,
                           uint32_t *__restrict__ cursor, int32_t *__restrict__ blockmin, uint32_t *__restrict__ edges,
                           uint32_t *__restrict__ tree, uint32_t *__restrict__ top, uint32_t *__restrict__ ecnt)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v > nv) return;
    deg[v] = 0u;
    if (v == nv) return;
    fill[v] = 0u; cpar[v] = bpar[v] = epar[v] = (int32_t)v; level[v] = -1; nd[v] = 1u; cursor[v] = 0u;
    blockmin[v] = 0x7FFFFFFF; edges[v] = 0u; tree[v] = 0u; top[v] = 0u; ecnt[v] = 0u;
}

// the member list in canonical order; the degrees of the member graph; its connected components (cpar)
__global__ void k_bc_compact(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int32_t *__restrict__ truss,
                             uint32_t m, int32_t k, const uint32_t *__restrict__ pos, int32_t *__restrict__ kept,
                             int32_t *__restrict__ mu, int32_t *__restrict__ mv, uint32_t *deg, int32_t *cpar)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || truss[i] < k) return;
    const uint32_t j = pos[i];
    const int32_t u = eu[i], v = ev[i];
    kept[j] = (int32_t)i; mu[j] = u; mv[j] = v;
    atomicAdd(deg + u, 1u); atomicAdd(deg + v, 1u);
    comp_link(cpar, u, v);
}

// both directions of every member edge into the rows (row order: whoever comes first)
__global__ void k_bc_fill(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, uint32_t nm, const uint32_t *__restrict__ rowptr,
                          uint32_t *fill, int32_t *__restrict__ adj)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nm) return;
    const int32_t u = mu[j], v = mv[j];
    adj[rowptr[u] + atomicAdd(fill + u, 1u)] = v;
    adj[rowptr[v] + atomicAdd(fill + v, 1u)] = u;
}

// level 0: a member whose word of cpar still holds its own id is the smallest id of its component (every link has landed)
__global__ void k_bc_roots(uint32_t nv, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ cpar, int32_t *__restrict__ level,
                           int32_t *__restrict__ par, int32_t *__restrict__ order, BiconnCtl *ctl)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool root = v < nv && rowptr[v + 1] > rowptr[v] && cpar[v] == (int32_t)v;
    const uint32_t slot = wave_append(root, &ctl->tail);
    if (v < nv) par[v] = -1;
    if (root) { level[v] = 0; order[slot] = (int32_t)v; }
}

// entry i of the row of frontier vertex v: whoever moves level[w] from -1 owns w
__device__ __forceinline__ void bc_claim(bool act, int32_t v, uint32_t i, int32_t next_level, const int32_t *__restrict__ adj, int32_t *level,
                                         int32_t *__restrict__ par, int32_t *__restrict__ order, BiconnCtl *ctl)
{
    bool won = false;
    int32_t w = -1;
    if (act) {
        w = adj[i];
        if (pload(level + w) < 0) won = atomicCAS(level + w, -1, next_level) == -1;
    }
    const uint32_t slot = wave_append(won, &ctl->tail);
    if (won) { par[w] = v; order[slot] = w; }
}

// one BFS level: the frontier is order[lo, hi).  A short row stays with its lane (the lanes of a wave step together: the
// appends are per wave), longer ones are walked by the whole wave one after the other, the longest by the workgroup.
__global__ void __launch_bounds__(kBlock) k_bc_bfs(uint32_t lo, uint32_t hi, int32_t next_level, const uint32_t *__restrict__ rowptr,
                                                   const int32_t *__restrict__ adj, int32_t *level, int32_t *__restrict__ par,
                                                   int32_t *__restrict__ order, BiconnCtl *ctl, uint32_t heavy)
{
    __shared__ int32_t s_big[kBlock];
    __shared__ uint32_t s_nbig;
    if (threadIdx.x == 0) s_nbig = 0u;
    __syncthreads();
    const uint32_t t = lo + blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int32_t v = -1;
    uint32_t b = 0, e = 0;
    if (t < hi) { v = order[t]; b = rowptr[v]; e = rowptr[v + 1]; }
    const uint32_t deg = e - b;
    const bool big = deg > heavy && deg >= kBiconnBlockRow, mid = !big && deg > heavy;
    if (big) s_big[atomicAdd(&s_nbig, 1u)] = v;
    const uint32_t se = big || mid ? b : e;              // (the lane's own walk: empty for a row it hands on)
    for (uint32_t i = b; __any(i < se); ++i) bc_claim(i < se, v, i, next_level, adj, level, par, order, ctl);
    unsigned long long m = __ballot(mid);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int32_t rv = __shfl(v, src);
        const uint32_t rb = (uint32_t)__shfl((int32_t)b, src), re = (uint32_t)__shfl((int32_t)e, src);
        for (uint32_t i = rb + (uint32_t)lane; __any(i < re); i += kWave) bc_claim(i < re, rv, i, next_level, adj, level, par, order, ctl);
    }
    __syncthreads();
    const uint32_t nbig = s_nbig;
    for (uint32_t h = 0; h < nbig; ++h) {
        const int32_t rv = s_big[h];
        const uint32_t rb = rowptr[rv], re = rowptr[rv + 1];
        for (uint32_t i = rb + threadIdx.x; __any(i < re); i += kBlock) bc_claim(i < re, rv, i, next_level, adj, level, par, order, ctl);
    }
}

// bottom-up, level by level: nd[parent] += nd[x] (nd[x] is complete: the level below ran in the launch before)
__global__ void k_bc_nd_up(uint32_t lo, uint32_t hi, const int32_t *__restrict__ order, const int32_t *__restrict__ par, uint32_t *nd)
{
    const uint32_t t = lo + blockIdx.x * kBlock + threadIdx.x;
    if (t >= hi) return;
    const int32_t x = order[t];
    atomicAdd(nd + par[x], nd[x]);
}

// top-down, level by level: roots take disjoint intervals from one cursor, a child the next nd[x] numbers behind its parent's
__global__ void k_bc_pre_down(uint32_t lo, uint32_t hi, bool roots, const int32_t *__restrict__ order, const int32_t *__restrict__ par,
                              const uint32_t *__restrict__ nd, uint32_t *cursor, int32_t *__restrict__ pre, int32_t *__restrict__ low,
                              int32_t *__restrict__ high, BiconnCtl *ctl)
{
    const uint32_t t = lo + blockIdx.x * kBlock + threadIdx.x;
    if (t >= hi) return;
    const int32_t x = order[t];
    uint32_t p;
    if (roots) p = atomicAdd(&ctl->pre_next, nd[x]);
    else { const int32_t q = par[x]; p = (uint32_t)pre[q] + 1u + atomicAdd(cursor + q, nd[x]); }
    pre[x] = low[x] = high[x] = (int32_t)p;
}

constexpr uint32_t kBiconnTree = 0x80000000u;   // ec[]: the edge is a tree edge (the low bits: its child)

// one flat pass over the member edges once pre[] and nd[] stand.  ec[j] = the vertex whose tree edge names j's class (rule iii):
// the child of a tree edge, the endpoint of larger preorder number of a non-tree edge.  A non-tree edge gives each end the
// other's preorder number, and joins the two tree edges when its ends are unrelated (rule i).
__global__ void k_bc_reach(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, uint32_t nm, const int32_t *__restrict__ par,
                           const int32_t *__restrict__ pre, const uint32_t *__restrict__ nd, int32_t *low, int32_t *high, int32_t *bpar,
                           uint32_t *__restrict__ ec)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nm) return;
    int32_t u = mu[j], v = mv[j];
    if (par[v] == u) { ec[j] = (uint32_t)v | kBiconnTree; return; }
    if (par[u] == v) { ec[j] = (uint32_t)u | kBiconnTree; return; }
    int32_t pu = pre[u], pv = pre[v];
    // (low[] only falls and high[] only rises in this launch: a value read as reached already is reached, however stale the
    // read, and the atomic is skipped -- a hub's two words settle after a few of its edges instead of taking one atomic each)
    if (pload(low + u) > pv) atomicMin(low + u, pv);
    if (pload(high + u) < pv) atomicMax(high + u, pv);
    if (pload(low + v) > pu) atomicMin(low + v, pu);
    if (pload(high + v) < pu) atomicMax(high + v, pu);
    if (pu > pv) { int32_t t = u; u = v; v = t; t = pu; pu = pv; pv = t; }
    ec[j] = (uint32_t)v;
    if (pu + (int32_t)nd[u] <= pv) comp_link(bpar, u, v);
}

// bottom-up, level by level: a child's pair folds into its parent's
__global__ void k_bc_reach_up(uint32_t lo, uint32_t hi, const int32_t *__restrict__ order, const int32_t *__restrict__ par, int32_t *low, int32_t *high)
{
    const uint32_t t = lo + blockIdx.x * kBlock + threadIdx.x;
    if (t >= hi) return;
    const int32_t x = order[t], p = par[x], lx = low[x], hx = high[x];
    if (pload(low + p) > lx) atomicMin(low + p, lx);      // (skipped when it is reached already: k_bc_reach)
    if (pload(high + p) < hx) atomicMax(high + p, hx);
}

// rule (ii) per non-root w whose parent is no root; n_blocks[] starts with the block of the vertex' own tree edge
__global__ void k_bc_link_tree(uint32_t nv, const int32_t *__restrict__ level, const int32_t *__restrict__ par, const int32_t *__restrict__ pre,
                               const uint32_t *__restrict__ nd, const int32_t *__restrict__ low, const int32_t *__restrict__ high,
                               int32_t *bpar, int32_t *__restrict__ n_blocks)
{
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w >= nv) return;
    const int32_t lw = level[w];
    n_blocks[w] = lw > 0 ? 1 : 0;
    if (lw < 2) return;                                   // (level 1: the parent is a root)
    const int32_t v = par[w], pv = pre[v];
    if (low[w] < pv || high[w] >= pv + (int32_t)nd[v]) comp_link(bpar, v, (int32_t)w);
}

// !kFinal: every vertex points itself at the root it finds, its walk splitting the paths it passes.  kFinal: parent[v] = root
// of v; read-only walks.
template <bool kFinal>
__global__ void k_bc_flatten(uint32_t nv, int32_t *parent)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    comp_flatten<kFinal>(parent, v);
}

// eblk[j] = the class of member edge j, read off ec[j] (the same words: every lane rewrites its own); per class the edges,
// the tree edges and the smallest canonical index.  k_class_count's scheme with three accumulators: lanes of a wave that share
// a class add once (the lowest lane of them holds the smallest index: kept[] ascends), and what a workgroup adds to the class
// its first tile starts with (the giant block's, nearly always) it sums in LDS first.
__global__ void k_bc_edge_blocks(const int32_t *__restrict__ kept, uint32_t nm, const int32_t *__restrict__ blabel, int32_t *eblk,
                                 int32_t *blockmin, uint32_t *edges, uint32_t *tree)
{
    __shared__ int32_t s_first, s_min;
    __shared__ uint32_t s_sum, s_tree;
    if (threadIdx.x == 0) { s_first = -1; s_min = 0x7FFFFFFF; s_sum = 0u; s_tree = 0u; }
    __syncthreads();
    for (uint32_t base = blockIdx.x * kBlock; base < nm; base += gridDim.x * kBlock) {      // (uniform per workgroup: the ballots see whole waves)
        const uint32_t j = base + threadIdx.x;
        int32_t lab = -1, idx = 0x7FFFFFFF;
        bool is_tree = false;
        if (j < nm) {
            const uint32_t c = (uint32_t)eblk[j];
            is_tree = (c & kBiconnTree) != 0u;
            lab = blabel[c & ~kBiconnTree]; idx = kept[j];
            eblk[j] = lab;
        }
        if (base == blockIdx.x * kBlock) {                // the class of the workgroup's first edge
            if (threadIdx.x == 0) s_first = lab;
            __syncthreads();
        }
        const int32_t first = s_first;
        const bool act = lab >= 0;
        wave_by_key(act, lab, [&](int32_t lead, unsigned long long same, bool is_leader) {
            const uint32_t n_tree = (uint32_t)__popcll(__ballot(act && lab == lead && is_tree));
            if (!is_leader) return;
            if (lead == first) { atomicAdd(&s_sum, (uint32_t)__popcll(same)); atomicAdd(&s_tree, n_tree); atomicMin(&s_min, idx); }
            else { atomicAdd(edges + lead, (uint32_t)__popcll(same)); if (n_tree) atomicAdd(tree + lead, n_tree); atomicMin(blockmin + lead, idx); }
        });
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) {
        atomicAdd(edges + s_first, s_sum);
        if (s_tree) atomicAdd(tree + s_first, s_tree);
        atomicMin(blockmin + s_first, s_min);
    }
}

// the top of a block: the parent p of a vertex x of it that is a root of the forest or whose own tree edge lies in another
// block.  The first such x of a block adds it to n_blocks[p] (n_blocks[] holds the vertex' own block already).
__global__ void k_bc_tops(uint32_t nv, const int32_t *__restrict__ level, const int32_t *__restrict__ par, const int32_t *__restrict__ blabel,
                          uint32_t *top, int32_t *n_blocks)
{
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= nv || level[x] < 1) return;
    const int32_t p = par[x], lab = blabel[x];
    if (level[p] > 0 && blabel[p] == lab) return;
    if (atomicExch(top + lab, 1u) == 0u) atomicAdd(n_blocks + p, 1);
}

// the 2-edge-connected components: the endpoints of every member edge that is no bridge are joined
__global__ void k_bc_ecc_link(const int32_t *__restrict__ mu, const int32_t *__restrict__ mv, uint32_t nm, const int32_t *__restrict__ eblk,
                              const uint32_t *__restrict__ edges, int32_t *epar)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nm || edges[eblk[j]] < 2u) return;
    comp_link(epar, mu[j], mv[j]);
}

// ecc_label[v] = the smallest id of v's class (members), -1 (others); read-only walks, the result in an array of its own
__global__ void k_bc_ecc_label(uint32_t nv, const int32_t *__restrict__ level, const int32_t *epar, int32_t *__restrict__ label)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    label[v] = level[v] >= 0 ? comp_find_ro(epar, (int32_t)v) : -1;
}

// ecc_size[v]; the 2-edge-connected components and the largest; the articulation points; the largest block
__global__ void k_bc_vfinish(uint32_t nv, const int32_t *__restrict__ label, const uint32_t *__restrict__ cnt, const int32_t *__restrict__ n_blocks,
                             const uint32_t *__restrict__ edges, int32_t *__restrict__ ecc_size, BiconnCtl *ctl)
{
    uint32_t n_ecc = 0, n_art = 0, mx = 0, mxb = 0;
    for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nv; v += gridDim.x * kBlock) {
        const int32_t lab = label[v];
        const uint32_t sz = lab >= 0 ? cnt[lab] : 0u, eb = edges[v];
        ecc_size[v] = (int32_t)sz;
        if (lab == (int32_t)v) { ++n_ecc; mx = sz > mx ? sz : mx; }
        n_art += n_blocks[v] >= 2 ? 1u : 0u;
        mxb = eb > mxb ? eb : mxb;
    }
    n_ecc = wave_sum(n_ecc); n_art = wave_sum(n_art); mx = wave_max(mx); mxb = wave_max(mxb);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (n_ecc) { atomicAdd(&ctl->n_ecc, n_ecc); atomicMax(&ctl->largest_ecc, mx); }
        if (n_art) atomicAdd(&ctl->n_articulation, n_art);
        if (mxb) atomicMax(&ctl->largest_block, mxb);
    }
}

// canonical order again: block[i], size[i] (-1 / 0 for a non-member); is_rep[i] = edge i is the smallest of its block
// (is_rep[m] = 0: the scan's last entry is the number of blocks); member edges and bridges summed up per wave
__global__ void k_bc_efinish(uint32_t m, const int32_t *__restrict__ truss, int32_t k, const uint32_t *__restrict__ pos,
                             const int32_t *__restrict__ eblk, const int32_t *__restrict__ blockmin, const uint32_t *__restrict__ edges,
                             int32_t *__restrict__ block, int32_t *__restrict__ size, uint32_t *__restrict__ is_rep, BiconnCtl *ctl)
{
    uint32_t n_mem = 0, n_bridge = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i <= m; i += gridDim.x * kBlock) {
        if (i == m) { is_rep[i] = 0u; continue; }
        int32_t lab = -1; uint32_t sz = 0u;
        if (truss[i] >= k) {
            const int32_t r = eblk[pos[i]];
            lab = blockmin[r]; sz = edges[r];
            ++n_mem; n_bridge += sz == 1u ? 1u : 0u;
        }
        block[i] = lab; size[i] = (int32_t)sz;
        is_rep[i] = lab == (int32_t)i ? 1u : 0u;
    }
    n_mem = wave_sum(n_mem); n_bridge = wave_sum(n_bridge);
    if ((threadIdx.x & (kWave - 1)) == 0 && n_mem) { atomicAdd(&ctl->n_member_edges, n_mem); if (n_bridge) atomicAdd(&ctl->n_bridges, n_bridge); }
}

// the block list in ascending rep order: the reps are canonical indices, so a scan over is_rep[] places them
__global__ void k_bc_list(uint32_t m, const int32_t *__restrict__ block, const int32_t *__restrict__ size, const uint32_t *__restrict__ rpos,
                          const uint32_t *__restrict__ pos, const int32_t *__restrict__ eblk, const uint32_t *__restrict__ tree,
                          int32_t *__restrict__ rep, int32_t *__restrict__ n_edges, int32_t *__restrict__ n_verts)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || block[i] != (int32_t)i) return;
    const uint32_t b = rpos[i];
    rep[b] = (int32_t)i; n_edges[b] = size[i]; n_verts[b] = (int32_t)tree[eblk[pos[i]]] + 1;
}

// a result without members: block = -1, size = 0
__global__ void k_bc_no_edges(uint32_t m, int32_t *__restrict__ block, int32_t *__restrict__ size)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    block[i] = -1; size[i] = 0;
}

__global__ void k_bc_no_vertices(uint32_t nv, int32_t *__restrict__ n_blocks, int32_t *__restrict__ ecc_label, int32_t *__restrict__ ecc_size)
{
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    n_blocks[v] = 0; ecc_label[v] = -1; ecc_size[v] = 0;
}

} // namespace

// k is checked and resolved by the caller (api.cpp): >= 2
int biconnected_run(komb_ctx *ctx, int32_t k)
{
    hipStream_t s = ctx->stream;
    const int64_t m = ctx->t_ne > 0 ? ctx->t_ne : 0, nv = ctx->nv;
    ctx->bc = {};                                        // a run that fails leaves no result (include/komb_accel.h)
    komb_ctx::Biconnected res;                           // goes back to the pool unless it is installed
    res.k = k;
    if (m > 0) KOMB_TRY(truss_edges_canonical(ctx));     // (a whole-graph result whose endpoints no fetch has asked for yet)

    Range r_all("komb_biconnected_run");
    KOMB_HIP(ctx, ctx->pool.get((void **)res.block.slot(&ctx->pool), (size_t)m * sizeof(int32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.size.slot(&ctx->pool), (size_t)m * sizeof(int32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.nblocks.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.ecc_label.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.ecc_size.slot(&ctx->pool), (size_t)nv * sizeof(int32_t)));
    int32_t *block = res.block, *size = res.size, *n_blocks = res.nblocks, *ecc_label = res.ecc_label;
    const int32_t *eu = ctx->d_t_eu, *ev = ctx->d_t_ev, *truss = ctx->d_t_truss;
    const int vgrid = tiles_of(nv), egrid = tiles_of(m);

    DevBufs bufs(ctx);
    BiconnCtl *d_ctl = nullptr;
    uint32_t *d_flag = nullptr, *d_pos = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_ctl, 1));
    KOMB_HIP(ctx, bufs.alloc(&d_flag, (size_t)m + 1));   // membership for the scan; then is_rep[] for the block list's
    KOMB_HIP(ctx, bufs.alloc(&d_pos, (size_t)m + 1));
    ctx->timer.start(s);
    KOMB_HIP(ctx, hipMemsetAsync(d_ctl, 0, sizeof(BiconnCtl), s));
    uint32_t nm = 0;
    if (m > 0) {
        KOMB_TRY(prim_flag_ge_scan(ctx, truss, m, k, d_flag, d_pos));
        KOMB_HIP(ctx, d2h(ctx, &nm, d_pos + m, sizeof(uint32_t)));
    }
    if (nm == 0) {                                       // no member edge: nothing to traverse
        if (m > 0) k_bc_no_edges<<<egrid, kBlock, 0, s>>>((uint32_t)m, block, size);
        if (nv > 0) k_bc_no_vertices<<<vgrid, kBlock, 0, s>>>((uint32_t)nv, n_blocks, ecc_label, res.ecc_size);
        res.ms = ctx->timer.stop(s);
        KOMB_HIP(ctx, hipGetLastError());
        res.done = true;
        ctx->bc = std::move(res);
        return KOMB_OK;
    }
    if (2ull * nm > 0xFFFFFFFFull)
        KOMB_FAIL(ctx, KOMB_ERR_LIMIT, "komb_biconnected_run: %u member edges; the rows of both directions need 32-bit offsets", nm);

    // ---- the member list, its symmetric CSR, the roots
    uint32_t *d_rowptr = nullptr, *d_fill = nullptr, *d_nd = nullptr, *d_cursor = nullptr, *d_edges = nullptr, *d_tree = nullptr,
             *d_top = nullptr, *d_ecnt = nullptr;
    int32_t *d_kept = nullptr, *d_mu = nullptr, *d_mv = nullptr, *d_eblk = nullptr, *d_adj = nullptr, *d_cpar = nullptr, *d_bpar = nullptr,
            *d_epar = nullptr, *d_level = nullptr, *d_par = nullptr, *d_order = nullptr, *d_pre = nullptr, *d_low = nullptr, *d_high = nullptr,
            *d_blockmin = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&d_kept, (size_t)nm));
    KOMB_HIP(ctx, bufs.alloc(&d_mu, (size_t)nm));
    KOMB_HIP(ctx, bufs.alloc(&d_mv, (size_t)nm));
    KOMB_HIP(ctx, bufs.alloc(&d_eblk, (size_t)nm));
    KOMB_HIP(ctx, bufs.alloc(&d_adj, 2 * (size_t)nm));
    KOMB_HIP(ctx, bufs.alloc(&d_rowptr, (size_t)nv + 1));
    for (uint32_t **p : {&d_fill, &d_nd, &d_cursor, &d_edges, &d_tree, &d_top, &d_ecnt}) KOMB_HIP(ctx, bufs.alloc(p, (size_t)nv));
    for (int32_t **p : {&d_cpar, &d_bpar, &d_epar, &d_level, &d_par, &d_order, &d_pre, &d_low, &d_high, &d_blockmin})
        KOMB_HIP(ctx, bufs.alloc(p, (size_t)nv));
    const uint32_t heavy = ctx_opt_u32(ctx, "BICONN_HEAVY", kBiconnHeavy);      // (tests: every row through the wave)
    const int mgrid = tiles_of(nm);

    Range r_part("biconnected: member graph");
    k_bc_vinit<<<tiles_of(nv + 1), kBlock, 0, s>>>((uint32_t)nv, d_rowptr, d_fill, d_cpar, d_bpar, d_epar, d_level, d_nd, d_cursor, d_blockmin,
                                                   d_edges, d_tree, d_top, d_ecnt);
    k_bc_compact<<<egrid, kBlock, 0, s>>>(eu, ev, truss, (uint32_t)m, k, d_pos, d_kept, d_mu, d_mv, d_rowptr, d_cpar);
    KOMB_TRY(prim_exclusive_sum_u32(ctx, d_rowptr, d_rowptr, nv + 1));
    k_bc_fill<<<mgrid, kBlock, 0, s>>>(d_mu, d_mv, nm, d_rowptr, d_fill, d_adj);
    k_bc_roots<<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_rowptr, d_cpar, d_level, d_par, d_order, d_ctl);

    // ---- the BFS: off[L] = where level L starts in order[]; the host reads the cursor once per level
    r_part.next("biconnected: BFS");
    std::vector<uint32_t> off{0u};
    uint32_t tail = 0;
    KOMB_HIP(ctx, d2h(ctx, &tail, &d_ctl->tail, sizeof(uint32_t)));
    while (tail > off.back()) {
        if (tail > (uint32_t)nv) KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_biconnected_run: the BFS queued %u of %lld vertices", tail, (long long)nv);
        const uint32_t lo = off.back();
        off.push_back(tail);
        k_bc_bfs<<<tiles_of(tail - lo), kBlock, 0, s>>>(lo, tail, (int32_t)off.size() - 1, d_rowptr, d_adj, d_level, d_par, d_order, d_ctl, heavy);
        KOMB_HIP(ctx, d2h(ctx, &tail, &d_ctl->tail, sizeof(uint32_t)));
    }
    const int depth = (int)off.size() - 1;               // levels 0 .. depth - 1 are order[off[L], off[L + 1])
    const uint32_t nmv = tail;

    // ---- the three sweeps
    r_part.next("biconnected: sweeps");
    for (int L = depth - 1; L >= 1; --L)
        k_bc_nd_up<<<tiles_of(off[L + 1] - off[L]), kBlock, 0, s>>>(off[L], off[L + 1], d_order, d_par, d_nd);
    for (int L = 0; L < depth; ++L)
        k_bc_pre_down<<<tiles_of(off[L + 1] - off[L]), kBlock, 0, s>>>(off[L], off[L + 1], L == 0, d_order, d_par, d_nd, d_cursor, d_pre, d_low, d_high, d_ctl);
    k_bc_reach<<<mgrid, kBlock, 0, s>>>(d_mu, d_mv, nm, d_par, d_pre, d_nd, d_low, d_high, d_bpar, (uint32_t *)d_eblk);
    for (int L = depth - 1; L >= 1; --L)
        k_bc_reach_up<<<tiles_of(off[L + 1] - off[L]), kBlock, 0, s>>>(off[L], off[L + 1], d_order, d_par, d_low, d_high);

    // ---- the blocks
    r_part.next("biconnected: blocks");
    k_bc_link_tree<<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_level, d_par, d_pre, d_nd, d_low, d_high, d_bpar, n_blocks);
    k_bc_flatten<false><<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_bpar);
    k_bc_flatten<true><<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_bpar);
    k_bc_edge_blocks<<<class_tail_grid(nm), kBlock, 0, s>>>(d_kept, nm, d_bpar, d_eblk, d_blockmin, d_edges, d_tree);
    k_bc_tops<<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_level, d_par, d_bpar, d_top, n_blocks);
    k_bc_efinish<<<class_tail_grid(m + 1), kBlock, 0, s>>>((uint32_t)m, truss, k, d_pos, d_eblk, d_blockmin, d_edges, block, size, d_flag, d_ctl);

    // ---- the 2-edge-connected components
    r_part.next("biconnected: 2-edge-connected");
    k_bc_ecc_link<<<mgrid, kBlock, 0, s>>>(d_mu, d_mv, nm, d_eblk, d_edges, d_epar);
    k_bc_flatten<false><<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_epar);
    k_bc_ecc_label<<<vgrid, kBlock, 0, s>>>((uint32_t)nv, d_level, d_epar, ecc_label);
    class_count(ctx, nv, nullptr, ecc_label, d_ecnt);
    k_bc_vfinish<<<class_tail_grid(nv), kBlock, 0, s>>>((uint32_t)nv, ecc_label, d_ecnt, n_blocks, d_edges, res.ecc_size, d_ctl);

    // ---- the block list
    r_part.next("biconnected: block list");
    KOMB_TRY(prim_exclusive_sum_u32(ctx, d_flag, d_flag, m + 1));      // (in place: is_rep[] becomes the position in the list)
    uint32_t nb = 0;
    KOMB_HIP(ctx, d2h(ctx, &nb, d_flag + m, sizeof(uint32_t)));
    KOMB_HIP(ctx, ctx->pool.get((void **)res.list.slot(&ctx->pool), 3 * (size_t)(nb ? nb : 1) * sizeof(int32_t)));
    if (nb) k_bc_list<<<egrid, kBlock, 0, s>>>((uint32_t)m, block, size, d_flag, d_pos, d_eblk, d_tree, res.list, res.list + nb,
                                               res.list + 2 * (size_t)nb);
    const double ms = ctx->timer.stop(s);
    KOMB_HIP(ctx, hipGetLastError());
    BiconnCtl h;
    KOMB_HIP(ctx, d2h(ctx, &h, d_ctl, sizeof(BiconnCtl)));
    if (h.n_member_edges != nm || h.tail != nmv || h.pre_next != nmv)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "komb_biconnected_run: inconsistent counts (%u of %u member edges, %u of %u vertices numbered)",
                  h.n_member_edges, nm, h.pre_next, nmv);
    res.n_member_edges = (int64_t)nm; res.n_member_vertices = (int64_t)nmv; res.n_blocks = (int64_t)nb;
    res.n_bridges = (int64_t)h.n_bridges; res.n_articulation = (int64_t)h.n_articulation; res.largest_block = (int64_t)h.largest_block;
    res.n_ecc = (int64_t)h.n_ecc; res.largest_ecc = (int64_t)h.largest_ecc;
    res.depth = depth; res.ms = ms;
    res.done = true;
    ctx->bc = std::move(res);
    return KOMB_OK;
}

} // namespace komb
