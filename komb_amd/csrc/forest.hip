// forest.hip -- the forest builder: what the nesting forests of hierarchy.hip (components of the k-cores / k-trusses over
// vertices), community_hierarchy.hip (k-truss communities over edges) and nucleus_hierarchy.hip ((3,4)-nuclei over triangles)
// share.  DESIGN.md section 4.6d, "The forest builder".
//
// The caller has ITEMS, each with a level, bucketed by level (a sort and forest_offsets), and one union-find over item ids
// (unionfind_dev.h: a root is the smallest id of its tree, whatever the schedule).  It takes the levels from the largest k
// down; at each populated level its own LINK kernels join what binds at that level -- so that the trees are then the
// classes of threshold k -- and log every HOOK: comp_link_hooked reports the root it hung under a smaller id.  An item is
// hooked at most once in the whole run (it is never a root again), so one log of `cap` entries holds all levels, each a
// segment.  Behind LINK, forest_level queues two launches, a kernel boundary between all three: no hook is in flight
// when roots are read, and a word written by one launch is read by a later one only.
//   CLAIM  for every hooked x: cnt[root] += cnt[x] (x was a root before this level: cnt[x] is final), and ONE lane per root
//          makes the node (k, root); a node the root stood for before becomes its child.  For every item of the level:
//          cnt[root] += 1.
//   ADOPT  for every hooked x that stood for a node: that node's parent is its root's node.  For every item of the level:
//          node[item] = its root's node, whose shell counts it.  A node's size is its root's count.
// forest_tail sorts the nodes by (k, rep), which numbers them whatever order the schedule made them in, and maps the parents
// through the ranks; the caller maps node[] (its *_out kernel).
//
// Why this is right, whoever the items are:
// - At most `cap` nodes, nothing counted first.  The item set of a class changes at level k exactly when one of its items is
//   hooked at level k: an item that enters at level k binds to something at this level (each caller's header says why), it
//   was alone before, so the tree it ends the level in holds an item hooked at this level.  Hence the roots of the hooked
//   items are this level's nodes and every node has a hooked item of its own -- or is an item that nothing binds (the core
//   kind's isolated vertices at k = 0: `isolated`, every item of the level claims for itself).  The host checks n_nodes and
//   log_n against cap all the same, and every append is guarded.
// - One node per root and level.  claimk[r] is the level r's latest node was made at; it only falls, since the levels
//   descend.  The lane whose atomicMin lowers it to k makes the node; a plain read that is stale costs the atomic, no more.
// - cur[r] is private to the claimer.  CLAIM hooks nothing, so an item read as a root after the LINK launches is one (a
//   stale parent word ends a walk early only DURING linking launches), there is one claimer per root and launch, and nobody
//   else touches cur[r] in CLAIM.  ADOPT only reads cur[].  CLAIM's walks still split the paths they pass -- parent[] is no
//   output here, and ADOPT's read-only walks are then a step or two.
// - Every walk ends.  Union-find walks go through strictly decreasing ids.  In the final numbering a parent has a smaller
//   number than its child ((k, rep) order: a parent has a smaller k), and the depth walk and forest_walk_up follow only such
//   parents.
// - Every ballot sits in a loop whose bounds are uniform over its workgroup, so all lanes of a wave take part in it.
// - The hot word.  Nearly all items end in one giant class, whose cnt / shell word would take one atomic per wave.  What
//   goes to the root (CLAIM) or node (ADOPT) of the workgroup's first entry is summed in LDS and added once per workgroup
//   (k_class_count's scheme).
// Every access to parent[] is a relaxed agent-scope atomic (the header comment of components.hip says why that suffices).
#include "forest_dev.h"

namespace komb {

namespace {

__global__ void k_forest_offsets(uint32_t n, const uint32_t *__restrict__ keys, uint32_t levels, uint32_t *__restrict__ off)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    const uint32_t first = i > 0 ? keys[i - 1] + 1u : 0u;
    const uint32_t last = i < n ? keys[i] : levels;
    for (uint32_t k = first; k <= last && k <= levels; ++k) off[k] = i;      // (every word written exactly once)
}

// arr[key] += 1 for every lane with key >= 0: the lanes of a wave that share a key add once, and what goes to `first` is
// summed in *s_sum (LDS) for the workgroup's one global atomic.  Every lane of the wave calls it.
__device__ __forceinline__ void forest_group_add(uint32_t *arr, int32_t key, int32_t first, uint32_t *s_sum)
{
    wave_by_key(key >= 0, key, [&](int32_t lead, unsigned long long same, bool is_leader) {
        if (!is_leader) return;
        if (lead == first) atomicAdd(s_sum, (uint32_t)__popcll(same));
        else atomicAdd(arr + lead, (uint32_t)__popcll(same));
    });
}

// the node (k, r) of root r, made by the first lane that asks for it at this level
__device__ __forceinline__ void forest_claim(int32_t r, int32_t k, ForestCtl *ctl, int32_t *claimk, int32_t *cur, const ForestNodes &t, uint32_t cap)
{
    if (pload(claimk + r) <= k) return;
    if (atomicMin(claimk + r, k) <= k) return;
    const uint32_t id = atomicAdd(&ctl->n_nodes, 1u);
    if (id >= cap) return;                   // (cannot happen; the host checks n_nodes)
    t.k[id] = k; t.rep[id] = r; t.par[id] = -1; t.size[id] = 0u; t.shell[id] = 0u;
    const int32_t prev = cur[r];
    if (prev >= 0) t.par[prev] = (int32_t)id;    // the same root stood for a class of a higher level: now a child
    cur[r] = (int32_t)id;
}

// CLAIM.  seg[li] .. log_n is the level's segment of the log; order[sh_b .. sh_b + sh_n) are the level's items.
__global__ void k_forest_claim(int32_t k, uint32_t li, bool isolated, const uint32_t *__restrict__ order, uint32_t sh_b, uint32_t sh_n,
                               int32_t *parent, const int32_t *__restrict__ log, uint32_t *seg, ForestCtl *ctl, int32_t *claimk,
                               int32_t *cur, uint32_t *cnt, ForestNodes t, uint32_t cap)
{
    __shared__ int32_t s_first;
    __shared__ uint32_t s_sum;
    const uint32_t lb = seg[li];
    uint32_t le = ctl->log_n;
    if (le > cap) le = cap;
    const uint32_t b0 = blockIdx.x * kBlock, stride = gridDim.x * kBlock;
    if (b0 + threadIdx.x == 0) seg[li + 1] = le;                 // (read by later launches only)
    if (threadIdx.x == 0) {                                      // the root this workgroup's first entry has
        s_first = lb + b0 < le ? comp_find(parent, log[lb + b0]) : (b0 < sh_n ? comp_find(parent, (int32_t)order[sh_b + b0]) : -1);
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
        mine = wave_sum(mine);
        if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(&s_sum, mine);
        wave_by_key(r >= 0, r, [&](int32_t lead, unsigned long long, bool is_leader) {   // one lane per distinct root asks for its node
            if (is_leader) forest_claim(lead, k, ctl, claimk, cur, t, cap);
        });
    }
    for (uint32_t base = b0; base < sh_n; base += stride) {      // (uniform per workgroup)
        const uint32_t j = base + threadIdx.x;
        const int32_t r = j < sh_n ? comp_find(parent, (int32_t)order[sh_b + j]) : -1;
        if (isolated && r >= 0) forest_claim(r, k, ctl, claimk, cur, t, cap);    // every item is its own root
        forest_group_add(cnt, r, first, &s_sum);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(cnt + first, s_sum);
}

// ADOPT (after CLAIM: cur[] of this level's roots is settled)
__global__ void k_forest_adopt(uint32_t li, const uint32_t *__restrict__ order, uint32_t sh_b, uint32_t sh_n, const int32_t *parent,
                               const int32_t *__restrict__ log, const uint32_t *__restrict__ seg, const int32_t *__restrict__ cur,
                               const uint32_t *__restrict__ cnt, ForestNodes t, int32_t *__restrict__ node)
{
    __shared__ int32_t s_first;
    __shared__ uint32_t s_sum;
    const uint32_t lb = seg[li], le = seg[li + 1];
    const uint32_t b0 = blockIdx.x * kBlock, stride = gridDim.x * kBlock;
    if (threadIdx.x == 0) {                                      // the node this workgroup's first item goes to
        s_first = b0 < sh_n ? cur[comp_find_ro(parent, (int32_t)order[sh_b + b0])] : -1;
        s_sum = 0u;
    }
    __syncthreads();
    const int32_t first = s_first;
    for (uint32_t i = lb + b0 + threadIdx.x; i < le; i += stride) {
        const int32_t x = log[i];
        const int32_t r = comp_find_ro(parent, x);
        const int32_t nr = cur[r], nx = cur[x];
        if (nr < 0) continue;
        if (nx >= 0) t.par[nx] = nr;         // x was the root of a class of a higher level
        t.size[nr] = cnt[r];                 // (every writer stores the same word)
    }
    for (uint32_t base = b0; base < sh_n; base += stride) {      // (uniform per workgroup)
        const uint32_t j = base + threadIdx.x;
        int32_t nr = -1;
        if (j < sh_n) {
            const int32_t e = (int32_t)order[sh_b + j];
            const int32_t r = comp_find_ro(parent, e);
            nr = cur[r];
            node[e] = nr;
            if (nr >= 0) t.size[nr] = cnt[r];
        }
        forest_group_add(t.shell, nr, first, &s_sum);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum && first >= 0) atomicAdd(t.shell + first, s_sum);
}

// ---- the tail: nodes into (k, rep) order
__global__ void k_forest_node_keys(uint32_t n, ForestNodes t, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((uint64_t)(uint32_t)t.k[i] << 32) | (uint32_t)t.rep[i];      // (rep_map is monotone: the order is that of the mapped reps)
    vals[i] = i;
}

__global__ void k_forest_ranks(uint32_t n, const uint32_t *__restrict__ order, int32_t *__restrict__ rank)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) rank[order[j]] = (int32_t)j;
}

__global__ void k_forest_nodes_out(uint32_t n, const uint32_t *__restrict__ order, const int32_t *__restrict__ rank,
                                   const int32_t *__restrict__ rep_map, ForestNodes t, ForestNodes out, ForestCtl *ctl)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool root = false;
    if (j < n) {
        const uint32_t i = order[j];
        const int32_t p = t.par[i], r = t.rep[i];
        out.k[j] = t.k[i]; out.rep[j] = rep_map ? rep_map[r] : r; out.par[j] = p >= 0 ? rank[p] : -1;
        out.size[j] = t.size[i]; out.shell[j] = t.shell[i];
        root = p < 0;
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(&ctl->n_roots, (uint32_t)__popcll(m));
}

// the most nodes on a path from a root down
__global__ void k_forest_depth(uint32_t n, const int32_t *__restrict__ par, ForestCtl *ctl)
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

} // namespace

void forest_offsets(komb_ctx *ctx, uint32_t n, const uint32_t *keys, uint32_t levels, uint32_t *off)
{
    k_forest_offsets<<<tiles_of((int64_t)n + 1), kBlock, 0, ctx->stream>>>(n, keys, levels, off);
}

void forest_level(komb_ctx *ctx, const ForestState &f, int32_t k, uint32_t li, bool isolated, const uint32_t *order, uint32_t sh_b,
                  uint32_t sh_n, uint64_t hooks)
{
    const uint64_t work = hooks > sh_n ? hooks : sh_n, wgs = (work + kBlock - 1) / kBlock;
    const int g = wgs < (uint64_t)kForestStepGrid ? (wgs > 0 ? (int)wgs : 1) : kForestStepGrid;
    k_forest_claim<<<g, kBlock, 0, ctx->stream>>>(k, li, isolated, order, sh_b, sh_n, f.parent, f.log, f.seg, f.ctl, f.claimk, f.cur, f.cnt,
                                                  f.made, f.cap);
    k_forest_adopt<<<g, kBlock, 0, ctx->stream>>>(li, order, sh_b, sh_n, f.parent, f.log, f.seg, f.cur, f.cnt, f.made, f.node);
}

int forest_tail(komb_ctx *ctx, DevBufs &bufs, const ForestState &f, uint32_t n, int bits, ForestNodes out, int32_t *rank,
                const int32_t *rep_map, uint32_t *vals, uint32_t *vals_alt)
{
    hipStream_t s = ctx->stream;
    uint64_t *nkeys = nullptr, *nkeys2 = nullptr, *nsorted = nullptr;
    uint32_t *order = nullptr;
    KOMB_HIP(ctx, bufs.alloc(&nkeys, (size_t)n));
    KOMB_HIP(ctx, bufs.alloc(&nkeys2, (size_t)n));
    const int grid = tiles_of(n);
    k_forest_node_keys<<<grid, kBlock, 0, s>>>(n, f.made, nkeys, vals);
    KOMB_TRY(prim_sort_pairs_u64_u32(ctx, nkeys, nkeys2, vals, vals_alt, n, 32 + bits, &nsorted, &order));
    k_forest_ranks<<<grid, kBlock, 0, s>>>(n, order, rank);
    k_forest_nodes_out<<<grid, kBlock, 0, s>>>(n, order, rank, rep_map, f.made, out, f.ctl);
    k_forest_depth<<<grid, kBlock, 0, s>>>(n, out.par, f.ctl);
    return KOMB_OK;
}

} // namespace komb
