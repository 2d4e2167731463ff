// unionfind_dev.h -- the scheduling-independent union-find by hooking that components.hip (over vertex ids) and
// communities.hip (over edge ids) share.  parent[x] <= x always: a root is hooked under a SMALLER id by a
// compare-and-swap, every walk goes through strictly decreasing ids (so it ends, whatever it reads), and the root of a
// finished class is its smallest id.  Why stale reads across the non-coherent per-XCD L2s are harmless, and why the
// labels are read by a later, store-free launch: the header comment of components.hip.  Behind the union-find, the tail its
// users share: the flatten step, the members counted per class (k_class_count), and the totals of a finish kernel.
#pragma once

#include "wave_dev.h"

namespace komb {

// every access to parent[] inside a linking launch: a relaxed agent-scope atomic (it bypasses the L1)
__device__ __forceinline__ int32_t pload(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pstore(int32_t *p, int32_t x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this lane can tell (a stale read ends the walk early: at a vertex of the same tree);
// path splitting on the way: every vertex passed is pointed at what was read as its grandparent
__device__ __forceinline__ int32_t comp_find(int32_t *parent, int32_t x)
{
    int32_t p = pload(parent + x);
    while (p < x) {
        const int32_t gp = pload(parent + p);
        if (gp < p) pstore(parent + x, gp);  // x is a non-root for good; gp was on the way up from it
        x = p; p = gp;
    }
    return x;
}

// the same walk without stores (the labelling launch: a word of parent[] is then written by its own vertex' lane only)
__device__ __forceinline__ int32_t comp_find_ro(const int32_t *parent, int32_t x)
{
    int32_t p = pload(parent + x);
    while (p < x) { x = p; p = pload(parent + x); }
    return x;
}

__device__ __forceinline__ void comp_link(int32_t *parent, int32_t u, int32_t v)
{
    int32_t a = comp_find(parent, u), b = comp_find(parent, v);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;               // hi was a root: it hangs under the smaller id now
        a = comp_find(parent, old);          // hi had been hooked already: go on from its parent (< hi)
        b = lo;
    }
}

// comp_link that reports its hook (hierarchy.hip): the root this call hung under a smaller id, -1 when u and v were in
// one tree already.  A vertex is a root until it is hooked and never again: over any number of launches every vertex is
// reported at most once.
__device__ __forceinline__ int32_t comp_link_hooked(int32_t *parent, int32_t u, int32_t v)
{
    int32_t a = comp_find(parent, u), b = comp_find(parent, v);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return hi;
        a = comp_find(parent, old);
        b = lo;
    }
    return -1;
}

// ---- the class tail
// One item of a flatten launch.  !kFinal: x points itself at the root it finds, its walk splitting the paths it passes (a hint:
// it may be overwritten by another walk's compression).  kFinal: parent[x] = root of x; read-only walks.
template <bool kFinal>
__device__ __forceinline__ void comp_flatten(int32_t *parent, uint32_t x)
{
    const int32_t r = kFinal ? comp_find_ro(parent, (int32_t)x) : comp_find(parent, (int32_t)x);
    if (r != (int32_t)x) pstore(parent + x, r);
}

// k_class_count and the finish kernels over n items: at most 2048 workgroups, each over several tiles
inline int class_tail_grid(int64_t n) { const int g = tiles_of(n); return g < 2048 ? g : 2048; }

// cnt[label] += the items that carry it, over label[0, n) (n, or *n_dev when the length is known on the device only: k_rows'
// convention).  An item has a label when (uint32_t)label < n -- a label indexes cnt[n], so the one test covers -1, a "none" word
// above every id and the lanes past the end alike.  What a workgroup adds to the label its first tile starts with (the giant
// class', nearly always) it sums in LDS first: one global atomic per workgroup, where the same-address atomics of every wave
// took 1.8 ms.  (&s_sum is named where it is added to: through a pointer argument the compiler merges
// the two adds into one flat atomic on a selected address.)
static __global__ void k_class_count(uint32_t n, const uint32_t *__restrict__ n_dev, const int32_t *__restrict__ label, uint32_t *cnt)
{
    __shared__ int32_t s_first;
    __shared__ uint32_t s_sum;
    if (n_dev) n = *n_dev;
    const uint32_t i0 = blockIdx.x * kBlock;
    if (threadIdx.x == 0) { s_first = i0 < n ? label[i0] : -1; s_sum = 0u; }
    __syncthreads();
    const int32_t first = s_first;
    for (uint32_t base = i0; base < n; base += gridDim.x * kBlock) {       // (uniform per workgroup: the ballots see whole waves)
        const uint32_t i = base + threadIdx.x;
        const int32_t lab = i < n ? label[i] : -1;
        wave_by_key((uint32_t)lab < n, lab, [&](int32_t lead, unsigned long long same, bool is_leader) {
            if (!is_leader) return;
            if (lead == first) atomicAdd(&s_sum, (uint32_t)__popcll(same));
            else atomicAdd(cnt + lead, (uint32_t)__popcll(same));
        });
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(cnt + first, s_sum);
}

// ... queued on the context's stream; n is the host's bound when n_dev is set, and sizes the grid
inline void class_count(komb_ctx *ctx, int64_t n, const uint32_t *n_dev, const int32_t *label, uint32_t *cnt)
{
    k_class_count<<<class_tail_grid(n), kBlock, 0, ctx->stream>>>((uint32_t)n, n_dev, label, cnt);
}

// The end of a finish kernel: this thread's members, classes (items that are their class' root) and largest class into the
// three words of the control block -- per wave, then per workgroup in LDS, then thread 0's atomics.  Every thread of the
// workgroup calls it once.
__device__ __forceinline__ void class_totals(uint32_t members, uint32_t classes, uint32_t largest, uint32_t *ctl_members, uint32_t *ctl_classes,
                                             uint32_t *ctl_largest)
{
    __shared__ uint32_t s_mem, s_cls, s_max;
    if (threadIdx.x == 0) { s_mem = 0u; s_cls = 0u; s_max = 0u; }
    __syncthreads();
    members = wave_sum(members); classes = wave_sum(classes); largest = wave_max(largest);
    if ((threadIdx.x & (kWave - 1)) == 0 && members) { atomicAdd(&s_mem, members); atomicAdd(&s_cls, classes); atomicMax(&s_max, largest); }
    __syncthreads();
    if (threadIdx.x == 0 && s_mem) {
        atomicAdd(ctl_members, s_mem);
        if (s_cls) { atomicAdd(ctl_classes, s_cls); atomicMax(ctl_largest, s_max); }
    }
}

} // namespace komb
