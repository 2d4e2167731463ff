// unionfind_dev.h -- the scheduling-independent union-find by hooking that components.hip (over vertex ids) and
// communities.hip (over edge ids) share.  parent[x] <= x always: a root is hooked under a SMALLER id by a
// compare-and-swap, every walk goes through strictly decreasing ids (so it ends, whatever it reads), and the root of a
// finished class is its smallest id.  Why stale reads across the non-coherent per-XCD L2s are harmless, and why the
// labels are read by a later, store-free launch: the header comment of components.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

} // namespace komb
