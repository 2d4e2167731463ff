// forest_dev.h -- what the LINK and labels kernels of the three nesting forests (hierarchy.hip, community_hierarchy.hip,
// nucleus_hierarchy.hip) take from the forest builder (forest.hip): the append to the hook log and the walk over a stored
// forest.  The structures and the host side are in common.h.
#pragma once

#include "common.h"
#include "unionfind_dev.h"

namespace komb {

// a wave's hooks (hooked >= 0) into the log, its slots taken with one atomic.  Every lane of the wave calls it: a LINK
// kernel whose lanes diverge around the call (row loops of different lengths) appends per lane instead.
__device__ __forceinline__ void forest_log_wave(int32_t hooked, ForestCtl *ctl, int32_t *__restrict__ log, uint32_t cap)
{
    const unsigned long long m = __ballot(hooked >= 0);
    if (!m) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int lead = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(&ctl->log_n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int32_t)base, lead);
    if (hooked < 0) return;
    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (slot < cap) log[slot] = hooked;      // (cannot overflow: an item is hooked once)
}

// from node c (0 <= c < the number of nodes, level nk[c] >= k) up while the parent's level is still >= k: the node of c's
// class at threshold k.  Parents have smaller numbers, and the walk follows no other: it ends whatever par[] holds.
__device__ __forceinline__ int32_t forest_walk_up(int32_t c, int32_t k, const int32_t *__restrict__ nk, const int32_t *__restrict__ par)
{
    for (int32_t a = par[c]; a >= 0 && a < c && nk[a] >= k; a = par[a]) c = a;
    return c;
}

} // namespace komb
