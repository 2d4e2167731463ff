// forest_dev.h -- what the LINK and labels kernels of the three nesting forests (hierarchy.hip, community_hierarchy.hip,
// nucleus_hierarchy.hip) take from the forest builder (forest.hip): the append to the hook log and the walk over a stored
// forest.  The structures and the host side are in common.h.
#pragma once

#include "unionfind_dev.h"

namespace komb {

// a wave's hooks (hooked >= 0) into the log, its slots taken with one atomic (wave_append).  Every lane of the wave calls
// it: a LINK kernel whose lanes diverge around the call (row loops of different lengths) appends per lane instead.
__device__ __forceinline__ void forest_log_wave(int32_t hooked, ForestCtl *ctl, int32_t *__restrict__ log, uint32_t cap)
{
    const uint32_t slot = wave_append(hooked >= 0, &ctl->log_n);
    if (hooked >= 0 && slot < cap) log[slot] = hooked;      // (cannot overflow: an item is hooked once)
}

// from node c (0 <= c < the number of nodes, level nk[c] >= k) up while the parent's level is still >= k: the node of c's
// class at threshold k.  Parents have smaller numbers, and the walk follows no other: it ends whatever par[] holds.
__device__ __forceinline__ int32_t forest_walk_up(int32_t c, int32_t k, const int32_t *__restrict__ nk, const int32_t *__restrict__ par)
{
    for (int32_t a = par[c]; a >= 0 && a < c && nk[a] >= k; a = par[a]) c = a;
    return c;
}

} // namespace komb
