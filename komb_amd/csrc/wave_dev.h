// wave_dev.h -- the steps in which the 64 lanes of a wave cooperate: the turns of a wave over its lanes' long units, the
// ballot-ranked append to a list, and the grouping of the lanes by a key.  wave_sum / wave_max stay in common.h: the peel
// engine uses them, and it includes nothing of this.
//
// THE WAVE RULE, for everything below that ballots or shuffles (wave_turns, from_lane, wave_walk_all, wave_append, wave_by_key)
// and for every functor that does: all 64 lanes of the wave get there together.  So it is called from straight-line kernel code
// or from loops whose bounds are uniform over the wave, never under a condition that differs between lanes; a lane with nothing
// to do comes along with mid = false, n = 0, in = false, take = false or act = false.  wave_walk is the one exception: its lanes
// leave when their entries run out, so its functor must neither ballot nor shuffle.
#pragma once

#include "common.h"

namespace komb {

// ---- the tiers.  One lane per unit (a row, an edge and its sides, a triangle and its tails).  A unit whose walked part is short
// stays with its lane; the longer ones (mid) are walked by the whole wave, one after the other: unit(src) is called once for
// every lane src with mid set, in ascending lane order, and fetches that lane's unit with from_lane.
template <class F>
__device__ __forceinline__ void wave_turns(bool mid, F unit)
{
    unsigned long long todo = __ballot(mid);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        unit(src);
    }
}

__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) { return (uint32_t)__shfl((int32_t)v, src); }

// the wave over the entries [it, it + n) of one unit, free form: entry(x) by the lane that x falls to, its hits its own affair
template <class F>
__device__ __forceinline__ void wave_walk(uint32_t it, uint32_t n, int lane, F entry)
{
    for (uint32_t x = it + (uint32_t)lane; x < it + n; x += kWave) entry(x);
}

// ... uniform form, for an entry that ballots: every lane calls entry(x, in) on every trip, in = x is an entry of the unit
template <class F>
__device__ __forceinline__ void wave_walk_all(uint32_t it, uint32_t n, int lane, F entry)
{
    for (uint32_t x0 = it; x0 < it + n; x0 += kWave) {
        const uint32_t x = x0 + (uint32_t)lane;
        entry(x, x < it + n);
    }
}

// ---- `per` slots of a list for every lane that takes some: one atomic per wave, the lanes ranked by a ballot.  Returns the
// lane's first slot (meaningless without take); whether it is inside the list is the caller's check.
__device__ __forceinline__ uint32_t wave_append(bool take, uint32_t *counter, uint32_t per = 1u)
{
    const unsigned long long m = __ballot(take);
    if (!m) return 0u;
    const int lane = threadIdx.x & (kWave - 1), lead = __ffsll((long long)m) - 1;
    uint32_t base = 0u;
    if (lane == lead) base = atomicAdd(counter, per * (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int32_t)base, lead);
    return base + per * (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// ---- the lanes with act grouped by equal key.  For every distinct key among them, in ascending order of the first lane that
// holds it, every lane of the wave calls fn(lead, same, is_leader): lead = the key, same = the ballot of the lanes that hold
// it, is_leader = this is the first of those lanes.  All lanes are in fn together, so fn may ballot; what is done once per
// key -- an atomic of __popcll(same) where every lane would have added one -- goes under is_leader.
template <class F>
__device__ __forceinline__ void wave_by_key(bool act, int32_t key, F fn)
{
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long m = __ballot(act);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        const int32_t lead = __shfl(key, src);
        const unsigned long long same = __ballot(act && key == lead);
        fn(lead, same, lane == src);
        m &= ~same;
    }
}

} // namespace komb
