// im_keyed.hpp -- the keyed table behind the clip tails (-V, im_cliptail.hip), the pair links (-M), the mate links (-T) and the split
// links (-S, all three im_links.hip): its one definition (gfx950).  DESIGN.md 4.5f has the cost.  The four users keep their key and
// payload layouts and what they do with an entry.
//
// THE TABLE (KeyedTable, im_device.hpp): 2^k slots of 16 bytes in HBM, open addressing, a multimap.
//   word 0   the key: bit 63 set, so that an empty slot is 0; the other bits are the user's
//   word 1   the payload, the user's
// The home slot of a key is (hashed * kKeyedHashMul) >> (64 - k), where `hashed` is what the user lets into the hash: every entry
// that one query has to see hashes alike and so lies on ONE probe run.  Probing is linear and wraps.
//   THE TICKET RULE  An insert first draws a ticket (a returning atomic add on counters[0]); tickets at or above 2^k / 2 store nothing
//     and are counted in counters[1].  So at least half of the slots stay empty, every probe run ends at an empty slot, the number
//     stored is exactly min(inserts, 2^k / 2), and a table with counters[1] > 0 is one whose answers the entry points withhold.
//   THE CLAIM  A slot is claimed by a 64-bit compare-and-swap of its key from 0; the payload is a plain store behind it.  Readers are
//     later launches, so nobody sees a key without its payload.
//   THE BOUNDS  Every probe loop, of an insert or of a walk, is bounded by the slot count as well as by the empty slot it expects.
#pragma once

#include "im_device.hpp"

namespace im {

// one wave per query in workgroups of 256 threads: the grid for n queries, which a wave takes in a loop beyond 2048 workgroups
inline unsigned wave_grid(int64_t n)
{
    const int64_t b = (n + 3) / 4;
    return (unsigned)(b > 2048 ? 2048 : b);
}

constexpr uint64_t kKeyedUsed = 1ull << 63;
constexpr uint64_t kKeyedHashMul = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t keyed_home(uint64_t hashed, int32_t log2_slots) { return (hashed * kKeyedHashMul) >> (64 - log2_slots); }

// A ticket decides whether an entry is stored: tickets at or above half of the slots are counted in counters[1] and dropped.
__device__ __forceinline__ bool keyed_admit(const KeyedTable& T, unsigned long long ticket)
{
    if (ticket < (1ull << T.log2_slots) / 2ull) return true;
    atomicAdd(&T.counters[1], 1ull);
    return false;
}

// An admitted entry into the first empty slot of the probe run that starts at home (there is one: half of the slots stay empty).
__device__ __forceinline__ void keyed_place(const KeyedTable& T, uint64_t home, uint64_t key, uint64_t payload)
{
    const uint64_t slots = 1ull << T.log2_slots, mask = slots - 1ull;
    uint64_t s = home;
    for (uint64_t step = 0; step < slots; step++, s = (s + 1ull) & mask) {
        unsigned long long* k = &T.slots[2ull * s];
        // the home slot gets the compare-and-swap at once (in a table at most half full it is mostly empty: one trip to memory,
        // not two); further along a run a slot that reads non-zero stays taken and is passed by a load
        if (step != 0ull && __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) continue;
        if (atomicCAS(k, 0ull, (unsigned long long)key) == 0ull) { T.slots[2ull * s + 1ull] = payload; return; }
    }
}

// The same, for a user that keeps something of its own beside a slot (the split links' overlap array, im_links.hip): returns the slot
// the entry claimed, or the slot count when the run held none (it always holds one: the ticket rule).  The other users keep keyed_place,
// which is not written on top of this one: forwarding changed the instructions the compiler makes for their kernels.
__device__ __forceinline__ uint64_t keyed_place_at(const KeyedTable& T, uint64_t home, uint64_t key, uint64_t payload)
{
    const uint64_t slots = 1ull << T.log2_slots, mask = slots - 1ull;
    uint64_t s = home;
    for (uint64_t step = 0; step < slots; step++, s = (s + 1ull) & mask) {
        unsigned long long* k = &T.slots[2ull * s];
        if (step != 0ull && __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) continue;
        if (atomicCAS(k, 0ull, (unsigned long long)key) == 0ull) { T.slots[2ull * s + 1ull] = payload; return s; }
    }
    return slots;
}

// One entry in, the ticket drawn by the lane itself (counters[0]: inserts): the form for callers that name the events themselves.
__device__ __forceinline__ void keyed_insert(const KeyedTable& T, uint64_t home, uint64_t key, uint64_t payload)
{
    if (keyed_admit(T, atomicAdd(&T.counters[0], 1ull))) keyed_place(T, home, key, payload);
}

// The tickets of a workgroup of kBlock threads, drawn by ONE atomic add: returning atomics of a whole chunk on one address take
// turns, and one per inserting lane made them most of a scatter's launch.  mine: the entries of this lane, 0 .. kMaxPerLane (1 or 2).
// The lanes count through one ballot per wave (two where a lane may hold two; kMaxPerLane is a compile-time parameter so that the
// one-entry form does not carry the second) and 64 bytes of LDS, thread 0 adds the workgroup's total to counters[0], and the lane's
// tickets are *first_ticket .. *first_ticket + mine - 1.  Returns false, for the whole workgroup and before the atomic, when the
// workgroup has nothing to insert -- most workgroups of a chunk.  Every thread of the workgroup calls it, once per kernel.
// block_tickets is that draw on the counter it is given (the split-junction sweep of im_links.hip ranks the slots it lists with it);
// keyed_block_tickets, behind it, is the table's.
template <int kBlock, int kMaxPerLane>
__device__ __forceinline__ bool block_tickets(unsigned long long* counter, uint32_t mine, unsigned long long* first_ticket)
{
    static_assert(kBlock % 64 == 0 && (kMaxPerLane == 1 || kMaxPerLane == 2), "whole waves; one ballot per entry a lane may hold");
    __shared__ uint32_t s_wave[kBlock / 64];
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t one = __ballot(mine >= 1u);
    uint32_t rank = (uint32_t)__builtin_popcountll(one & below), in_wave = (uint32_t)__builtin_popcountll(one);
    if constexpr (kMaxPerLane == 2) {
        const uint64_t two = __ballot(mine == 2u);
        rank += (uint32_t)__builtin_popcountll(two & below); in_wave += (uint32_t)__builtin_popcountll(two);
    }
    if (lane == 0) s_wave[wave] = in_wave;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) { before += w < wave ? s_wave[w] : 0u; total += s_wave[w]; }
    if (total == 0u) return false;                                  // uniform over the workgroup
    if (t == 0) s_base = atomicAdd(counter, (unsigned long long)total);
    __syncthreads();
    *first_ticket = s_base + before + rank;
    return true;
}

template <int kBlock, int kMaxPerLane>
__device__ __forceinline__ bool keyed_block_tickets(const KeyedTable& T, uint32_t mine, unsigned long long* first_ticket)
{
    return block_tickets<kBlock, kMaxPerLane>(&T.counters[0], mine, first_ticket);
}

// The walk every query shares: the wave goes along the probe run that starts at home 64 slots at a time until a batch shows an empty
// slot.  match(key) says whether a slot's key is one the query wants; each(has, key, slot) is called, by the whole wave, for every
// batch in which some lane's slot (in front of the first empty one) holds such an entry: has says whether this lane's does.  Returns
// the entries of the run that matched (wave-uniform).
template <class Match, class Each>
__device__ __forceinline__ uint32_t keyed_walk(const KeyedTable& T, uint64_t home, Match match, int lane, Each each)
{
    uint32_t stored = 0;
    const uint64_t slots = 1ull << T.log2_slots, mask = slots - 1ull;
    for (uint64_t base = 0; base < slots; base += 64ull) {
        const uint64_t s = (home + base + (uint64_t)lane) & mask;
        const uint64_t key = T.slots[2ull * s];
        const uint64_t empty = __ballot(key == 0ull);
        const int stop = empty ? (int)__builtin_ctzll(empty) : 64;
        const bool has = lane < stop && match(key);
        const uint64_t holders = __ballot(has);
        if (holders) {
            stored += (uint32_t)__builtin_popcountll(holders);
            each(has, key, s);
        }
        if (empty) break;
    }
    return stored;
}

}  // namespace im
