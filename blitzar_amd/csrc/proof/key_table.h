// The open-addressing table of first occurrences that the multiplicity count
// (proof/multiplicities.hip) and the sums by key (proof/key_sums.hip) probe: one copy of the clear
// of the slots, the insert kernel, the find loop, the wavefront's aggregated adds to a u64 column
// and the launch geometry.  The invariants of the insert, why its slot words are touched through
// agent-scope atomics alone and how wave_adder aggregates are described in the head comment of
// proof/multiplicities.hip; the hash, the slot count and the sequential model are the plain C++
// half of proof/multiplicities.h.
//
// Device header: everything lies in an unnamed namespace, so each translation unit that includes
// it instantiates kernels of its own (and the compiler's resource report of a unit lists exactly
// the kernels that unit launches).
#pragma once

#include <algorithm>

#include "blitzar_amd/csrc/proof/column_key.h"

namespace bz::proof {
namespace {
constexpr u32 kCountThreads = 256;
// 8 workgroups of 4 wavefronts per CU: the probes are dependent loads, more wavefronts hide more
constexpr u32 kCountBlocks = 2048;

// slots [0, slots) <- kEmptySlot, grid-stride from `first`
__device__ __forceinline__ void clear_slots(u32* slot_rows, u64 slots, u64 first, u64 stride) {
  for (u64 s = first; s < slots; s += stride) slot_rows[s] = kEmptySlot;
}

template <class E>
__global__ void __launch_bounds__(kCountThreads)
    k_insert_rows(u32* slot_rows, u64 slots, const column_view table) {
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  for (u64 t = static_cast<u64>(blockIdx.x) * kCountThreads + threadIdx.x; t < table.n;
       t += stride) {
    const lookup_key key = key_of<E>(table, t);
    const u32 mine = static_cast<u32>(t);
    u64 slot = first_slot(key, slots);
    for (u64 step = 0; step < slots; ++step, slot = (slot + 1) & (slots - 1)) {
      u32 row = __hip_atomic_load(slot_rows + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (row == kEmptySlot) {
        row = atomicCAS(slot_rows + slot, kEmptySlot, mine);
        if (row == kEmptySlot) break;
      }
      // a row of the table (the clear and this kernel write nothing else); guarded all the same
      if (row >= table.n) break;
      if (same_key(key_of<E>(table, row), key)) {
        if (mine < row) atomicMin(slot_rows + slot, mine);
        break;
      }
    }
  }
}

// the row a key's probe ends on, or kEmptySlot: an empty slot (a slot that holds no row of the
// table counts as empty), or `slots` steps without the key.  For a launch after the insert: the
// slots are read with plain loads
template <class E>
__device__ __forceinline__ u32 find_row(const u32* __restrict__ slot_rows, u64 slots,
                                        const column_view& table, const lookup_key& key) {
  u32 found = kEmptySlot;
  u64 slot = first_slot(key, slots);
  for (u64 step = 0; step < slots; ++step, slot = (slot + 1) & (slots - 1)) {
    const u32 row = slot_rows[slot];
    if (row >= table.n) break; // empty
    if (same_key(key_of<E>(table, row), key)) {
      found = row;
      break;
    }
  }
  return found;
}

// One wavefront's adds to `multiplicities`, aggregated: add() takes a row per lane, and while lanes
// remain it broadcasts the first remaining lane's row, ballots the lanes that share it and counts
// them.  The count is not added at once but kept, with its row, in two wave-uniform registers, and
// added by one lane when the next row differs or at flush(): runs of one row, within a wavefront and
// from one turn of its loop to the next, cost one atomic.  Called by all 64 lanes together
// (wave-uniform control flow around every call); a wavefront sees fewer than 2^32 rows
struct wave_adder {
  u32 row = kEmptySlot, count = 0;
  __device__ __forceinline__ void flush(u64* multiplicities) {
    if (count != 0 && __lane_id() == 0) {
      (void)__hip_atomic_fetch_add(multiplicities + row, static_cast<u64>(count), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
    count = 0;
  }
  __device__ __forceinline__ void add(u64* multiplicities, u32 lane_row, bool hit) {
    u64 remaining = __ballot(hit);
    while (remaining != 0) {
      const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(remaining))) - 1;
      const u32 leader_row = static_cast<u32>(
          __builtin_amdgcn_readlane(static_cast<int>(lane_row), static_cast<int>(leader)));
      const u64 same = __ballot(hit && lane_row == leader_row);
      if (leader_row != row) {
        flush(multiplicities);
        row = leader_row;
      }
      count += static_cast<u32>(__popcll(same));
      remaining &= ~same;
    }
  }
};

// workgroups of kCountThreads for `rows` rows, at least one and at most `most`
inline u32 blocks_for(u64 rows, u32 most) {
  const u64 blocks = (rows + kCountThreads - 1) / kCountThreads;
  return static_cast<u32>(std::min<u64>(most, std::max<u64>(blocks, 1)));
}
} // namespace
} // namespace bz::proof
