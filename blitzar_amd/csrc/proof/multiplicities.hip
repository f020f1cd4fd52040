// The multiplicity column of a log-derivative argument (bzamd_count_multiplicities*):
//   multiplicities[t] = #{i < n : key(lookups[i]) = key(table[t])}  for the first row t of a key,
//   0 for its later rows;   misses = #{i < n : key(lookups[i]) is in no table row},
// exact, over the typed columns of the sumcheck.  The key of a row is the canonical integer in
// [0, p) of its value, so rows of any width and signedness, unreduced 32-byte rows and (field 1)
// Montgomery words compare by value.
//
// Hashed form, three launches whatever m, n and the data are; every loop is grid-stride:
//   * k_clear_multiplicities: slots <- kEmptySlot, multiplicities <- 0, misses <- 0 (a kernel, not
//     a memset: bzamd_kernel_launch_count sees a fixed number).
//   * k_insert_rows: table row t hashes its key and probes linearly through S slots of 32 bits
//     (S: the least power of two >= 2 m).  On an empty slot it tries atomicCAS(slot, empty, t) and,
//     losing, goes on WITH THE RETURNED ROW AT THE SAME SLOT; on a row of its own key it
//     atomicMin(slot, t)s and is done; on a row of another key it moves to the next slot.
//     Invariant: a slot that is not empty only ever changes among rows of ONE key (the CAS fills
//     empty slots alone, the min is taken by rows that compared equal).  So the slots a probe has
//     passed stay passed, every row of a key stops at the same slot, a key lives in exactly one
//     slot, and that slot ends with the key's least row, whatever the order of arrival.  What
//     depends on the order is WHICH slot of a cluster a key takes, which no result shows.
//     Slot words are touched through agent-scope atomics alone in this kernel (the read is a
//     relaxed agent-scope atomic load): workgroups on other XCDs write them in the same launch, and
//     a plain load may be served a stale line from this XCD's L2.  Keys are read from the caller's
//     table, which nobody writes.
//   * k_count_rows: a later launch, so the slots are read with plain loads.  Lookup row i probes:
//     an empty slot is a miss, a row of its key a hit on that row, anything else the next slot.
//     Hits are added with 64-bit atomics whose result nobody reads, AGGREGATED IN THE WAVEFRONT
//     first (wave_adder): while lanes remain, the first remaining lane's row is broadcast, the
//     lanes that share it are balloted and counted, and the count is carried, with its row, until a
//     different row turns up or the wavefront is done; then one lane adds it.  A constant lookup
//     column costs one add per wavefront and CALL, not 64 on one word per wavefront and turn; 64
//     different rows cost 64 short uniform iterations and the 64 adds they need anyway.  Misses:
//     one add per wavefront.  One word takes some 80 adds a microsecond, so what counts
//     is how many adds reach the busiest word.  Tables of at most kLdsBins rows do not add to
//     global memory row by row at all: a workgroup counts in 32-bit bins in LDS, one per table row,
//     and adds its non-zero bins at the end (at most kLdsBlocks adds a word).
// Every probe loop ends after S steps at the latest (insert gives up, count reports a miss), and a
// slot that holds no row of the table counts as empty: no workspace contents make a kernel spin or
// read outside the table.
//
// Range form (table.data null: T[t] = t), two launches: the clear and k_count_range.  For
// m <= kLdsBins each workgroup counts into 32-bit bins in LDS (it sees fewer than 2^32 rows), then
// adds its non-zero bins and, once, its misses; for larger m rows go to global memory through
// wave_adder.  One- and two-byte columns are read 16 bytes a lane where the address allows
// (the rows before the first and after the last whole 16 bytes go the general way).
//
// The clear of the slots, k_insert_rows, the find loop, wave_adder and the launch geometry are in
// proof/key_table.h, shared with proof/key_sums.hip (each unit instantiates its own kernels).
// Key extraction is key_of of proof/column_key.h, shared with proof/word_columns.hip.
// No scratch memory in any kernel (tests/test_multiplicities.py reads the compiler's report).
#include "blitzar_amd/csrc/proof/multiplicities.h"

#include <vector>

#include "blitzar_amd/csrc/proof/host_call.h"
#include "blitzar_amd/csrc/proof/key_table.h"

namespace bz::proof {
namespace {
constexpr u32 kLdsBins = 4096;        // 16 KB of u32 bins
constexpr u32 kLdsBlocks = 1024;    // each adds its non-zero bins at the end

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCountThreads)
    k_clear_multiplicities(u32* slot_rows, u64 slots, u64* multiplicities, u64 table_rows,
                           u64* misses) {
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  const u64 first = static_cast<u64>(blockIdx.x) * kCountThreads + threadIdx.x;
  clear_slots(slot_rows, slots, first, stride);
  for (u64 t = first; t < table_rows; t += stride) multiplicities[t] = 0;
  if (first == 0 && misses != nullptr) *misses = 0;
}

// kLds (tables of at most kLdsBins rows): hits go to 32-bit bins in LDS, one per table row, and the
// workgroup adds its non-zero bins at the end (it sees fewer than 2^32 rows)
template <class E, bool kLds>
__global__ void __launch_bounds__(kCountThreads)
    k_count_rows(u64* multiplicities, u64* misses, const u32* __restrict__ slot_rows, u64 slots,
                 const column_view table, const column_view lookups) {
  __shared__ u32 bins[kLds ? kLdsBins : 1];
  const u32 used_bins = kLds ? static_cast<u32>(table.n) : 0;
  for (u32 b = threadIdx.x; b < used_bins; b += kCountThreads) bins[b] = 0;
  if constexpr (kLds) __syncthreads();
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  u64 wave_misses = 0;
  wave_adder adder;
  // `base` is the workgroup's: every lane of a wavefront takes the same number of turns
  for (u64 base = static_cast<u64>(blockIdx.x) * kCountThreads; base < lookups.n; base += stride) {
    const u64 i = base + threadIdx.x;
    const bool active = i < lookups.n;
    u32 found = kEmptySlot;
    if (active) found = find_row<E>(slot_rows, slots, table, key_of<E>(lookups, i));
    const bool hit = found != kEmptySlot;
    if constexpr (kLds) {
      if (hit) atomicAdd(bins + found, 1u);
    } else {
      adder.add(multiplicities, found, hit);
    }
    wave_misses += static_cast<u64>(__popcll(__ballot(active && !hit)));
  }
  adder.flush(multiplicities);
  if (__lane_id() == 0 && wave_misses != 0 && misses != nullptr) {
    (void)__hip_atomic_fetch_add(misses, wave_misses, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (kLds) {
    __syncthreads();
    for (u32 b = threadIdx.x; b < used_bins; b += kCountThreads) {
      const u32 count = bins[b];
      if (count != 0) {
        (void)__hip_atomic_fetch_add(multiplicities + b, static_cast<u64>(count), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// how k_count_range walks a column: rows [0, head) and [head + chunks * (16 / nbytes), n) the
// general way, the rows between as `chunks` aligned 16-byte loads
struct range_walk {
  u64 head, chunks;
};

template <class E, bool kLds>
__global__ void __launch_bounds__(kCountThreads)
    k_count_range(u64* multiplicities, u64* misses, u64 table_rows, const column_view lookups,
                  const range_walk walk) {
  __shared__ u32 bins[kLds ? kLdsBins : 1];
  __shared__ u32 block_misses;
  const u32 tid = threadIdx.x;
  const u32 used_bins = kLds ? static_cast<u32>(table_rows) : 0;
  for (u32 b = tid; b < used_bins; b += kCountThreads) bins[b] = 0;
  if (tid == 0) block_misses = 0;
  __syncthreads();
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  const u64 first = static_cast<u64>(blockIdx.x) * kCountThreads;
  u32 wave_misses = 0; // the workgroup sees fewer than 2^32 rows
  wave_adder adder;
  // called by all 64 lanes together
  auto visit = [&](bool active, bool hit, u32 row) {
    if constexpr (kLds) {
      if (active && hit) atomicAdd(bins + row, 1u);
    } else {
      adder.add(multiplicities, row, active && hit);
    }
    wave_misses += static_cast<u32>(__popcll(__ballot(active && !hit)));
  };
  const u32 per_chunk = 16 / lookups.nbytes; // chunks != 0: nbytes is 1 or 2
  const u64 body_rows = walk.chunks * (walk.chunks != 0 ? per_chunk : 0);
  const u64 loose = lookups.n - body_rows;
  for (u64 base = first; base < loose; base += stride) {
    const u64 j = base + tid;
    const bool active = j < loose;
    bool hit = false;
    u32 row = 0;
    if (active) {
      const lookup_key key = key_of<E>(lookups, j < walk.head ? j : j + body_rows);
      hit = (key.w[1] | key.w[2] | key.w[3]) == 0 && key.w[0] < table_rows;
      row = static_cast<u32>(key.w[0]);
    }
    visit(active, hit, row);
  }
  const uint4* body = reinterpret_cast<const uint4*>(lookups.data + walk.head * lookups.nbytes);
  for (u64 base = first; base < walk.chunks; base += stride) {
    const u64 c = base + tid;
    const bool active = c < walk.chunks;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (active) v = body[c];
    const u32 words[4] = {v.x, v.y, v.z, v.w};
    if (lookups.nbytes == 1) {
      // a negative byte is p - |x|: a miss
      const u32 limit = lookups.is_signed != 0 ? 128u : 256u;
#pragma unroll
      for (u32 e = 0; e < 16; ++e) {
        const u32 value = (words[e / 4] >> (8 * (e % 4))) & 0xFFu;
        visit(active, value < limit && value < table_rows, value);
      }
    } else {
      const u32 limit = lookups.is_signed != 0 ? 32768u : 65536u;
#pragma unroll
      for (u32 e = 0; e < 8; ++e) {
        const u32 value = (words[e / 2] >> (16 * (e % 2))) & 0xFFFFu;
        visit(active, value < limit && value < table_rows, value);
      }
    }
  }
  adder.flush(multiplicities);
  if (__lane_id() == 0 && wave_misses != 0) atomicAdd(&block_misses, wave_misses);
  __syncthreads();
  for (u32 b = tid; b < used_bins; b += kCountThreads) {
    const u32 count = bins[b];
    if (count != 0) {
      (void)__hip_atomic_fetch_add(multiplicities + b, static_cast<u64>(count), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid == 0 && block_misses != 0 && misses != nullptr) {
    (void)__hip_atomic_fetch_add(misses, static_cast<u64>(block_misses), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  }
}

//--------------------------------------------------------------------------------------------------
// launch geometry
//--------------------------------------------------------------------------------------------------
range_walk walk_of(const sumcheck_column& lookups) {
  const uintptr_t address = reinterpret_cast<uintptr_t>(lookups.data);
  if (lookups.nbytes > 2 || address % lookups.nbytes != 0) return {0, 0};
  const u64 head = std::min<u64>(lookups.n, (16 - address % 16) % 16 / lookups.nbytes);
  return {head, (lookups.n - head) * lookups.nbytes / 16};
}

//--------------------------------------------------------------------------------------------------
// host backend: the sequential model
//--------------------------------------------------------------------------------------------------
template <class E> void count_host(u64* multiplicities, u64* misses, const multiplicity_count& c) {
  const column_view table = make_column_view(c.table), lookups = make_column_view(c.lookups);
  const auto key_of_lookup = [&](u64 i) { return key_of<E>(lookups, i); };
  if (c.table.data == nullptr) {
    for (u64 t = 0; t < table.n; ++t) multiplicities[t] = 0;
    u64 missed = 0;
    for (u64 i = 0; i < lookups.n; ++i) {
      const lookup_key key = key_of_lookup(i);
      if ((key.w[1] | key.w[2] | key.w[3]) == 0 && key.w[0] < table.n) {
        ++multiplicities[key.w[0]];
      } else {
        ++missed;
      }
    }
    if (misses != nullptr) *misses = missed;
    return;
  }
  const auto table_key = [&](u64 t) { return key_of<E>(table, t); };
  const u64 slots = slot_count(table.n);
  std::vector<u32> slot_rows(slots);
  model_insert(slot_rows.data(), slots, table.n, table_key);
  model_count(multiplicities, misses, slot_rows.data(), slots, table.n, table_key, lookups.n,
              key_of_lookup);
}

//--------------------------------------------------------------------------------------------------
// device form: enqueue only
//--------------------------------------------------------------------------------------------------
template <class E>
void count_enqueue(u64* multiplicities, u64* misses, const multiplicity_count& c, void* workspace,
                   hipStream_t stream) {
  const column_view lookups = make_column_view(c.lookups);
  const u64 m = c.table.n;
  if (c.table.data == nullptr) {
    hipLaunchKernelGGL(k_clear_multiplicities, dim3(blocks_for(m, kCountBlocks)),
                       dim3(kCountThreads), 0, stream, static_cast<u32*>(nullptr), u64{0},
                       multiplicities, m, misses);
    BZ_HIP_CHECK(hipGetLastError());
    const range_walk walk = walk_of(c.lookups);
    const u64 per_chunk = walk.chunks != 0 ? 16 / c.lookups.nbytes : 0;
    const u64 turns = std::max<u64>(c.lookups.n - walk.chunks * per_chunk, walk.chunks);
    if (m <= kLdsBins) {
      hipLaunchKernelGGL((k_count_range<E, true>), dim3(blocks_for(turns, kLdsBlocks)),
                         dim3(kCountThreads), 0, stream, multiplicities, misses, m, lookups, walk);
    } else {
      hipLaunchKernelGGL((k_count_range<E, false>), dim3(blocks_for(turns, kCountBlocks)),
                         dim3(kCountThreads), 0, stream, multiplicities, misses, m, lookups, walk);
    }
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 2;
    return;
  }
  const column_view table = make_column_view(c.table);
  const u64 slots = slot_count(m);
  u32* slot_rows = reinterpret_cast<u32*>(workspace_carver::aligned(workspace));
  hipLaunchKernelGGL(k_clear_multiplicities, dim3(blocks_for(slots, kCountBlocks)),
                     dim3(kCountThreads), 0, stream, slot_rows, slots, multiplicities, m, misses);
  BZ_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_insert_rows<E>), dim3(blocks_for(m, kCountBlocks)), dim3(kCountThreads), 0,
                     stream, slot_rows, slots, table);
  BZ_HIP_CHECK(hipGetLastError());
  if (m <= kLdsBins) {
    hipLaunchKernelGGL((k_count_rows<E, true>), dim3(blocks_for(c.lookups.n, kLdsBlocks)),
                       dim3(kCountThreads), 0, stream, multiplicities, misses, slot_rows, slots,
                       table, lookups);
  } else {
    hipLaunchKernelGGL((k_count_rows<E, false>), dim3(blocks_for(c.lookups.n, kCountBlocks)),
                       dim3(kCountThreads), 0, stream, multiplicities, misses, slot_rows, slots,
                       table, lookups);
  }
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 3;
}
} // namespace

void check_multiplicity_count(const void* multiplicities, const void* misses, unsigned field_id,
                              const multiplicity_count& c, const void* workspace,
                              u64 workspace_bytes, bool device_form) {
  BZ_RELEASE_ASSERT(multiplicities != nullptr, "null argument to the multiplicity count");
  BZ_RELEASE_ASSERT(c.table.n >= 1 && c.table.n <= kMaxTableRows,
                    "the multiplicity count needs 1 <= table rows <= 2^28");
  BZ_RELEASE_ASSERT(c.lookups.n <= kMaxLookupRows,
                    "the multiplicity count needs lookup rows <= 2^30");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(multiplicities) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(misses) % 8 == 0,
                    "the outputs of the multiplicity count must be 8-byte aligned");
  // the hashed device form alone reads or writes a workspace
  if (device_form && c.table.data != nullptr) {
    BZ_RELEASE_ASSERT(workspace != nullptr &&
                          workspace_bytes >= multiplicity_workspace_bytes(c.table.n),
                      "the workspace of the multiplicity count is too small");
  } else {
    workspace_bytes = 0;
  }
  const byte_range outputs[2] = {{multiplicities, 8 * c.table.n}, {misses, 8}};
  BZ_RELEASE_ASSERT(!overlap(outputs[0], outputs[1]),
                    "the outputs of the multiplicity count overlap");
  for (const byte_range& out : outputs) {
    BZ_RELEASE_ASSERT(!overlap(out, {c.table.data, c.table.n * c.table.nbytes}) &&
                          !overlap(out, {c.lookups.data, c.lookups.n * c.lookups.nbytes}),
                      "an output overlaps an input of the same call");
    BZ_RELEASE_ASSERT(!overlap(out, {workspace, workspace_bytes}),
                      "an output overlaps the workspace of the same call");
  }
  BZ_RELEASE_ASSERT(field_id <= 1, "unsupported field id");
}

void count_multiplicities_device(u64* multiplicities, u64* misses, unsigned field_id,
                                 const multiplicity_count& c, void* workspace, hipStream_t stream) {
  with_elements(field_id, [&](auto elements) {
    count_enqueue<decltype(elements)>(multiplicities, misses, c, workspace, stream);
  });
}

void count_multiplicities(api_state& st, u64* multiplicities, u64* misses, unsigned field_id,
                          const multiplicity_count& c) {
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      count_host<E>(multiplicities, misses, c);
      return;
    }
    // the columns up at their own width, the device form, the results down
    host_call call{st};
    const size_t lookup_bytes = c.lookups.n * c.lookups.nbytes;
    u64 *d_multiplicities, *d_misses;
    multiplicity_count staged = c;
    void* workspace = nullptr;
    // the misses are counted whether the caller asks for them or not
    u64 missed = 0;
    call.output(&d_multiplicities, multiplicities, 8 * c.table.n);
    call.output(&d_misses, &missed, 8);
    // a range table has no rows to upload and stays null; so do lookups of no rows
    call.input(&staged.table.data, c.table.data, c.table.n * c.table.nbytes);
    call.input(&staged.lookups.data, lookup_bytes != 0 ? c.lookups.data : nullptr, lookup_bytes);
    // the hashed form alone has a workspace
    if (c.table.data != nullptr) call.scratch(&workspace, multiplicity_workspace_bytes(c.table.n));
    call.allocate();
    count_enqueue<E>(d_multiplicities, d_misses, staged, workspace, call.stream());
    call.finish();
    if (misses != nullptr) *misses = missed;
  });
}

u64 multiplicity_first_slot(unsigned field_id, const void* element, u64 table_rows) {
  const u64 slots = slot_count(table_rows);
  if (slots == 0 || field_id > 1 || element == nullptr) return ~u64{0};
  return with_elements(field_id, [&](auto elements) -> u64 {
    const column_view one{static_cast<const u8*>(element), 1, 32, kAccessBytes, 0, 0};
    return first_slot(key_of<decltype(elements)>(one, 0), slots);
  });
}
} // namespace bz::proof
