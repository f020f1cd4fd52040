// Sums of typed value columns by key (bzamd_sum_by_key*): with first(t) the least table row that
// has the key of row t,
//   sums_v[t]  = sum over {i < n : key(lookups[i]) = key(table[t])} of value_v[i]   (first(t) = t)
//   counts[t]  = the number of those i (the multiplicities of bzamd_count_multiplicities)
//   matches[i] = first(t) of the row lookups[i] hits, 0xFFFFFFFF for a miss;  misses = their number,
// exact, over the typed columns of the sumcheck: the result columns of a group-by, and the match
// index of a join.  The table of first occurrences, its insert kernel and the find loop are those
// of the multiplicity count (proof/key_table.h).
//
// Four launches whatever m, n, num_values and the data are (the range table T[t] = t: three, it
// has nothing to insert); every loop is grid-stride, 256 threads, at most 2048 workgroups:
//   * k_clear_key_sums: slots <- kEmptySlot, accumulators <- 0, counts <- 0, misses <- 0.
//   * k_insert_rows (proof/key_table.h).
//   * k_accumulate_rows: lookup row i probes as k_count_rows does (at most S steps; a slot that
//     holds no row of the table is empty), writes matches[i], counts through the existing
//     aggregation (bins in LDS, or wave_adder) and adds its values WITHOUT FIELD ARITHMETIC: the
//     magnitude of value_v[i] (load_magnitude; a 32-byte row is its four words as they are,
//     unreduced or Montgomery) is cut into 32-bit chunks, and chunk k is added to, or for a
//     negative row subtracted from, the signed 64-bit accumulator acc[t][v][k] with a relaxed,
//     agent-scope atomic whose result nobody reads; zero chunks are skipped.  |acc| < 2^62
//     (proof/key_sums.h).  Integer adds commute, so a call's result is the same bits whatever the
//     order of arrival.  An i64 column costs at most two atomics a row, a 32-byte column eight.
//     Accumulators lie as [row][value][chunk], a row's side by side; a column of w bytes has
//     ceil(w / 4) of them.
//     Contention (what shares a destination is summed on chip first):
//       - m <= kLdsBins rows and m x (chunks of all columns) <= kLdsSumBins: a workgroup
//         accumulates in 64-bit bins in LDS (ds_add_u64) and adds its non-zero bins to global
//         memory once, at its end, as k_count_rows<kLds> does with its counts: at most kLdsBlocks
//         adds a word and call.  kLdsSumBins = 4096 is 32 KB; with the 16 KB of count bins a
//         workgroup holds 48 KB of the CU's 160 KB, so three workgroups (twelve wavefronts) still
//         fit a CU, which the dependent loads of the probe need; twice the bins would leave one.
//         It covers 2048 groups of one i64 column, 512 of four, 512 of one 32-byte column.
//       - larger tables: a wavefront whose hit lanes (two or more) ALL hit one row, the hot key,
//         sums each chunk across its lanes (six shuffles of a 64-bit word) and adds once per
//         chunk, not 64 times; any other wavefront adds lane by lane.
//   * k_finish_sums: the only field arithmetic, once per (table row, value column): the
//     accumulators are put together into the wide integer sum_k acc_k 2^(32 k) (proof/key_sums.h),
//     its magnitude goes into the field as low 256 bits + top word x 2^256, the sign negates.  The
//     sum of narrow rows is the value itself and is converted to element form (field 1: one
//     product by 2^256); the sum of 32-byte rows is already in element form, Montgomery form being
//     linear, and takes one product by 2^-256 for scalar form (field 1).  Rows that are no first
//     occurrence were never hit: their accumulators are zero and so are their sums.
// No workspace contents make a kernel spin or read outside the table, the accumulators or the
// outputs: the clear writes every word that is read later.  No scratch memory in any kernel
// (tests/test_key_sums.py reads the compiler's report).
//
// The cpu backend does not use this scheme: it goes row by row with one field addition per row and
// value column, so the two forms check each other.
#include "blitzar_amd/csrc/proof/key_sums.h"

#include <cstring>
#include <type_traits>
#include <vector>

#include "blitzar_amd/csrc/proof/host_call.h"
#include "blitzar_amd/csrc/proof/key_table.h"

namespace bz::proof {
namespace {
constexpr u32 kLdsBins = 4096;    // 16 KB of u32 count bins
constexpr u32 kLdsSumBins = 4096; // 32 KB of 64-bit accumulators
constexpr u32 kLdsBlocks = 1024;  // each adds its non-zero bins at the end

// the value columns of a call and where their chunks lie among a table row's accumulators; travels
// as a kernel argument and is indexed by wave-uniform values alone
struct sum_columns {
  column_view v[kMaxKeySumValues];
  u32 first_chunk[kMaxKeySumValues], chunks[kMaxKeySumValues];
  u32 count, row_chunks;
};

// 2^256 R as a residue: F::mul(x, this) = x 2^256
template <class E> BZ_HD typename E::F::fe two_pow_256() {
  using F = typename E::F;
  const u64 w[4] = {0, 0, 1, 0};
  const typename F::fe k128 = F::mul(F::from_words(w), E::conversion(false)); // 2^128 R
  return F::mul(k128, k128);
}
// the residue of a magnitude of 320 bits with its sign
template <class E>
BZ_HD typename E::F::fe residue_of_wide(const u64* wide, bool negative,
                                        const typename E::F::fe& k256) {
  using F = typename E::F;
  const u64 top[4] = {wide[4], 0, 0, 0};
  const typename F::fe low = F::reduce(F::from_words(wide));
  const typename F::fe high = F::mul(F::reduce(F::from_words(top)), k256);
  const typename F::fe v = fadd<F>(low, high);
  return F::select(v, fneg<F>(v), negative);
}
// row `index` of sums (element form) and scalars (scalar form) from the residue of the sum of a
// column's rows as they lie in memory: of narrow rows the value itself, of 32-byte rows (`element`)
// the value in element form.  Field 0: one form.  Field 1: element form is the value times 2^256
template <class E>
BZ_HD void store_sum(u64* sums, u64* scalars, u64 index, const typename E::F::fe& sum, bool element,
                     const typename E::F::fe& k256) {
  using F = typename E::F;
  typename F::fe in_element = sum, in_scalar = sum;
  if constexpr (std::is_same_v<E, grumpkin_elements>) {
    if (element) {
      typename F::fe c5 = F::zero();
      c5.v[0] = 1u << (F::LB * F::N - 256); // 2^5 / R = 2^-256
      in_scalar = F::mul(sum, c5);
    } else {
      in_element = F::mul(sum, k256);
    }
  }
  u64 w[4];
  if (sums != nullptr) {
    F::to_words(w, F::canonical(in_element));
#pragma unroll
    for (u32 k = 0; k < 4; ++k) sums[4 * index + k] = w[k];
  }
  if (scalars != nullptr) {
    F::to_words(w, F::canonical(in_scalar));
#pragma unroll
    for (u32 k = 0; k < 4; ++k) scalars[4 * index + k] = w[k];
  }
}

// the row of the range table T[t] = t a key hits, or kEmptySlot
BZ_HD u32 range_row(const lookup_key& key, u64 table_rows) {
  const bool hit = (key.w[1] | key.w[2] | key.w[3]) == 0 && key.w[0] < table_rows;
  return hit ? static_cast<u32>(key.w[0]) : kEmptySlot;
}

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCountThreads)
    k_clear_key_sums(u32* slot_rows, u64 slots, u64* acc, u64 acc_words, u64* counts,
                     u64 table_rows, u64* misses) {
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  const u64 first = static_cast<u64>(blockIdx.x) * kCountThreads + threadIdx.x;
  clear_slots(slot_rows, slots, first, stride);
  for (u64 a = first; a < acc_words; a += stride) acc[a] = 0;
  if (counts != nullptr) {
    for (u64 t = first; t < table_rows; t += stride) counts[t] = 0;
  }
  if (first == 0 && misses != nullptr) *misses = 0;
}

// the sum of a 64-bit word over the 64 lanes, in every lane; called by all lanes together
__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
  for (int offset = 32; offset >= 1; offset >>= 1) {
    x += static_cast<u64>(__shfl_xor(static_cast<unsigned long long>(x), offset));
  }
  return x;
}

// kRange: the range table (table.data null, nothing to probe).  kLds: counts and accumulators in
// bins in LDS, added to global memory at the workgroup's end (a workgroup sees fewer than 2^32 rows)
template <class E, bool kRange, bool kLds>
__global__ void __launch_bounds__(kCountThreads)
    k_accumulate_rows(u64* acc, u64* counts, u64* misses, u32* matches,
                      const u32* __restrict__ slot_rows, u64 slots, const column_view table,
                      const column_view lookups, const sum_columns values) {
  __shared__ u32 bins[kLds ? kLdsBins : 1];
  __shared__ u64 sum_bins[kLds ? kLdsSumBins : 1];
  const u32 used_bins = kLds && counts != nullptr ? static_cast<u32>(table.n) : 0;
  const u32 used_sum_bins = kLds ? static_cast<u32>(table.n) * values.row_chunks : 0;
  for (u32 b = threadIdx.x; b < used_bins; b += kCountThreads) bins[b] = 0;
  for (u32 b = threadIdx.x; b < used_sum_bins; b += kCountThreads) sum_bins[b] = 0;
  if constexpr (kLds) __syncthreads();
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  u64 wave_misses = 0;
  wave_adder adder;
  // `base` is the workgroup's: every lane of a wavefront takes the same number of turns
  for (u64 base = static_cast<u64>(blockIdx.x) * kCountThreads; base < lookups.n; base += stride) {
    const u64 i = base + threadIdx.x;
    const bool active = i < lookups.n;
    u32 found = kEmptySlot;
    if (active) {
      const lookup_key key = key_of<E>(lookups, i);
      if constexpr (kRange) {
        found = range_row(key, table.n);
      } else {
        found = find_row<E>(slot_rows, slots, table, key);
      }
      if (matches != nullptr) matches[i] = found;
    }
    const bool hit = found != kEmptySlot;
    if (counts != nullptr) {
      if constexpr (kLds) {
        if (hit) atomicAdd(bins + found, 1u);
      } else {
        adder.add(counts, found, hit);
      }
    }
    wave_misses += static_cast<u64>(__popcll(__ballot(active && !hit)));
    // the hot key: every hit lane of the wavefront, two at least, on one row
    bool one_row = false;
    u32 shared_row = 0;
    if constexpr (!kLds) {
      const u64 hits = __ballot(hit);
      if (__popcll(hits) >= 2) {
        const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(hits))) - 1;
        shared_row = static_cast<u32>(
            __builtin_amdgcn_readlane(static_cast<int>(found), static_cast<int>(leader)));
        one_row = __ballot(hit && found == shared_row) == hits;
      }
    }
    for (u32 v = 0; v < values.count; ++v) {
      const column_view c = values.v[v];
      const u32 chunks = values.chunks[v];
      const bool present = hit && i < c.n;
      u64 w[4] = {0, 0, 0, 0};
      bool negative = false;
      if (present) negative = load_magnitude(w, c, i);
      const u64 at = static_cast<u64>(one_row ? shared_row : hit ? found : 0) * values.row_chunks +
                     values.first_chunk[v];
#pragma unroll
      for (u32 k = 0; k < kMaxValueChunks; ++k) {
        if (k < chunks) {
          const u32 chunk = chunk_of(w, k); // zero in a lane without a row
          const u64 delta = chunk_delta(chunk, negative);
          if constexpr (kLds) {
            if (chunk != 0) {
              (void)__hip_atomic_fetch_add(sum_bins + at + k, delta, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          } else if (one_row) {
            const u64 total = wave_sum(delta);
            if (total != 0 && __lane_id() == 0) {
              (void)__hip_atomic_fetch_add(acc + at + k, total, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
          } else if (chunk != 0) {
            (void)__hip_atomic_fetch_add(acc + at + k, delta, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
  }
  if (counts != nullptr) adder.flush(counts);
  if (__lane_id() == 0 && wave_misses != 0 && misses != nullptr) {
    (void)__hip_atomic_fetch_add(misses, wave_misses, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (kLds) {
    __syncthreads();
    for (u32 b = threadIdx.x; b < used_bins; b += kCountThreads) {
      const u32 count = bins[b];
      if (count != 0) {
        (void)__hip_atomic_fetch_add(counts + b, static_cast<u64>(count), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    for (u32 b = threadIdx.x; b < used_sum_bins; b += kCountThreads) {
      const u64 total = sum_bins[b];
      if (total != 0) {
        (void)__hip_atomic_fetch_add(acc + b, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

template <class E>
__global__ void __launch_bounds__(kCountThreads)
    k_finish_sums(u64* sums, u64* scalars, const u64* __restrict__ acc, u64 table_rows,
                  const sum_columns values) {
  using F = typename E::F;
  const u64 stride = static_cast<u64>(gridDim.x) * kCountThreads;
  const typename F::fe k256 = two_pow_256<E>();
  for (u32 v = 0; v < values.count; ++v) {
    const u32 chunks = values.chunks[v];
    const bool element = values.v[v].nbytes == E::element_bytes;
    for (u64 t = static_cast<u64>(blockIdx.x) * kCountThreads + threadIdx.x; t < table_rows;
         t += stride) {
      const u64* mine = acc + t * values.row_chunks + values.first_chunk[v];
      u64 words[kMaxValueChunks], wide[kWideWords];
#pragma unroll
      for (u32 k = 0; k < kMaxValueChunks; ++k) words[k] = k < chunks ? mine[k] : 0;
      recombine_chunks(wide, words);
      const bool negative = wide_magnitude(wide);
      store_sum<E>(sums, scalars, v * table_rows + t, residue_of_wide<E>(wide, negative, k256),
                   element, k256);
    }
  }
}

//--------------------------------------------------------------------------------------------------
// host backend: row by row, one field addition per row and value column
//--------------------------------------------------------------------------------------------------
template <class E> void sum_host(const key_sum_outputs& out, const key_sums& k) {
  using F = typename E::F;
  using fe = typename F::fe;
  const column_view table = make_column_view(k.table), lookups = make_column_view(k.lookups);
  const u64 m = table.n;
  std::vector<column_view> views(k.num_values);
  for (u32 v = 0; v < k.num_values; ++v) views[v] = make_column_view(k.values[v]);
  const auto table_key = [&](u64 t) { return key_of<E>(table, t); };
  const bool range = k.table.data == nullptr;
  const u64 slots = range ? 0 : slot_count(m);
  std::vector<u32> slot_rows(slots);
  if (!range) model_insert(slot_rows.data(), slots, m, table_key);
  std::vector<fe> totals(m * k.num_values, F::zero());
  std::vector<u64> counts(m, 0);
  u64 missed = 0;
  u32* matches = static_cast<u32*>(out.matches);
  for (u64 i = 0; i < lookups.n; ++i) {
    const lookup_key key = key_of<E>(lookups, i);
    const u32 row =
        range ? range_row(key, m) : model_find(slot_rows.data(), slots, m, table_key, key);
    if (matches != nullptr) matches[i] = row;
    if (row == kEmptySlot) {
      ++missed;
      continue;
    }
    ++counts[row];
    for (u32 v = 0; v < k.num_values; ++v) {
      fe& total = totals[v * m + row];
      if (i < views[v].n) total = fadd<F>(total, load_raw<F>(views[v], i));
    }
  }
  if (out.counts != nullptr) std::memcpy(out.counts, counts.data(), 8 * m);
  if (out.misses != nullptr) *static_cast<u64*>(out.misses) = missed;
  const fe k256 = two_pow_256<E>();
  for (u64 j = 0; j < m * k.num_values; ++j) {
    store_sum<E>(static_cast<u64*>(out.sums), static_cast<u64*>(out.scalars), j, totals[j],
                 views[j / m].nbytes == E::element_bytes, k256);
  }
}

//--------------------------------------------------------------------------------------------------
// device form: enqueue only
//--------------------------------------------------------------------------------------------------
sum_columns sum_columns_of(const key_sums& k) {
  sum_columns values;
  std::memset(&values, 0, sizeof(values));
  values.count = k.num_values;
  for (u32 v = 0; v < k.num_values; ++v) {
    values.v[v] = make_column_view(k.values[v]);
    values.first_chunk[v] = values.row_chunks;
    values.chunks[v] = value_chunks(k.values[v].nbytes);
    values.row_chunks += values.chunks[v];
  }
  return values;
}

template <class E, bool kRange>
void accumulate_enqueue(u64* acc, const key_sum_outputs& out, const u32* slot_rows, u64 slots,
                        const column_view& table, const column_view& lookups,
                        const sum_columns& values, hipStream_t stream) {
  u64* counts = static_cast<u64*>(out.counts);
  u64* misses = static_cast<u64*>(out.misses);
  u32* matches = static_cast<u32*>(out.matches);
  if (table.n <= kLdsBins && table.n * values.row_chunks <= kLdsSumBins) {
    hipLaunchKernelGGL((k_accumulate_rows<E, kRange, true>), dim3(blocks_for(lookups.n, kLdsBlocks)),
                       dim3(kCountThreads), 0, stream, acc, counts, misses, matches, slot_rows,
                       slots, table, lookups, values);
  } else {
    hipLaunchKernelGGL((k_accumulate_rows<E, kRange, false>),
                       dim3(blocks_for(lookups.n, kCountBlocks)), dim3(kCountThreads), 0, stream,
                       acc, counts, misses, matches, slot_rows, slots, table, lookups, values);
  }
  BZ_HIP_CHECK(hipGetLastError());
}

template <class E>
void sum_enqueue(const key_sum_outputs& out, const key_sums& k, void* workspace,
                 hipStream_t stream) {
  const column_view lookups = make_column_view(k.lookups);
  const column_view table = make_column_view(k.table);
  const sum_columns values = sum_columns_of(k);
  const u64 m = k.table.n;
  const bool range = k.table.data == nullptr;
  const u64 slots = range ? 0 : slot_count(m);
  const u64 acc_words = m * values.row_chunks;
  // the range table with no value column has no workspace
  u8* base = workspace != nullptr ? workspace_carver::aligned(workspace) : nullptr;
  u32* slot_rows = range ? nullptr : reinterpret_cast<u32*>(base);
  u64* acc = acc_words != 0 ? reinterpret_cast<u64*>(base + key_sum_slot_bytes(m)) : nullptr;
  const u64 most = std::max(std::max(slots, acc_words), m);
  hipLaunchKernelGGL(k_clear_key_sums, dim3(blocks_for(most, kCountBlocks)), dim3(kCountThreads), 0,
                     stream, slot_rows, slots, acc, acc_words, static_cast<u64*>(out.counts), m,
                     static_cast<u64*>(out.misses));
  BZ_HIP_CHECK(hipGetLastError());
  if (range) {
    accumulate_enqueue<E, true>(acc, out, slot_rows, slots, table, lookups, values, stream);
  } else {
    hipLaunchKernelGGL((k_insert_rows<E>), dim3(blocks_for(m, kCountBlocks)), dim3(kCountThreads),
                       0, stream, slot_rows, slots, table);
    BZ_HIP_CHECK(hipGetLastError());
    accumulate_enqueue<E, false>(acc, out, slot_rows, slots, table, lookups, values, stream);
  }
  hipLaunchKernelGGL((k_finish_sums<E>), dim3(blocks_for(m, kCountBlocks)), dim3(kCountThreads), 0,
                     stream, static_cast<u64*>(out.sums), static_cast<u64*>(out.scalars), acc, m,
                     values);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += range ? 3 : 4;
}
} // namespace

void check_key_sums(const key_sum_outputs& out, unsigned field_id, const key_sums& k,
                    const void* workspace, u64 workspace_bytes, bool device_form) {
  const u64 m = k.table.n, n = k.lookups.n;
  BZ_RELEASE_ASSERT(k.num_values <= kMaxKeySumValues, "the sums by key need num_values <= 8");
  BZ_RELEASE_ASSERT(k.num_values != 0 || (out.sums == nullptr && out.scalars == nullptr),
                    "the sums by key with num_values = 0 need sums and scalars null");
  BZ_RELEASE_ASSERT(k.num_values == 0 || out.sums != nullptr || out.scalars != nullptr,
                    "the sums by key with num_values >= 1 need sums or scalars");
  BZ_RELEASE_ASSERT(out.sums != nullptr || out.scalars != nullptr || out.counts != nullptr ||
                        out.misses != nullptr || out.matches != nullptr,
                    "the sums by key need an output");
  BZ_RELEASE_ASSERT(m >= 1 && m <= kMaxTableRows, "the sums by key need 1 <= table rows <= 2^28");
  BZ_RELEASE_ASSERT(n <= kMaxLookupRows, "the sums by key need lookup rows <= 2^30");
  for (u32 v = 0; v < k.num_values; ++v) {
    BZ_RELEASE_ASSERT(k.values[v].n <= n, "a value column of the sums by key is longer than n");
  }
  const auto address = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  BZ_RELEASE_ASSERT(address(out.sums) % 8 == 0 && address(out.scalars) % 8 == 0 &&
                        address(out.counts) % 8 == 0 && address(out.misses) % 8 == 0,
                    "the outputs of the sums by key must be 8-byte aligned");
  BZ_RELEASE_ASSERT(address(out.matches) % 4 == 0, "the matches must be 4-byte aligned");
  // the range table without value columns alone has no workspace
  if (device_form && (k.table.data != nullptr || k.num_values != 0)) {
    BZ_RELEASE_ASSERT(workspace != nullptr &&
                          workspace_bytes >= key_sum_workspace_bytes(m, k.num_values),
                      "the workspace of the sums by key is too small");
  } else {
    workspace_bytes = 0;
  }
  const u64 sum_bytes = 32 * m * k.num_values;
  const byte_range outputs[5] = {{out.sums, sum_bytes},
                                 {out.scalars, sum_bytes},
                                 {out.counts, 8 * m},
                                 {out.misses, 8},
                                 {out.matches, 4 * n}};
  for (u32 a = 0; a < 5; ++a) {
    for (u32 b = a + 1; b < 5; ++b) {
      BZ_RELEASE_ASSERT(!overlap(outputs[a], outputs[b]), "the outputs of the sums by key overlap");
    }
    BZ_RELEASE_ASSERT(!overlap(outputs[a], {k.table.data, m * k.table.nbytes}) &&
                          !overlap(outputs[a], {k.lookups.data, n * k.lookups.nbytes}),
                      "an output overlaps an input of the same call");
    for (u32 v = 0; v < k.num_values; ++v) {
      BZ_RELEASE_ASSERT(!overlap(outputs[a], {k.values[v].data, k.values[v].n * k.values[v].nbytes}),
                        "an output overlaps an input of the same call");
    }
    BZ_RELEASE_ASSERT(!overlap(outputs[a], {workspace, workspace_bytes}),
                      "an output overlaps the workspace of the same call");
  }
  BZ_RELEASE_ASSERT(field_id <= 1, "unsupported field id");
}

void sum_by_key_device(const key_sum_outputs& out, unsigned field_id, const key_sums& k,
                       void* workspace, hipStream_t stream) {
  with_elements(field_id, [&](auto elements) {
    sum_enqueue<decltype(elements)>(out, k, workspace, stream);
  });
}

void sum_by_key(api_state& st, const key_sum_outputs& out, unsigned field_id, const key_sums& k) {
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      sum_host<E>(out, k);
      return;
    }
    // the columns up at their own width, the device form, the results down
    host_call call{st};
    const u64 m = k.table.n, n = k.lookups.n;
    const size_t sum_bytes = static_cast<size_t>(32) * m * k.num_values;
    key_sum_outputs staged_out;
    key_sums staged = k;
    std::vector<sumcheck_column> values;
    void* workspace = nullptr;
    call.output(&staged_out.sums, out.sums, sum_bytes);
    call.output(&staged_out.scalars, out.scalars, sum_bytes);
    call.output(&staged_out.counts, out.counts, 8 * m);
    call.output(&staged_out.misses, out.misses, 8);
    call.output(&staged_out.matches, n != 0 ? out.matches : nullptr, 4 * n);
    // a range table has no rows to upload and stays null; so do lookups of no rows
    call.input(&staged.table.data, k.table.data, m * k.table.nbytes);
    call.input(&staged.lookups.data, n != 0 ? k.lookups.data : nullptr, n * k.lookups.nbytes);
    call.columns(&values, k.values, k.num_values);
    call.scratch(&workspace, key_sum_workspace_bytes(m, k.num_values));
    call.allocate();
    staged.values = values.data();
    sum_enqueue<E>(staged_out, staged, workspace, call.stream());
    call.finish();
  });
}
} // namespace bz::proof
