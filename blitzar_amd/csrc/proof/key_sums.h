// Sums of typed value columns by key (proof/key_sums.hip, bzamd_sum_by_key*): per table row t that
// is the first of its key, the sum in the field of every value column over the lookup rows that
// carry the key, their count, and per lookup row the table row it hit.  The definitions are those
// above bzamd_sum_by_key in include/blitzar_amd.h.
//
// The first half of this file is plain C++ that g++ compiles without HIP and without the field
// headers: how the device form sums exactly without field arithmetic per row.  A row's magnitude is
// cut into 32-bit chunks; chunk k of a non-negative row is added to a signed 64-bit accumulator,
// that of a negative row subtracted; the accumulators of one (table row, value column) are put
// together once, at the end, into one wide two's-complement integer sum_k acc[k] 2^(32 k), whose
// magnitude and sign go into the field.  Integer adds commute: the result does not depend on the
// order of arrival.  The finish kernel, the stand-alone check tests/native/key_sums_check.cc and
// its sequential model share this one copy.
#pragma once

#include "blitzar_amd/csrc/proof/multiplicities.h"

namespace bz::proof {
constexpr u32 kMaxKeySumValues = 8;
constexpr u32 kMaxValueChunks = 8; // a 32-byte row in 32-bit chunks
constexpr u32 kWideWords = 5;      // the wide sum: 320 bits, two's complement

// An accumulator takes at most one chunk of every lookup row: with n <= 2^30 rows and chunks below
// 2^32 its magnitude stays below 2^62, so a signed 64-bit word never wraps, and the wide sum stays
// below 2^62 (2^224 + 2^192 + ...) < 2^287 in magnitude
static_assert(kMaxLookupRows <= (u64{1} << 30), "|accumulator| < 2^62 needs n <= 2^30");

// 32-bit chunks of a row of `nbytes` bytes
BZ_HD u32 value_chunks(u32 nbytes) { return (nbytes + 3) / 4; }
// chunk k < 8 of a magnitude of four little-endian words
BZ_HD u32 chunk_of(const u64* magnitude, u32 k) {
  return static_cast<u32>(magnitude[k / 2] >> (32 * (k % 2)));
}
// what chunk `chunk` of a row adds to its accumulator (two's complement: the adds are unsigned)
BZ_HD u64 chunk_delta(u32 chunk, bool negative) {
  return negative ? ~static_cast<u64>(chunk) + 1 : static_cast<u64>(chunk);
}
// one row into the accumulators of its (table row, value column), sequentially
BZ_HD void accumulate_row(u64* acc, const u64* magnitude, bool negative, u32 chunks) {
  for (u32 k = 0; k < chunks; ++k) acc[k] += chunk_delta(chunk_of(magnitude, k), negative);
}

// wide[0 .. 5) = sum_k acc[k] 2^(32 k) as a two's-complement integer of 320 bits; acc: eight signed
// words below 2^62 in magnitude (those past a column's chunks are zero).  Every index is a
// constant once the loops are unrolled: the words stay in registers on the device
BZ_HD void recombine_chunks(u64* wide, const u64* acc) {
#pragma unroll
  for (u32 j = 0; j < kWideWords; ++j) wide[j] = 0;
#pragma unroll
  for (u32 k = 0; k < kMaxValueChunks; ++k) {
    const i64 a = static_cast<i64>(acc[k]);
    const u64 sign = static_cast<u64>(a >> 63); // all ones for a negative word
    const u32 j = k / 2;
    // the sign-extended word shifted by 32 (k % 2) bits: two words, then `sign` up to the top
    const u64 low = k % 2 == 0 ? static_cast<u64>(a) : static_cast<u64>(a) << 32;
    const u64 high = k % 2 == 0 ? sign : static_cast<u64>(a >> 32);
    u64 carry = 0;
#pragma unroll
    for (u32 i = j; i < kWideWords; ++i) {
      const u64 x = i == j ? low : i == j + 1 ? high : sign;
      const u64 s = wide[i] + x;
      const u64 t = s + carry;
      carry = (s < x ? 1u : 0u) | (t < s ? 1u : 0u);
      wide[i] = t;
    }
  }
}
// wide <- |wide|; returns whether it was negative
BZ_HD bool wide_magnitude(u64* wide) {
  const bool negative = (wide[kWideWords - 1] >> 63) != 0;
  u64 carry = 1;
#pragma unroll
  for (u32 j = 0; j < kWideWords; ++j) {
    const u64 flipped = ~wide[j] + carry;
    carry = carry != 0 && flipped == 0 ? 1 : 0;
    wide[j] = negative ? flipped : wide[j];
  }
  return negative;
}

// what the device form's workspace holds: the slots of the table (proof/multiplicities.h), eight
// accumulators of eight bytes per table row and value column (the widest kind; narrower columns
// use the front of it), and what the caller's pointer may lack to a multiple of 256.  0 outside
// 1 <= table_rows <= 2^28, num_values <= 8
BZ_HD u64 key_sum_slot_bytes(u64 table_rows) {
  return (4 * slot_count(table_rows) + 255) / 256 * 256;
}
BZ_HD u64 key_sum_workspace_bytes(u64 table_rows, u32 num_values) {
  if (slot_count(table_rows) == 0 || num_values > kMaxKeySumValues) return 0;
  return key_sum_slot_bytes(table_rows) + 8 * kMaxValueChunks * table_rows * num_values + 256;
}
} // namespace bz::proof

//--------------------------------------------------------------------------------------------------
// the library's entry points (HIP translation units only)
//--------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
// `table.data` null: the range table T[t] = t of table.n rows (the C ABI has checked its width);
// `values`: num_values of them, widths checked by the caller, on the host
struct key_sums {
  sumcheck_column table, lookups;
  const sumcheck_column* values;
  u32 num_values;
};
// sums, scalars: num_values x m x 32 bytes; counts: m x u64; misses: one u64; matches: n x u32;
// any may be null within the rules above bzamd_sum_by_key
struct key_sum_outputs {
  void *sums, *scalars, *counts, *misses, *matches;
};
// the checks both forms share (which outputs may be null, limits, alignment, overlaps, the
// workspace, the field id): aborts.  The C ABI runs them before either form below (and before it
// asks for the backend), which do not repeat them.  `device_form`: needs its workspace
void check_key_sums(const key_sum_outputs& out, unsigned field_id, const key_sums& k,
                    const void* workspace, u64 workspace_bytes, bool device_form);
// bzamd_sum_by_key: host operands, blocking, st.backend; cpu backend: row by row, one field
// addition per row and value column; GPU backend: the columns uploaded at their own width to
// devices[0], whose lease the caller holds
void sum_by_key(api_state& st, const key_sum_outputs& out, unsigned field_id, const key_sums& k);
// everything but `k` and the values array is memory of the current device; enqueue-only, four
// kernel launches (the range table: three)
void sum_by_key_device(const key_sum_outputs& out, unsigned field_id, const key_sums& k,
                       void* workspace, hipStream_t stream);
} // namespace bz::proof
#endif
