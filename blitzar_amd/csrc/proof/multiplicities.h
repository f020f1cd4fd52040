// The multiplicity column of a log-derivative argument (proof/multiplicities.hip,
// bzamd_count_multiplicities*): multiplicities[t] = how many rows of the lookup column have the key
// of table row t, given to the FIRST table row of that key, and the number of lookup rows whose key
// is in no table row.  The definitions are those above bzamd_count_multiplicities in
// include/blitzar_amd.h.
//
// The first half of this file is plain C++ that g++ compiles without HIP and without the field
// headers: the key of a row as four words, the hash, the slot count and a sequential model of the
// insert and count kernels over one open-addressing table with linear probing.  The kernels, the
// cpu backend, bzamd_multiplicity_first_slot and tests/native/multiplicities_check.cc share this
// one copy.  The hash is not part of the ABI.
#pragma once

#include "blitzar_amd/csrc/base/macros.h"

namespace bz::proof {
constexpr u64 kMaxTableRows = u64{1} << 28;
constexpr u64 kMaxLookupRows = u64{1} << 30;
constexpr u32 kEmptySlot = 0xFFFFFFFFu; // no row: rows are below 2^28

// the canonical integer in [0, p) of a row's value, little-endian words
struct lookup_key {
  u64 w[4];
};
BZ_HD bool same_key(const lookup_key& a, const lookup_key& b) {
  return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) == 0;
}

// the finaliser of splitmix64: a bijection of 64 bits that spreads consecutive integers, 0 -> 0
BZ_HD u64 mix64(u64 x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
// the words chained from the top down, each through the finaliser with an odd constant added, so
// that a narrow key (upper words zero) and the key 0 are mixed as well
BZ_HD u64 hash_key(const lookup_key& k) {
  u64 h = 0;
#pragma unroll
  for (int i = 3; i >= 0; --i) h = mix64((h ^ k.w[i]) + 0x9E3779B97F4A7C15ull);
  return h;
}

// slots of a table of m rows: the least power of two >= 2 m (no minimum: m = 1 has two); 0 outside
// 1 <= m <= 2^28
BZ_HD u64 slot_count(u64 table_rows) {
  if (table_rows < 1 || table_rows > kMaxTableRows) return 0;
  u64 slots = 2;
  while (slots < 2 * table_rows) slots *= 2;
  return slots;
}
// where the probe for `key` starts; slots: a power of two
BZ_HD u64 first_slot(const lookup_key& key, u64 slots) { return hash_key(key) & (slots - 1); }
// what the device form's workspace holds: the slots and what the caller's pointer may lack to a
// multiple of 256
BZ_HD u64 multiplicity_workspace_bytes(u64 table_rows) {
  const u64 slots = slot_count(table_rows);
  return slots == 0 ? 0 : 4 * slots + 256;
}

//--------------------------------------------------------------------------------------------------
// the sequential model: what the kernels compute, one row after the other.  table_key(t) and
// lookup_key(i) return the key of a row
//--------------------------------------------------------------------------------------------------
// slots[0 .. slots) <- kEmptySlot, then every table row in turn.  A key ends in exactly one slot,
// which holds its least row
template <class TableKey>
void model_insert(u32* slot_rows, u64 slots, u64 table_rows, const TableKey& table_key) {
  for (u64 s = 0; s < slots; ++s) slot_rows[s] = kEmptySlot;
  for (u64 t = 0; t < table_rows; ++t) {
    const lookup_key key = table_key(t);
    u64 slot = first_slot(key, slots);
    for (u64 step = 0; step < slots; ++step, slot = (slot + 1) & (slots - 1)) {
      const u32 row = slot_rows[slot];
      if (row == kEmptySlot) {
        slot_rows[slot] = static_cast<u32>(t);
        break;
      }
      if (same_key(table_key(row), key)) {
        if (t < row) slot_rows[slot] = static_cast<u32>(t);
        break;
      }
    }
  }
}
// the row a key's probe ends on, or kEmptySlot: an empty slot, or `slots` steps without the key
template <class TableKey>
u32 model_find(const u32* slot_rows, u64 slots, u64 table_rows, const TableKey& table_key,
               const lookup_key& key) {
  u64 slot = first_slot(key, slots);
  for (u64 step = 0; step < slots; ++step, slot = (slot + 1) & (slots - 1)) {
    const u32 row = slot_rows[slot];
    if (row >= table_rows) return kEmptySlot;
    if (same_key(table_key(row), key)) return row;
  }
  return kEmptySlot;
}
// multiplicities[0 .. table_rows) and *misses (may be null) from an inserted table
template <class TableKey, class LookupKey>
void model_count(u64* multiplicities, u64* misses, const u32* slot_rows, u64 slots, u64 table_rows,
                 const TableKey& table_key, u64 lookup_rows, const LookupKey& key_of_lookup) {
  for (u64 t = 0; t < table_rows; ++t) multiplicities[t] = 0;
  u64 missed = 0;
  for (u64 i = 0; i < lookup_rows; ++i) {
    const u32 row = model_find(slot_rows, slots, table_rows, table_key, key_of_lookup(i));
    if (row == kEmptySlot) {
      ++missed;
    } else {
      ++multiplicities[row];
    }
  }
  if (misses != nullptr) *misses = missed;
}
} // namespace bz::proof

//--------------------------------------------------------------------------------------------------
// the library's entry points (HIP translation units only)
//--------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
// `table.data` null: the range table T[t] = t of table.n rows (the C ABI has checked its width)
struct multiplicity_count {
  sumcheck_column table, lookups;
};
// the checks both forms share (limits, alignment, overlaps, the workspace, the field id): aborts.
// The C ABI runs them before either form below (and before it asks for the backend), which do not
// repeat them.  `device_form`: the hashed form needs its workspace
void check_multiplicity_count(const void* multiplicities, const void* misses, unsigned field_id,
                              const multiplicity_count& c, const void* workspace,
                              u64 workspace_bytes, bool device_form);
// bzamd_count_multiplicities: host operands, blocking, st.backend; GPU backend: the columns
// uploaded at their own width to devices[0], whose lease the caller holds
void count_multiplicities(api_state& st, u64* multiplicities, u64* misses, unsigned field_id,
                          const multiplicity_count& c);
// everything but `c` is memory of the current device; enqueue-only, three kernel launches (the
// range table: two)
void count_multiplicities_device(u64* multiplicities, u64* misses, unsigned field_id,
                                 const multiplicity_count& c, void* workspace, hipStream_t stream);
// the slot at which the probe for a 32-byte element (may be unreduced) starts; host arithmetic
u64 multiplicity_first_slot(unsigned field_id, const void* element, u64 table_rows);
} // namespace bz::proof
#endif
