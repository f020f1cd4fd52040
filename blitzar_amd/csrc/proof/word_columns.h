// The word columns of a range check (proof/word_columns.hip, bzamd_decompose_words*,
// bzamd_map_words*): byte k of the key of every row of a typed column as a u8 column of its own
// (plane k), the 256 counts of those bytes over all planes, the number of rows whose key does not
// fit the planes, and the columns table[word] a plane maps to (with the table of inverses
// 1 / (alpha + v), the inverse-word columns).  The definitions are those above
// bzamd_decompose_words and bzamd_map_words in include/blitzar_amd.h.
//
// The first half of this file is plain C++ that g++ compiles without HIP and without the field
// headers: what a key's bytes and its overflow are, the planes' extent, and sequential models of
// both calls.  The kernels, the cpu backend and tests/native/word_columns_check.cc share this one
// copy.
#pragma once

#include "blitzar_amd/csrc/proof/multiplicities.h"

namespace bz::proof {
constexpr u64 kMaxWordRows = u64{1} << 30;
constexpr u32 kMaxWords = 32; // the bytes of a key
constexpr u32 kWordValues = 256;

// byte k < 32 of a key
BZ_HD u32 key_byte(const lookup_key& key, u32 k) {
  return static_cast<u32>(key.w[k >> 3] >> (8 * (k & 7))) & 0xFFu;
}
// whether key >= 2^(8 num_words), 1 <= num_words <= 32
BZ_HD bool key_overflows(const lookup_key& key, u32 num_words) {
  u64 above = 0;
#pragma unroll
  for (u32 t = 0; t < 4; ++t) {
    if (8 * num_words <= 64 * t) {
      above |= key.w[t];
    } else if (8 * num_words < 64 * (t + 1)) {
      above |= key.w[t] >> (8 * num_words - 64 * t);
    }
  }
  return above != 0;
}
// the bytes from the first byte of plane 0 to the last byte of the last plane; columns of
// `row_bytes` bytes a row likewise
BZ_HD u64 planes_extent(u32 num_planes, u64 stride, u64 n, u64 row_bytes = 1) {
  return num_planes == 0 || n == 0 ? 0 : (num_planes - 1) * stride + row_bytes * n;
}

// the sequential model of bzamd_decompose_words: key_at(i) returns the key of row i.  Every output
// may be null
template <class KeyAt>
void model_decompose(u8* words, u64* counts, u64* overflow, u64 n, u32 num_words, u64 plane_stride,
                     const KeyAt& key_at) {
  u64 counted[kWordValues] = {}, overflowed = 0;
  for (u64 i = 0; i < n; ++i) {
    const lookup_key key = key_at(i);
    for (u32 k = 0; k < num_words; ++k) {
      const u32 word = key_byte(key, k);
      if (words != nullptr) words[k * plane_stride + i] = static_cast<u8>(word);
      ++counted[word];
    }
    overflowed += key_overflows(key, num_words) ? 1 : 0;
  }
  if (counts != nullptr) {
    for (u32 v = 0; v < kWordValues; ++v) counts[v] = counted[v];
  }
  if (overflow != nullptr) *overflow = overflowed;
}

// bzamd_word_map, and its sequential model: mapped_k[i] = table[words_k[i]], 32 bytes a row
struct word_map {
  const void* words;
  const void* table;
  u32 num_planes;
  u64 n, plane_stride, mapped_stride;
};
inline void model_map(void* mapped, const word_map& m) {
  const u8* words = static_cast<const u8*>(m.words);
  const u8* table = static_cast<const u8*>(m.table);
  u8* out = static_cast<u8*>(mapped);
  for (u32 k = 0; k < m.num_planes; ++k) {
    for (u64 i = 0; i < m.n; ++i) {
      const u8* row = table + 32 * static_cast<u64>(words[k * m.plane_stride + i]);
      for (u32 b = 0; b < 32; ++b) out[k * m.mapped_stride + 32 * i + b] = row[b];
    }
  }
}
} // namespace bz::proof

//--------------------------------------------------------------------------------------------------
// the library's entry points (HIP translation units only)
//--------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
struct word_decomposition {
  sumcheck_column column; // checked by the C ABI
  const void* shift;
  u32 num_words;
  u64 plane_stride;
};
// the checks both forms share (nulls, limits, strides, alignment, overlaps, the field id): aborts.
// The C ABI runs them before either form below (and before it asks for the backend), which do not
// repeat them
void check_word_decomposition(const void* words, const void* counts, const void* overflow,
                              unsigned field_id, const word_decomposition& d);
void check_word_map(const void* mapped, const word_map& m);
// bzamd_decompose_words / bzamd_map_words: host operands, blocking, st.backend; GPU backend: the
// column uploaded at its own width (the planes one after the other) to devices[0], whose lease the
// caller holds
void decompose_words(api_state& st, void* words, u64* counts, u64* overflow, unsigned field_id,
                     const word_decomposition& d);
void map_words(api_state& st, void* mapped, const word_map& m);
// everything but `d` / `m` is memory of the current device; enqueue-only: TWO kernel launches
// (decompose: the clear of counts and overflow, then the one pass over the rows), ONE (map)
constexpr u32 kDecomposeLaunches = 2, kMapLaunches = 1;
void decompose_words_device(void* words, u64* counts, u64* overflow, unsigned field_id,
                            const word_decomposition& d, hipStream_t stream);
void map_words_device(void* mapped, const word_map& m, hipStream_t stream);
} // namespace bz::proof
#endif
