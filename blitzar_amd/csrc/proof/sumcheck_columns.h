// What the provers over typed columns share (proof/sumcheck_columns.hip: the callback form;
// proof/sumcheck_transcript.hip: the chain with the built-in transcript): how a column is described
// to a kernel, how an element is fetched as the raw residue of its bytes, round 0's `Tables` over
// the columns, the first fold of one element, and what both forms prepare on the host (views,
// multipliers scaled by conversion constants, the length check).  Why raw residues are enough is
// in the head comment of proof/sumcheck_columns.hip.  The round-0 kernels are compiled once, in
// proof/sumcheck_columns.hip, and reached through launch_sumcheck_columns_round; the small loaders
// are inline, for the kernels of either translation unit that read a column.
#pragma once

#include "blitzar_amd/csrc/proof/sumcheck_rows.h"

namespace bz::proof {
// how an element's bytes are fetched (the same for a whole column: uniform over a wavefront)
enum : u32 {
  kAccessBytes = 0, // any width, any address
  kAccessWords = 1, // width a multiple of 8 at an address that is one
};

struct column_view {
  const u8* data;
  u64 n;
  u32 nbytes, access, is_signed, reserved;
};

inline u32 access_of(const void* data, u32 nbytes) {
  return nbytes % 8 == 0 && reinterpret_cast<uintptr_t>(data) % 8 == 0 ? kAccessWords : kAccessBytes;
}

// w = the little-endian integer of the c.nbytes bytes at p
BZ_HD void load_bytes(u64* w, const column_view& c, const u8* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the aligned 32-bit words the bytes lie in (never more memory than those: nothing outside the
  // words that hold a byte of the column is touched), shifted into place and cut to the width;
  // every array index is a constant, so the words stay in registers
  const u64 address = reinterpret_cast<u64>(p);
  const u32 offset = static_cast<u32>(address & 3);
  const u32* q = reinterpret_cast<const u32*>(address - offset);
  u32 d[9];
#pragma unroll
  for (u32 k = 0; k < 9; ++k) d[k] = 4 * k < offset + c.nbytes ? q[k] : 0;
#pragma unroll
  for (u32 k = 0; k < 8; ++k) {
    u32 x = __builtin_amdgcn_alignbyte(d[k + 1], d[k], offset);
    const u32 have = c.nbytes > 4 * k ? c.nbytes - 4 * k : 0;
    if (have < 4) x &= (1u << (8 * have)) - 1;
    if (k % 2 == 0) {
      w[k / 2] = x;
    } else {
      w[k / 2] |= static_cast<u64>(x) << 32;
    }
  }
#else
  for (u32 k = 0; k < c.nbytes; ++k) w[k >> 3] |= static_cast<u64>(p[k]) << (8 * (k & 7));
#endif
}

// w = magnitude of row i < c.n of the column (little-endian words); returns its sign
BZ_HD bool load_magnitude(u64* w, const column_view& c, u64 i) {
  const u8* p = c.data + i * c.nbytes;
  if (c.access == kAccessWords) {
    const u64* q = reinterpret_cast<const u64*>(p);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
      if (8 * k < c.nbytes) w[k] = q[k];
    }
  } else {
    load_bytes(w, c, p);
  }
  if (c.is_signed == 0) return false;
  // at most 16 bytes: sign-extend to 128 bits, take the magnitude
  u64 lo = w[0], hi = w[1];
  if (c.nbytes <= 8) {
    const u32 s = 64 - 8 * c.nbytes;
    lo = static_cast<u64>(static_cast<i64>(lo << s) >> s);
    hi = static_cast<u64>(static_cast<i64>(lo) >> 63);
  } else {
    const u32 s = 128 - 8 * c.nbytes;
    hi = static_cast<u64>(static_cast<i64>(hi << s) >> s);
  }
  const bool negative = static_cast<i64>(hi) < 0;
  if (negative) {
    lo = ~lo + 1;
    hi = ~hi + (lo == 0 ? 1 : 0);
  }
  w[0] = lo;
  w[1] = hi;
  return negative;
}

// row i < c.n as the raw residue of its bytes, normalised, V < 4 (32 bytes may hold up to 16 p)
template <class F> BZ_HD typename F::fe load_raw(const column_view& c, u64 i) {
  u64 w[4] = {0, 0, 0, 0};
  const bool negative = load_magnitude(w, c, i);
  const typename F::fe v = F::reduce(F::from_words(w));
  return F::select(v, fneg<F>(v), negative);
}

// the `Tables` of round 0 (proof/sumcheck_rows.h), raw: rows past a column's end are zero; nothing
// is common to the columns of a row (every column has its own length)
struct no_row_state {};
template <class F> struct column_tables {
  const column_view* views;
  u64 mid;
  BZ_HD no_row_state row(u64) const { return {}; }
  BZ_HD void pair(u32 mle, u64 i, no_row_state, typename F::fe& a, typename F::fe& b) const {
    const column_view c = views[mle];
    a = i < c.n ? load_raw<F>(c, i) : F::zero();
    b = mid + i < c.n ? fsub<F>(load_raw<F>(c, mid + i), a) : fneg<F>(a);
  }
};

// The first fold, one output element in engine form from raw rows; rows past the column's end are
// zero.  r() and one_minus_r(): the challenge and its complement times the conversion constant of
// the column's kind, asked for only where a row exists (each fold kernel has its own way of
// obtaining them, and keeps it where it was: inside the branch)
template <class F, class R, class OneMinusR>
BZ_HD typename F::fe fold_column_element(const column_view& c, u64 mid, u64 i, const R& r,
                                         const OneMinusR& one_minus_r) {
  typename F::fe v = F::zero();
  if (i < c.n) v = F::mul(load_raw<F>(c, i), one_minus_r());
  if (mid + i < c.n) v = fadd<F>(v, F::mul(r(), load_raw<F>(c, mid + i)));
  return v;
}

//--------------------------------------------------------------------------------------------------
// host side
//--------------------------------------------------------------------------------------------------
inline column_view make_column_view(const sumcheck_column& c) {
  return column_view{static_cast<const u8*>(c.data), c.n, c.nbytes, access_of(c.data, c.nbytes),
                     c.is_signed ? 1u : 0u, 0};
}

// out[p] = products[p] with its multiplier times the conversion constants of its terms' columns:
// what round 0 on raw rows takes
template <class E>
void conversion_scaled_products(product_desc<typename E::F>* out,
                                const product_desc<typename E::F>* products, u32 num_products,
                                const u32* terms, const column_view* views) {
  using F = typename E::F;
  for (u32 p = 0; p < num_products; ++p) {
    product_desc<F> raw = products[p];
    for (u32 t = 0; t < raw.num_terms; ++t) {
      const column_view& c = views[terms[raw.first_term + t]];
      raw.multiplier = F::mul(raw.multiplier, E::conversion(c.nbytes == E::element_bytes));
    }
    out[p] = raw;
  }
}

inline void check_column_lengths(const sumcheck_inputs& d, const sumcheck_column* columns) {
  for (u32 j = 0; j < d.num_mles; ++j) {
    BZ_RELEASE_ASSERT(columns[j].n <= d.n, "a sumcheck column is longer than n");
  }
}

// round 0 on the columns, enqueued on `stream` (kernels of proof/sumcheck_columns.hip):
// partials[block][k] as the round kernels of proof/sumcheck.hip leave them; `products`: the
// conversion-scaled ones
template <class F>
void launch_sumcheck_columns_round(hipStream_t stream, u32 blocks, typename F::fe* partials,
                                   const column_view* views, u64 mid,
                                   const product_desc<F>* products, u32 num_products,
                                   const u32* terms, u32 degree);
} // namespace bz::proof
