// The key of a row of a typed column: the canonical integer in [0, p) of its value, as four
// little-endian words (lookup_key, proof/multiplicities.h).  One copy for the kernels and the cpu
// backends of proof/multiplicities.hip (rows compare by key) and proof/word_columns.hip (the byte
// words of a range check are those of the key).
//
// Key extraction reuses load_magnitude of proof/sumcheck_columns.h: a non-negative row below 32
// bytes is its own key (below 2^248 < p); a negative row takes one subtraction; a 32-byte row one
// reduction, and in field 1 one product by 2^5 (x 2^256 2^5 / 2^261 = x) to leave Montgomery form.
#pragma once

#include <type_traits>

#include "blitzar_amd/csrc/proof/multiplicities.h"
#include "blitzar_amd/csrc/proof/sumcheck_columns.h"

namespace bz::proof {
template <class E> BZ_HD lookup_key key_of(const column_view& c, u64 i) {
  using F = typename E::F;
  lookup_key key = {{0, 0, 0, 0}};
  const bool negative = load_magnitude(key.w, c, i);
  if (c.nbytes < E::element_bytes && !negative) return key;
  typename F::fe v = F::reduce(F::from_words(key.w));
  if (negative) v = fneg<F>(v);
  if constexpr (std::is_same_v<E, grumpkin_elements>) {
    if (c.nbytes == E::element_bytes) {
      typename F::fe c5 = F::zero();
      c5.v[0] = 1u << (F::LB * F::N - 256);
      v = F::mul(v, c5);
    }
  }
  F::to_words(key.w, F::canonical(v));
  return key;
}

// the key of 32 bytes in element form at any address (may be unreduced)
template <class E> BZ_HD lookup_key key_of_element(const void* element) {
  const column_view one{static_cast<const u8*>(element), 1, 32, kAccessBytes, 0, 0};
  return key_of<E>(one, 0);
}

// the key of the sum of two values given by their keys
template <class E> BZ_HD lookup_key key_sum(const lookup_key& a, const lookup_key& b) {
  using F = typename E::F;
  lookup_key sum;
  F::to_words(sum.w, F::canonical(fadd<F>(F::reduce(F::from_words(a.w)),
                                          F::reduce(F::from_words(b.w)))));
  return sum;
}
} // namespace bz::proof
