// The sumcheck transcript protocol of proof/sumcheck_transcript.hip (prfsk::reference_transcript<T>:
// the init, a round's append and challenge, r from the challenge bytes by field), apart from its
// kernels so that the test harness (tests/native/device_hooks.hip) can run the same text.
#pragma once

#include <cstring>

#include "blitzar_amd/csrc/proof/sumcheck_rows.h"
#include "blitzar_amd/csrc/proof/transcript.h"

namespace bz::proof {
//--------------------------------------------------------------------------------------------------
// the protocol, over the sponge of the host or of a wavefront
//--------------------------------------------------------------------------------------------------
// r from the 32 challenge bytes x: writes r in the caller's representation, returns it in engine form
template <class E> struct challenge;
template <> struct challenge<scalar25519_elements> {
  using F = scalar25_field;
  BZ_HD static F::fe make(u8* r_bytes, const u8* x) {
    const F::fe r = scalar25519_elements::load(x); // any 256-bit integer: V < 16 before the product
    scalar25519_elements::store(r_bytes, r);
    return r;
  }
};
template <> struct challenge<grumpkin_elements> {
  using F = grumpkin_fq29;
  BZ_HD static F::fe make(u8* r_bytes, const u8* x) {
    // load() takes x for Montgomery limbs (x < 2^256: V < 6 before the product): the value x / 2^256;
    // one more product takes the engine's R out and leaves that value as a plain integer
    F::fe plain_one = F::zero();
    plain_one.v[0] = 1;
    const F::fe y = F::mul(grumpkin_elements::load(x), plain_one);
    u64 w[4];
    F::to_words(w, F::canonical(y));
    std::memcpy(r_bytes, w, 32);
    return F::from_mont64(w);
  }
};

template <class Sponge> BZ_HD void transcript_begin(transcript_state* t, u64 num_variables, u64 degree) {
  transcript_over<Sponge> tr{t};
  tr.set_domain(label("sumcheck proof v1"));
  tr.append_u64(label("n"), num_variables);
  tr.append_u64(label("k"), degree);
}
// `x`: 32 bytes for the squeezed challenge (LDS for a wavefront)
template <class E, class Sponge>
BZ_HD typename E::F::fe transcript_round(u8* r_bytes, u8* x, transcript_state* t, const u8* polynomial,
                                         u32 length) {
  transcript_over<Sponge> tr{t};
  tr.append_message(label("P"), polynomial, static_cast<size_t>(32) * length);
  tr.challenge_bytes(x, 32, label("R"));
  return challenge<E>::make(r_bytes, x);
}
} // namespace bz::proof
