// The pieces of the inner-product protocol of proof/inner_product.hip that do not depend on its
// kernels: the joint fold digits and the shared double-and-add over them, and the transcript steps;
// apart so that the test harness (tests/native/device_hooks.hip) can run the same text.
#pragma once

#include "blitzar_amd/csrc/curve/ed29.h"
#include "blitzar_amd/csrc/proof/scalar25.h"
#include "blitzar_amd/csrc/proof/transcript.h"

namespace bz::proof {
constexpr u32 kScalarBits = 253; // s25cn::max_bits_v

// the joint bit pattern of (m_low, m_high), least significant first: digit = bit(m_low) +
// 2 bit(m_high); trailing zero digits dropped (generator_fold.cc:32-59)
struct fold_digits {
  u8 d[256];
  u32 count;
};

// what the challenge kernel leaves in the workspace for the folds of its round
struct fold_slot {
  s25::fe x, x_inv;   // Montgomery form
  fold_digits digits; // of (m_low, m_high) = (x^-1, x)
};

inline fold_digits decompose_fold(const u8 m_low[32], const u8 m_high[32]) {
  fold_digits r{};
  for (u32 bit = 0; bit < kScalarBits; ++bit) {
    const u32 lo = (m_low[bit >> 3] >> (bit & 7)) & 1, hi = (m_high[bit >> 3] >> (bit & 7)) & 1;
    r.d[bit] = static_cast<u8>(lo + 2 * hi);
  }
  r.count = kScalarBits;
  while (r.count > 0 && r.d[r.count - 1] == 0) --r.count;
  return r;
}

// m_low g_low + m_high g_high by one shared double-and-add over the joint digits
// (generator_fold.cc:64-90); `term(k)` yields g_low, g_high, g_low + g_high as cached addends
template <class Term> BZ_HD ed29_point fold_point(const fold_digits& digits, Term&& term) {
  ed29_point acc = ed29::identity();
  for (u32 bit = digits.count; bit-- > 0;) {
    const u32 d = digits.d[bit];
    // T is only needed by a following addition and by the caller (the last step)
    if (bit + 1 != digits.count) acc = ed29::dbl(acc, d != 0 || bit == 0);
    if (d != 0) acc = ed29::add_cached(acc, term(d - 1), false);
  }
  return acc;
}

//--------------------------------------------------------------------------------------------------
// the transcript of the protocol, over the sponge of the host or of a wavefront
// (proof_computation.cc:36-52); prover and verifier, host and device run this text
//--------------------------------------------------------------------------------------------------
template <class Sponge> BZ_HD void init_transcript(transcript_state* t, u64 n) {
  transcript_over<Sponge> tr{t};
  tr.set_domain(label("inner product proof v1"));
  tr.append_u64(label("n"), n);
}
// `x`: 32 bytes for the squeezed challenge (LDS for a wavefront); returns x mod l in Montgomery
// form (== s25o::reduce32: every later use is modulo l)
template <class Sponge>
BZ_HD s25::fe round_challenge(u8* x, transcript_state* t, const u8* l_value, const u8* r_value) {
  transcript_over<Sponge> tr{t};
  tr.append_message(label("L"), l_value, 32);
  tr.append_message(label("R"), r_value, 32);
  tr.challenge_bytes(x, 32, label("x"));
  return s25::to_mont(s25::load(x));
}
} // namespace bz::proof
