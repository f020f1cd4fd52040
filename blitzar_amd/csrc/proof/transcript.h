// Merlin transcripts over STROBE-128 / Keccak-f[1600], operating in place on the caller's
// 203-byte `sxt_transcript` (cbindings/blitzar_api.h:61-63 = prft::transcript: the 200-byte
// sponge state followed by pos, pos_begin, cur_flags; sxt/proof/transcript/strobe128.h:41-45).
// Behaviour restated from the reference (sxt/proof/transcript/strobe128.cc, transcript.cc,
// transcript_utility.h, themselves ports of libmerlin): the byte-for-byte state after every
// operation is observable by the caller, who continues the same transcript after the proof.
//
// The strobe and merlin logic is written once over a `Sponge` policy that says how bytes get into
// and out of the 200-byte state and how it is permuted: host_sponge runs on one host thread;
// wave_sponge (device code only, below) keeps the state in LDS and is executed by all 64 lanes of
// one wavefront in lockstep -- positions and lengths are the same in every lane, byte ranges are
// spread over the lanes, and Keccak-f[1600] holds one 64-bit Keccak lane per SIMD lane.
#pragma once

#include <cstdint>
#include <cstring>
#include <string_view>

#include "blitzar_amd/csrc/base/macros.h"

namespace bz::proof {

// Keccak-f[1600] on 25 little-endian 64-bit lanes (FIPS 202, section 3.3), lane (x, y) at a[x + 5 y]
inline void keccak_f1600(u64 a[25]) {
  static constexpr u64 round_constant[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
      0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
      0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // rotation offsets r[x][y] (FIPS 202 table 2)
  static constexpr unsigned rotation[5][5] = {{0, 36, 3, 41, 18},
                                              {1, 44, 10, 45, 2},
                                              {62, 6, 43, 15, 61},
                                              {28, 55, 25, 21, 56},
                                              {27, 20, 39, 8, 14}};
  auto rotl = [](u64 v, unsigned s) { return s == 0 ? v : (v << s) | (v >> (64 - s)); };
  for (int round = 0; round < 24; ++round) {
    // theta
    u64 parity[5];
    for (int x = 0; x < 5; ++x) {
      parity[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
    }
    for (int x = 0; x < 5; ++x) {
      const u64 d = parity[(x + 4) % 5] ^ rotl(parity[(x + 1) % 5], 1);
      for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
    }
    // rho and pi: b[y][2x + 3y] = rot(a[x][y], r[x][y])
    u64 b[25];
    for (int x = 0; x < 5; ++x) {
      for (int y = 0; y < 5; ++y) {
        b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], rotation[x][y]);
      }
    }
    // chi
    for (int y = 0; y < 5; ++y) {
      for (int x = 0; x < 5; ++x) {
        a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
      }
    }
    // iota
    a[0] ^= round_constant[round];
  }
}

// the caller's transcript, viewed in place
struct transcript_state {
  u8 state[200];
  u8 pos;
  u8 pos_begin;
  u8 cur_flags;
};
static_assert(sizeof(transcript_state) == 203);

// byte sources of an absorb: memory, or the little-endian bytes of an integer (no address of a
// local is taken: in a kernel that would be scratch memory)
struct memory_bytes {
  const u8* p;
  BZ_HD u8 operator()(u32 i) const { return p[i]; }
};
struct integer_bytes {
  u64 v;
  BZ_HD u8 operator()(u32 i) const { return static_cast<u8>(v >> (8 * i)); }
};

// one host thread on the caller's bytes
struct host_sponge {
  static void permute(u8* state) {
    u64 lanes[25];
    std::memcpy(lanes, state, 200); // little-endian host (the ABI is little-endian throughout)
    keccak_f1600(lanes);
    std::memcpy(state, lanes, 200);
  }
  static void zero(u8* state) { std::memset(state, 0, 200); }
  static void xor_byte(u8* state, u32 at, u8 v) { state[at] ^= v; }
  template <class Source>
  static void absorb(u8* state, u32 pos, const Source& source, u32 offset, u32 n) {
    for (u32 i = 0; i < n; ++i) state[pos + i] ^= source(offset + i);
  }
  static void squeeze(u8* out, u8* state, u32 pos, u32 n) {
    for (u32 i = 0; i < n; ++i) {
      out[i] = state[pos + i];
      state[pos + i] = 0;
    }
  }
  static void store_tail(transcript_state* s, u32 pos, u32 pos_begin, u32 cur_flags) {
    s->pos = static_cast<u8>(pos);
    s->pos_begin = static_cast<u8>(pos_begin);
    s->cur_flags = static_cast<u8>(cur_flags);
  }
};

#if defined(__HIPCC__)
// One wavefront, state in LDS (8-byte aligned).  Every function is called by all 64 lanes with the
// same arguments; whatever one lane wrote is visible to the others when the function returns.
struct wave_sponge {
  BZ_DEV static u32 lane() { return threadIdx.x & 63u; }
  // LDS operations of one wavefront execute in order; the fence keeps the compiler from moving
  // them and waits for the outstanding ones
  BZ_DEV static void sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

  // Keccak-f[1600], lane-spread: SIMD lane l < 25 holds Keccak lane (x, y) = (l % 5, l / 5); the
  // column parities of theta, the source of rho / pi and the row neighbours of chi come through
  // __shfl, rho is a rotation by a per-lane constant, iota goes to lane 0.  Lanes 25 .. 63 run
  // along on in-range indices and are discarded.
  BZ_DEV static void permute(u8* state) {
    static constexpr u64 round_constant[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
        0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
        0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
        0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
        0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    // rotation offsets by Keccak lane index x + 5 y (FIPS 202 table 2)
    static constexpr u32 rotation[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                         25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
    const u32 l = lane() < 25 ? lane() : 0;
    const u32 x = l % 5, y = l / 5;
    const int up5 = static_cast<int>((l + 5) % 25), up10 = static_cast<int>((l + 10) % 25),
              up15 = static_cast<int>((l + 15) % 25), up20 = static_cast<int>((l + 20) % 25);
    const int left = static_cast<int>((x + 4) % 5 + 5 * y);
    const int right = static_cast<int>((x + 1) % 5 + 5 * y);
    const int right2 = static_cast<int>((x + 2) % 5 + 5 * y);
    // pi: b[x'][y'] = rot(a[x][y]) with x' = y, y' = 2 x + 3 y, so x = x' + 3 y', y = x'
    const u32 source = (x + 3 * y) % 5 + 5 * x;
    const u32 turn = rotation[source];
    sync();
    u64 a = reinterpret_cast<const u64*>(state)[l];
    for (int round = 0; round < 24; ++round) {
      // theta
      const u64 parity = a ^ shuffle(a, up5) ^ shuffle(a, up10) ^ shuffle(a, up15) ^ shuffle(a, up20);
      const u64 next = shuffle(parity, right);
      a ^= shuffle(parity, left) ^ ((next << 1) | (next >> 63));
      // rho and pi
      const u64 moved = shuffle(a, static_cast<int>(source));
      const u64 b = (moved << turn) | (moved >> ((64 - turn) & 63));
      // chi
      a = b ^ (~shuffle(b, right) & shuffle(b, right2));
      // iota
      if (l == 0) a ^= round_constant[round];
    }
    if (lane() < 25) reinterpret_cast<u64*>(state)[l] = a;
    sync();
  }
  BZ_DEV static u64 shuffle(u64 v, int from) {
    const u32 lo = static_cast<u32>(__shfl(static_cast<int>(static_cast<u32>(v)), from));
    const u32 hi = static_cast<u32>(__shfl(static_cast<int>(static_cast<u32>(v >> 32)), from));
    return (static_cast<u64>(hi) << 32) | lo;
  }
  BZ_DEV static void zero(u8* state) {
    for (u32 i = lane(); i < 200; i += 64) state[i] = 0;
    sync();
  }
  BZ_DEV static void xor_byte(u8* state, u32 at, u8 v) {
    if (lane() == 0) state[at] ^= v;
    sync();
  }
  template <class Source>
  BZ_DEV static void absorb(u8* state, u32 pos, const Source& source, u32 offset, u32 n) {
    for (u32 i = lane(); i < n; i += 64) state[pos + i] ^= source(offset + i);
    sync();
  }
  BZ_DEV static void squeeze(u8* out, u8* state, u32 pos, u32 n) {
    for (u32 i = lane(); i < n; i += 64) {
      out[i] = state[pos + i];
      state[pos + i] = 0;
    }
    sync();
  }
  BZ_DEV static void store_tail(transcript_state* s, u32 pos, u32 pos_begin, u32 cur_flags) {
    if (lane() == 0) {
      s->pos = static_cast<u8>(pos);
      s->pos_begin = static_cast<u8>(pos_begin);
      s->cur_flags = static_cast<u8>(cur_flags);
    }
    sync();
  }
};

// the caller's 203 bytes into / out of the LDS copy wavefront 0 works on
BZ_DEV void wave_load_transcript(transcript_state& lds, const u8* transcript) {
  u8* t = reinterpret_cast<u8*>(&lds);
  for (u32 i = wave_sponge::lane(); i < sizeof(transcript_state); i += 64) t[i] = transcript[i];
  wave_sponge::sync();
}
BZ_DEV void wave_store_transcript(u8* transcript, const transcript_state& lds) {
  const u8* t = reinterpret_cast<const u8*>(&lds);
  for (u32 i = wave_sponge::lane(); i < sizeof(transcript_state); i += 64) transcript[i] = t[i];
}
#endif

// a label: characters and their number (device code has no std::string_view)
struct label_view {
  const char* p;
  u32 n;
  BZ_HD u8 operator()(u32 i) const { return static_cast<u8>(p[i]); }
};
// the length of a literal, without its terminator
template <u32 M> BZ_HD constexpr label_view label(const char (&text)[M]) { return {text, M - 1}; }

template <class Sponge> class strobe128_over {
public:
  static constexpr u32 kRate = 166; // STROBE-128: 200 - 2 * 128 / 8 - 2
  static constexpr u32 kFlagI = 1, kFlagA = 2, kFlagC = 4, kFlagT = 8, kFlagM = 16, kFlagK = 32;

  BZ_HD explicit strobe128_over(transcript_state* s)
      : s_{s}, pos_{s->pos}, pos_begin_{s->pos_begin}, cur_flags_{s->cur_flags} {}

  // a fresh STROBE-128 state with the given protocol label (strobe128.cc:70-73; the initial block
  // is [1, R + 2, 1, 0, 1, 96] || "STROBEv1.0.2", strobe128.h:41-42)
  BZ_HD static void init(transcript_state* s, const label_view& protocol) {
    Sponge::zero(s->state);
    // [1, 168, 1, 0, 1, 96, 'S', 'T'], "ROBEv1.0", ".2"
    Sponge::absorb(s->state, 0, integer_bytes{0x5453'6001'0001'a801ull}, 0, 8);
    Sponge::absorb(s->state, 8, integer_bytes{0x302e'3176'4542'4f52ull}, 0, 8);
    Sponge::absorb(s->state, 16, integer_bytes{0x322eull}, 0, 2);
    Sponge::store_tail(s, 0, 0, 0);
    Sponge::permute(s->state);
    strobe128_over st{s};
    st.meta_ad(protocol, protocol.n, false);
  }

  template <class Source> BZ_HD void meta_ad(const Source& data, u32 n, bool more) {
    begin_op(kFlagM | kFlagA, more);
    absorb(data, n);
    Sponge::store_tail(s_, pos_, pos_begin_, cur_flags_);
  }
  template <class Source> BZ_HD void ad(const Source& data, u32 n, bool more) {
    begin_op(kFlagA, more);
    absorb(data, n);
    Sponge::store_tail(s_, pos_, pos_begin_, cur_flags_);
  }
  BZ_HD void prf(u8* out, u32 n, bool more) {
    begin_op(kFlagI | kFlagA | kFlagC, more);
    squeeze(out, n);
    Sponge::store_tail(s_, pos_, pos_begin_, cur_flags_);
  }

private:
  transcript_state* s_;
  u32 pos_, pos_begin_, cur_flags_; // the same in every lane of a wave_sponge

  // strobe128.cc:112-124
  BZ_HD void run_f() {
    Sponge::xor_byte(s_->state, pos_, static_cast<u8>(pos_begin_));
    Sponge::xor_byte(s_->state, pos_ + 1, 0x04);
    Sponge::xor_byte(s_->state, kRate + 1, 0x80);
    Sponge::permute(s_->state);
    pos_ = 0;
    pos_begin_ = 0;
  }
  // byte by byte in the reference; here in runs up to the rate boundary
  template <class Source> BZ_HD void absorb(const Source& data, u32 n) {
    for (u32 done = 0; done < n;) {
      const u32 run = n - done < kRate - pos_ ? n - done : kRate - pos_;
      Sponge::absorb(s_->state, pos_, data, done, run);
      done += run;
      pos_ += run;
      if (pos_ == kRate) run_f();
    }
  }
  BZ_HD void squeeze(u8* out, u32 n) {
    for (u32 done = 0; done < n;) {
      const u32 run = n - done < kRate - pos_ ? n - done : kRate - pos_;
      Sponge::squeeze(out + done, s_->state, pos_, run);
      done += run;
      pos_ += run;
      if (pos_ == kRate) run_f();
    }
  }
  // strobe128.cc:142-166
  BZ_HD void begin_op(u32 flags, bool more) {
    if (more) return; // continuing the previous operation
    const u32 old_begin = pos_begin_;
    pos_begin_ = (pos_ + 1) & 0xff;
    cur_flags_ = flags;
    absorb(integer_bytes{old_begin | (flags << 8)}, 2);
    if ((flags & (kFlagC | kFlagK)) != 0 && pos_ != 0) run_f();
  }
};
using strobe128 = strobe128_over<host_sponge>;

// Merlin (transcript.cc:48-88, transcript_utility.h)
template <class Sponge> class transcript_over {
public:
  BZ_HD explicit transcript_over(void* caller_bytes)
      : s_{static_cast<transcript_state*>(caller_bytes)} {}

  // prft::transcript{label}: what an API consumer constructs before calling the prover
  static void init(void* caller_bytes, std::string_view name) {
    auto* s = static_cast<transcript_state*>(caller_bytes);
    strobe128_over<Sponge>::init(s, label("Merlin v1.0"));
    transcript_over t{caller_bytes};
    t.append_message(label("dom-sep"), reinterpret_cast<const u8*>(name.data()), name.size());
  }

  BZ_HD void append_message(const label_view& name, const u8* message, size_t n) {
    append_bytes(name, memory_bytes{message}, static_cast<u32>(n));
  }
  BZ_HD void challenge_bytes(u8* dest, size_t n, const label_view& name) {
    strobe128_over<Sponge> st{s_};
    st.meta_ad(name, name.n, false);
    st.meta_ad(integer_bytes{static_cast<u32>(n)}, 4, true);
    st.prf(dest, static_cast<u32>(n), false);
  }
  BZ_HD void set_domain(const label_view& name) {
    append_bytes(label("domain-sep"), name, name.n);
  }
  BZ_HD void append_u64(const label_view& name, u64 v) { append_bytes(name, integer_bytes{v}, 8); }

  // the string_view forms of the host callers
  void append_message(std::string_view name, const u8* message, size_t n) {
    append_message(view(name), message, n);
  }
  void challenge_bytes(u8* dest, size_t n, std::string_view name) {
    challenge_bytes(dest, n, view(name));
  }
  void set_domain(std::string_view name) { set_domain(view(name)); }
  void append_u64(std::string_view name, u64 v) { append_u64(view(name), v); }

private:
  transcript_state* s_;

  static label_view view(std::string_view name) {
    return {name.data(), static_cast<u32>(name.size())};
  }
  template <class Source>
  BZ_HD void append_bytes(const label_view& name, const Source& message, u32 n) {
    strobe128_over<Sponge> st{s_};
    st.meta_ad(name, name.n, false);
    st.meta_ad(integer_bytes{n}, 4, true);
    st.ad(message, n, false);
  }
};
using transcript = transcript_over<host_sponge>;
} // namespace bz::proof
