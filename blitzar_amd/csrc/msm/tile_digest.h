// 128-bit digest of one tile of caller generators (64 rows of the C-ABI layout, the piece one
// wavefront of k_prepare_addends_staged stages).  The kernel compares it with the digest it stored
// when it last converted the tile and converts again only when they differ (engine.h, caller_slot).
// One text for the device and the host (tests run the host form): integer multiply / xor-shift only.
// Not a cryptographic hash: it guards against generators rewritten in place, not against an
// adversary who constructs colliding tiles.
//
// The state is 128 bits, (a, b), and `digest_permute` is a bijection of it: three multiply /
// xor-shift steps, each folding one half into the other, so both halves depend on both afterwards.
//   * Lane l of the wavefront absorbs the 16-byte words l, l + 64, l + 128, ... of the tile, in that
//     order: a word is xor-ed into the whole state (its index into `a`) and the state is permuted.
//     When the tile's byte count is 8 (mod 16) -- generator strides of 8 (mod 16) and an odd row
//     count -- lane 0 absorbs the last 8 bytes as one more word with a zero upper half.
//   * Every lane then FINISHES its state (two more permutations) before the lanes are combined by
//     xor: without that, the difference a changed last word leaves in a lane is a fixed bit pattern
//     for some bits, and the same change in two lanes cancels in the xor.  After it, differences in
//     several lanes meet as unrelated 128-bit values.
//   * The xor of the lanes is finished once more with the tile's row count.
// What is shown (tests/native/tile_digest_check.cc): a word enters by xor into a state that only
// goes through bijections until the lanes are combined, so two tiles that differ in ONE 16-byte word
// (or in words of one lane whose states do not collide) have different 128-bit digests -- a single
// half may well agree; tiles that differ in several lanes are told apart with the probability of a
// 128-bit mixing function, which the host checks probe with the same bit changed in the words of
// two and four lanes.
#pragma once

#include "blitzar_amd/csrc/base/macros.h"

namespace bz {

struct tile_digest {
  u64 a, b;
};

constexpr u64 kDigestMul0 = 0x9e3779b97f4a7c15ull, kDigestMul1 = 0xbf58476d1ce4e5b9ull;
constexpr u64 kDigestMul2 = 0x94d049bb133111ebull;

// a bijection of the 128-bit state (every step is invertible given the half it leaves alone)
BZ_HD tile_digest digest_permute(tile_digest s) {
  s.a *= kDigestMul0;
  s.a ^= s.a >> 32;
  s.b = (s.b + s.a) * kDigestMul1;
  s.b ^= s.b >> 29;
  s.a = (s.a + s.b) * kDigestMul2;
  s.a ^= s.a >> 32;
  return s;
}
// a lane's state before its first word
BZ_HD tile_digest digest_lane_begin(u32 lane, u32 count) {
  return digest_permute({0x243f6a8885a308d3ull ^ lane, 0x13198a2e03707344ull ^ count});
}
// word `index` of the tile = bytes [16 index, 16 index + 16): `lo` the first eight, `hi` the rest
BZ_HD tile_digest digest_absorb(tile_digest s, u32 index, u64 lo, u64 hi) {
  return digest_permute({s.a ^ lo ^ (static_cast<u64>(index) + 1) << 32, s.b ^ hi});
}
// a lane's state after its last word, as it enters the xor of the lanes
BZ_HD tile_digest digest_lane_end(tile_digest s) { return digest_permute(digest_permute(s)); }
// `x` = the xor of the 64 finished lane states
BZ_HD tile_digest digest_finish(tile_digest x, u32 count) {
  return digest_permute(digest_permute({x.a ^ count, x.b}));
}

// Digest of ONE row (`row_bytes` a multiple of 8; `row` = its 64-bit words), taken by the row's lane
// when the tile's digest does not settle the matter.  The same chain over the row's own words.
BZ_HD tile_digest digest_of_row(const u64* row, u32 row_bytes, u32 row_in_tile) {
  tile_digest s = digest_lane_begin(row_in_tile, row_bytes);
  const u32 words = row_bytes / 16;
  for (u32 k = 0; k < words; ++k) s = digest_absorb(s, k, row[2 * k], row[2 * k + 1]);
  if ((row_bytes & 8) != 0) s = digest_absorb(s, words, row[2 * words], 0);
  return digest_finish(digest_lane_end(s), row_bytes);
}

// The host form: what the wavefront computes for `count` rows of `row_bytes` bytes each
// (64 * row_bytes a multiple of 16, row_bytes a multiple of 8).
inline tile_digest digest_of_tile(const u8* tile, u32 count, u32 row_bytes) {
  const u32 bytes = count * row_bytes;
  auto word = [&](u32 off) { // little-endian, like the device's loads
    u64 v;
    __builtin_memcpy(&v, tile + off, 8);
    return v;
  };
  tile_digest x{0, 0};
  for (u32 lane = 0; lane < 64; ++lane) {
    tile_digest s = digest_lane_begin(lane, count);
    for (u32 off = lane * 16; off + 16 <= bytes; off += 64 * 16) {
      s = digest_absorb(s, off / 16, word(off), word(off + 8));
    }
    if ((bytes & 8) != 0 && lane == 0) s = digest_absorb(s, bytes / 16, word(bytes - 8), 0);
    s = digest_lane_end(s);
    x.a ^= s.a;
    x.b ^= s.b;
  }
  return digest_finish(x, count);
}

} // namespace bz
