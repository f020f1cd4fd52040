// Stand-alone host check of the tile digest (blitzar_amd/csrc/msm/tile_digest.h): the text the
// staged prepare kernel runs per wavefront, compiled for the host.  tests/test_caller_table_digest.py
// builds and runs it (once more with -fsanitize=address,undefined) and reads the lines it prints:
//   <stride> <check> <failures> <cases>
// Exit status 0 when every check of every stride has no failure.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "blitzar_amd/csrc/msm/tile_digest.h"

using namespace bz;

static bool same(tile_digest x, tile_digest y) { return x.a == y.a && x.b == y.b; }

int main() {
  int bad = 0;
  for (u32 stride : {160u, 104u, 72u}) {
    std::mt19937_64 rng(0x5eed0000 + stride);
    std::vector<u8> tile(64 * stride);
    for (u8& v : tile) v = static_cast<u8>(rng());
    const tile_digest base = digest_of_tile(tile.data(), 64, stride);

    // every single-bit flip, and each half of the digest on its own
    unsigned long flips = 0, flip_same = 0, half_same = 0;
    for (size_t byte = 0; byte < tile.size(); ++byte) {
      for (int bit = 0; bit < 8; ++bit) {
        tile[byte] ^= static_cast<u8>(1u << bit);
        const tile_digest d = digest_of_tile(tile.data(), 64, stride);
        tile[byte] ^= static_cast<u8>(1u << bit);
        flips += 1;
        flip_same += same(d, base) ? 1 : 0;
        half_same += (d.a == base.a || d.b == base.b) ? 1 : 0;
      }
    }
    std::printf("%u bit_flip %lu %lu\n", stride, flip_same, flips);
    std::printf("%u bit_flip_either_half %lu %lu\n", stride, half_same, flips);
    bad += flip_same != 0 || half_same != 0;

    // swapping two different 16-byte words: neighbours, the same lane one round apart (64 words),
    // first and last
    const u32 words = 64 * stride / 16;
    unsigned long swaps = 0, swap_same = 0;
    auto swap_words = [&](u32 i, u32 j) {
      u8 t[16];
      std::memcpy(t, &tile[16 * i], 16);
      std::memcpy(&tile[16 * i], &tile[16 * j], 16);
      std::memcpy(&tile[16 * j], t, 16);
    };
    auto try_swap = [&](u32 i, u32 j) {
      if (i == j || j >= words || std::memcmp(&tile[16 * i], &tile[16 * j], 16) == 0) return;
      swap_words(i, j);
      swaps += 1;
      swap_same += same(digest_of_tile(tile.data(), 64, stride), base) ? 1 : 0;
      swap_words(i, j);
    };
    for (u32 i = 0; i < words; ++i) {
      try_swap(i, i + 1);
      try_swap(i, i + 64);
      try_swap(i, words - 1 - i);
    }
    std::printf("%u word_swap %lu %lu\n", stride, swap_same, swaps);
    bad += swap_same != 0 || swaps == 0;

    // 63 rows against the same bytes padded to 64 rows (zeros, and a copy of row 62)
    std::vector<u8> padded(tile.begin(), tile.begin() + 63 * stride);
    padded.resize(64 * stride, 0);
    const tile_digest short_tile = digest_of_tile(tile.data(), 63, stride);
    unsigned long pad_same = same(short_tile, digest_of_tile(padded.data(), 64, stride)) ? 1 : 0;
    std::memcpy(&padded[63 * stride], &padded[62 * stride], stride);
    pad_same += same(short_tile, digest_of_tile(padded.data(), 64, stride)) ? 1 : 0;
    // (and the digest of 63 rows reads none of row 63)
    std::vector<u8> exact(tile.begin(), tile.begin() + 63 * stride);
    const unsigned long prefix_differs = same(short_tile, digest_of_tile(exact.data(), 63, stride)) ? 0 : 1;
    std::printf("%u partial_tile %lu 2\n", stride, pad_same);
    std::printf("%u partial_tile_reads_its_rows_only %lu 1\n", stride, prefix_differs);
    bad += pad_same != 0 || prefix_differs != 0;

    // the SAME bit changed in the words of two and of four lanes at once (the lane states are
    // combined by xor: equal differences would cancel): the top and the lowest bit of each half of a
    // word, in the lanes' last and first words, over fresh random tiles.  Neither the digest nor
    // either of its halves may come out equal (chance: cases x 2^-64).
    {
      const u32 rounds = words / 64; // full rounds: word r * 64 + lane belongs to `lane`
      unsigned long cases = 0, full_same = 0, half_same_multi = 0;
      std::vector<u8> t(64 * stride);
      for (int trial = 0; trial < 1500; ++trial) {
        for (u8& v : t) v = static_cast<u8>(rng());
        const tile_digest b0 = digest_of_tile(t.data(), 64, stride);
        for (u32 lanes : {2u, 4u}) {
          for (u32 round : {rounds - 1, 0u}) {
            for (u32 byte : {15u, 7u, 8u, 0u}) {
              const u8 mask = (byte == 15 || byte == 7) ? 0x80 : 0x01;
              const u32 l0 = static_cast<u32>(rng() % 64);
              auto flip = [&] {
                for (u32 k = 0; k < lanes; ++k) {
                  const u32 lane = (l0 + 1 + 13 * k) % 64; // distinct lanes (13 k mod 64, k < 4)
                  t[16 * (round * 64 + lane) + byte] ^= mask;
                }
              };
              flip();
              const tile_digest d = digest_of_tile(t.data(), 64, stride);
              flip();
              cases += 1;
              full_same += same(d, b0) ? 1 : 0;
              half_same_multi += (d.a == b0.a || d.b == b0.b) ? 1 : 0;
            }
          }
        }
      }
      std::printf("%u multi_lane_same_bit %lu %lu\n", stride, full_same, cases);
      std::printf("%u multi_lane_same_bit_either_half %lu %lu\n", stride, half_same_multi, cases);
      bad += full_same != 0 || half_same_multi != 0;
    }

    // the per-row digest: every single-bit flip of a row, each half on its own
    std::vector<u64> row(stride / 8);
    std::memcpy(row.data(), tile.data(), stride);
    const tile_digest row_base = digest_of_row(row.data(), stride, 0);
    unsigned long row_flips = 0, row_same = 0;
    for (size_t w = 0; w < row.size(); ++w) {
      for (int bit = 0; bit < 64; ++bit) {
        row[w] ^= u64{1} << bit;
        const tile_digest d = digest_of_row(row.data(), stride, 0);
        row[w] ^= u64{1} << bit;
        row_flips += 1;
        row_same += (d.a == row_base.a || d.b == row_base.b) ? 1 : 0;
      }
    }
    std::printf("%u row_bit_flip_either_half %lu %lu\n", stride, row_same, row_flips);
    bad += row_same != 0;
  }
  return bad == 0 ? 0 : 1;
}
