// Stand-alone check of the plain C++ half of blitzar_amd/csrc/proof/key_sums.h: the chunk split,
// the signed accumulation and the recombination into a wide two's-complement integer, against
// arithmetic of its own (a 320-bit two's-complement integer in 32-bit digits held in 64-bit words,
// one row added at a time).  tests/test_key_sums_host.py compiles it twice, plain and under the
// address / undefined-behaviour sanitizers, compares the two outputs with each other and checks the
// printed sums with Python integers.  Lines:
//   bounds signs=<8 bits> wide=<80 hex digits, two's complement> negative=<0|1> magnitude=<hex>
//   random case=<i> rows=<count> chunks=<c> wide=<hex> sum=<hex of the reference>
//   workspace <m>:<values>:<bytes> ...
// and a last line "ok"; any disagreement prints "MISMATCH ..." and the exit status is 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "blitzar_amd/csrc/proof/key_sums.h"

using namespace bz;
using namespace bz::proof;

namespace {
int failures = 0;

// a two's-complement integer of 320 bits, ten digits of 32 bits, least significant first
struct big {
  u64 d[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
void add(big& a, const big& b) {
  u64 carry = 0;
  for (int j = 0; j < 10; ++j) {
    const u64 s = a.d[j] + b.d[j] + carry;
    a.d[j] = s & 0xFFFFFFFFu;
    carry = s >> 32;
  }
}
big negated(const big& a) {
  big out, one;
  for (int j = 0; j < 10; ++j) out.d[j] = ~a.d[j] & 0xFFFFFFFFu;
  one.d[0] = 1;
  add(out, one);
  return out;
}
// a signed 64-bit word times 2^(32 k)
big shifted(i64 a, u32 k) {
  big out;
  const u64 bits = static_cast<u64>(a);
  const u64 sign = a < 0 ? 0xFFFFFFFFu : 0;
  for (u32 j = 0; j < 10; ++j) {
    out.d[j] = j < k ? 0 : j == k ? bits & 0xFFFFFFFFu : j == k + 1 ? bits >> 32 : sign;
  }
  return out;
}
// a row: a magnitude of four words with its sign
big row_value(const u64* magnitude, bool negative) {
  big out;
  for (int j = 0; j < 8; ++j) out.d[j] = (magnitude[j / 2] >> (32 * (j % 2))) & 0xFFFFFFFFu;
  return negative ? negated(out) : out;
}
big of_wide(const u64* wide) {
  big out;
  for (int j = 0; j < 10; ++j) out.d[j] = (wide[j / 2] >> (32 * (j % 2))) & 0xFFFFFFFFu;
  return out;
}
bool equal(const big& a, const big& b) { return std::memcmp(a.d, b.d, sizeof(a.d)) == 0; }
void print_hex(const char* label, const big& a) {
  std::printf(" %s=", label);
  for (int j = 9; j >= 0; --j) std::printf("%08" PRIx64, a.d[j]);
}
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("MISMATCH %s\n", what);
    ++failures;
  }
}

// every accumulator at +-(2^62 - 1), all 256 combinations of signs
void bounds() {
  const i64 most = (i64{1} << 62) - 1;
  for (u32 signs = 0; signs < 256; ++signs) {
    u64 acc[kMaxValueChunks], wide[kWideWords];
    big want;
    for (u32 k = 0; k < kMaxValueChunks; ++k) {
      const i64 a = (signs >> k) & 1 ? -most : most;
      acc[k] = static_cast<u64>(a);
      add(want, shifted(a, k));
    }
    recombine_chunks(wide, acc);
    expect(equal(of_wide(wide), want), "recombine at the bounds");
    std::printf("bounds signs=%02x", signs);
    print_hex("wide", of_wide(wide));
    const bool negative = wide_magnitude(wide);
    expect(negative == ((want.d[9] >> 31) != 0), "sign at the bounds");
    expect(equal(of_wide(wide), negative ? negated(want) : want), "magnitude at the bounds");
    std::printf(" negative=%d", negative ? 1 : 0);
    print_hex("magnitude", of_wide(wide));
    std::printf("\n");
  }
  // zero, and the least wide integer an accumulator set can give
  u64 acc[kMaxValueChunks] = {0, 0, 0, 0, 0, 0, 0, 0}, wide[kWideWords];
  recombine_chunks(wide, acc);
  expect(!wide_magnitude(wide) && equal(of_wide(wide), big{}), "zero");
}

// rows of one kind added one at a time: accumulate_row and the recombination against the sum of
// the rows as wide integers
void random_cases() {
  std::mt19937_64 rng(12345);
  const u32 widths[] = {1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 31, 32};
  u32 index = 0;
  for (const u32 width : widths) {
    for (const bool is_signed : {false, true}) {
      if (is_signed && width > 16) continue;
      const u32 chunks = value_chunks(width);
      const u32 rows = 1000 + 37 * width;
      u64 acc[kMaxValueChunks] = {0, 0, 0, 0, 0, 0, 0, 0}, wide[kWideWords];
      big want;
      for (u32 i = 0; i < rows; ++i) {
        u64 magnitude[4] = {rng(), rng(), rng(), rng()};
        // cut to the width; every eighth row the largest magnitude the kind holds
        for (u32 b = 0; b < 32; ++b) {
          if (b >= width) magnitude[b / 8] &= ~(u64{0xFF} << (8 * (b % 8)));
        }
        bool negative = is_signed && (rng() & 1) != 0;
        if (is_signed) magnitude[(width - 1) / 8] &= ~(u64{0x80} << (8 * ((width - 1) % 8)));
        if (i % 8 == 0) {
          for (u32 b = 0; b < width; ++b) magnitude[b / 8] |= u64{0xFF} << (8 * (b % 8));
          if (is_signed) {
            // |minimum| = 2^(8 width - 1)
            for (u32 w = 0; w < 4; ++w) magnitude[w] = 0;
            magnitude[(width - 1) / 8] = u64{0x80} << (8 * ((width - 1) % 8));
            negative = true;
          }
        }
        for (u32 k = 0; k < kMaxValueChunks; ++k) {
          expect(k < chunks || chunk_of(magnitude, k) == 0, "a chunk past the width");
        }
        accumulate_row(acc, magnitude, negative, chunks);
        add(want, row_value(magnitude, negative));
      }
      recombine_chunks(wide, acc);
      expect(equal(of_wide(wide), want), "recombine of random rows");
      std::printf("random case=%u rows=%u chunks=%u", index++, rows, chunks);
      print_hex("wide", of_wide(wide));
      print_hex("sum", want);
      std::printf("\n");
      const bool negative = wide_magnitude(wide);
      expect(equal(of_wide(wide), negative ? negated(want) : want), "magnitude of random rows");
    }
  }
  // positive and negative rows that cancel
  u64 acc[kMaxValueChunks] = {0, 0, 0, 0, 0, 0, 0, 0}, wide[kWideWords];
  const u64 magnitude[4] = {~u64{0}, ~u64{0}, ~u64{0}, ~u64{0}};
  for (u32 i = 0; i < 100; ++i) accumulate_row(acc, magnitude, i % 2 != 0, 8);
  for (u32 k = 0; k < kMaxValueChunks; ++k) expect(acc[k] == 0, "cancelled accumulators");
  recombine_chunks(wide, acc);
  expect(!wide_magnitude(wide) && equal(of_wide(wide), big{}), "cancelled rows");
}

void workspace() {
  std::printf("workspace");
  const u64 rows[] = {0, 1, 2, 3, 64, 65, u64{1} << 28, (u64{1} << 28) + 1};
  for (const u64 m : rows) {
    for (const u32 values : {0u, 1u, 8u, 9u}) {
      std::printf(" %" PRIu64 ":%u:%" PRIu64, m, values, key_sum_workspace_bytes(m, values));
    }
  }
  std::printf("\n");
}
} // namespace

int main() {
  bounds();
  random_cases();
  workspace();
  std::puts(failures == 0 ? "ok" : "failed");
  return failures == 0 ? 0 : 1;
}
