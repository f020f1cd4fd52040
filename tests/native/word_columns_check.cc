// Stand-alone check of the plain-C++ half of the word columns
// (blitzar_amd/csrc/proof/word_columns.h: key_byte, key_overflows, planes_extent, model_decompose,
// model_map) on buffers of exactly the size the calls may touch, so that a byte outside is the
// sanitizer's to find.  Built and run by tests/test_word_columns.py, plain and under the address /
// undefined-behaviour sanitizers; the test compares the two outputs with each other and with the
// Python model.  Lines:
//   extent <planes_extent at five shapes>
//   overflow_edges <w>=<overflows(2^(8 w) - 1)><overflows(2^(8 w))> ... (32: 2^256 - 1 and 2^255)
//   decompose num_words=<w> keys=<hex> words=<hex bytes, plane after plane> counts=<256 counts>
//     overflow=<count> gaps=kept|written
//   map planes=<count> ok|wrong
// keys in hex, most significant word first.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "blitzar_amd/csrc/proof/word_columns.h"

using namespace bz;
using namespace bz::proof;

namespace {
lookup_key power_of_two(u32 bit) {
  lookup_key key = {{0, 0, 0, 0}};
  key.w[bit / 64] = u64{1} << (bit % 64);
  return key;
}
lookup_key minus_one(lookup_key key) {
  for (u32 t = 0; t < 4; ++t) {
    if (key.w[t]-- != 0) break;
  }
  return key;
}

void run(u32 num_words, u64 gap, const std::vector<lookup_key>& keys) {
  const u64 n = keys.size(), stride = n + gap;
  // exactly the planes' extent, the gaps marked
  std::vector<u8> words(planes_extent(num_words, stride, n), 0xA5);
  std::vector<u64> counts(kWordValues, ~u64{0});
  u64 overflow = ~u64{0};
  model_decompose(words.data(), counts.data(), &overflow, n, num_words, stride,
                  [&](u64 i) { return keys[i]; });
  // every output null in turn: the others are the same
  std::vector<u8> words_only(words.size(), 0xA5);
  std::vector<u64> counts_only(kWordValues, ~u64{0});
  u64 overflow_only = ~u64{0};
  const auto key_at = [&](u64 i) { return keys[i]; };
  model_decompose(words_only.data(), static_cast<u64*>(nullptr), static_cast<u64*>(nullptr), n,
                  num_words, stride, key_at);
  model_decompose(static_cast<u8*>(nullptr), counts_only.data(), static_cast<u64*>(nullptr), n,
                  num_words, stride, key_at);
  model_decompose(static_cast<u8*>(nullptr), static_cast<u64*>(nullptr), &overflow_only, n,
                  num_words, stride, key_at);
  const bool same = words_only == words && counts_only == counts && overflow_only == overflow;
  std::printf("decompose num_words=%u keys=", num_words);
  for (u64 i = 0; i < n; ++i) {
    std::printf("%s%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64, i ? "," : "",
                keys[i].w[3], keys[i].w[2], keys[i].w[1], keys[i].w[0]);
  }
  std::printf(" words=");
  bool gaps_kept = true;
  for (u32 k = 0; k < num_words; ++k) {
    for (u64 i = 0; i < n; ++i) std::printf("%s%02x", k + i ? "," : "", words[k * stride + i]);
    // no rows: no planes, no gaps
    for (u64 i = n; n != 0 && i < stride && k + 1 < num_words; ++i) {
      gaps_kept &= words[k * stride + i] == 0xA5;
    }
  }
  std::printf(" counts=");
  for (u32 v = 0; v < kWordValues; ++v) std::printf("%s%" PRIu64, v ? "," : "", counts[v]);
  std::printf(" overflow=%" PRIu64 " gaps=%s\n", overflow, gaps_kept && same ? "kept" : "written");
}

void run_map(u32 planes, u64 n, u64 plane_gap, u64 mapped_gap) {
  const u64 plane_stride = n + plane_gap, mapped_stride = 32 * n + mapped_gap;
  std::vector<u8> words(planes_extent(planes, plane_stride, n));
  std::vector<u8> table(32 * kWordValues);
  std::vector<u8> mapped(planes_extent(planes, mapped_stride, n, 32), 0xA5);
  for (size_t i = 0; i < words.size(); ++i) words[i] = static_cast<u8>(i * 37 + 11);
  for (u32 v = 0; v < kWordValues; ++v) {
    for (u32 b = 0; b < 32; ++b) table[32 * v + b] = static_cast<u8>(v ^ (11 * b));
  }
  model_map(mapped.data(), word_map{words.data(), table.data(), planes, n, plane_stride,
                                    mapped_stride});
  bool ok = true;
  for (u32 k = 0; k < planes; ++k) {
    for (u64 i = 0; i < n; ++i) {
      const u8 word = words[k * plane_stride + i];
      for (u32 b = 0; b < 32; ++b) {
        ok &= mapped[k * mapped_stride + 32 * i + b] == static_cast<u8>(word ^ (11 * b));
      }
    }
    for (u64 g = 32 * n; g < mapped_stride && k + 1 < planes; ++g) {
      ok &= mapped[k * mapped_stride + g] == 0xA5;
    }
  }
  std::printf("map planes=%u %s\n", planes, ok ? "ok" : "wrong");
}
} // namespace

int main() {
  std::printf("extent %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
              planes_extent(0, 100, 10), planes_extent(4, 100, 0), planes_extent(1, 100, 10),
              planes_extent(2, 100, 16), planes_extent(3, 1024, 32, 32));
  std::printf("overflow_edges");
  for (u32 w = 1; w <= 31; ++w) {
    const lookup_key edge = power_of_two(8 * w);
    std::printf(" %u=%d%d", w, key_overflows(minus_one(edge), w) ? 1 : 0,
                key_overflows(edge, w) ? 1 : 0);
  }
  std::printf(" 32=%d%d\n", key_overflows(minus_one(lookup_key{{0, 0, 0, 0}}), 32) ? 1 : 0,
              key_overflows(power_of_two(255), 32) ? 1 : 0);

  const lookup_key wide = {{0x0807060504030201ull, 0x100F0E0D0C0B0A09ull, 0x1817161514131211ull,
                            0x201F1E1D1C1B1A19ull}};
  const lookup_key zero = {{0, 0, 0, 0}};
  const lookup_key ones = minus_one(zero);
  std::vector<lookup_key> mixed = {zero, wide, ones, power_of_two(8), minus_one(power_of_two(8)),
                                   power_of_two(64), minus_one(power_of_two(64)),
                                   power_of_two(248), minus_one(power_of_two(248)), wide};
  for (u32 num_words : {1u, 2u, 8u, 9u, 16u, 31u, 32u}) {
    run(num_words, 0, mixed);
    run(num_words, 5, mixed);
  }
  run(8, 3, {});                                  // no rows
  run(32, 0, std::vector<lookup_key>(7, wide));   // a constant column
  run(1, 9, {ones});
  run_map(1, 33, 0, 0);
  run_map(32, 19, 3, 8);
  return 0;
}
