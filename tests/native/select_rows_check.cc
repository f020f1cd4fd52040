// Stand-alone check of the plain C++ half of blitzar_amd/csrc/proof/select_rows.h: the span
// partition, the rank of a lane from a wavefront's four ballots and the workspace size, and a
// sequential model of the two launches (count per span -> bases -> scatter tile by tile, wavefront
// by wavefront) built from them, against a plain loop.  tests/test_select_rows_host.py compiles it
// twice, plain and under the address / undefined-behaviour sanitizers, and compares the two
// outputs.  Lines:
//   partition n=<n> spans=<s> tiles_per_span=<t>
//   model n=<n> width=<w> kept=<count> invert=<0|1>
//   ranks masks=<count>
//   workspace <n>:<bytes> ...
// and a last line "ok"; any disagreement prints "MISMATCH ..." and the exit status is 1.
#include <cinttypes>
#include <cstdio>
#include <random>
#include <vector>

#include "blitzar_amd/csrc/proof/select_rows.h"

using namespace bz;
using namespace bz::proof;

namespace {
int failures = 0;

void mismatch(const char* what, u64 a, u64 b) {
  std::printf("MISMATCH %s %" PRIu64 " %" PRIu64 "\n", what, a, b);
  ++failures;
}

// the spans cover [0, n) exactly once, in order, each a whole number of tiles except the last
void check_partition(u64 n, bool print) {
  const span_partition p = partition_rows(n);
  if (p.spans < 1 || p.spans > kMaxSelectSpans || p.tiles_per_span < 1) mismatch("spans", n, p.spans);
  u64 at = 0;
  for (u32 g = 0; g < p.spans; ++g) {
    const u64 first = span_first_row(p, n, g), end = span_first_row(p, n, g + 1);
    if (first != at || end < first) mismatch("span order", n, g);
    if (g + 1 < p.spans &&
        (end == first || (end - first) != u64{p.tiles_per_span} * kSelectTileRows)) {
      mismatch("span tiles", n, g);
    }
    if (n != 0 && end == first) mismatch("empty span", n, g);
    if (end - first > u64{p.tiles_per_span} * kSelectTileRows) mismatch("span rows", n, g);
    at = end;
  }
  if (at != n) mismatch("cover", n, at);
  if (print) {
    std::printf("partition n=%" PRIu64 " spans=%u tiles_per_span=%u\n", n, p.spans,
                p.tiles_per_span);
  }
}

// count -> bases -> scatter as the kernels do it, one step after the other: ranks[i] for kept rows
std::vector<u64> model_ranks(const std::vector<u8>& selector, u32 width, u64 reject, bool invert,
                             u64* count) {
  const u64 n = selector.size() / width;
  const span_partition p = partition_rows(n);
  const auto kept = [&](u64 i) {
    return i < n && row_kept(selector_bits(selector.data() + i * width, width), reject, invert);
  };
  // launch 1
  std::vector<u32> span_counts(p.spans, 0);
  for (u32 g = 0; g < p.spans; ++g) {
    for (u64 i = span_first_row(p, n, g); i < span_first_row(p, n, g + 1); ++i) {
      span_counts[g] += kept(i) ? 1 : 0;
    }
  }
  // launch 2
  std::vector<u64> ranks(n, ~u64{0});
  u64 total = 0;
  for (u32 g = 0; g < p.spans; ++g) total += span_counts[g];
  for (u32 g = 0; g < p.spans; ++g) {
    u64 base = 0;
    for (u32 q = 0; q < g; ++q) base += span_counts[q];
    const u64 end = span_first_row(p, n, g + 1);
    for (u64 tile = span_first_row(p, n, g); tile < end; tile += kSelectTileRows) {
      u64 ballots[kSelectWaves][kSelectRounds];
      u32 totals[kSelectWaves];
      for (u32 wave = 0; wave < kSelectWaves; ++wave) {
        for (u32 r = 0; r < kSelectRounds; ++r) {
          ballots[wave][r] = 0;
          for (u32 lane = 0; lane < kSelectLanes; ++lane) {
            const u64 i = tile + wave * kSelectWaveRows + r * kSelectLanes + lane;
            if (i < end && kept(i)) ballots[wave][r] |= u64{1} << lane;
          }
        }
        totals[wave] = ballot_total(ballots[wave]);
      }
      u32 lower = 0;
      for (u32 wave = 0; wave < kSelectWaves; ++wave) {
        for (u32 r = 0; r < kSelectRounds; ++r) {
          for (u32 lane = 0; lane < kSelectLanes; ++lane) {
            if (((ballots[wave][r] >> lane) & 1) == 0) continue;
            const u64 i = tile + wave * kSelectWaveRows + r * kSelectLanes + lane;
            ranks[i] = base + lower + ballot_rank(ballots[wave], r, lane);
          }
        }
        lower += totals[wave];
      }
      base += lower;
    }
  }
  *count = total;
  return ranks;
}

void check_model(std::mt19937_64& rng, u64 n, u32 width, u32 keep_of_256, bool invert) {
  std::vector<u8> selector(n * width);
  const u64 reject = width == 8 ? ~u64{0} : (u64{1} << (8 * width)) - 1;
  for (u64 i = 0; i < n; ++i) {
    const bool keep = (rng() & 255) < keep_of_256;
    for (u32 k = 0; k < width; ++k) {
      selector[i * width + k] = keep != invert ? static_cast<u8>(k == 0 ? rng() & 0x7F : rng()) : 0xFF;
    }
  }
  u64 count = 0;
  const std::vector<u64> ranks = model_ranks(selector, width, reject, invert, &count);
  u64 plain = 0;
  for (u64 i = 0; i < n; ++i) {
    const bool kept = row_kept(selector_bits(selector.data() + i * width, width), reject, invert);
    if (ranks[i] != (kept ? plain : ~u64{0})) mismatch("rank", n, i);
    plain += kept ? 1 : 0;
  }
  if (plain != count) mismatch("count", plain, count);
  std::printf("model n=%" PRIu64 " width=%u kept=%" PRIu64 " invert=%d\n", n, width, count,
              invert ? 1 : 0);
}

void check_ranks(std::mt19937_64& rng) {
  std::vector<u64> masks = {0, ~u64{0}, 1, u64{1} << 63, 0x5555555555555555ull,
                            0xAAAAAAAAAAAAAAAAull, 0xFFFFFFFFull, 0xFFFFFFFF00000000ull};
  for (int k = 0; k < 256; ++k) masks.push_back(rng() & (k % 3 == 0 ? rng() : ~u64{0}));
  u64 checked = 0;
  for (size_t m = 0; m + kSelectRounds <= masks.size(); ++m) {
    const u64* ballots = masks.data() + m;
    u32 plain = 0;
    for (u32 r = 0; r < kSelectRounds; ++r) {
      for (u32 lane = 0; lane < kSelectLanes; ++lane) {
        if (ballot_rank(ballots, r, lane) != plain) mismatch("ballot rank", m, 64 * r + lane);
        plain += static_cast<u32>((ballots[r] >> lane) & 1);
      }
    }
    if (ballot_total(ballots) != plain) mismatch("ballot total", m, plain);
    ++checked;
  }
  std::printf("ranks masks=%" PRIu64 "\n", checked);
}
} // namespace

int main() {
  std::mt19937_64 rng(20261021);
  const u64 tile = kSelectTileRows;
  for (u64 n = 0; n <= 3 * tile + 1; ++n) check_partition(n, n % tile <= 1 || n % tile == tile - 1);
  for (u64 k = 1; k <= 2; ++k) {
    for (u64 n = k * tile * kMaxSelectSpans - 1; n <= k * tile * kMaxSelectSpans + 1; ++n) {
      check_partition(n, true);
    }
  }
  check_partition(kMaxSelectRows, true);

  const u64 sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 7};
  u32 width = 1;
  for (const u64 n : sizes) {
    for (const u32 keep : {0u, 4u, 128u, 252u, 256u}) {
      check_model(rng, n, width, keep, (n + keep) % 3 == 0);
      width = width % 8 + 1;
    }
  }
  // more than one tile a span, and the last span short
  check_model(rng, 2 * tile * kMaxSelectSpans + 1, 1, 128, false);
  check_model(rng, tile * kMaxSelectSpans + 1, 2, 200, true);

  check_ranks(rng);

  std::printf("workspace");
  for (const u64 n : {u64{0}, u64{1}, tile, tile + 1, tile * kMaxSelectSpans,
                      tile * kMaxSelectSpans + 1, 3 * tile * kMaxSelectSpans + 5, kMaxSelectRows,
                      kMaxSelectRows + 1, ~u64{0}}) {
    std::printf(" %" PRIu64 ":%" PRIu64, n, select_rows_workspace_bytes(n));
  }
  std::printf("\n");
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
