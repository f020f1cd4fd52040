// Selection of rows of typed columns (proof/select_rows.hip, bzamd_select_rows*, bzamd_take_rows*):
// the stable compaction of up to 16 columns by a selector column, with the kept rows' indices and
// their number, and the gather of rows by index.  Both copy rows at their own width and do no field
// arithmetic.  The definitions are those above bzamd_select_rows in include/blitzar_amd.h.
//
// The first half of this file is plain C++ that g++ compiles without HIP: which rows a selector
// keeps, how the rows are cut into spans of whole tiles (one workgroup each), the rank of a lane
// among the kept rows of its wavefront's part of a tile, and the workspace size.  The kernels, the
// cpu backend and the stand-alone check tests/native/select_rows_check.cc with its sequential model
// of count -> bases -> scatter share this one copy.
#pragma once

#include "blitzar_amd/csrc/base/macros.h"

namespace bz::proof {
constexpr u64 kMaxSelectRows = u64{1} << 30; // rows and capacity
constexpr u32 kMaxSelectColumns = 16;
constexpr u32 kSelectThreads = 256;
constexpr u32 kSelectLanes = 64;
constexpr u32 kSelectWaves = kSelectThreads / kSelectLanes;
// a wavefront takes kSelectRounds x 64 consecutive rows of a tile, 64 a round: the rows of one
// round, and so the stores of their kept rows, are neighbours
constexpr u32 kSelectRounds = 4;
constexpr u32 kSelectWaveRows = kSelectRounds * kSelectLanes;  // 256
constexpr u32 kSelectTileRows = kSelectWaves * kSelectWaveRows; // 1024
constexpr u32 kMaxSelectSpans = 2048;
static_assert(kMaxSelectRows / kSelectTileRows / kMaxSelectSpans * kSelectTileRows < (u64{1} << 32),
              "a span's count is one 32-bit word");

// kept(i): `bits` is the selector row's bytes as a little-endian integer, zero-extended
BZ_HD bool row_kept(u64 bits, u64 reject, bool invert) { return (bits != reject) != invert; }
// the bits of a row of `nbytes` <= 8 bytes at any address, byte by byte
BZ_HD u64 selector_bits(const u8* row, u32 nbytes) {
  u64 bits = 0;
  for (u32 k = 0; k < nbytes; ++k) bits |= static_cast<u64>(row[k]) << (8 * k);
  return bits;
}

// n rows as `spans` contiguous spans of `tiles_per_span` tiles each (the last one may be shorter
// and end inside a tile): 1 <= spans <= 2048, also for n = 0, whose one span is empty
struct span_partition {
  u32 spans, tiles_per_span;
};
BZ_HD span_partition partition_rows(u64 n) {
  const u64 tiles = (n + kSelectTileRows - 1) / kSelectTileRows;
  if (tiles == 0) return {1, 1};
  const u64 tiles_per_span = (tiles + kMaxSelectSpans - 1) / kMaxSelectSpans;
  return {static_cast<u32>((tiles + tiles_per_span - 1) / tiles_per_span),
          static_cast<u32>(tiles_per_span)};
}
// the first row of span g <= spans (g = spans: n)
BZ_HD u64 span_first_row(const span_partition& p, u64 n, u32 g) {
  const u64 first = static_cast<u64>(g) * p.tiles_per_span * kSelectTileRows;
  return first < n ? first : n;
}

// A wavefront's rows of a tile are wave_row + 64 r + lane, r < 4, and ballots[r] has bit `lane` set
// where that row is kept.  The number of kept rows of the wavefront before the row (r, lane):
BZ_HD u32 ballot_rank(const u64* ballots, u32 r, u32 lane) {
  u32 rank = 0;
#pragma unroll
  for (u32 q = 0; q < kSelectRounds; ++q) {
    const u64 below = q < r ? ~u64{0} : q == r ? (u64{1} << lane) - 1 : 0;
    rank += static_cast<u32>(__builtin_popcountll(ballots[q] & below));
  }
  return rank;
}
// all kept rows of the wavefront in the tile
BZ_HD u32 ballot_total(const u64* ballots) {
  u32 total = 0;
#pragma unroll
  for (u32 q = 0; q < kSelectRounds; ++q) total += static_cast<u32>(__builtin_popcountll(ballots[q]));
  return total;
}

// what the device form's workspace holds: one 32-bit count per span, and what the caller's pointer
// may lack to a multiple of 256.  0 outside n <= 2^30
BZ_HD u64 select_rows_workspace_bytes(u64 n) {
  if (n > kMaxSelectRows) return 0;
  return 4 * static_cast<u64>(partition_rows(n).spans) + 256;
}
} // namespace bz::proof

//--------------------------------------------------------------------------------------------------
// the library's entry points (HIP translation units only)
//--------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
// `columns`, `selected`: num_columns of them, on the host, descriptors checked by the caller
struct row_selection {
  sumcheck_column selector;
  u64 reject;
  bool invert;
  const sumcheck_column* columns;
  void* const* selected;
  u32 num_columns;
  u64 capacity;
  bool zero_tail;
};
struct row_take {
  const void* indices;
  u64 num_rows;
  const sumcheck_column* columns;
  void* const* taken;
  u32 num_columns;
};
// the checks both forms share (nulls, limits, alignment, overlaps, the workspace): aborts.  The C
// ABI runs them before either form below (and before it asks for the backend), which do not repeat
// them.  `device_form`: needs its workspace
void check_row_selection(const void* count, const void* indices, const row_selection& s,
                         const void* workspace, u64 workspace_bytes, bool device_form);
void check_row_take(const row_take& t);
// bzamd_select_rows / bzamd_take_rows: host operands, blocking, st.backend; cpu backend: row by
// row; GPU backend: the columns uploaded at their own width to devices[0], whose lease the caller
// holds
void select_rows(api_state& st, u64* count, void* indices, const row_selection& s);
void take_rows(api_state& st, const row_take& t);
// everything but the structs and their arrays is memory of the current device; enqueue-only, two
// kernel launches and one
void select_rows_device(void* count, void* indices, const row_selection& s, void* workspace,
                        hipStream_t stream);
void take_rows_device(const row_take& t, hipStream_t stream);
// the store shape of k_select_scatter: columns of at most `width` bytes a row (0 .. 32) go through
// LDS (shape b), wider ones are stored lane by lane (shape a); a negative width changes nothing.
// Returns the width in force before.  For the measurement of DESIGN 9 and for tests
int select_rows_packed_width(int width);
} // namespace bz::proof
#endif
