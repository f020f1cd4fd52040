// Wavefront-cooperative row gather of k_accumulate (kernels.h) for traits with
// C::has_lds_gather: the 64 rows a wavefront adds next are fetched as whole lines straight into the
// wavefront's LDS region instead of 16 bytes of 64 different lines per instruction.
//
// A row is kPieces pieces of 16 bytes (the used front of the 128-byte row).  Instruction i of the
// kPieces a wavefront issues per round moves the 64 pieces 64 i .. 64 i + 63, lane L piece
// c = 64 i + L: chunk c % kPieces of the row that lane c / kPieces asked for.  The LDS-DMA writes
// the 64 pieces of one instruction to a wave-uniform base + lane * 16, here region + 1024 i, so
// piece c lands at byte 16 c and the row of lane L is the kPieces * 16 contiguous bytes from
// L * kPieces * 16: kPieces consecutive lanes read kPieces * 16 contiguous bytes of one line.
//
// Every lane of the wavefront takes part in every round, whether or not it has an entry to add:
// a lane without one asks for a row that some lane of the task did get from its sorted entries
// (valid_entry below), never for a value that was not read from the task's entries.
#pragma once

#include "blitzar_amd/csrc/base/macros.h"

namespace bz::lds_gather {
constexpr u32 kLanes = 64;
constexpr u32 kPieceBytes = 16;
constexpr u32 kPieces = 7; // 112 of a row's 128 bytes: 3 x 36 bytes of limbs
constexpr u32 kRowBytes = kPieces * kPieceBytes;
constexpr u32 kInstructionBytes = kLanes * kPieceBytes;      // what one LDS-DMA writes
constexpr u32 kRegionBytes = kPieces * kInstructionBytes;    // per wavefront
static_assert(kRegionBytes == kLanes * kRowBytes && kRegionBytes == 7168);

struct piece {
  u32 source_lane; // whose row
  u32 chunk;       // which 16 bytes of it
};
// the piece lane `lane` moves in instruction `i` (< kPieces)
BZ_HD constexpr piece piece_of(u32 i, u32 lane) {
  const u32 c = kLanes * i + lane;
  return {c / kPieces, c % kPieces};
}
// where instruction i puts its 64 pieces (wave-uniform) and where lane `lane`'s piece lands
BZ_HD constexpr u32 instruction_base(u32 i) { return kInstructionBytes * i; }
BZ_HD constexpr u32 landing_offset(u32 i, u32 lane) { return instruction_base(i) + kPieceBytes * lane; }
// byte offset of chunk j of lane `lane`'s row in the region (the lane's j-th 16-byte read)
BZ_HD constexpr u32 read_offset(u32 lane, u32 j) { return kRowBytes * lane + kPieceBytes * j; }

// A lane's entries [lo, lane_hi) of a task with `total` sorted entries in segments of
// `seg_entries`: empty (lane_hi == lo) for a lane behind the task's end.
BZ_HD constexpr u32 lane_hi(u32 lo, u32 seg_entries, u32 total) {
  return lo >= total ? lo : lo + seg_entries < total ? lo + seg_entries : total;
}
// Rounds of a wavefront whose lane 0 starts at wave_lo < total: lane 0's entry count.  Segments
// are consecutive and only the task's last one is short, so no lane of the wavefront has more.
BZ_HD constexpr u32 wave_trips(u32 wave_lo, u32 seg_entries, u32 total) {
  return seg_entries < total - wave_lo ? seg_entries : total - wave_lo;
}
// The entry (sign << 31 | row) a lane hands to the round that fetches position `next` of its
// segment: that entry while the lane still has one, else the one it handed over last (`current`,
// valid by induction).  A lane with no entry at all starts from lane 0's first entry; lane 0 has
// one whenever the wavefront runs the loop.
BZ_HD constexpr u32 valid_entry(bool has_next, u32 next_entry, u32 current_entry) {
  return has_next ? next_entry : current_entry;
}

// Piece addresses.  A stored row is kStoredRowBytes apart from the next; while every row a task can
// name (its entries are row_base + row, row < rows: plan.h, task_desc) lies in the table's first
// 4 GiB, the byte offset of a piece fits 32 bits and is a shift and an OR (chunk < 8), so the fetch
// takes the wave-uniform table base and this lane offset.  Other tasks (merged window tables, up to
// 2^31 rows) form the 64-bit address.
constexpr u32 kStoredRowBytes = 128;
constexpr u32 kStoredRowLog2 = 7;
static_assert(kPieces * kPieceBytes <= kStoredRowBytes && (1u << kStoredRowLog2) == kStoredRowBytes);
BZ_HD constexpr bool narrow_offsets(u64 row_base, u64 rows) {
  return row_base + rows <= (u64{1} << (32 - kStoredRowLog2));
}
// for row < 2^25: the same value as u64(row) * kStoredRowBytes + chunk * kPieceBytes
BZ_HD constexpr u32 piece_offset32(u32 row, u32 chunk) {
  return row << kStoredRowLog2 | chunk * kPieceBytes;
}
} // namespace bz::lds_gather
