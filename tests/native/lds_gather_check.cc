// Stand-alone host model of the wavefront-cooperative row gather of k_accumulate
// (blitzar_amd/csrc/msm/lds_gather.h, and the walk of accumulate_lds_gather in msm/kernels.h with
// the LDS-DMA replaced by the copy it performs: lane L of instruction i moves 16 bytes from its own
// source address to region + 1024 i + 16 L).  tests/test_accumulate_lds_gather_host.py runs it, plain
// and built with -fsanitize=address,undefined, and reads the lines it prints:
//   <check> <failures> <cases>
// The table and the region are heap blocks of their exact sizes, so a read outside the table or a
// write outside the region is also an address-sanitizer report.  Row 0 of the table never occurs in
// the entries: a lane that handed over "row 0" instead of a row it was given is counted.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "blitzar_amd/csrc/msm/lds_gather.h"

using namespace bz;
namespace lg = bz::lds_gather;

constexpr u32 kTableRowBytes = 128;

struct report {
  unsigned long fail = 0, cases = 0;
  void expect(bool ok) {
    cases += 1;
    fail += ok ? 0 : 1;
  }
};

static int print(const char* name, const report& r) {
  std::printf("%s %lu %lu\n", name, r.fail, r.cases);
  return r.fail != 0;
}

// one round of the 64 lanes: entry[l] is what lane l hands over
static void round_of(std::vector<u8>& region, const std::vector<u8>& table,
                     const std::vector<u8>& row_is_valid, const u32* entry, report& handed) {
  for (u32 i = 0; i < lg::kPieces; ++i) {
    for (u32 lane = 0; lane < lg::kLanes; ++lane) {
      const lg::piece p = lg::piece_of(i, lane);
      const u32 row = entry[p.source_lane] & 0x7fffffffu;
      const bool ok = row < row_is_valid.size() && row_is_valid[row];
      handed.expect(ok);
      if (!ok) continue; // (the kernel would read outside the table here)
      std::memcpy(region.data() + lg::landing_offset(i, lane),
                  table.data() + static_cast<size_t>(row) * kTableRowBytes + p.chunk * lg::kPieceBytes,
                  lg::kPieceBytes);
    }
  }
}

// lane's row as its kPieces reads deliver it
static bool landed_row_is(const std::vector<u8>& region, const std::vector<u8>& table, u32 lane, u32 row) {
  u8 got[lg::kRowBytes];
  for (u32 j = 0; j < lg::kPieces; ++j) {
    std::memcpy(got + j * lg::kPieceBytes, region.data() + lg::read_offset(lane, j), lg::kPieceBytes);
  }
  return std::memcmp(got, table.data() + static_cast<size_t>(row) * kTableRowBytes, lg::kRowBytes) == 0;
}

int main() {
  int bad = 0;
  // 1. the piece mapping: every (lane, chunk) exactly once, inside the region, where the lane reads it
  {
    report once, inside, reads;
    std::vector<u32> count(lg::kLanes * lg::kPieces, 0);
    std::vector<u32> byte_writes(lg::kRegionBytes, 0);
    for (u32 i = 0; i < lg::kPieces; ++i) {
      for (u32 lane = 0; lane < lg::kLanes; ++lane) {
        const lg::piece p = lg::piece_of(i, lane);
        const bool in_range = p.source_lane < lg::kLanes && p.chunk < lg::kPieces;
        once.expect(in_range);
        if (in_range) count[p.source_lane * lg::kPieces + p.chunk] += 1;
        const u32 at = lg::landing_offset(i, lane);
        const bool fits = at % lg::kPieceBytes == 0 && at + lg::kPieceBytes <= lg::kRegionBytes &&
                          at == lg::instruction_base(i) + lane * lg::kPieceBytes;
        inside.expect(fits);
        if (fits) {
          for (u32 k = 0; k < lg::kPieceBytes; ++k) byte_writes[at + k] += 1;
        }
        reads.expect(in_range && at == lg::read_offset(p.source_lane, p.chunk));
      }
    }
    for (u32 c : count) once.expect(c == 1);
    for (u32 c : byte_writes) inside.expect(c == 1);
    for (u32 lane = 0; lane < lg::kLanes; ++lane) {
      for (u32 j = 0; j < lg::kPieces; ++j) {
        inside.expect(lg::read_offset(lane, j) + lg::kPieceBytes <= lg::kRegionBytes);
      }
    }
    bad += print("pieces_exactly_once", once);
    bad += print("offsets_inside_region", inside);
    bad += print("piece_lands_where_its_lane_reads", reads);
  }

  // 2. the walk of a task: segment sizes 8..128, totals that leave 0..63 lanes of the last
  //    wavefront with a short or no segment, one entry, whole wavefronts behind the end
  std::mt19937 rng(0x1d5);
  const u32 rows = 5000;
  std::vector<u8> table(static_cast<size_t>(rows) * kTableRowBytes);
  for (u8& v : table) v = static_cast<u8>(rng());
  report handed, landed, consumed, trip_counts, idle_wavefronts;
  for (u32 seg_log2 = 3; seg_log2 <= 7; ++seg_log2) {
    const u32 seg_entries = 1u << seg_log2;
    const u32 per_wave = lg::kLanes * seg_entries;
    std::vector<u32> totals = {1, 2, seg_entries - 1, seg_entries, seg_entries + 1, per_wave - 1, per_wave,
                               per_wave + 1, per_wave + seg_entries, 2 * per_wave - seg_entries - 1};
    for (u32 k = 0; k < 6; ++k) totals.push_back(1 + rng() % (3 * per_wave));
    for (u32 lanes = 1; lanes < lg::kLanes; lanes += 7) totals.push_back(per_wave + lanes * seg_entries - 3);
    for (u32 total : totals) {
      // entries: sign << 31 | row, rows 1..rows-1; only rows that occur are valid
      std::vector<u32> sorted(total);
      std::vector<u8> row_is_valid(rows, 0);
      for (u32& e : sorted) {
        const u32 row = 1 + rng() % (rows - 1);
        e = row | (rng() & 1u) << 31;
        row_is_valid[row] = 1;
      }
      std::vector<u32> times(total, 0);
      std::vector<u8> region(lg::kRegionBytes);
      // the grid covers the task's segments in workgroups of four wavefronts, and one more
      const u32 waves = (total + per_wave - 1) / per_wave + 4;
      for (u32 wave = 0; wave < waves; ++wave) {
        const u32 wave_lo = wave * per_wave;
        if (wave_lo >= total) { // returns before any cooperative operation
          idle_wavefronts.expect(true);
          continue;
        }
        const u32 trips = lg::wave_trips(wave_lo, seg_entries, total);
        u32 lo[lg::kLanes], hi[lg::kLanes], e_cur[lg::kLanes], e_next[lg::kLanes];
        for (u32 l = 0; l < lg::kLanes; ++l) {
          lo[l] = wave_lo + l * seg_entries;
          hi[l] = lg::lane_hi(lo[l], seg_entries, total);
          trip_counts.expect(hi[l] - lo[l] <= trips && (hi[l] <= total || hi[l] == lo[l]) &&
                             (l != 0 || hi[l] - lo[l] == trips));
          e_cur[l] = lo[l] < total ? sorted[lo[l]] : 0;
        }
        const u32 wave_entry = e_cur[0];
        for (u32 l = 0; l < lg::kLanes; ++l) e_cur[l] = lg::valid_entry(lo[l] < total, e_cur[l], wave_entry);
        round_of(region, table, row_is_valid, e_cur, handed);
        for (u32 l = 0; l < lg::kLanes; ++l) e_next[l] = lo[l] + 1 < hi[l] ? sorted[lo[l] + 1] : 0;
        for (u32 k = 0; k < trips; ++k) {
          // land
          for (u32 l = 0; l < lg::kLanes; ++l) {
            const u32 i = lo[l] + k;
            if (i >= hi[l]) continue; // masked out of the addition
            landed.expect(e_cur[l] == sorted[i] && landed_row_is(region, table, l, sorted[i] & 0x7fffffffu));
            times[i] += 1;
          }
          for (u32 l = 0; l < lg::kLanes; ++l) {
            e_cur[l] = lg::valid_entry(lo[l] + k + 1 < hi[l], e_next[l], e_cur[l]);
          }
          if (k + 1 < trips) round_of(region, table, row_is_valid, e_cur, handed);
          for (u32 l = 0; l < lg::kLanes; ++l) {
            if (lo[l] + k + 2 < hi[l]) e_next[l] = sorted[lo[l] + k + 2];
          }
        }
      }
      for (u32 t : times) consumed.expect(t == 1);
    }
  }
  bad += print("handed_rows_were_supplied", handed);
  bad += print("lane_reads_its_row", landed);
  bad += print("every_entry_added_once", consumed);
  bad += print("trip_counts", trip_counts);
  bad += print("wavefronts_without_entries", idle_wavefronts);
  return bad != 0;
}
