// Selection of rows of typed columns (bzamd_select_rows*, bzamd_take_rows*): with
//   kept(i) = (bits(selector[i]) != reject) != invert,   rank(i) = #{i' < i : kept(i')},
//   selected_j[rank(i)] = column_j[i],  indices[rank(i)] = i   for kept rows with rank(i) < capacity,
//   count = #{i < n : kept(i)},
// the stable compaction of a WHERE, of the distinct keys of a group-by and of the hits of a join,
// and  taken_j[r] = column_j[indices[r]]  (zero bytes where the index is past the column), the
// gather that goes with it.  Rows are copied at their own width, 1 .. 32 bytes; nothing here is
// field arithmetic, so both fields and both forms are served.
//
// The compaction is TWO launches whatever n, the columns and the data are, and no workgroup waits
// on another: no look-back flags, no tickets, no spins, no atomics.  The rows are cut into at most
// 2048 contiguous spans of whole tiles of 1024 rows (proof/select_rows.h), one workgroup of 256
// threads each:
//   * k_select_count: workgroup g counts the kept rows of span g and writes one 32-bit word to the
//     workspace.  Order does not matter here, so one- and two-byte selectors at an address of their
//     own alignment are read 16 bytes a lane (the rows before the first and after the last whole
//     16 bytes of the span go the general way), as k_count_range of proof/multiplicities.hip does.
//   * k_select_scatter: every workgroup sums the words of the spans before its own and all of them
//     (at most 2048 loads, reduced across the workgroup), then walks its span tile by tile.  In a
//     tile wavefront w takes rows 256 w + 64 r + lane, r < 4: four 64-bit ballots, the rank of a
//     lane among its wavefront's kept rows from them (ballot_rank), the wavefronts' totals through
//     LDS (two sets of four words, alternating by tile: one barrier a tile), and a running base
//     carried across the tiles.  STORE SHAPE (a): each kept lane stores its own row at rank x w.
//     The kept rows of one ballot have consecutive ranks, so the stores of a round are neighbours.
//     A row is copied in pieces of 16, 8, 4, 2 or 1 bytes: the largest that divides the width, the
//     column's address and the output's (uniform over the launch).  Rows at or past a column's end
//     are stored as zeros.  The last span's workgroup writes `count`.  The zero tail is a
//     grid-stride loop over [min(count, capacity), capacity), whose bounds every workgroup has from
//     the same words; with a tail the grid has workgroups beyond the spans that only zero.
//     STORE SHAPE (b), k_select_scatter<true>: the columns in turn, a tile's kept rows of one
//     column are first packed side by side in LDS, as many bytes in as the output address is past
//     a multiple of 16, so that an aligned 16-byte piece of LDS is an aligned 16-byte piece of the
//     output; whole pieces are then written one a lane in lane order, the ragged ends byte by
//     byte, two barriers a column.  LDS: 32 880 bytes (one tile of 32-byte rows, 16 for the skew,
//     96 as in (a)): four workgroups a CU.  Measured: (a) is the faster one at 2^22
//     rows for a 1- and an 8-byte column at every keep rate and for a 32-byte column at 1/64; (b)
//     only for 32-byte rows at 63/64.  (a) is kept: kDefaultPackedWidth = 0.  (b) stays behind
//     bzamd_select_rows_packed_width, per column by width, and the device tests run both.
// Every word of the workspace that launch 2 reads is written by launch 1; nothing is cleared.
// LDS of (a): 96 bytes.  No scratch memory in any kernel (tests/test_select_rows.py reads the
// compiler's report).
//
// The gather is ONE launch: a grid-stride loop over the output rows, the same row copy.
//
// The cpu backend goes row by row.
#include "blitzar_amd/csrc/proof/select_rows.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "blitzar_amd/csrc/proof/host_call.h"

namespace bz::proof {
namespace {
constexpr u32 kNoRow = 0xFFFFFFFFu; // the zero tail of `indices`
constexpr u32 kTakeBlocks = 2048;
constexpr u32 kDefaultPackedWidth = 0;
// shape (b): a tile's kept rows of one column at their widest, and what the skew may add
constexpr u32 kStageBytes = kSelectTileRows * 32 + 16;
// columns of at most this many bytes a row are stored in shape (b); 0: shape (a) for all
// (bzamd_select_rows_packed_width changes it, for the measurement of DESIGN 9 and for tests)
std::atomic<u32> g_packed_width{kDefaultPackedWidth};

// the selector as a kernel argument.  `natural`: 1, 2, 4 or 8 bytes at an address that is a
// multiple of the width: a row is one load
struct selector_view {
  const u8* data;
  u64 n, reject;
  u32 nbytes, natural, invert, reserved;
};
// the columns of a call: source, output, rows, width and the piece a row is copied in; travels as
// a kernel argument and is indexed by wave-uniform values alone
struct copied_columns {
  const u8* data[kMaxSelectColumns];
  u8* out[kMaxSelectColumns];
  u64 n[kMaxSelectColumns];
  u32 nbytes[kMaxSelectColumns], unit[kMaxSelectColumns];
  u32 packed[kMaxSelectColumns]; // k_select_scatter: the column's kept rows go through LDS (shape b)
  u32 count;
};

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 least(u64 a, u64 b) { return a < b ? a : b; }

__device__ __forceinline__ u64 load_selector(const selector_view& s, u64 i) {
  const u8* p = s.data + i * s.nbytes;
  if (s.natural != 0) {
    switch (s.nbytes) {
    case 1: return *p;
    case 2: return *reinterpret_cast<const u16*>(p);
    case 4: return *reinterpret_cast<const u32*>(p);
    default: return *reinterpret_cast<const u64*>(p);
    }
  }
  return selector_bits(p, s.nbytes);
}

template <class T>
__device__ __forceinline__ void copy_pieces(u8* dst, const u8* src, bool present, u32 pieces) {
  for (u32 k = 0; k < pieces; ++k) {
    T v{};
    if (present) v = reinterpret_cast<const T*>(src)[k];
    reinterpret_cast<T*>(dst)[k] = v;
  }
}
// dst[0 .. nbytes) <- src[0 .. nbytes), or zeros without a row (src is not read then); `unit`
// divides nbytes and both addresses
__device__ __forceinline__ void copy_row(u8* dst, const u8* src, bool present, u32 nbytes,
                                         u32 unit) {
  switch (unit) {
  case 16: copy_pieces<uint4>(dst, src, present, nbytes / 16); break;
  case 8: copy_pieces<u64>(dst, src, present, nbytes / 8); break;
  case 4: copy_pieces<u32>(dst, src, present, nbytes / 4); break;
  case 2: copy_pieces<u16>(dst, src, present, nbytes / 2); break;
  default: copy_pieces<u8>(dst, src, present, nbytes); break;
  }
}
// row `from` of every column (zeros at or past its end) to row `to` of its output; `loose_only`:
// the columns that do not go through LDS
__device__ __forceinline__ void copy_columns(const copied_columns& c, u64 to, u64 from,
                                             bool loose_only = false) {
  for (u32 j = 0; j < c.count; ++j) {
    if (loose_only && c.packed[j] != 0) continue;
    const u64 w = c.nbytes[j];
    const bool present = from < c.n[j];
    copy_row(c.out[j] + to * w, c.data[j] + (present ? from : 0) * w, present, c.nbytes[j],
             c.unit[j]);
  }
}

// the sum of x over the workgroup, in every thread; `slots`: four words of LDS nobody else uses
// before the next barrier.  Called by all threads together
__device__ __forceinline__ u64 block_sum(u64 x, u64* slots) {
#pragma unroll
  for (int offset = 32; offset >= 1; offset >>= 1) {
    x += static_cast<u64>(__shfl_xor(static_cast<unsigned long long>(x), offset));
  }
  if (threadIdx.x % kSelectLanes == 0) slots[threadIdx.x / kSelectLanes] = x;
  __syncthreads();
  u64 sum = 0;
#pragma unroll
  for (u32 w = 0; w < kSelectWaves; ++w) sum += slots[w];
  return sum;
}

__global__ void __launch_bounds__(kSelectThreads)
    k_select_count(u32* span_counts, const selector_view s, const span_partition p) {
  __shared__ u64 slots[kSelectWaves];
  const u32 tid = threadIdx.x;
  const u64 first = span_first_row(p, s.n, blockIdx.x);
  const u64 rows = span_first_row(p, s.n, blockIdx.x + 1) - first;
  const bool invert = s.invert != 0;
  u32 kept = 0;
  // rows [0, head) and [head + chunks * per_chunk, rows) of the span the general way, the rows
  // between as `chunks` aligned 16-byte loads
  u64 head = 0, chunks = 0;
  const u32 per_chunk = 16 / (s.nbytes <= 2 ? s.nbytes : 16); // 16, 8 or 1
  if (s.natural != 0 && s.nbytes <= 2) {
    const u64 address = reinterpret_cast<u64>(s.data + first * s.nbytes);
    head = least(rows, (16 - address % 16) % 16 / s.nbytes);
    chunks = (rows - head) / per_chunk;
  }
  const u64 body_rows = chunks * per_chunk;
  const u64 loose = rows - body_rows;
  for (u64 j = tid; j < loose; j += kSelectThreads) {
    const u64 i = first + (j < head ? j : j + body_rows);
    kept += row_kept(load_selector(s, i), s.reject, invert) ? 1u : 0u;
  }
  const uint4* body = reinterpret_cast<const uint4*>(s.data + (first + head) * s.nbytes);
  for (u64 c = tid; c < chunks; c += kSelectThreads) {
    const uint4 v = body[c];
    const u32 words[4] = {v.x, v.y, v.z, v.w};
    if (s.nbytes == 1) {
#pragma unroll
      for (u32 e = 0; e < 16; ++e) {
        const u32 bits = (words[e / 4] >> (8 * (e % 4))) & 0xFFu;
        kept += row_kept(bits, s.reject, invert) ? 1u : 0u;
      }
    } else {
#pragma unroll
      for (u32 e = 0; e < 8; ++e) {
        const u32 bits = (words[e / 2] >> (16 * (e % 2))) & 0xFFFFu;
        kept += row_kept(bits, s.reject, invert) ? 1u : 0u;
      }
    }
  }
  const u64 total = block_sum(kept, slots);
  if (tid == 0) span_counts[blockIdx.x] = static_cast<u32>(total);
}

// kPacked: some column is stored in shape (b) and the kernel has the stage in LDS
template <bool kPacked>
__global__ void __launch_bounds__(kSelectThreads)
    k_select_scatter(u64* count, u32* indices, const u32* __restrict__ span_counts,
                     const selector_view s, const span_partition p, const copied_columns columns,
                     u64 capacity, u32 zero_tail) {
  __shared__ u64 slots[2][kSelectWaves];
  __shared__ u32 wave_totals[2][kSelectWaves];
  __shared__ __attribute__((aligned(16))) u8 stage[kPacked ? kStageBytes : 16];
  const u32 tid = threadIdx.x, lane = tid % kSelectLanes, wave = tid / kSelectLanes;
  const u32 g = blockIdx.x;
  // the kept rows before this span, and all of them
  u64 before = 0, total = 0;
  for (u32 q = tid; q < p.spans; q += kSelectThreads) {
    const u64 c = span_counts[q];
    total += c;
    before += q < g ? c : 0;
  }
  before = block_sum(before, slots[0]);
  total = block_sum(total, slots[1]);
  const bool writes = indices != nullptr || columns.count != 0;
  if (g < p.spans && writes) {
    const u64 first = span_first_row(p, s.n, g), end = span_first_row(p, s.n, g + 1);
    const bool invert = s.invert != 0;
    u64 base = before;
    u32 parity = 0;
    // `tile` is the workgroup's: every wavefront takes every turn and every barrier
    for (u64 tile = first; tile < end; tile += kSelectTileRows, parity ^= 1) {
      const u64 wave_row = tile + wave * kSelectWaveRows + lane;
      u64 ballots[kSelectRounds];
#pragma unroll
      for (u32 r = 0; r < kSelectRounds; ++r) {
        const u64 i = wave_row + r * kSelectLanes;
        bool kept = false;
        if (i < end) kept = row_kept(load_selector(s, i), s.reject, invert);
        ballots[r] = __ballot(kept);
      }
      if (lane == 0) wave_totals[parity][wave] = ballot_total(ballots);
      __syncthreads();
      u32 lower = 0, all = 0;
#pragma unroll
      for (u32 q = 0; q < kSelectWaves; ++q) {
        const u32 t = wave_totals[parity][q];
        all += t;
        lower += q < wave ? t : 0;
      }
#pragma unroll
      for (u32 r = 0; r < kSelectRounds; ++r) {
        if (((ballots[r] >> lane) & 1) != 0) {
          const u64 rank = base + lower + ballot_rank(ballots, r, lane);
          if (rank < capacity) {
            const u64 i = wave_row + r * kSelectLanes;
            if (indices != nullptr) indices[rank] = static_cast<u32>(i);
            copy_columns(columns, rank, i, kPacked);
          }
        }
      }
      if constexpr (kPacked) {
        // shape (b), the columns in turn: the tile's kept rows side by side in LDS, `skew` bytes
        // in, so that an aligned 16-byte piece of LDS is an aligned 16-byte piece of the output;
        // whole pieces one a lane in lane order, the ragged ends byte by byte
        const u64 room = base < capacity ? capacity - base : 0;
        const u32 stored = static_cast<u32>(least(all, room)); // the tile's rows below capacity
        for (u32 j = 0; j < columns.count && stored != 0; ++j) {
          if (columns.packed[j] == 0) continue;
          const u32 w = columns.nbytes[j];
          u8* dst = columns.out[j] + base * w;
          const u32 skew = static_cast<u32>(reinterpret_cast<u64>(dst) % 16);
#pragma unroll
          for (u32 r = 0; r < kSelectRounds; ++r) {
            const u32 at = lower + ballot_rank(ballots, r, lane);
            if (((ballots[r] >> lane) & 1) != 0 && at < stored) {
              const u64 i = wave_row + r * kSelectLanes;
              const bool present = i < columns.n[j];
              copy_row(stage + skew + at * w, columns.data[j] + (present ? i : 0) * w, present, w,
                       columns.unit[j]);
            }
          }
          __syncthreads();
          const u32 total_bytes = skew + stored * w;
          const u32 first_whole = (skew + 15) / 16, whole_end = total_bytes / 16;
          u8* aligned = dst - skew;
          for (u32 c = first_whole + tid; c < whole_end; c += kSelectThreads) {
            reinterpret_cast<uint4*>(aligned)[c] = reinterpret_cast<const uint4*>(stage)[c];
          }
          const u32 head_end = static_cast<u32>(least(16 * first_whole, total_bytes));
          const u32 tail_begin = 16 * whole_end > head_end ? 16 * whole_end : head_end;
          if (tid < 16 && skew + tid < head_end) aligned[skew + tid] = stage[skew + tid];
          if (tid >= 16 && tid < 32 && tail_begin + (tid - 16) < total_bytes) {
            aligned[tail_begin + (tid - 16)] = stage[tail_begin + (tid - 16)];
          }
          __syncthreads();
        }
      }
      base += all;
    }
  }
  if (g + 1 == p.spans && tid == 0 && count != nullptr) *count = total;
  if (zero_tail != 0) {
    const u64 stride = static_cast<u64>(gridDim.x) * kSelectThreads;
    for (u64 to = least(total, capacity) + static_cast<u64>(g) * kSelectThreads + tid; to < capacity;
         to += stride) {
      if (indices != nullptr) indices[to] = kNoRow;
      copy_columns(columns, to, ~u64{0}); // no column has that row: zeros
    }
  }
}

__global__ void __launch_bounds__(kSelectThreads)
    k_take_rows(const u32* __restrict__ indices, u64 num_rows, const copied_columns columns) {
  const u64 stride = static_cast<u64>(gridDim.x) * kSelectThreads;
  for (u64 r = static_cast<u64>(blockIdx.x) * kSelectThreads + threadIdx.x; r < num_rows;
       r += stride) {
    copy_columns(columns, r, indices[r]);
  }
}

//--------------------------------------------------------------------------------------------------
// host backend: row by row
//--------------------------------------------------------------------------------------------------
// row `from` of the column (zeros at or past its end) to row `to` of `out`
void copy_row_host(void* out, u64 to, const sumcheck_column& c, u64 from) {
  u8* dst = static_cast<u8*>(out) + to * c.nbytes;
  if (from < c.n) {
    std::memcpy(dst, static_cast<const u8*>(c.data) + from * c.nbytes, c.nbytes);
  } else {
    std::memset(dst, 0, c.nbytes);
  }
}

void select_host(u64* count, void* indices, const row_selection& s) {
  const u8* selector = static_cast<const u8*>(s.selector.data);
  u32* index_of = static_cast<u32*>(indices);
  u64 kept = 0;
  for (u64 i = 0; i < s.selector.n; ++i) {
    const u64 bits = selector_bits(selector + i * s.selector.nbytes, s.selector.nbytes);
    if (!row_kept(bits, s.reject, s.invert)) continue;
    if (kept < s.capacity) {
      if (index_of != nullptr) index_of[kept] = static_cast<u32>(i);
      for (u32 j = 0; j < s.num_columns; ++j) copy_row_host(s.selected[j], kept, s.columns[j], i);
    }
    ++kept;
  }
  if (count != nullptr) *count = kept;
  for (u64 to = std::min(kept, s.capacity); s.zero_tail && to < s.capacity; ++to) {
    if (index_of != nullptr) index_of[to] = kNoRow;
    for (u32 j = 0; j < s.num_columns; ++j) copy_row_host(s.selected[j], to, s.columns[j], ~u64{0});
  }
}

void take_host(const row_take& t) {
  const u32* indices = static_cast<const u32*>(t.indices);
  for (u64 r = 0; r < t.num_rows; ++r) {
    for (u32 j = 0; j < t.num_columns; ++j) copy_row_host(t.taken[j], r, t.columns[j], indices[r]);
  }
}

//--------------------------------------------------------------------------------------------------
// device form: enqueue only
//--------------------------------------------------------------------------------------------------
// the largest of 16, 8, 4, 2, 1 that divides the width and both addresses
u32 copy_unit(u32 nbytes, const void* from, const void* to) {
  const uintptr_t all = nbytes | reinterpret_cast<uintptr_t>(from) | reinterpret_cast<uintptr_t>(to);
  u32 unit = 16;
  while (all % unit != 0) unit /= 2;
  return unit;
}
copied_columns copied_columns_of(const sumcheck_column* columns, void* const* outputs, u32 count,
                                 u32 packed_width = 0) {
  copied_columns c;
  std::memset(&c, 0, sizeof(c));
  c.count = count;
  for (u32 j = 0; j < count; ++j) {
    c.data[j] = static_cast<const u8*>(columns[j].data);
    c.out[j] = static_cast<u8*>(outputs[j]);
    c.n[j] = columns[j].n;
    c.nbytes[j] = columns[j].nbytes;
    c.unit[j] = copy_unit(columns[j].nbytes, columns[j].data, outputs[j]);
    c.packed[j] = columns[j].nbytes <= packed_width ? 1 : 0;
  }
  return c;
}

void select_enqueue(void* count, void* indices, const row_selection& s, void* workspace,
                    hipStream_t stream) {
  const u32 w = s.selector.nbytes;
  const bool natural =
      (w & (w - 1)) == 0 && reinterpret_cast<uintptr_t>(s.selector.data) % w == 0;
  const selector_view selector{static_cast<const u8*>(s.selector.data), s.selector.n, s.reject, w,
                               natural ? 1u : 0u, s.invert ? 1u : 0u, 0};
  const span_partition p = partition_rows(s.selector.n);
  const copied_columns columns =
      copied_columns_of(s.columns, s.selected, s.num_columns, g_packed_width.load());
  bool packed = false;
  for (u32 j = 0; j < s.num_columns; ++j) packed = packed || columns.packed[j] != 0;
  u32* span_counts = reinterpret_cast<u32*>(workspace_carver::aligned(workspace));
  hipLaunchKernelGGL(k_select_count, dim3(p.spans), dim3(kSelectThreads), 0, stream, span_counts,
                     selector, p);
  BZ_HIP_CHECK(hipGetLastError());
  // with a tail, workgroups beyond the spans zero with the others
  u64 blocks = p.spans;
  if (s.zero_tail) {
    const u64 tail_blocks = (s.capacity + kSelectThreads - 1) / kSelectThreads;
    blocks = std::max<u64>(blocks, std::min<u64>(tail_blocks, kMaxSelectSpans));
  }
  if (packed) {
    hipLaunchKernelGGL(k_select_scatter<true>, dim3(static_cast<u32>(blocks)), dim3(kSelectThreads),
                       0, stream, static_cast<u64*>(count), static_cast<u32*>(indices), span_counts,
                       selector, p, columns, s.capacity, s.zero_tail ? 1u : 0u);
  } else {
    hipLaunchKernelGGL(k_select_scatter<false>, dim3(static_cast<u32>(blocks)),
                       dim3(kSelectThreads), 0, stream, static_cast<u64*>(count),
                       static_cast<u32*>(indices), span_counts, selector, p, columns, s.capacity,
                       s.zero_tail ? 1u : 0u);
  }
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 2;
}

void take_enqueue(const row_take& t, hipStream_t stream) {
  const copied_columns columns = copied_columns_of(t.columns, t.taken, t.num_columns);
  const u64 blocks =
      std::min<u64>((t.num_rows + kSelectThreads - 1) / kSelectThreads, kTakeBlocks);
  hipLaunchKernelGGL(k_take_rows, dim3(static_cast<u32>(blocks)), dim3(kSelectThreads), 0, stream,
                     static_cast<const u32*>(t.indices), t.num_rows, columns);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}

uintptr_t address(const void* p) { return reinterpret_cast<uintptr_t>(p); }
byte_range range_of(const sumcheck_column& c) { return {c.data, c.n * c.nbytes}; }
} // namespace

void check_row_selection(const void* count, const void* indices, const row_selection& s,
                         const void* workspace, u64 workspace_bytes, bool device_form) {
  const u64 n = s.selector.n;
  BZ_RELEASE_ASSERT(s.selector.nbytes >= 1 && s.selector.nbytes <= 8,
                    "the row selection needs a selector of 1 .. 8 bytes");
  BZ_RELEASE_ASSERT(s.num_columns <= kMaxSelectColumns, "the row selection needs num_columns <= 16");
  BZ_RELEASE_ASSERT(n <= kMaxSelectRows, "the row selection needs n <= 2^30");
  BZ_RELEASE_ASSERT(s.capacity <= kMaxSelectRows, "the row selection needs capacity <= 2^30");
  BZ_RELEASE_ASSERT(count != nullptr || indices != nullptr || s.num_columns != 0,
                    "the row selection needs an output");
  std::vector<byte_range> outputs{{count, 8}, {indices, 4 * s.capacity}};
  for (u32 j = 0; j < s.num_columns; ++j) {
    BZ_RELEASE_ASSERT(s.columns[j].n <= n, "a column of the row selection is longer than n");
    BZ_RELEASE_ASSERT(s.capacity == 0 || s.selected[j] != nullptr,
                      "null output of the row selection with capacity > 0");
    BZ_RELEASE_ASSERT(address(s.selected[j]) % 8 == 0,
                      "the outputs of the row selection must be 8-byte aligned");
    outputs.push_back({s.selected[j], s.capacity * s.columns[j].nbytes});
  }
  BZ_RELEASE_ASSERT(address(count) % 8 == 0,
                    "the outputs of the row selection must be 8-byte aligned");
  BZ_RELEASE_ASSERT(address(indices) % 4 == 0, "the indices must be 4-byte aligned");
  if (device_form) {
    BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= select_rows_workspace_bytes(n),
                      "the workspace of the row selection is too small");
  } else {
    workspace_bytes = 0;
  }
  for (size_t a = 0; a < outputs.size(); ++a) {
    for (size_t b = a + 1; b < outputs.size(); ++b) {
      BZ_RELEASE_ASSERT(!overlap(outputs[a], outputs[b]), "the outputs of the row selection overlap");
    }
    BZ_RELEASE_ASSERT(!overlap(outputs[a], range_of(s.selector)),
                      "an output overlaps an input of the same call");
    for (u32 j = 0; j < s.num_columns; ++j) {
      BZ_RELEASE_ASSERT(!overlap(outputs[a], range_of(s.columns[j])),
                        "an output overlaps an input of the same call");
    }
    BZ_RELEASE_ASSERT(!overlap(outputs[a], {workspace, workspace_bytes}),
                      "an output overlaps the workspace of the same call");
  }
}

void check_row_take(const row_take& t) {
  BZ_RELEASE_ASSERT(t.num_rows >= 1 && t.num_rows <= kMaxSelectRows,
                    "the row gather needs 1 <= num_rows <= 2^30");
  BZ_RELEASE_ASSERT(t.num_columns >= 1 && t.num_columns <= kMaxSelectColumns,
                    "the row gather needs 1 <= num_columns <= 16");
  BZ_RELEASE_ASSERT(address(t.indices) % 4 == 0, "the indices must be 4-byte aligned");
  std::vector<byte_range> outputs;
  for (u32 j = 0; j < t.num_columns; ++j) {
    BZ_RELEASE_ASSERT(t.taken[j] != nullptr, "null output of the row gather");
    BZ_RELEASE_ASSERT(address(t.taken[j]) % 8 == 0,
                      "the outputs of the row gather must be 8-byte aligned");
    outputs.push_back({t.taken[j], t.num_rows * t.columns[j].nbytes});
  }
  for (size_t a = 0; a < outputs.size(); ++a) {
    for (size_t b = a + 1; b < outputs.size(); ++b) {
      BZ_RELEASE_ASSERT(!overlap(outputs[a], outputs[b]), "the outputs of the row gather overlap");
    }
    BZ_RELEASE_ASSERT(!overlap(outputs[a], {t.indices, 4 * t.num_rows}),
                      "an output overlaps an input of the same call");
    for (u32 j = 0; j < t.num_columns; ++j) {
      BZ_RELEASE_ASSERT(!overlap(outputs[a], range_of(t.columns[j])),
                        "an output overlaps an input of the same call");
    }
  }
}

void select_rows_device(void* count, void* indices, const row_selection& s, void* workspace,
                        hipStream_t stream) {
  select_enqueue(count, indices, s, workspace, stream);
}

void take_rows_device(const row_take& t, hipStream_t stream) { take_enqueue(t, stream); }

int select_rows_packed_width(int width) {
  const u32 now = g_packed_width.load();
  if (width >= 0) g_packed_width.store(std::min<u32>(static_cast<u32>(width), 32));
  return static_cast<int>(now);
}

void select_rows(api_state& st, u64* count, void* indices, const row_selection& s) {
  if (st.backend != 2) {
    select_host(count, indices, s);
    return;
  }
  // the columns up at their own width, the device form, the results down.  Without the zero tail
  // the rows from min(count, capacity) on are not written: the outputs go up first, so that what
  // comes down there is what the caller had
  host_call call{st};
  const u64 n = s.selector.n;
  void *d_count = nullptr, *d_indices = nullptr, *workspace = nullptr;
  std::vector<void*> selected(s.num_columns, nullptr);
  std::vector<sumcheck_column> columns;
  row_selection staged = s;
  const auto result = [&](void** slot, void* host, size_t bytes) {
    if (host == nullptr || bytes == 0 || s.zero_tail) {
      call.output(slot, bytes != 0 ? host : nullptr, bytes);
    } else {
      call.in_out(slot, host, bytes);
    }
  };
  call.output(&d_count, count, 8);
  result(&d_indices, indices, 4 * s.capacity);
  for (u32 j = 0; j < s.num_columns; ++j) {
    result(&selected[j], s.selected[j], s.capacity * s.columns[j].nbytes);
  }
  call.input(&staged.selector.data, n != 0 ? s.selector.data : nullptr, n * s.selector.nbytes);
  call.columns(&columns, s.columns, s.num_columns);
  call.scratch(&workspace, select_rows_workspace_bytes(n));
  call.allocate();
  staged.columns = columns.data();
  staged.selected = selected.data();
  select_enqueue(d_count, d_indices, staged, workspace, call.stream());
  call.finish();
}

void take_rows(api_state& st, const row_take& t) {
  if (st.backend != 2) {
    take_host(t);
    return;
  }
  host_call call{st};
  std::vector<void*> taken(t.num_columns, nullptr);
  std::vector<sumcheck_column> columns;
  row_take staged = t;
  for (u32 j = 0; j < t.num_columns; ++j) {
    call.output(&taken[j], t.taken[j], t.num_rows * t.columns[j].nbytes);
  }
  call.input(&staged.indices, t.indices, 4 * t.num_rows);
  call.columns(&columns, t.columns, t.num_columns);
  call.allocate();
  staged.columns = columns.data();
  staged.taken = taken.data();
  take_enqueue(staged, call.stream());
  call.finish();
}
} // namespace bz::proof
