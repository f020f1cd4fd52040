// The word columns of a range check (bzamd_decompose_words*, bzamd_map_words*):
//   words[k * plane_stride + i] = byte k of key(i),   key(i) = shift + column[i] in [0, p),
//   counts[v] = #{(k, i) : that byte = v},   overflow = #{i : key(i) >= 2^(8 num_words)},
//   mapped[k * mapped_stride + 32 i ..+32] = table[words_k[i]],
// over the typed columns of the sumcheck; the key is key_of of proof/column_key.h, the one the
// multiplicity count compares rows by.
//
// Decompose, two launches whatever n, num_words and the data are; every loop is grid-stride:
//   * k_clear_words: counts <- 0, overflow <- 0 (a kernel, not a memset: bzamd_kernel_launch_count
//     sees a fixed number).
//   * k_decompose_words: a workgroup of kWordThreads lanes owns a tile of kWordTile consecutive
//     rows and walks tiles grid-stride.  Each row is read once.
//       - Keys.  Lane t takes rows t, t + kWordThreads, ... of the tile (a wavefront's load of an
//         i64 column is 512 consecutive bytes), computes the key, adds the shift's key (computed
//         once per workgroup, kept in LDS) and writes byte k to LDS plane k, one plane after the
//         other (kPlanePitch bytes apart).  Rows at or above 2^(8 num_words) are balloted and
//         counted per wavefront.
//       - Planes k >= lds_planes are zero by construction (an unsigned column below 32 bytes
//         without a shift has no bytes at or above its width): no key byte is taken for them, they
//         do not pass through LDS, their stores are zeros and their count goes to bin 0 once per
//         tile.
//       - Stores.  LDS plane k starts skew(k) = (address of global plane k) mod 16 bytes into its
//         pitch, so that an aligned 16-byte chunk of LDS is an aligned 16-byte chunk of global
//         memory (a tile starts at a multiple of 16 rows).  A work item is (plane, chunk):
//         consecutive lanes take consecutive chunks of one plane, one ds_read_b128 and one 16-byte
//         store each, 1 KiB a wavefront.  The chunks a tile only partly covers (the plane's first
//         and last bytes, and with a skew the ends of every tile) are stored byte by byte, never
//         more than the rows the tile owns.
//       - Counts.  32-bit bins in LDS (a workgroup sees fewer than 2^32 (row, word) pairs: at most
//         2^30 rows x 32 words over kDecomposeBlocks workgroups), added to `counts` once at the
//         end, non-zero bins only.  A lane counts the 16 bytes of its chunk.  The common case is
//         the contended one: upper words of small values are all zero, a constant column has one
//         value a plane.  So a chunk whose 16 bytes are equal is ONE add of 16, and those adds are
//         aggregated in the wavefront as wave_adder (proof/multiplicities.hip) does: the first
//         remaining lane's byte is broadcast, the lanes that share it are balloted, one lane adds
//         16 x their number.  A constant plane costs one LDS add per wavefront and turn.  Mixed
//         chunks take one LDS add a byte.
//   No scratch memory (tests/test_word_columns.py reads the compiler's report): key bytes are taken
//   with constant indices in unrolled loops.  LDS: 32 planes x 1040 bytes, the bins, 34.3 KB.
//
// Map, one launch: the table (8 KB) sits in LDS; a workgroup owns a tile of kMapTile rows of one
// plane, loads its words into LDS 16 bytes a lane (with the same skew, so the loads are aligned;
// byte loads at the ragged ends, nothing outside the plane is read), and then lane t of turn u
// stores half-row 256 u + t: the word of row (256 u + t) / 2 from LDS, 16 bytes of its table row
// from LDS, one 16-byte store; a wavefront's stores are 1 KiB of consecutive bytes.  A byte copy:
// no field arithmetic, either field, either form.
#include "blitzar_amd/csrc/proof/word_columns.h"

#include <algorithm>

#include "blitzar_amd/csrc/proof/column_key.h"
#include "blitzar_amd/csrc/proof/host_call.h"

namespace bz::proof {
namespace {
constexpr u32 kWordThreads = 256;
constexpr u32 kWordLaneRows = 4;
constexpr u32 kWordTile = kWordLaneRows * kWordThreads;
constexpr u32 kPlanePitch = kWordTile + 16;   // room for the skew, a multiple of 16
constexpr u32 kTileChunks = kPlanePitch / 16; // 16-byte chunks a tile's rows of one plane touch
// 4 workgroups per CU (LDS: 34 KB each); kDecomposeBlocks * kWordTile = 2^20 rows in flight
constexpr u32 kDecomposeBlocks = 1024;
constexpr u32 kMapTile = 4096;
constexpr u32 kMapPitch = kMapTile + 16;
constexpr u32 kMapChunks = kMapPitch / 16;
constexpr u32 kMapBlocks = 2048;
static_assert(kWordThreads == kWordValues, "one lane per bin");

struct decompose_args {
  u8* words;
  u64* counts;
  u64* overflow;
  column_view column;
  const u8* shift;
  u32 num_words, lds_planes; // planes k >= lds_planes are zero by construction
  u64 plane_stride;
};

// byte e < 16 of a chunk; e is a constant wherever this is called
__device__ __forceinline__ u32 chunk_byte(const uint4& v, u32 e) {
  const u32 word = e < 4 ? v.x : e < 8 ? v.y : e < 12 ? v.z : v.w;
  return (word >> (8 * (e & 3))) & 0xFFu;
}
// global plane k's address mod 16: where LDS plane k starts in its pitch
__device__ __forceinline__ u32 plane_skew(const void* planes, u64 plane_stride, u32 k) {
  return (static_cast<u32>(reinterpret_cast<u64>(planes)) + k * static_cast<u32>(plane_stride)) & 15;
}

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWordThreads) k_clear_words(u64* counts, u64* overflow) {
  if (counts != nullptr) counts[threadIdx.x] = 0;
  if (threadIdx.x == 0 && overflow != nullptr) *overflow = 0;
}

// one wavefront's adds of 16 to the bins, aggregated; called by all 64 lanes together
__device__ __forceinline__ void add_uniform_chunks(u32* bins, u32 value, bool uniform) {
  u64 remaining = __ballot(uniform);
  while (remaining != 0) {
    const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(remaining))) - 1;
    const u32 leader_value = static_cast<u32>(
        __builtin_amdgcn_readlane(static_cast<int>(value), static_cast<int>(leader)));
    const u64 same = __ballot(uniform && value == leader_value);
    if (__lane_id() == leader) atomicAdd(bins + leader_value, 16 * static_cast<u32>(__popcll(same)));
    remaining &= ~same;
  }
}

template <class E>
__global__ void __launch_bounds__(kWordThreads) k_decompose_words(const decompose_args a) {
  __shared__ __attribute__((aligned(16))) u8 tile[kMaxWords * kPlanePitch];
  __shared__ u32 bins[kWordValues];
  __shared__ u32 block_overflow;
  __shared__ lookup_key shift_key;
  const u32 tid = threadIdx.x;
  bins[tid] = 0;
  if (tid == 0) {
    block_overflow = 0;
    if (a.shift != nullptr) shift_key = key_of_element<E>(a.shift);
  }
  __syncthreads();
  const bool shifted = a.shift != nullptr;
  const u64 n = a.column.n;
  const u64 num_tiles = (n + kWordTile - 1) / kWordTile;
  const u32 items = a.num_words * kTileChunks;
  u32 wave_overflow = 0; // the workgroup sees fewer than 2^32 rows
  for (u64 t = blockIdx.x; t < num_tiles; t += gridDim.x) {
    const u64 base = t * kWordTile;
    const u32 rows = static_cast<u32>(std::min<u64>(kWordTile, n - base));
    // keys: byte k of row r to LDS plane k
    for (u32 j = 0; j < kWordLaneRows; ++j) {
      const u32 r = j * kWordThreads + tid;
      bool over = false;
      if (r < rows) {
        lookup_key key = key_of<E>(a.column, base + r);
        if (shifted) key = key_sum<E>(key, shift_key);
        over = key_overflows(key, a.num_words);
#pragma unroll
        for (u32 k = 0; k < kMaxWords; ++k) {
          if (k < a.lds_planes) {
            tile[k * kPlanePitch + plane_skew(a.words, a.plane_stride, k) + r] =
                static_cast<u8>(key_byte(key, k));
          }
        }
      }
      wave_overflow += static_cast<u32>(__popcll(__ballot(over)));
    }
    __syncthreads();
    // stores and counts: item = (plane, chunk); every lane of a wavefront takes the same turns
    for (u32 first = 0; first < items; first += kWordThreads) {
      const u32 item = first + tid;
      const u32 k = item / kTileChunks, c = item % kTileChunks;
      // the tile's rows [from, to) of the 16 the chunk covers, [lo, lo + 16)
      const int lo = static_cast<int>(16 * c) - static_cast<int>(plane_skew(a.words, a.plane_stride, k));
      const int from = std::max(lo, 0), to = std::min(lo + 16, static_cast<int>(rows));
      const bool active = item < items && from < to;
      const bool full = active && to - from == 16;
      const bool keyed = active && k < a.lds_planes;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (keyed) v = *reinterpret_cast<const uint4*>(tile + k * kPlanePitch + 16 * c);
      if (a.words != nullptr && active) {
        u8* at = a.words + k * a.plane_stride + base + static_cast<i64>(lo);
        if (full) {
          *reinterpret_cast<uint4*>(at) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            if (lo + e >= from && lo + e < to) at[e] = static_cast<u8>(chunk_byte(v, e));
          }
        }
      }
      if (a.counts != nullptr) {
        const u32 value = v.x & 0xFFu;
        const bool uniform = keyed && full && v.x == value * 0x01010101u && v.y == v.x &&
                             v.z == v.x && v.w == v.x;
        add_uniform_chunks(bins, value, uniform);
        if (keyed && !uniform) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            if (lo + e >= from && lo + e < to) atomicAdd(bins + chunk_byte(v, e), 1u);
          }
        }
      }
    }
    if (tid == 0 && a.counts != nullptr && a.num_words > a.lds_planes) {
      atomicAdd(bins, (a.num_words - a.lds_planes) * rows);
    }
    __syncthreads();
  }
  if (__lane_id() == 0 && wave_overflow != 0) atomicAdd(&block_overflow, wave_overflow);
  __syncthreads();
  if (a.counts != nullptr) {
    const u32 count = bins[tid];
    if (count != 0) {
      (void)__hip_atomic_fetch_add(a.counts + tid, static_cast<u64>(count), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid == 0 && block_overflow != 0 && a.overflow != nullptr) {
    (void)__hip_atomic_fetch_add(a.overflow, static_cast<u64>(block_overflow), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  }
}

// 16 bytes of a mapped row: `mapped` is 8-byte aligned
struct half_row {
  u64 lo, hi;
};

__global__ void __launch_bounds__(kWordThreads) k_map_words(u8* mapped, const word_map m) {
  __shared__ __attribute__((aligned(16))) u8 table[32 * kWordValues];
  __shared__ __attribute__((aligned(16))) u8 stage[kMapPitch];
  const u32 tid = threadIdx.x;
  const u8* table_rows = static_cast<const u8*>(m.table);
  if (reinterpret_cast<u64>(table_rows) % 16 == 0) {
    for (u32 q = tid; q < 2 * kWordValues; q += kWordThreads) {
      reinterpret_cast<uint4*>(table)[q] = reinterpret_cast<const uint4*>(table_rows)[q];
    }
  } else {
    for (u32 b = tid; b < 32 * kWordValues; b += kWordThreads) table[b] = table_rows[b];
  }
  __syncthreads();
  const u64 tiles_per_plane = (m.n + kMapTile - 1) / kMapTile;
  const u64 num_tiles = m.num_planes * tiles_per_plane;
  for (u64 t = blockIdx.x; t < num_tiles; t += gridDim.x) {
    const u32 k = static_cast<u32>(t / tiles_per_plane);
    const u64 base = (t % tiles_per_plane) * kMapTile;
    const u32 rows = static_cast<u32>(std::min<u64>(kMapTile, m.n - base));
    const u8* plane = static_cast<const u8*>(m.words) + k * m.plane_stride;
    const u32 skew = plane_skew(plane, 0, 0);
    // the tile's words to LDS: row r at stage[skew + r]
    for (u32 c = tid; c < kMapChunks; c += kWordThreads) {
      const int lo = static_cast<int>(16 * c) - static_cast<int>(skew);
      const int from = std::max(lo, 0), to = std::min(lo + 16, static_cast<int>(rows));
      if (from >= to) continue;
      const u8* at = plane + base + static_cast<i64>(lo);
      if (to - from == 16) {
        *reinterpret_cast<uint4*>(stage + 16 * c) = *reinterpret_cast<const uint4*>(at);
      } else {
        for (int e = from - lo; e < to - lo; ++e) stage[16 * c + e] = at[e];
      }
    }
    __syncthreads();
    half_row* out = reinterpret_cast<half_row*>(mapped + k * m.mapped_stride + 32 * base);
#pragma unroll 4
    for (u32 h = tid; h < 2 * rows; h += kWordThreads) {
      const u32 word = stage[skew + (h >> 1)];
      const uint4 v = *reinterpret_cast<const uint4*>(table + 32 * word + 16 * (h & 1));
      out[h] = half_row{v.x | static_cast<u64>(v.y) << 32, v.z | static_cast<u64>(v.w) << 32};
    }
    __syncthreads();
  }
}

//--------------------------------------------------------------------------------------------------
// host backend: the sequential models of the header
//--------------------------------------------------------------------------------------------------
template <class E>
void decompose_host(u8* words, u64* counts, u64* overflow, const word_decomposition& d) {
  const column_view column = make_column_view(d.column);
  const bool shifted = d.shift != nullptr;
  const lookup_key shift_key = shifted ? key_of_element<E>(d.shift) : lookup_key{{0, 0, 0, 0}};
  model_decompose(words, counts, overflow, column.n, d.num_words, d.plane_stride, [&](u64 i) {
    const lookup_key key = key_of<E>(column, i);
    return shifted ? key_sum<E>(key, shift_key) : key;
  });
}

//--------------------------------------------------------------------------------------------------
// device forms: enqueue only
//--------------------------------------------------------------------------------------------------
template <class E>
void decompose_enqueue(u8* words, u64* counts, u64* overflow, const word_decomposition& d,
                       hipStream_t stream) {
  hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(kWordThreads), 0, stream, counts, overflow);
  BZ_HIP_CHECK(hipGetLastError());
  // an unsigned column below 32 bytes without a shift has no bytes at or above its width
  const bool narrow = d.shift == nullptr && !d.column.is_signed && d.column.nbytes < 32;
  const decompose_args args{words,
                            counts,
                            overflow,
                            make_column_view(d.column),
                            static_cast<const u8*>(d.shift),
                            d.num_words,
                            narrow ? std::min(d.num_words, d.column.nbytes) : d.num_words,
                            d.plane_stride};
  const u64 num_tiles = (d.column.n + kWordTile - 1) / kWordTile;
  const u32 blocks = static_cast<u32>(std::min<u64>(kDecomposeBlocks, std::max<u64>(num_tiles, 1)));
  hipLaunchKernelGGL((k_decompose_words<E>), dim3(blocks), dim3(kWordThreads), 0, stream, args);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += kDecomposeLaunches;
}

void map_enqueue(void* mapped, const word_map& m, hipStream_t stream) {
  const u64 num_tiles = m.num_planes * ((m.n + kMapTile - 1) / kMapTile);
  const u32 blocks = static_cast<u32>(std::min<u64>(kMapBlocks, num_tiles));
  hipLaunchKernelGGL(k_map_words, dim3(blocks), dim3(kWordThreads), 0, stream,
                     static_cast<u8*>(mapped), m);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += kMapLaunches;
}
} // namespace

void check_word_decomposition(const void* words, const void* counts, const void* overflow,
                              unsigned field_id, const word_decomposition& d) {
  BZ_RELEASE_ASSERT(d.column.n <= kMaxWordRows, "the word decomposition needs n <= 2^30");
  BZ_RELEASE_ASSERT(d.num_words >= 1 && d.num_words <= kMaxWords,
                    "the word decomposition needs 1 <= num_words <= 32");
  BZ_RELEASE_ASSERT(d.plane_stride >= d.column.n, "the word decomposition needs plane_stride >= n");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(counts) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(overflow) % 8 == 0,
                    "counts and overflow of the word decomposition must be 8-byte aligned");
  const byte_range outputs[3] = {{words, planes_extent(d.num_words, d.plane_stride, d.column.n)},
                                 {counts, 8 * kWordValues},
                                 {overflow, 8}};
  BZ_RELEASE_ASSERT(!overlap(outputs[0], outputs[1]) && !overlap(outputs[0], outputs[2]) &&
                        !overlap(outputs[1], outputs[2]),
                    "the outputs of the word decomposition overlap");
  for (const byte_range& out : outputs) {
    BZ_RELEASE_ASSERT(!overlap(out, {d.column.data, d.column.n * d.column.nbytes}) &&
                          !overlap(out, {d.shift, 32}),
                      "an output overlaps an input of the same call");
  }
  BZ_RELEASE_ASSERT(field_id <= 1, "unsupported field id");
}

void check_word_map(const void* mapped, const word_map& m) {
  BZ_RELEASE_ASSERT(m.n >= 1 && m.n <= kMaxWordRows, "the word map needs 1 <= n <= 2^30");
  BZ_RELEASE_ASSERT(m.num_planes >= 1 && m.num_planes <= kMaxWords,
                    "the word map needs 1 <= num_planes <= 32");
  BZ_RELEASE_ASSERT(m.plane_stride >= m.n, "the word map needs plane_stride >= n");
  BZ_RELEASE_ASSERT(m.mapped_stride >= 32 * m.n && m.mapped_stride % 8 == 0,
                    "the word map needs mapped_stride >= 32 n, a multiple of 8");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(mapped) % 8 == 0,
                    "the mapped columns must be 8-byte aligned");
  const byte_range out{mapped, planes_extent(m.num_planes, m.mapped_stride, m.n, 32)};
  BZ_RELEASE_ASSERT(!overlap(out, {m.words, planes_extent(m.num_planes, m.plane_stride, m.n)}) &&
                        !overlap(out, {m.table, 32 * kWordValues}),
                    "an output overlaps an input of the same call");
}

void decompose_words_device(void* words, u64* counts, u64* overflow, unsigned field_id,
                            const word_decomposition& d, hipStream_t stream) {
  with_elements(field_id, [&](auto elements) {
    decompose_enqueue<decltype(elements)>(static_cast<u8*>(words), counts, overflow, d, stream);
  });
}

void map_words_device(void* mapped, const word_map& m, hipStream_t stream) {
  map_enqueue(mapped, m, stream);
}

void decompose_words(api_state& st, void* words, u64* counts, u64* overflow, unsigned field_id,
                     const word_decomposition& d) {
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    u8* host_words = static_cast<u8*>(words);
    if (st.backend != 2) {
      decompose_host<E>(host_words, counts, overflow, d);
      return;
    }
    // the column up at its own width, the device form, the results down: every plane is a buffer
    // of its own, so the caller's bytes between n and plane_stride are not touched
    host_call call{st};
    const size_t n = d.column.n, column_bytes = n * d.column.nbytes;
    u8* d_planes[kMaxWords] = {};
    u64 *d_counts, *d_overflow;
    word_decomposition staged = d;
    for (u32 k = 0; k < d.num_words; ++k) {
      call.output(&d_planes[k], host_words != nullptr ? host_words + k * d.plane_stride : nullptr, n);
    }
    call.output(&d_counts, counts, 8 * kWordValues);
    call.output(&d_overflow, overflow, 8);
    call.input(&staged.shift, d.shift, 32);
    call.input(&staged.column.data, column_bytes != 0 ? d.column.data : nullptr, column_bytes);
    call.allocate();
    // consecutive declarations of one size lie one padded size apart
    if (d.num_words > 1 && host_words != nullptr) staged.plane_stride = d_planes[1] - d_planes[0];
    decompose_enqueue<E>(d_planes[0], d_counts, d_overflow, staged, call.stream());
    call.finish();
  });
}

void map_words(api_state& st, void* mapped, const word_map& m) {
  if (st.backend != 2) {
    model_map(mapped, m);
    return;
  }
  // planes and mapped columns as buffers of their own: the gaps of the caller's strides stay
  host_call call{st};
  const u8* d_planes[kMaxWords] = {};
  u8* d_mapped[kMaxWords] = {};
  word_map staged = m;
  for (u32 k = 0; k < m.num_planes; ++k) {
    call.input(&d_planes[k], static_cast<const u8*>(m.words) + k * m.plane_stride, m.n);
  }
  for (u32 k = 0; k < m.num_planes; ++k) {
    call.output(&d_mapped[k], static_cast<u8*>(mapped) + k * m.mapped_stride, 32 * m.n);
  }
  call.input(&staged.table, m.table, 32 * kWordValues);
  call.allocate();
  staged.words = d_planes[0];
  if (m.num_planes > 1) {
    staged.plane_stride = d_planes[1] - d_planes[0];
    staged.mapped_stride = d_mapped[1] - d_mapped[0];
  }
  map_enqueue(d_mapped[0], staged, call.stream());
  call.finish();
}
} // namespace bz::proof
