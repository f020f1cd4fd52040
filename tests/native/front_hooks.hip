// Test-only device hooks for the front of every variable-base MSM: the recode kernels (k_recode,
// k_recode_rows32_c16, k_recode_packed) and the two-pass bucket sort (k_group_hist, k_group_scatter,
// k_group_sort_all, k_task_sort) of msm/kernels.h, included unchanged together with the planner of
// msm/plan.h and launched exactly as msm/engine.h launches them, so that
// tests/test_msm_front_device.py can compare every array the front hands to k_accumulate -- and
// every intermediate -- with the integer model of tests/front_cases.py.  Sibling of tail_hooks.hip.
// The front kernels depend on the digit type only, not on a curve: ONE object, compiled by
// tests/front_hooks.py with the flags of msm/msm_curve25519.hip.
//
// Entry points (host pointers; they allocate, copy, launch, synchronise and return the HIP status, or
// -3 before anything is launched when a parameter is outside the contract):
//     bz_fh_front   scalars in, driven by make_msm_plan and packed_recode_ranges
//     bz_fh_sort    explicit task geometry and stored digits in: the sort alone
// Both fill `plan_words` / `task_words` (and bz_fh_front `column_words`) with the descriptors as plain
// 64-bit words, so that Python never guesses a struct layout; with plan_only = 1 they do that and
// nothing else (no device is touched), which is how the caller learns the sizes of the output
// arrays.  Every output array is copied to the device as the caller filled it, so a word the
// kernels do not write keeps the caller's sentinel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "blitzar_amd/csrc/msm/kernels.h"
#include "blitzar_amd/csrc/msm/plan.h"

namespace bz {
namespace fh {

constexpr u64 kMaxColumns = 4096, kMaxRows = u64{1} << 22, kMaxEntries = u64{1} << 26;
constexpr u64 kMaxBuckets = u64{1} << 26, kMaxTasks = 65000, kMaxGeneratorOffset = u64{1} << 30;
constexpr u32 kMaxLdsGroups = 32768; // one LDS counter per group in pass 1: 128 KiB of the 140 allowed
constexpr u32 kPlanWords = 24, kColumnWords = 8, kTaskWords = 16;

struct buffers {
  std::vector<void*> held;
  ~buffers() {
    for (void* p : held) (void)hipFree(p);
  }
  // `bytes` of device memory holding what `host` holds (at least 16 bytes, never a null pointer)
  hipError_t upload(void** dev, const void* host, u64 bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes < 16 ? 16 : bytes);
    if (e != hipSuccess) return e;
    held.push_back(p);
    *dev = p;
    return bytes == 0 || host == nullptr ? hipSuccess : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
  }
};

// what engine.h reads off an msm_plan between its lines 872 and 969
struct geometry {
  std::vector<column_desc> columns;
  std::vector<task_desc> tasks;
  std::vector<recode_range> ranges;
  u64 total_entries = 0, total_groups = 0, total_buckets = 0, total_segments = 0;
  u64 max_task_rows = 0, max_recode_rows = 0, max_rows = 0;
  u32 max_task_groups = 0, max_task_slices = 0, max_slice_rows = 0;
  bool wide_digits = false;
  bool recode = true; // false: the digits are the caller's (bz_fh_sort)
};

// the kernels engine.h would launch for the geometry
struct choice {
  u32 recoder = 0; // 0 k_recode<D>, 1 k_recode_rows32_c16, 2 k_recode_packed<D>, 3 none
  bool small_tasks = false, staged = false;
  u32 stream_limit = 0;
  u64 zero_words = 0;
};

// host arrays of the caller, filled with its sentinel
struct outputs {
  void* digits;        // D [total_entries + 8]
  u32* zeroed;         // [zeroed_block_words]
  u32* group_start;    // [total_groups + 1]
  u32* group_chunk;    // [total_groups + 1]
  u32* records;        // [total_entries + 8]
  u32* sorted;         // [total_entries + 8]
  u32* bucket_end;     // [total_buckets + 1]
  u32* segment_bucket; // [total_segments + 1]
};

// engine.h:467, restated: cursors [total_groups + 1] | tickets [tasks] | barrier [1] | big_tasks [1 + tasks]
size_t zeroed_block_words(u64 total_groups, size_t num_tasks) {
  return static_cast<size_t>(total_groups) + 1 + num_tasks + 1 + 1 + num_tasks;
}

bool choose(const geometry& g, u32 stream_mode, choice& ch) {
  const size_t num_tasks = g.tasks.size();
  // engine.h:873
  ch.zero_words = g.total_groups + 1 + num_tasks + 2;
  // engine.h:876-883: the common shape has a recode kernel of its own
  bool rows32_c16 = g.columns.size() <= 65535;
  for (const column_desc& c : g.columns) {
    rows32_c16 = rows32_c16 &&
                 (c.n == 0 || (c.bit_offset == 0 && c.bit_width == 256 && c.row_stride == 32 &&
                               c.is_signed == 0 && c.merged_stride == 0 && c.window_bits == 16 &&
                               c.num_windows == 17 && (reinterpret_cast<uintptr_t>(c.data) & 15) == 0));
  }
  // engine.h:905-925: packed when ranges exist, then rows32_c16 (16-bit digits only), else generic
  ch.recoder = !g.recode ? 3u : !g.ranges.empty() ? 2u : (!g.wide_digits && rows32_c16) ? 1u : 0u;
  // engine.h:895-896
  const u32 engine_limit = g.total_entries <= (u64{1} << 22) ? kLocalSortCapacity : kStreamedSortRecords;
  if (stream_mode > 2) return false;
  ch.stream_limit = stream_mode == 0 ? engine_limit : stream_mode == 1 ? kLocalSortCapacity : kStreamedSortRecords;
  // engine.h:899
  ch.small_tasks = g.max_task_groups == 1 && g.max_task_rows <= kLocalSortCapacity;
  // engine.h:939: staged unless some column needs the direct form
  ch.staged = g.max_task_groups <= kMaxStagedGroups && g.max_slice_rows <= kStagedSliceRows;
  return true;
}

// limits of the harness itself (grid dimensions, dynamic LDS, memory)
bool within_limits(const geometry& g) {
  if (g.tasks.empty() || g.tasks.size() > kMaxTasks || g.columns.size() > kMaxColumns) return false;
  if (g.total_entries > kMaxEntries || g.total_buckets > kMaxBuckets) return false;
  if (g.max_task_groups == 0 || g.max_task_groups > kMaxLdsGroups) return false;
  if (g.max_task_slices == 0 || g.max_task_slices > 65535) return false;
  return true;
}

void describe(const geometry& g, const choice& ch, u32 workers, u64* plan_words, u64* task_words) {
  const u64 words[kPlanWords] = {g.tasks.size(),
                                 g.columns.size(),
                                 g.total_entries,
                                 g.total_groups,
                                 g.total_buckets,
                                 g.total_segments,
                                 g.max_task_groups,
                                 g.max_task_slices,
                                 g.max_slice_rows,
                                 g.max_task_rows,
                                 g.max_recode_rows,
                                 g.max_rows,
                                 g.wide_digits ? 1u : 0u,
                                 ch.recoder,
                                 ch.small_tasks ? 1u : 0u,
                                 ch.staged ? 1u : 0u,
                                 ch.stream_limit,
                                 ch.zero_words,
                                 zeroed_block_words(g.total_groups, g.tasks.size()),
                                 g.ranges.size(),
                                 workers, // what k_group_sort_all is handed (0: nothing was launched)
                                 0,
                                 0,
                                 0};
  std::memcpy(plan_words, words, sizeof(words));
  for (size_t t = 0; t < g.tasks.size(); ++t) {
    const task_desc& d = g.tasks[t];
    const u64 w[kTaskWords] = {d.column,     d.window,     d.rows,         d.num_buckets, d.num_slices, d.slice_rows,
                               d.group_bits, d.num_groups, d.segment_log2, d.bucket_base, d.entry_base, d.group_base,
                               d.segment_base, d.row_base, 0, 0};
    std::memcpy(task_words + kTaskWords * t, w, sizeof(w));
  }
}

// the dynamic-LDS attribute, on the kernels of configure_sort_kernels (engine.h:439-454)
hipError_t configure_sort_kernels() {
  static bool done = false;
  if (done) return hipSuccess;
  hipError_t e = hipSuccess;
  auto allow_lds = [&](auto kernel) {
    if (e == hipSuccess) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024);
    }
  };
  allow_lds(k_recode_packed<i16>);
  allow_lds(k_recode_packed<i32>);
  allow_lds(k_group_hist<i16>);
  allow_lds(k_group_hist<i32>);
  allow_lds(k_group_scatter<true, i16>);
  allow_lds(k_group_scatter<true, i32>);
  allow_lds(k_group_scatter<false, i16>);
  allow_lds(k_group_scatter<false, i32>);
  done = e == hipSuccess;
  return e;
}

// engine.h:962-963: min(2 x compute units, kBigSortBlocks); the default stream carries no CU mask
hipError_t engine_workers(u32* workers) {
  int device = 0, cus = 0;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  const u32 usable = cus > 0 ? static_cast<u32>(cus) : 1;
  *workers = 2 * usable < kBigSortBlocks ? 2 * usable : kBigSortBlocks;
  return e;
}

// The launches of engine.h:901-969 on the default stream.  `d_columns`' data pointers are device
// pointers already.  stage: 1 recode only, 2 + k_group_hist and k_group_scatter, 3 everything.
template <class D>
void launch_front(const geometry& g, const choice& ch, u32 stage, u32 workers, D* digits,
                  const column_desc* cols, const task_desc* tasks, const recode_range* d_ranges, u32* zeroed,
                  u32* group_start, u32* group_chunk, u32* records, u32* sorted, u32* bucket_count,
                  u32* bucket_end, u32* segment_bucket) {
  const u32 num_tasks = static_cast<u32>(g.tasks.size());
  const u32 num_cols = static_cast<u32>(g.columns.size());
  // engine.h:801-806
  u32* group_cursor = zeroed;
  u32* arrivals = group_cursor + g.total_groups + 1;
  u32* big_barrier = arrivals + num_tasks;
  u32* big_tasks = big_barrier + 1;
  // engine.h:842
  const size_t part_lds = sizeof(u32) * g.max_task_groups;
  if (ch.recoder == 2) { // engine.h:905-912
    hipLaunchKernelGGL((k_recode_packed<D>), dim3(ceil_div_u32(g.max_recode_rows, kPackedTileRows)),
                       dim3(kPackedRecodeThreads), kPackedTileBytes, 0, digits, cols, tasks, d_ranges,
                       static_cast<u32>(g.ranges.size()), g.columns[0].row_stride, g.max_recode_rows,
                       g.max_rows, group_cursor, ch.zero_words);
  } else if (ch.recoder != 3) { // engine.h:914-925
    const u32 chunks = ceil_div_u32(g.max_recode_rows, 256);
    bool launched = false;
    if constexpr (sizeof(D) == 2) {
      if (ch.recoder == 1) {
        hipLaunchKernelGGL(k_recode_rows32_c16, dim3(chunks, num_cols), dim3(256), 0, 0, digits, cols, tasks,
                           group_cursor, ch.zero_words);
        launched = true;
      }
    }
    if (!launched) {
      const u64 items = 8 * static_cast<u64>((chunks + 7) / 8) * num_cols;
      const u32 recode_blocks = static_cast<u32>(items < (u64{1} << 30) ? items : (u64{1} << 30));
      hipLaunchKernelGGL((k_recode<D>), dim3(recode_blocks), dim3(256), 0, 0, digits, cols, tasks, num_cols,
                         chunks, group_cursor, ch.zero_words);
    }
  }
  if (stage < 2) return;
  u32* bucket_fill = bucket_count + g.total_buckets + 1; // engine.h:933
  if (ch.small_tasks) {                                   // engine.h:928-931: one launch instead of three
    if (stage < 3) return;
    hipLaunchKernelGGL((k_task_sort<D>), dim3(num_tasks), dim3(kGroupSortThreads), 0, 0, sorted, segment_bucket,
                       bucket_end, digits, tasks);
    return;
  }
  // engine.h:935-937
  hipLaunchKernelGGL((k_group_hist<D>), dim3(g.max_task_slices, num_tasks), dim3(kSortThreads), part_lds, 0,
                     group_cursor, big_tasks, digits, tasks, arrivals, group_start, group_chunk, bucket_count,
                     bucket_fill, ch.stream_limit);
  if (ch.staged) { // engine.h:939-948
    const size_t staged_lds = sizeof(u32) * (3 * g.max_task_groups + 1 + kStagedSliceRows);
    hipLaunchKernelGGL((k_group_scatter<true, D>), dim3(g.max_task_slices, num_tasks), dim3(kSortThreads),
                       staged_lds, 0, records, group_cursor, digits, tasks);
  } else {
    hipLaunchKernelGGL((k_group_scatter<false, D>), dim3(g.max_task_slices, num_tasks), dim3(kSortThreads),
                       part_lds, 0, records, group_cursor, digits, tasks);
  }
  if (stage < 3) return;
  // engine.h:964-967
  hipLaunchKernelGGL(k_group_sort_all, dim3(g.max_task_groups, num_tasks + 1), dim3(kGroupSortThreads), 0, 0,
                     sorted, segment_bucket, bucket_end, records, group_start, group_chunk, tasks, num_tasks,
                     bucket_count, bucket_fill, big_tasks, big_barrier, workers);
}

// allocate, upload, launch, synchronise, download.  `digits_in`: the stored digits when g.recode is
// false (already of the launch's digit type, total_entries + 8 of them).
int run(const geometry& g, const choice& ch, u32 stage, u32 max_workers, const outputs& o, buffers& dev,
        const void* digits_in, u64* plan_words, u64* task_words) {
  const size_t num_tasks = g.tasks.size();
  hipError_t e = configure_sort_kernels();
  u32 workers = 0;
  if (e == hipSuccess) e = engine_workers(&workers);
  if (e != hipSuccess) return static_cast<int>(e);
  // never more workers than the engine would pass
  if (max_workers != 0 && max_workers < workers) workers = max_workers;
  const size_t digit_bytes = (g.wide_digits ? sizeof(i32) : sizeof(i16)) * (g.total_entries + 8);
  const size_t entry_bytes = sizeof(u32) * (g.total_entries + 8);
  const size_t zeroed_bytes = sizeof(u32) * zeroed_block_words(g.total_groups, num_tasks);
  const size_t group_bytes = sizeof(u32) * (g.total_groups + 1);
  const size_t bucket_bytes = sizeof(u32) * (g.total_buckets + 1);
  const size_t segment_bytes = sizeof(u32) * (g.total_segments + 1);
  void *d_cols, *d_tasks, *d_ranges = nullptr, *d_digits, *d_zeroed, *d_start, *d_chunk, *d_records, *d_sorted;
  void *d_count, *d_end, *d_segment;
  e = dev.upload(&d_cols, g.columns.data(), sizeof(column_desc) * g.columns.size());
  if (e == hipSuccess) e = dev.upload(&d_tasks, g.tasks.data(), sizeof(task_desc) * num_tasks);
  if (e == hipSuccess && !g.ranges.empty()) {
    e = dev.upload(&d_ranges, g.ranges.data(), sizeof(recode_range) * g.ranges.size());
  }
  if (e == hipSuccess) e = dev.upload(&d_digits, g.recode ? o.digits : digits_in, digit_bytes);
  if (e == hipSuccess) e = dev.upload(&d_zeroed, o.zeroed, zeroed_bytes);
  if (e == hipSuccess) e = dev.upload(&d_start, o.group_start, group_bytes);
  if (e == hipSuccess) e = dev.upload(&d_chunk, o.group_chunk, group_bytes);
  if (e == hipSuccess) e = dev.upload(&d_records, o.records, entry_bytes);
  if (e == hipSuccess) e = dev.upload(&d_sorted, o.sorted, entry_bytes);
  if (e == hipSuccess) e = dev.upload(&d_count, nullptr, 2 * bucket_bytes);
  if (e == hipSuccess) e = hipMemset(d_count, 0xA5, 2 * bucket_bytes); // stale counters, as in an arena
  if (e == hipSuccess) e = dev.upload(&d_end, o.bucket_end, bucket_bytes);
  if (e == hipSuccess) e = dev.upload(&d_segment, o.segment_bucket, segment_bytes);
  // no recode kernel runs: what it would have cleared -- the barrier word of the workers among it --
  // is cleared here, before every launch (with a recode kernel, by that kernel)
  if (e == hipSuccess && !g.recode) e = hipMemset(d_zeroed, 0, sizeof(u32) * ch.zero_words);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return static_cast<int>(e);
  auto go = [&](auto digit_tag) {
    using D = decltype(digit_tag);
    launch_front<D>(g, ch, stage, workers, static_cast<D*>(d_digits), static_cast<const column_desc*>(d_cols),
                    static_cast<const task_desc*>(d_tasks), static_cast<const recode_range*>(d_ranges),
                    static_cast<u32*>(d_zeroed), static_cast<u32*>(d_start), static_cast<u32*>(d_chunk),
                    static_cast<u32*>(d_records), static_cast<u32*>(d_sorted), static_cast<u32*>(d_count),
                    static_cast<u32*>(d_end), static_cast<u32*>(d_segment));
  };
  if (g.wide_digits) { // engine.h:951-955
    go(i32{});
  } else {
    go(i16{});
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(o.digits, d_digits, digit_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.zeroed, d_zeroed, zeroed_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.group_start, d_start, group_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.group_chunk, d_chunk, group_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.records, d_records, entry_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.sorted, d_sorted, entry_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.bucket_end, d_end, bucket_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(o.segment_bucket, d_segment, segment_bytes, hipMemcpyDeviceToHost);
  describe(g, ch, workers, plan_words, task_words);
  return static_cast<int>(e);
}

// params: {num_columns, buffer_bytes, force_window_bits, force_segment_log2, partition_group_entries,
//          table_stride, table_windows, table_bits, force_window_tables, stage, stream_mode, max_workers,
//          plan_only, task_capacity}
// columns: per column {offset into the buffer, n, row_stride, bit_offset, bit_width, is_signed, generator_offset}
int front(const u64* params, const u8* buffer, const u64* columns, u64* plan_words, u64* column_words,
          u64* task_words, const outputs& o) {
  const u64 num_columns = params[0], buffer_bytes = params[1];
  const u64 force_window_bits = params[2], force_segment_log2 = params[3], group_entries = params[4];
  const u64 table_stride = params[5], table_windows = params[6], table_bits = params[7];
  const u64 force_tables = params[8], stage = params[9], stream_mode = params[10], max_workers = params[11];
  const u64 plan_only = params[12], task_capacity = params[13];
  if (num_columns == 0 || num_columns > kMaxColumns || buffer_bytes > (u64{1} << 30)) return -3;
  if (force_window_bits == 1 || force_window_bits > 16) return -3;
  if (force_segment_log2 != 0 && (force_segment_log2 < kSegmentLog2Min || force_segment_log2 > kSegmentLog2Max)) {
    return -3;
  }
  if (group_entries > (u64{1} << 20) || force_tables > 1 || plan_only > 1) return -3;
  if (stage < 1 || stage > 3 || stream_mode > 2 || max_workers > 16) return -3;
  const bool with_table = table_windows != 0;
  if (with_table) {
    if (table_bits < 2 || table_bits > kMaxTableWindowBits || table_windows > 129) return -3;
    if (table_stride == 0 || table_stride % 8 != 0 || table_stride > kMaxRows) return -3;
  }
  bool any_signed = false;
  for (u64 i = 0; i < num_columns; ++i) {
    const u64* c = columns + 7 * i;
    const u64 offset = c[0], n = c[1], row_stride = c[2], bit_offset = c[3], bit_width = c[4];
    if (n > kMaxRows || row_stride > (u64{1} << 20) || bit_offset > 7 || bit_width < 1 || bit_width > 256) return -3;
    if (c[5] > 1 || c[6] > kMaxGeneratorOffset || offset > buffer_bytes) return -3;
    // every byte a recoder reads lies inside the caller's buffer (recode.h: the field's bytes)
    const u64 field_bytes = (bit_offset + bit_width + 7) / 8;
    if (n != 0 && offset + (n - 1) * row_stride + field_bytes > buffer_bytes) return -3;
    any_signed = any_signed || c[5] != 0;
  }
  buffers dev;
  // plan_only: a base with the alignment hipMalloc gives, never dereferenced
  u8* base = reinterpret_cast<u8*>(uintptr_t{1} << 28);
  if (!plan_only) {
    void* p = nullptr;
    const hipError_t e = dev.upload(&p, buffer, buffer_bytes);
    if (e != hipSuccess) return static_cast<int>(e);
    base = static_cast<u8*>(p);
  }
  std::vector<host_column> cols(num_columns);
  for (u64 i = 0; i < num_columns; ++i) {
    const u64* c = columns + 7 * i;
    cols[i] = host_column{base + c[0], c[1], c[2], static_cast<u32>(c[3]), static_cast<u32>(c[4]), c[5] != 0, c[6]};
  }
  msm_tuning tune;
  tune.force_window_bits = static_cast<u32>(force_window_bits);
  tune.force_segment_log2 = static_cast<u32>(force_segment_log2);
  if (group_entries != 0) tune.partition_group_entries = static_cast<u32>(group_entries);
  tune.force_window_tables = force_tables != 0;
  // engine.h:576-577: signed columns use |x| with all digits negated: c <= 15 so that -D fits int16
  if (any_signed && tune.max_window_bits > 15) tune.max_window_bits = 15;
  window_table table;
  table.stride = table_stride;
  table.windows = static_cast<u32>(table_windows);
  table.bits = static_cast<u32>(table_bits);
  // (make_msm_plan aborts on generator_offset + task rows >= 2^31: excluded by the limits above,
  // 2^30 + 129 x 2^22 < 2^31)
  const msm_plan plan = make_msm_plan(cols, tune, with_table ? &table : nullptr);
  geometry g;
  g.columns = plan.columns;
  g.tasks = plan.tasks;
  g.ranges = packed_recode_ranges(plan);
  g.total_entries = plan.total_entries;
  g.total_groups = plan.total_groups;
  g.total_buckets = plan.total_buckets;
  g.total_segments = plan.total_segments;
  g.max_task_rows = plan.max_task_rows;
  g.max_recode_rows = plan.max_recode_rows;
  g.max_rows = plan.max_rows;
  g.max_task_groups = plan.max_task_groups;
  g.max_task_slices = plan.max_task_slices;
  g.max_slice_rows = plan.max_slice_rows;
  g.wide_digits = plan.wide_digits;
  choice ch;
  if (!within_limits(g) || g.tasks.size() > task_capacity || !choose(g, static_cast<u32>(stream_mode), ch)) return -3;
  // k_recode_packed copies a range's span of EVERY row below the longest column's end, whichever
  // columns reach that far: all of it inside the caller's buffer
  for (const recode_range& r : g.ranges) {
    const u64 last_row = g.max_rows == 0 ? 0 : g.max_rows - 1;
    if (static_cast<u64>(r.base - base) + last_row * g.columns[0].row_stride + r.span > buffer_bytes) return -3;
  }
  for (const column_desc& c : g.columns) {
    if (c.is_signed != 0 && c.window_bits > 15) return -3;
    if (c.window_bits > (g.wide_digits ? kMaxTableWindowBits : 16u)) return -3;
  }
  for (u64 i = 0; i < num_columns; ++i) {
    const column_desc& c = g.columns[i];
    const u64 w[kColumnWords] = {c.n, c.window_bits, c.num_windows, c.first_task, c.num_tasks, c.merged_stride,
                                 static_cast<u64>(c.data - base), 0};
    std::memcpy(column_words + kColumnWords * i, w, sizeof(w));
  }
  if (plan_only) {
    describe(g, ch, 0, plan_words, task_words);
    return 0;
  }
  return run(g, ch, static_cast<u32>(stage), static_cast<u32>(max_workers), o, dev, nullptr, plan_words, task_words);
}

// params: {num_tasks, segment_log2, wide_digits, stage, stream_mode, max_workers, plan_only, digits_len}
// tasks:  per task {rows, window_bits, group_bits, slice_rows, row_base}
// digits_in: int32 [digits_len = total_entries + 8], laid out as the planner lays the tasks out (entry
// ranges padded to 8); what lies past a task's rows is handed to the kernels as it is
int sort(const u64* params, const u64* tasks, const i32* digits_in, u64* plan_words, u64* task_words,
         const outputs& o) {
  const u64 num_tasks = params[0], segment_log2 = params[1], wide = params[2], stage = params[3];
  const u64 stream_mode = params[4], max_workers = params[5], plan_only = params[6], digits_len = params[7];
  if (num_tasks == 0 || num_tasks > kMaxTasks || wide > 1 || plan_only > 1) return -3;
  if (segment_log2 < kSegmentLog2Min || segment_log2 > kSegmentLog2Max) return -3;
  if (stage < 2 || stage > 3 || stream_mode > 2 || max_workers > 16) return -3;
  geometry g;
  g.recode = false;
  g.wide_digits = wide != 0;
  g.columns.push_back(column_desc{}); // no kernel of the sort reads a column
  const u64 seg_entries = u64{1} << segment_log2;
  for (u64 t = 0; t < num_tasks; ++t) {
    const u64* p = tasks + 5 * t;
    const u64 rows = p[0], c = p[1], s = p[2], slice_rows = p[3], row_base = p[4];
    if (c < 2 || c > (wide ? kMaxTableWindowBits : 16u) || s > kMaxGroupBits || s > c - 1) return -3;
    // num_groups << group_bits == 2^(c-1)
    const u32 num_groups = 1u << (c - 1 - s);
    if (rows == 0 || rows >= (u64{1} << (31 - s)) || row_base + rows >= (u64{1} << 31)) return -3;
    if (slice_rows != kStagedSliceRows && slice_rows != kDirectSliceRows) return -3;
    if (num_groups <= kMaxStagedGroups && slice_rows != kStagedSliceRows) return -3;
    task_desc d{};
    d.column = 0;
    d.window = static_cast<u32>(t);
    d.rows = rows;
    d.num_buckets = 1u << (c - 1);
    d.slice_rows = static_cast<u32>(slice_rows);
    d.num_slices = static_cast<u32>((rows + slice_rows - 1) / slice_rows);
    d.group_bits = static_cast<u32>(s);
    d.num_groups = num_groups;
    d.segment_log2 = static_cast<u32>(segment_log2);
    d.bucket_base = g.total_buckets;
    d.entry_base = g.total_entries;
    d.group_base = g.total_groups;
    d.segment_base = g.total_segments;
    d.row_base = static_cast<u32>(row_base);
    g.total_buckets += d.num_buckets;
    g.total_entries += (rows + 7) & ~7ull;
    g.total_groups += num_groups + 1;
    g.total_segments += (rows + seg_entries - 1) / seg_entries;
    if (g.total_entries > kMaxEntries || g.total_buckets > kMaxBuckets) return -3;
    g.max_task_rows = std::max(g.max_task_rows, rows);
    g.max_task_groups = std::max(g.max_task_groups, num_groups);
    g.max_task_slices = std::max(g.max_task_slices, d.num_slices);
    g.max_slice_rows = std::max(g.max_slice_rows, d.slice_rows);
    g.tasks.push_back(d);
  }
  choice ch;
  if (!within_limits(g) || !choose(g, static_cast<u32>(stream_mode), ch)) return -3;
  if (plan_only) {
    describe(g, ch, 0, plan_words, task_words);
    return 0;
  }
  if (digits_len != g.total_entries + 8) return -3;
  // every stored digit E of a row satisfies |E| <= 2^(c-1); converted to the launch's digit type
  std::vector<i16> narrow;
  if (!g.wide_digits) narrow.resize(digits_len);
  for (const task_desc& d : g.tasks) {
    const i32 bound = static_cast<i32>(d.num_buckets);
    for (u64 r = 0; r < d.rows; ++r) {
      const i32 e = digits_in[d.entry_base + r];
      if (e > bound || e < -bound || (!g.wide_digits && e == 32768)) return -3;
    }
  }
  if (!g.wide_digits) {
    for (u64 i = 0; i < digits_len; ++i) narrow[i] = static_cast<i16>(digits_in[i]);
  }
  buffers dev;
  return run(g, ch, static_cast<u32>(stage), static_cast<u32>(max_workers), o, dev,
             g.wide_digits ? static_cast<const void*>(digits_in) : static_cast<const void*>(narrow.data()),
             plan_words, task_words);
}
} // namespace fh
} // namespace bz

extern "C" {
int bz_fh_front(const bz::u64* params, const bz::u8* buffer, const bz::u64* columns, bz::u64* plan_words,
                bz::u64* column_words, bz::u64* task_words, void* digits, bz::u32* zeroed, bz::u32* group_start,
                bz::u32* group_chunk, bz::u32* records, bz::u32* sorted, bz::u32* bucket_end,
                bz::u32* segment_bucket) {
  const bz::fh::outputs o{digits, zeroed, group_start, group_chunk, records, sorted, bucket_end, segment_bucket};
  return bz::fh::front(params, buffer, columns, plan_words, column_words, task_words, o);
}
int bz_fh_sort(const bz::u64* params, const bz::u64* tasks, const bz::i32* digits_in, bz::u64* plan_words,
               bz::u64* task_words, void* digits, bz::u32* zeroed, bz::u32* group_start, bz::u32* group_chunk,
               bz::u32* records, bz::u32* sorted, bz::u32* bucket_end, bz::u32* segment_bucket) {
  const bz::fh::outputs o{digits, zeroed, group_start, group_chunk, records, sorted, bucket_end, segment_bucket};
  return bz::fh::sort(params, tasks, digits_in, plan_words, task_words, o);
}
// {words of a plan, of a column, of a task description; kLocalSortCapacity; kStreamedSortRecords;
//  kMaxStagedGroups; kStagedSliceRows; kBigSortBlocks}
void bz_fh_constants(bz::u32* out) {
  out[0] = bz::fh::kPlanWords;
  out[1] = bz::fh::kColumnWords;
  out[2] = bz::fh::kTaskWords;
  out[3] = bz::kLocalSortCapacity;
  out[4] = bz::kStreamedSortRecords;
  out[5] = bz::kMaxStagedGroups;
  out[6] = bz::kStagedSliceRows;
  out[7] = bz::kBigSortBlocks;
}
}
