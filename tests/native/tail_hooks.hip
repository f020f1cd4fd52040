// Test-only device hooks for the two kernels that end every variable-base MSM: k_reduce /
// k_reduce_compact and k_horner of msm/kernels.h, included unchanged and instantiated exactly as
// msm/engine.h launches them, so that tests/test_msm_tails_device.py can hand them plain arrays of
// points and offsets and compare the result with integers (tests/tail_cases.py).  Sibling of
// device_hooks.hip: compiled once per curve family by tests/tail_hooks.py with the flags of
// msm/msm_curve25519.hip or msm/msm_<curve>.hip and linked into a library of its own.
//     -DBZ_DH_TAG=<name>    suffix of the entry points
//     -DBZ_DH_C=<msm trait> ed25519_msm, bn254_msm, grumpkin_msm, bls12_381_msm
//     -DBZ_DH_SW_BLS=1      bls12-381: the define its product translation units set
//
// Entry points (host pointers; they allocate, copy, launch, synchronise and return the HIP status, or
// -3 before anything is launched when a parameter is out of range):
//     bz_dh_reduce_<tag>, bz_dh_horner_<tag>, bz_dh_heads_of_<tag>
// and bz_dh_tail_sizes_<tag>, which reports the trait's sizes and launches nothing.
// No kernel forms an address from unchecked input: task_desc and column_desc are built HERE from
// scalar parameters, and every range a kernel would index -- bucket offsets, head partials, partial
// slots, the grid -- is checked against the arrays supplied.  The output arrays (partials,
// task_total, out, state) are copied to the device as the caller filled them, so a slot the kernel
// does not write keeps the caller's sentinel.
#if defined(BZ_DH_SW_BLS)
#define BZ_MONT29_MAD_MODE 1 // as msm_bls12_381.hip
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "blitzar_amd/csrc/msm/kernels.h"

#define BZ_DH_CAT2(a, b) a##b
#define BZ_DH_CAT(a, b) BZ_DH_CAT2(a, b)

namespace bz {
namespace BZ_DH_CAT(dh_tails_, BZ_DH_TAG) {

using C = BZ_DH_C;
using point = typename C::point;
constexpr u32 kPointWords = sizeof(point) / 4;
constexpr u32 kMaxTasks = 1024, kMaxStride = 4096, kMaxColumns = 1024, kMaxLanes = 1u << 16;
constexpr u32 kMaxBuckets = 1u << 20, kMaxEntries = 1u << 26, kMaxWindowBits = 21, kHeadsReturned = 24;
static_assert(sizeof(point) % 4 == 0);

// k_reduce launches of engine.h: 0 k_reduce<C, true>, 1 k_reduce<C, true, 64>, 2 k_reduce<C, false>,
// 3 k_reduce<C, false, 64>, 4 k_reduce_compact<C>.  A curve whose trait keeps the scan for every
// launch (reduce_scan_few_columns_only = false) is never launched with Scan = false.
constexpr bool kHasNoScan = !C::has_wave_add_multiple || C::reduce_scan_few_columns_only;
static_assert(C::has_wave_add_multiple, "the scan variants are what engine.h launches for this trait");

bool variant_valid(u32 v) { return v == 0 || v == 1 || v == 4 || (kHasNoScan && (v == 2 || v == 3)); }
u32 variant_lanes(u32 v) { return v == 1 || v == 3 ? 64u : 256u; }

struct range {
  u64 lo, hi;
};
// half-open ranges, pairwise disjoint
bool disjoint(std::vector<range> r) {
  std::sort(r.begin(), r.end(), [](const range& a, const range& b) { return a.lo < b.lo; });
  for (size_t i = 1; i < r.size(); ++i) {
    if (r[i].lo < r[i - 1].hi) return false;
  }
  return true;
}

struct buffers {
  std::vector<void*> held;
  ~buffers() {
    for (void* p : held) (void)hipFree(p);
  }
  // a device copy of `words` 32-bit words (at least one, so that no launch sees a null pointer)
  hipError_t upload(u32** dev, const void* host, u64 words) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (words == 0 ? 1 : words) * 4);
    if (e != hipSuccess) return e;
    held.push_back(p);
    *dev = static_cast<u32*>(p);
    return words == 0 ? hipSuccess : hipMemcpy(p, host, words * 4, hipMemcpyHostToDevice);
  }
};

// task_params: per task {num_buckets, segment_log2, bucket_base, segment_base}
int reduce(u32 variant, u32 lane_log2, u32 num_tasks, const u32* task_params, const u32* bucket_end,
           const u32* bucket_sums, u64 num_buckets_total, const u32* heads, u64 num_heads,
           u32 partial_stride, u32* partials, u32* task_total) {
  if (!variant_valid(variant) || lane_log2 > 6) return -3;
  if (num_tasks == 0 || num_tasks > kMaxTasks || partial_stride == 0 || partial_stride > kMaxStride) return -3;
  if (num_buckets_total > (1u << 24) || num_heads > (1u << 24)) return -3;
  const u32 block_buckets = variant_lanes(variant) << lane_log2;
  std::vector<task_desc> tasks(num_tasks);
  std::vector<range> bucket_ranges, segment_ranges;
  for (u32 t = 0; t < num_tasks; ++t) {
    const u32 nb = task_params[4 * t], seg_log2 = task_params[4 * t + 1];
    const u64 bucket_base = task_params[4 * t + 2], segment_base = task_params[4 * t + 3];
    if (nb == 0 || nb > kMaxBuckets || seg_log2 < 3 || seg_log2 > 7) return -3;
    if (bucket_base + nb > num_buckets_total) return -3;
    const u32* ends = bucket_end + bucket_base;
    for (u32 b = 1; b < nb; ++b) {
      if (ends[b] < ends[b - 1]) return -3;
    }
    const u32 total = ends[nb - 1];
    if (total > kMaxEntries) return -3;
    const u64 segments = (total >> seg_log2) + 2; // the head slots k_accumulate's lanes would own
    if (segment_base + segments > num_heads) return -3;
    if ((nb + block_buckets - 1) / block_buckets > partial_stride) return -3; // the grid covers every block
    bucket_ranges.push_back({bucket_base, bucket_base + nb});
    segment_ranges.push_back({segment_base, segment_base + segments});
    task_desc& d = tasks[t];
    d = task_desc{};
    d.num_buckets = nb;
    d.segment_log2 = seg_log2;
    d.bucket_base = bucket_base;
    d.segment_base = segment_base;
  }
  if (!disjoint(bucket_ranges) || !disjoint(segment_ranges)) return -3;

  buffers dev;
  u32 *d_tasks, *d_ends, *d_sums, *d_heads, *d_partials, *d_total;
  const u64 partial_words = static_cast<u64>(num_tasks) * partial_stride * kPointWords;
  hipError_t e = dev.upload(&d_tasks, tasks.data(), tasks.size() * sizeof(task_desc) / 4);
  if (e == hipSuccess) e = dev.upload(&d_ends, bucket_end, num_buckets_total);
  if (e == hipSuccess) e = dev.upload(&d_sums, bucket_sums, num_buckets_total * kPointWords);
  if (e == hipSuccess) e = dev.upload(&d_heads, heads, num_heads * kPointWords);
  if (e == hipSuccess) e = dev.upload(&d_partials, partials, partial_words);
  if (e == hipSuccess) e = dev.upload(&d_total, task_total, num_tasks);
  if (e != hipSuccess) return static_cast<int>(e);
  const dim3 grid(partial_stride, num_tasks);
  auto launch = [&](auto kernel, u32 lanes) {
    hipLaunchKernelGGL(kernel, grid, dim3(lanes), 0, 0, reinterpret_cast<point*>(d_partials), partial_stride,
                       d_total, reinterpret_cast<const point*>(d_sums), reinterpret_cast<const point*>(d_heads),
                       d_ends, reinterpret_cast<const task_desc*>(d_tasks), lane_log2);
  };
  if (variant == 0) {
    launch(k_reduce<C, true>, kReduceThreads);
  } else if (variant == 1) {
    launch(k_reduce<C, true, 64>, 64);
  } else if (variant == 4) {
    launch(k_reduce_compact<C>, kReduceThreads);
  } else if constexpr (kHasNoScan) {
    if (variant == 2) {
      launch(k_reduce<C, false>, kReduceThreads);
    } else {
      launch(k_reduce<C, false, 64>, 64);
    }
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(partials, d_partials, partial_words * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(task_total, d_total, num_tasks * 4, hipMemcpyDeviceToHost);
  return static_cast<int>(e);
}

// column_params: per column {first_task, window_bits, num_tasks}.  partials == nullptr: the engine's
// launch for a call whose columns are all empty (no task, null partials, null task_total, null state)
int horner(u32 lanes, u32 num_columns, const u32* column_params, const u32* partials, u64 num_partials,
           u32 partial_stride, const u32* task_total, u32 num_tasks, u32 w_lo, u32 w_hi, u32 first, u32 last,
           u32 projective_out, u32 reduce_block_log2, u32* state, u8* out) {
  if (lanes != 64 && lanes != 256) return -3;
  if (num_columns == 0 || num_columns > kMaxColumns || first > 1 || last > 1 || projective_out > 1) return -3;
  if (partial_stride == 0 || partial_stride > kMaxStride || num_tasks > kMaxTasks) return -3;
  if (reduce_block_log2 < 6 || reduce_block_log2 > 14) return -3; // 64 x 2^0 .. 256 x 2^6 buckets
  if (num_partials != static_cast<u64>(num_tasks) * partial_stride) return -3;
  const bool null_launch = partials == nullptr;
  if (null_launch && (num_tasks != 0 || first != 1 || last != 1)) return -3;
  std::vector<column_desc> columns(num_columns);
  std::vector<range> task_ranges;
  for (u32 c = 0; c < num_columns; ++c) {
    const u32 first_task = column_params[3 * c], window_bits = column_params[3 * c + 1];
    const u32 tasks_of_column = column_params[3 * c + 2];
    if (window_bits < 1 || window_bits > kMaxWindowBits) return -3;
    if (tasks_of_column > lanes) return -3; // W <= T windows
    if (static_cast<u64>(first_task) + tasks_of_column > num_tasks) return -3;
    const u32 nb = 1u << (window_bits - 1);
    const u32 blocks = (nb + (1u << reduce_block_log2) - 1) >> reduce_block_log2;
    if (tasks_of_column != 0 && blocks > partial_stride) return -3;
    if (tasks_of_column != 0) task_ranges.push_back({first_task, static_cast<u64>(first_task) + tasks_of_column});
    column_desc& d = columns[c];
    d = column_desc{};
    d.window_bits = window_bits;
    d.num_windows = tasks_of_column;
    d.first_task = first_task;
    d.num_tasks = tasks_of_column;
  }
  if (!disjoint(task_ranges)) return -3;

  const u32 out_stride = projective_out ? C::projective_size : C::output_size;
  buffers dev;
  u32 *d_columns, *d_out, *d_partials = nullptr, *d_total = nullptr, *d_state = nullptr, *d_tasks = nullptr;
  const u64 out_words = static_cast<u64>(num_columns) * out_stride / 4;
  static_assert(C::projective_size % 4 == 0 && C::output_size % 4 == 0);
  hipError_t e = dev.upload(&d_columns, columns.data(), columns.size() * sizeof(column_desc) / 4);
  if (e == hipSuccess) e = dev.upload(&d_out, out, out_words);
  if (!null_launch) {
    const std::vector<task_desc> tasks(num_tasks == 0 ? 1 : num_tasks, task_desc{});
    if (e == hipSuccess) e = dev.upload(&d_tasks, tasks.data(), tasks.size() * sizeof(task_desc) / 4);
    if (e == hipSuccess) e = dev.upload(&d_partials, partials, num_partials * kPointWords);
    if (e == hipSuccess) e = dev.upload(&d_total, task_total, num_tasks);
    if (e == hipSuccess) e = dev.upload(&d_state, state, static_cast<u64>(num_columns) * kPointWords);
  }
  if (e != hipSuccess) return static_cast<int>(e);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(num_columns), dim3(lanes), 0, 0, reinterpret_cast<u8*>(d_out), out_stride,
                       static_cast<int>(projective_out), reinterpret_cast<point*>(d_state),
                       reinterpret_cast<const point*>(d_partials), partial_stride,
                       reinterpret_cast<const column_desc*>(d_columns), reinterpret_cast<const task_desc*>(d_tasks),
                       d_total, w_lo, w_hi, static_cast<int>(first), static_cast<int>(last), reduce_block_log2);
  };
  if (lanes == 64) {
    launch(k_horner<C, 64>);
  } else {
    launch(k_horner<C>);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_words * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && !null_launch) {
    e = hipMemcpy(state, d_state, static_cast<u64>(num_columns) * kPointWords * 4, hipMemcpyDeviceToHost);
  }
  return static_cast<int>(e);
}

// one lane per (begin, end, segment_log2): count, then index(j) for j < min(count, 24), zero beyond
__global__ void __launch_bounds__(64) k_heads_of(const u32* in, u32* out, u32 lanes) {
  const u32 t = blockIdx.x * 64 + threadIdx.x;
  if (t >= lanes) return;
  const bucket_heads h = heads_of(in[3 * t], in[3 * t + 1], in[3 * t + 2]);
  u32* o = out + static_cast<size_t>(t) * (1 + kHeadsReturned);
  o[0] = h.count;
  for (u32 j = 0; j < kHeadsReturned; ++j) o[1 + j] = j < h.count ? h.index(j) : 0;
}

int heads_of_lanes(const u32* in, u32 lanes, u32* out) {
  if (lanes == 0 || lanes > kMaxLanes) return -3;
  for (u32 t = 0; t < lanes; ++t) {
    if (in[3 * t] >= in[3 * t + 1] || in[3 * t + 2] < 3 || in[3 * t + 2] > 7) return -3;
  }
  buffers dev;
  u32 *d_in, *d_out;
  const u64 out_words = static_cast<u64>(lanes) * (1 + kHeadsReturned);
  hipError_t e = dev.upload(&d_in, in, static_cast<u64>(lanes) * 3);
  if (e == hipSuccess) e = dev.upload(&d_out, out, out_words);
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(k_heads_of, dim3((lanes + 63) / 64), dim3(64), 0, 0, d_in, d_out, lanes);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_words * 4, hipMemcpyDeviceToHost);
  return static_cast<int>(e);
}
} // namespace dh_tails_<tag>
} // namespace bz

extern "C" {
int BZ_DH_CAT(bz_dh_reduce_, BZ_DH_TAG)(bz::u32 variant, bz::u32 lane_log2, bz::u32 num_tasks,
                                        const bz::u32* task_params, const bz::u32* bucket_end,
                                        const bz::u32* bucket_sums, bz::u64 num_buckets_total,
                                        const bz::u32* heads, bz::u64 num_heads, bz::u32 partial_stride,
                                        bz::u32* partials, bz::u32* task_total) {
  return bz::BZ_DH_CAT(dh_tails_, BZ_DH_TAG)::reduce(variant, lane_log2, num_tasks, task_params, bucket_end,
                                                     bucket_sums, num_buckets_total, heads, num_heads,
                                                     partial_stride, partials, task_total);
}
int BZ_DH_CAT(bz_dh_horner_, BZ_DH_TAG)(bz::u32 lanes, bz::u32 num_columns, const bz::u32* column_params,
                                        const bz::u32* partials, bz::u64 num_partials, bz::u32 partial_stride,
                                        const bz::u32* task_total, bz::u32 num_tasks, bz::u32 w_lo, bz::u32 w_hi,
                                        bz::u32 first, bz::u32 last, bz::u32 projective_out,
                                        bz::u32 reduce_block_log2, bz::u32* state, bz::u8* out) {
  return bz::BZ_DH_CAT(dh_tails_, BZ_DH_TAG)::horner(lanes, num_columns, column_params, partials, num_partials,
                                                     partial_stride, task_total, num_tasks, w_lo, w_hi, first,
                                                     last, projective_out, reduce_block_log2, state, out);
}
int BZ_DH_CAT(bz_dh_heads_of_, BZ_DH_TAG)(const bz::u32* in, bz::u32 lanes, bz::u32* out) {
  return bz::BZ_DH_CAT(dh_tails_, BZ_DH_TAG)::heads_of_lanes(in, lanes, out);
}
// words of the trait's point, bytes of its encoded and projective outputs, 1 when Scan = false is launched
void BZ_DH_CAT(bz_dh_tail_sizes_, BZ_DH_TAG)(bz::u32* sizes) {
  using namespace bz::BZ_DH_CAT(dh_tails_, BZ_DH_TAG);
  sizes[0] = kPointWords;
  sizes[1] = C::output_size;
  sizes[2] = C::projective_size;
  sizes[3] = kHasNoScan ? 1 : 0;
}
}
