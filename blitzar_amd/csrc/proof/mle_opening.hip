// From the sumcheck's outputs to the inner-product prover's inputs (bzamd_mle_evaluation_vector*,
// bzamd_combine_columns*), both exact and both enqueue-only in their device forms.
//
// The evaluation vector.  vector[i] = prod_t (bit_{v-1-t}(i) ? r_t : 1 - r_t): bit b of the row
// index belongs to r_{v-1-b}, the bit order of the prover's fold (round 0 binds the top bit).  One
// product per challenge and row would be v Montgomery products per 32-byte store.  Instead the
// index is split into three bit fields,
//   low  = bits [0, lb)          lb = min(v, kLowBits)
//   mid  = bits [lb, lb + mb)    mb = min(v - lb, kMidBits)
//   high = bits [lb + mb, v)
// and a workgroup holds in LDS the table of the low field (2^lb elements) and of the mid field
// (2^mb), each built by doubling: the table over one bit more is [T (1 - r), T r], and T (1 - r) =
// T - T r, so a table of 2^k entries costs 2^k - 1 products.  A tile is the 2^(lb + mb) consecutive
// rows that share their high field; workgroups walk tiles grid-stride.  Per tile 2^mb lanes make
// pm[m] = mid[m] * (the high field's factors), hb products each, and a row is then the ONE product
// pm[mid(i)] * low[low(i)] plus the product inside E::store that leaves the engine's Montgomery
// form.  With lb = mb = 5 (tiles of 1024 rows, four rows per lane) that is per output element
//   1 + 32 hb / 1024 + 1 (store)  =  2.19 at v = 16,  2.31 at v = 20,  2.63 at v = 30
// plus the workgroup's tables and challenges (62 + v products) over the rows it writes (at least
// one tile: < 0.1).  No array is indexed at run time outside LDS: no scratch memory.  LDS: the two
// tables, pm and the challenges, (3 * 32 + 30) * 36 = 4536 bytes, which does not bound occupancy;
// larger fields (6 + 6) would save 0.1 products per element and leave 16 tiles, so 16 workgroups,
// at n = 2^16.
//
// The combination.  One row per lane; a row of column j is fetched as the raw residue of its bytes
// (load_raw, proof/sumcheck_columns.h), and the coefficient carries the conversion constant of the
// column's kind, multiplied in once per workgroup while the coefficients go to LDS: a row costs one
// product and one lazy addition per column (normalised and reduced every fourth).  The views
// travel as kernel arguments, kCombineChunk at a time; a call with more columns launches the kernel
// once per chunk and the later launches add to what `combined` holds, which is exact.  So the call
// needs no memory beside its operands, however many columns it takes.
//
// The evaluation (bzamd_evaluate_columns*): evaluations[j] = <column_j, vector>, the producer of
// the combination's `evaluations` for columns the sumcheck did not multiply.  Rows go to lanes
// grid-stride; a lane fetches vector[i] once, as the raw residue of its 32 bytes, and multiplies
// it into the raw row of each of the launch's kEvaluateChunk columns, one accumulator per column in
// registers.  Neither operand is converted: the Montgomery product of two raw residues is short of
// conversion(column's kind) * conversion(element) / R^2, one constant per column, which the finish
// multiplies in once.  The additions are lazy, swept and reduced every kEvaluateSweep rows.  A
// workgroup reduces each column in LDS and writes one partial per column to the caller's
// workspace; k_evaluate_finish, one workgroup per column, adds a column's partials, applies the
// constant and stores the bytes.  A call with more columns than a chunk launches the partial
// kernel once per chunk and reads the vector again each time: 32 bytes a row and chunk, 4 bytes a
// row and column at kEvaluateChunk = 8.
#include "blitzar_amd/csrc/proof/mle_opening.h"

#include <cstring>
#include <utility>
#include <vector>

#include "blitzar_amd/csrc/proof/host_call.h"
#include "blitzar_amd/csrc/proof/sumcheck_columns.h"

namespace bz::proof {
namespace {
constexpr u32 kLowBits = 5, kMidBits = 5;
constexpr u32 kVectorThreads = 256;
constexpr u32 kVectorBlocks = 2048; // 8 workgroups per CU: one wave per SIMD and workgroup, 2 deep
constexpr u32 kMaxVariables = 30;

constexpr u32 kCombineChunk = 32; // views per launch: 1 KiB of kernel arguments
constexpr u32 kCombineThreads = 256;
constexpr u32 kCombineBlocks = 4096;

// columns whose accumulators one lane holds (72 registers): the most that leaves two wavefronts per
// SIMD without scratch memory (249 / 227 VGPRs; 4: 148 / 126, 12 and more: one wavefront)
constexpr u32 kEvaluateChunk = 8;
constexpr u32 kEvaluateThreads = 256;
constexpr u32 kEvaluateBlocks = 1024; // 4 workgroups per CU: twice what is resident
constexpr u32 kEvaluateSweep = 4;     // rows a lane adds lazily between two carry sweeps

struct vector_split {
  u32 lb, mb, hb;
};
BZ_HD vector_split split_of(u32 num_variables) {
  const u32 lb = num_variables < kLowBits ? num_variables : kLowBits;
  const u32 mb = num_variables - lb < kMidBits ? num_variables - lb : kMidBits;
  return {lb, mb, num_variables - lb - mb};
}

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
template <class E>
__global__ void __launch_bounds__(kVectorThreads)
    k_mle_evaluation_vector(u64* __restrict__ vector, const u8* __restrict__ point,
                            u32 num_variables, u64 n) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe rs[kMaxVariables];      // r_t, engine form
  __shared__ fe tables[2][1u << kLowBits]; // [0]: the low field's, [1]: the mid field's
  __shared__ fe pm[1u << kMidBits];     // the tile's high-field product times the mid table
  const vector_split s = split_of(num_variables);
  const u32 t = threadIdx.x;
  if (t < num_variables) rs[t] = E::load(point + 32 * t);
  if (t == 0 || t == 32) tables[t >> 5][0] = F::one();
  __syncthreads();
  // both tables by doubling, lanes 0 .. 31 the low one and 32 .. 63 the mid one: step b appends bit
  // b of the field, whose challenge is r_{v-1-b} (low) or r_{v-1-lb-b} (mid)
  for (u32 b = 0; b < s.lb; ++b) {
    const u32 which = t >> 5, k = t & 31;
    if (t < 64 && k < (1u << b) && b < (which == 0 ? s.lb : s.mb)) {
      const fe r = rs[num_variables - 1 - (which == 0 ? 0 : s.lb) - b];
      const fe low = tables[which][k];
      const fe high = F::mul(low, r);
      tables[which][k + (1u << b)] = high;
      tables[which][k] = fsub<F>(low, high);
    }
    __syncthreads();
  }
  const u32 tile_bits = s.lb + s.mb;
  const u64 tile_rows = u64{1} << tile_bits;
  const u64 num_tiles = (n + tile_rows - 1) >> tile_bits;
  for (u64 h = blockIdx.x; h < num_tiles; h += gridDim.x) {
    if (t < (1u << s.mb)) {
      // bit b of h is bit lb + mb + b of the row: r_{hb-1-b}
      fe p = tables[1][t];
      for (u32 b = 0; b < s.hb; ++b) {
        const fe r = rs[s.hb - 1 - b];
        p = F::mul(p, ((h >> b) & 1) != 0 ? r : fsub<F>(F::one(), r));
      }
      pm[t] = p;
    }
    __syncthreads();
    for (u64 x = t; x < tile_rows; x += kVectorThreads) {
      const u64 i = (h << tile_bits) + x;
      if (i < n) {
        const fe value = F::mul(pm[x >> s.lb], tables[0][x & ((1u << s.lb) - 1)]);
        u64 w[4];
        E::store_words(w, value);
        u64* out = vector + 4 * i;
#pragma unroll
        for (u32 k = 0; k < 4; ++k) out[k] = w[k];
      }
    }
    __syncthreads();
  }
}

struct combine_views {
  column_view v[kCombineChunk];
};

// combined[i] (+)= sum_{j < count} coefficients[j] views.v[j][i], i < n; `add`: to what combined holds
template <class E>
__global__ void __launch_bounds__(kCombineThreads)
    k_combine_columns(u64* combined, const combine_views views, const u8* __restrict__ coefficients,
                      u32 count, u64 n, u32 add) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe scaled[kCombineChunk];
  if (threadIdx.x < count) {
    scaled[threadIdx.x] = F::mul(E::load(coefficients + 32 * threadIdx.x),
                                 E::conversion(views.v[threadIdx.x].nbytes == E::element_bytes));
  }
  __syncthreads();
  for (u64 i = static_cast<u64>(blockIdx.x) * kCombineThreads + threadIdx.x; i < n;
       i += static_cast<u64>(gridDim.x) * kCombineThreads) {
    u64* out = combined + 4 * i;
    fe acc = F::zero();
    if (add != 0) {
      u64 w[4];
#pragma unroll
      for (u32 k = 0; k < 4; ++k) w[k] = out[k];
      acc = E::load(reinterpret_cast<const u8*>(w));
    }
    for (u32 j = 0; j < count; ++j) {
      const column_view c = views.v[j];
      // lazy: limbs and value grow by one product's a column, swept and reduced every fourth
      if (i < c.n) acc = F::add(acc, F::mul(load_raw<F>(c, i), scaled[j]));
      if ((j & 3) == 3) acc = F::reduce(F::norm(acc));
    }
    acc = F::reduce(F::norm(acc));
    u64 w[4];
    E::store_words(w, acc);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) out[k] = w[k];
  }
}

// product = sum_j coefficients[j] evaluations[j]: one wavefront
template <class E>
__global__ void __launch_bounds__(64)
    k_combine_product(u8* __restrict__ product, const u8* __restrict__ coefficients,
                      const u8* __restrict__ evaluations, u32 count) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[64];
  fe sum = F::zero();
  for (u32 j = threadIdx.x; j < count; j += 64) {
    sum = fadd<F>(sum, F::mul(E::load(coefficients + 32 * j), E::load(evaluations + 32 * j)));
  }
  tree[threadIdx.x] = sum;
  __syncthreads();
  for (u32 stride = 32; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      tree[threadIdx.x] = fadd<F>(tree[threadIdx.x], tree[threadIdx.x + stride]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) E::store(product, tree[0]);
}

struct evaluate_views {
  column_view v[kEvaluateChunk];
};

// fn(constant j) for j = 0 .. kEvaluateChunk - 1, expanded at compile time: whatever fn indexes
// with j is indexed by a constant, so a lane's accumulators stay in registers
template <class Fn, u32... J>
BZ_HD void for_each_of_chunk(std::integer_sequence<u32, J...>, Fn&& fn) {
  (fn(std::integral_constant<u32, J>{}), ...);
}
template <class Fn> BZ_HD void for_each_of_chunk(Fn&& fn) {
  for_each_of_chunk(std::make_integer_sequence<u32, kEvaluateChunk>{}, fn);
}

// partials[j * gridDim.x + block] = sum over the block's rows i < rows of raw(views.v[j][i]) *
// raw(vector[i]) / R, j < count (normalised, V < 4; zero for a block or a column without rows), and
// kinds[j] = whether column j holds 32-byte elements, for the constant the finish multiplies in.
// `rows`: the longest column of the chunk.
template <class E>
__global__ void __launch_bounds__(kEvaluateThreads)
    k_evaluate_columns(typename E::F::fe* __restrict__ partials, u32* __restrict__ kinds,
                       const u64* __restrict__ vector, const evaluate_views views, u32 count,
                       u64 rows) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[kEvaluateThreads];
  if (blockIdx.x == 0 && threadIdx.x < count) {
    kinds[threadIdx.x] = views.v[threadIdx.x].nbytes == E::element_bytes ? 1u : 0u;
  }
  fe acc[kEvaluateChunk];
  for_each_of_chunk([&](auto j) { acc[j] = F::zero(); });
  u32 pending = 0;
  for (u64 i = static_cast<u64>(blockIdx.x) * kEvaluateThreads + threadIdx.x; i < rows;
       i += static_cast<u64>(gridDim.x) * kEvaluateThreads) {
    u64 w[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) w[k] = vector[4 * i + k];
    // the raw residue of the entry's bytes: normalised, V < 16 (2^256 - 1 over l)
    const fe b = F::from_words(w);
    for_each_of_chunk([&](auto j) {
      // lazy: a product is normalised with V < 2, so between two sweeps a limb stays below
      // (1 + kEvaluateSweep) 2^LB < 2^32 and the value below (4 + 2 kEvaluateSweep) p
      if (j < count && i < views.v[j].n) {
        acc[j] = F::add(acc[j], F::mul(load_raw<F>(views.v[j], i), b));
      }
    });
    if (++pending == kEvaluateSweep) {
      pending = 0;
      for_each_of_chunk([&](auto j) { acc[j] = F::reduce(F::norm(acc[j])); });
    }
  }
  for_each_of_chunk([&](auto j) {
    if (j < count) {
      tree[threadIdx.x] = F::reduce(F::norm(acc[j]));
      __syncthreads();
      for (u32 stride = kEvaluateThreads / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
          tree[threadIdx.x] = fadd<F>(tree[threadIdx.x], tree[threadIdx.x + stride]);
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) partials[static_cast<u64>(j) * gridDim.x + blockIdx.x] = tree[0];
      __syncthreads();
    }
  });
}

// evaluations[j] = (the sum of column j's `blocks` partials) * conversion(column's kind) *
// conversion(element: the vector's) / R^2, canonical; one workgroup per column.  A column without
// rows has zero partials: 0.
template <class E>
__global__ void __launch_bounds__(kEvaluateThreads)
    k_evaluate_finish(u8* __restrict__ evaluations, const typename E::F::fe* __restrict__ partials,
                      const u32* __restrict__ kinds, u32 blocks) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[kEvaluateThreads];
  const u64 j = blockIdx.x;
  fe sum = F::zero();
  for (u32 b = threadIdx.x; b < blocks; b += kEvaluateThreads) {
    sum = fadd<F>(sum, partials[j * blocks + b]);
  }
  tree[threadIdx.x] = sum;
  __syncthreads();
  for (u32 stride = kEvaluateThreads / 2; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      tree[threadIdx.x] = fadd<F>(tree[threadIdx.x], tree[threadIdx.x + stride]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const fe constant = F::mul(E::conversion(kinds[j] != 0), E::conversion(true));
    E::store(evaluations + 32 * j, F::mul(tree[0], constant));
  }
}

//--------------------------------------------------------------------------------------------------
// checks
//--------------------------------------------------------------------------------------------------
void check_vector_arguments(const void* vector, const void* point, unsigned num_variables, u64 n) {
  BZ_RELEASE_ASSERT(vector != nullptr && point != nullptr,
                    "null argument to the MLE evaluation vector");
  BZ_RELEASE_ASSERT(num_variables >= 1 && num_variables <= kMaxVariables,
                    "the MLE evaluation vector needs 1 <= num_variables <= 30");
  BZ_RELEASE_ASSERT(n >= 1 && n <= (u64{1} << num_variables),
                    "the MLE evaluation vector needs 1 <= n <= 2^num_variables");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(vector) % 8 == 0,
                    "the MLE evaluation vector must be 8-byte aligned");
}

void check_combination(const void* combined, const column_combination& c) {
  BZ_RELEASE_ASSERT(c.num_columns >= 1, "the column combination needs at least one column");
  BZ_RELEASE_ASSERT(combined != nullptr && c.columns != nullptr && c.coefficients != nullptr,
                    "null argument to the column combination");
  BZ_RELEASE_ASSERT(c.n >= 1 && c.n <= (u64{1} << 30), "the column combination needs 1 <= n <= 2^30");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(combined) % 8 == 0,
                    "the combined vector must be 8-byte aligned");
  for (u32 j = 0; j < c.num_columns; ++j) {
    BZ_RELEASE_ASSERT(c.columns[j].n <= c.n, "a combined column is longer than n");
  }
}

void check_evaluation(const void* evaluations, const void* vector, const column_evaluation& e) {
  BZ_RELEASE_ASSERT(e.num_columns >= 1, "the column evaluation needs at least one column");
  BZ_RELEASE_ASSERT(evaluations != nullptr && vector != nullptr && e.columns != nullptr,
                    "null argument to the column evaluation");
  BZ_RELEASE_ASSERT(e.n >= 1 && e.n <= (u64{1} << 30), "the column evaluation needs 1 <= n <= 2^30");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(vector) % 8 == 0,
                    "the evaluation vector must be 8-byte aligned");
  for (u32 j = 0; j < e.num_columns; ++j) {
    BZ_RELEASE_ASSERT(e.columns[j].n <= e.n, "an evaluated column is longer than n");
  }
}

// workgroups of every k_evaluate_columns launch of a call over n rows
u32 evaluate_blocks(u64 n) {
  return static_cast<u32>(
      std::min<u64>(kEvaluateBlocks, (n + kEvaluateThreads - 1) / kEvaluateThreads));
}

// the caller's workspace: partials[column][block], and the columns' kinds for the finish
template <class F> struct evaluate_layout {
  size_t partials, kinds, total;
  evaluate_layout(u32 num_columns, u64 n) {
    workspace_carver carve;
    partials = carve.take(sizeof(typename F::fe) * evaluate_blocks(n) * num_columns);
    kinds = carve.take(sizeof(u32) * num_columns);
    total = carve.total();
  }
};

//--------------------------------------------------------------------------------------------------
// host backend: plain loops over the same element arithmetic
//--------------------------------------------------------------------------------------------------
template <class E> void evaluate_host(u8* evaluations, const u64* vector, const column_evaluation& e) {
  using F = typename E::F;
  using fe = typename F::fe;
  for (u32 j = 0; j < e.num_columns; ++j) {
    const column_view view = make_column_view(e.columns[j]);
    fe acc = F::zero();
    for (u64 i = 0; i < view.n; ++i) {
      acc = fadd<F>(acc, F::mul(load_raw<F>(view, i), F::from_words(vector + 4 * i)));
    }
    const fe constant =
        F::mul(E::conversion(view.nbytes == E::element_bytes), E::conversion(true));
    E::store(evaluations + static_cast<size_t>(32) * j, F::mul(acc, constant));
  }
}

template <class E>
void evaluation_vector_host(u64* vector, const u8* point, u32 num_variables, u64 n) {
  using F = typename E::F;
  using fe = typename F::fe;
  fe r[kMaxVariables], one_minus_r[kMaxVariables];
  for (u32 t = 0; t < num_variables; ++t) {
    r[t] = E::load(point + 32 * t);
    one_minus_r[t] = fsub<F>(F::one(), r[t]);
  }
  for (u64 i = 0; i < n; ++i) {
    fe p = F::one();
    for (u32 t = 0; t < num_variables; ++t) {
      p = F::mul(p, ((i >> (num_variables - 1 - t)) & 1) != 0 ? r[t] : one_minus_r[t]);
    }
    E::store_words(vector + 4 * i, p);
  }
}

template <class E> void combine_host(u64* combined, u8* product, const column_combination& c) {
  using F = typename E::F;
  using fe = typename F::fe;
  const u8* coefficients = static_cast<const u8*>(c.coefficients);
  std::vector<column_view> views(c.num_columns);
  std::vector<fe> scaled(c.num_columns);
  for (u32 j = 0; j < c.num_columns; ++j) {
    views[j] = make_column_view(c.columns[j]);
    scaled[j] = F::mul(E::load(coefficients + 32 * j),
                       E::conversion(views[j].nbytes == E::element_bytes));
  }
  for (u64 i = 0; i < c.n; ++i) {
    fe acc = F::zero();
    for (u32 j = 0; j < c.num_columns; ++j) {
      if (i < views[j].n) acc = fadd<F>(acc, F::mul(load_raw<F>(views[j], i), scaled[j]));
    }
    E::store_words(combined + 4 * i, acc);
  }
  if (product != nullptr && c.evaluations != nullptr) {
    const u8* evaluations = static_cast<const u8*>(c.evaluations);
    fe sum = F::zero();
    for (u32 j = 0; j < c.num_columns; ++j) {
      sum = fadd<F>(sum, F::mul(E::load(coefficients + 32 * j), E::load(evaluations + 32 * j)));
    }
    E::store(product, sum);
  }
}

//--------------------------------------------------------------------------------------------------
// device forms: enqueue only
//--------------------------------------------------------------------------------------------------
template <class E>
void evaluation_vector_enqueue(u64* vector, const u8* point, u32 num_variables, u64 n,
                               hipStream_t stream) {
  const vector_split s = split_of(num_variables);
  const u64 tile_rows = u64{1} << (s.lb + s.mb);
  const u64 num_tiles = (n + tile_rows - 1) / tile_rows;
  const u32 blocks = static_cast<u32>(std::min<u64>(kVectorBlocks, num_tiles));
  hipLaunchKernelGGL((k_mle_evaluation_vector<E>), dim3(blocks), dim3(kVectorThreads), 0, stream,
                     vector, point, num_variables, n);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}

template <class E>
void combine_enqueue(u64* combined, u8* product, const column_combination& c, hipStream_t stream) {
  const u8* coefficients = static_cast<const u8*>(c.coefficients);
  const u32 blocks = static_cast<u32>(
      std::min<u64>(kCombineBlocks, (c.n + kCombineThreads - 1) / kCombineThreads));
  for (u32 first = 0; first < c.num_columns; first += kCombineChunk) {
    const u32 count = std::min(kCombineChunk, c.num_columns - first);
    combine_views views;
    std::memset(&views, 0, sizeof(views));
    for (u32 j = 0; j < count; ++j) views.v[j] = make_column_view(c.columns[first + j]);
    hipLaunchKernelGGL((k_combine_columns<E>), dim3(blocks), dim3(kCombineThreads), 0, stream,
                       combined, views, coefficients + static_cast<size_t>(32) * first, count, c.n,
                       first != 0 ? 1u : 0u);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
  }
  if (product != nullptr && c.evaluations != nullptr) {
    hipLaunchKernelGGL((k_combine_product<E>), dim3(1), dim3(64), 0, stream, product, coefficients,
                       static_cast<const u8*>(c.evaluations), c.num_columns);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
  }
}

// ceil(num_columns / kEvaluateChunk) launches of the partial sums and one finish over all columns
template <class E>
void evaluate_enqueue(u8* evaluations, const u64* vector, const column_evaluation& e,
                      void* workspace, u64 workspace_bytes, hipStream_t stream) {
  using fe = typename E::F::fe;
  const evaluate_layout<typename E::F> layout{e.num_columns, e.n};
  BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                    "the column evaluation workspace is too small");
  u8* base = workspace_carver::aligned(workspace);
  fe* d_partials = reinterpret_cast<fe*>(base + layout.partials);
  u32* d_kinds = reinterpret_cast<u32*>(base + layout.kinds);
  const u32 blocks = evaluate_blocks(e.n);
  for (u32 first = 0; first < e.num_columns; first += kEvaluateChunk) {
    const u32 count = std::min(kEvaluateChunk, e.num_columns - first);
    evaluate_views views;
    std::memset(&views, 0, sizeof(views));
    u64 rows = 0;
    for (u32 j = 0; j < count; ++j) {
      views.v[j] = make_column_view(e.columns[first + j]);
      rows = std::max(rows, views.v[j].n);
    }
    hipLaunchKernelGGL((k_evaluate_columns<E>), dim3(blocks), dim3(kEvaluateThreads), 0, stream,
                       d_partials + static_cast<size_t>(first) * blocks, d_kinds + first, vector,
                       views, count, rows);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
  }
  hipLaunchKernelGGL((k_evaluate_finish<E>), dim3(e.num_columns), dim3(kEvaluateThreads), 0, stream,
                     evaluations, d_partials, d_kinds, blocks);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}
} // namespace

void mle_evaluation_vector_device(void* vector, unsigned field_id, const void* evaluation_point,
                                  unsigned num_variables, u64 n, hipStream_t stream) {
  check_vector_arguments(vector, evaluation_point, num_variables, n);
  with_elements(field_id, [&](auto elements) {
    evaluation_vector_enqueue<decltype(elements)>(static_cast<u64*>(vector),
                                                  static_cast<const u8*>(evaluation_point),
                                                  num_variables, n, stream);
  });
}

void mle_evaluation_vector(api_state& st, void* vector, unsigned field_id,
                           const void* evaluation_point, unsigned num_variables, u64 n) {
  check_vector_arguments(vector, evaluation_point, num_variables, n);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      evaluation_vector_host<E>(static_cast<u64*>(vector), static_cast<const u8*>(evaluation_point),
                                num_variables, n);
      return;
    }
    // the point up, the device form, the vector down: memory of the call's own
    host_call call{st};
    u8* d_point;
    u64* d_vector;
    call.input(&d_point, evaluation_point, static_cast<size_t>(32) * num_variables);
    call.output(&d_vector, vector, static_cast<size_t>(32) * n);
    call.allocate();
    evaluation_vector_enqueue<E>(d_vector, d_point, num_variables, n, call.stream());
    call.finish();
  });
}

void combine_columns_device(void* combined, void* product, unsigned field_id,
                            const column_combination& c, hipStream_t stream) {
  check_combination(combined, c);
  with_elements(field_id, [&](auto elements) {
    combine_enqueue<decltype(elements)>(static_cast<u64*>(combined), static_cast<u8*>(product), c,
                                        stream);
  });
}

void combine_columns(api_state& st, void* combined, void* product, unsigned field_id,
                     const column_combination& c) {
  check_combination(combined, c);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      combine_host<E>(static_cast<u64*>(combined), static_cast<u8*>(product), c);
      return;
    }
    // the columns up at their own width, the device form, the results down
    host_call call{st};
    // the product and the evaluations it is made of: both or neither
    const bool with_product = product != nullptr && c.evaluations != nullptr;
    const size_t element_bytes = static_cast<size_t>(32) * c.num_columns;
    u64* d_combined;
    u8 *d_coefficients, *d_evaluations, *d_product;
    std::vector<sumcheck_column> on_device;
    call.output(&d_combined, combined, static_cast<size_t>(32) * c.n);
    call.input(&d_coefficients, c.coefficients, element_bytes);
    call.input(&d_evaluations, with_product ? c.evaluations : nullptr, element_bytes);
    call.output(&d_product, with_product ? product : nullptr, 32);
    call.columns(&on_device, c.columns, c.num_columns);
    call.allocate();
    const column_combination staged{on_device.data(), d_coefficients, d_evaluations, c.num_columns,
                                    c.n};
    combine_enqueue<E>(d_combined, d_product, staged, call.stream());
    call.finish();
  });
}

u64 evaluate_columns_workspace_bytes(unsigned field_id, u32 num_columns, u64 n) {
  if (field_id > 1 || num_columns == 0 || n == 0 || n > (u64{1} << 30)) return 0;
  return with_elements(field_id, [&](auto elements) -> u64 {
    return evaluate_layout<typename decltype(elements)::F>{num_columns, n}.total;
  });
}

void evaluate_columns_device(void* evaluations, unsigned field_id, const void* vector,
                             const column_evaluation& e, void* workspace, u64 workspace_bytes,
                             hipStream_t stream) {
  check_evaluation(evaluations, vector, e);
  with_elements(field_id, [&](auto elements) {
    evaluate_enqueue<decltype(elements)>(static_cast<u8*>(evaluations),
                                         static_cast<const u64*>(vector), e, workspace,
                                         workspace_bytes, stream);
  });
}

void evaluate_columns(api_state& st, void* evaluations, unsigned field_id, const void* vector,
                      const column_evaluation& e) {
  check_evaluation(evaluations, vector, e);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      evaluate_host<E>(static_cast<u8*>(evaluations), static_cast<const u64*>(vector), e);
      return;
    }
    // the vector and the columns up at their own width, the device form, the evaluations down
    host_call call{st};
    const size_t workspace_bytes = evaluate_layout<typename E::F>{e.num_columns, e.n}.total;
    u64* d_vector;
    u8 *d_evaluations, *d_workspace;
    std::vector<sumcheck_column> on_device;
    call.input(&d_vector, vector, static_cast<size_t>(32) * e.n);
    call.output(&d_evaluations, evaluations, static_cast<size_t>(32) * e.num_columns);
    call.scratch(&d_workspace, workspace_bytes);
    call.columns(&on_device, e.columns, e.num_columns);
    call.allocate();
    const column_evaluation staged{on_device.data(), e.num_columns, e.n};
    evaluate_enqueue<E>(d_evaluations, d_vector, staged, d_workspace, workspace_bytes,
                        call.stream());
    call.finish();
  });
}
} // namespace bz::proof
