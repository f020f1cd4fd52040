// The inverse column of a log-derivative argument (bzamd_invert_columns*):
//   inverses[i] = 1 / (shift + sum_j coefficients[j] column_j[i]),   i < n,   0 where that is 0,
// over the typed columns of the sumcheck, written in element form and in scalar form by one kernel
// launch, exact in both fields.
//
// One inversion per row would be a data-dependent Kaliski loop per lane (mont29::invert), the lanes
// of a wavefront each waiting for the slowest.  Instead a workgroup of kInverseThreads lanes owns a
// tile of kInverseTile = kInverseThreads * kLaneRows consecutive rows and inverts ONE value per
// tile (Montgomery's trick twice over: along a lane's rows in registers, across the lanes in the
// LDS product tree of msm/batch_tree.h); workgroups walk tiles grid-stride.  Lane t holds rows
// tile * kInverseTile + r * kInverseThreads + t, r < kLaneRows: interleaved, so that a wavefront's
// load of an i64 column is 512 consecutive bytes and its store of a row 2 KiB of consecutive bytes
// (a lane holding kLaneRows CONSECUTIVE rows would put every lane's 32-byte store into a line of
// its own).
//
//   * Denominators.  A row of column j is fetched as the raw residue of its bytes (load_raw,
//     proof/sumcheck_columns.h), the coefficient carries the conversion constant of the column's
//     kind, multiplied in once per workgroup while the coefficients go to LDS, as k_combine_columns
//     does; additions are lazy (swept and reduced every fourth column), the shift is the
//     accumulator's first value, in engine form.  Columns outside, rows inside: the kLaneRows loads
//     of a column are independent.  K products a row.
//   * A zero denominator (and a row past n) is replaced by one and remembered in a bit mask, so it
//     never reaches a shared product; its row is stored as zero.
//   * prefix[r] = d[0] ... d[r] in registers: 1 - 1 / kLaneRows products a row.  prefix[kLaneRows - 1]
//     is the lane's leaf of the tree.
//   * tree_products, ONE mont29::invert of the root by the 64 lanes of wavefront 0 on the same value
//     (uniform control flow: the cost of one lane; the other wavefronts of the workgroup wait at
//     the barrier, other workgroups of the CU do not), tree_inverses: 3 (T - 1) products and the
//     inversion per tile.
//   * The lane's inverse is multiplied ONCE by the constant that takes engine form to the form
//     that is stored (element form: 2^256 in field 1, 1 in field 0 where element form and scalar
//     form are the same bytes; scalar form alone: 1): every later product with an engine-form
//     prefix or denominator stays in that form, so a row leaves without a product of its own.
//     Walking back, row r is inv * prefix[r - 1] and inv becomes inv * d[r]: 2 - 2 / kLaneRows
//     products a row.  Field 1 with both outputs: one more product a row, by 2^5 (element form to
//     scalar form, as bzamd_fold_polynomial).
//
// Products per row, K columns, kLaneRows = 8, T = 256:
//   K + 7/8 + 14/8 + (3 * 255 + 256) / 2048 = K + 3.12   (+ 1 in field 1 with both outputs)
// and the tile's inversion over 2048 rows.  mont29::invert in the built object (-save-temps): hipcc
// moves the loop to the scalar unit, every lane holding the same value: a body of 301 (field 0) /
// 305 (field 1) instructions, 228 / 232 of them scalar, of which one pass runs one branch, 60 to
// 190 instructions; the algorithm takes about 2 * 0.7 * 254 = 360 passes (a subtraction and the
// shift that follows it per 1.4 bits), some 40 000 instructions against the ~290 of a product in
// this kernel: ~140 products' worth by count, 0.07 a row.  By TIME it is the kernel: a lone
// wavefront issues an instruction every five cycles or so, the chain takes ~130 us on the MI355X,
// and a call takes as long as the tiles one workgroup walks times that, whatever the columns are
// (150 us at 2^16 rows, 168 at 2^20, 636 at 2^22).  A shorter chain (a binary GCD on
// approximations, 31 steps at a time) is the next step, DESIGN 10.
//
// d[] and prefix[] are indexed by compile-time constants alone: no scratch memory (tests/
// test_column_inverse.py reads the compiler's report).  No waits between workgroups; one launch
// whatever n is; LDS: the tree (2 T elements), the scaled coefficients and the shift, 19.6 KB.
#include "blitzar_amd/csrc/proof/column_inverse.h"

#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "blitzar_amd/csrc/msm/batch_tree.h"
#include "blitzar_amd/csrc/proof/host_call.h"
#include "blitzar_amd/csrc/proof/sumcheck_columns.h"

namespace bz::proof {
namespace {
constexpr u32 kLaneRows = 8;
constexpr u32 kInverseThreads = 256;
constexpr u32 kInverseTile = kLaneRows * kInverseThreads;
// 2 workgroups per CU; kInverseBlocks * kInverseTile = 2^20 rows in flight at most
constexpr u32 kInverseBlocks = 512;
constexpr u32 kHostBlock = 256; // rows that share an inversion in the host form

struct inverse_views {
  column_view v[kMaxInvertedColumns];
};

// the field as the product tree sees it (msm/batch_tree.h; msm/kernels.h itself defines the MSM's
// kernels, so the levels are called here with the barriers tree_products / tree_inverses put
// between them)
template <class F> struct field_batch {
  using batch_fe = typename F::fe;
  BZ_HD static batch_fe batch_mul(const batch_fe& a, const batch_fe& b) { return F::mul(a, b); }
};

// engine form times this is the raw residue of element form (`element`) or of scalar form
template <class E> BZ_HD typename E::F::fe out_constant(bool element) {
  using F = typename E::F;
  typename F::fe c = F::zero();
  c.v[0] = 1;
  if constexpr (std::is_same_v<E, grumpkin_elements>) {
    if (element) {
#pragma unroll
      for (int i = 0; i < F::N; ++i) c.v[i] = F::params::c_out(i);
    }
  }
  return c;
}
// the raw residue of scalar form from that of element form: x 2^256 -> x is the product with
// 2^-256 R = 2^5 (field 1); field 0: the same value
template <class E> BZ_HD typename E::F::fe scalar_of_element(const typename E::F::fe& v) {
  using F = typename E::F;
  if constexpr (std::is_same_v<E, grumpkin_elements>) {
    typename F::fe c = F::zero();
    c.v[0] = 1u << (F::LB * F::N - 256);
    return F::mul(v, c);
  } else {
    return v;
  }
}
// canonical words of a normalised value, or zero
template <class F> BZ_HD void store_row(u64* rows, u64 i, const typename F::fe& v, bool zero) {
  u64 w[4];
  F::to_words(w, F::canonical(v));
#pragma unroll
  for (u32 k = 0; k < 4; ++k) rows[4 * i + k] = zero ? 0 : w[k];
}
// `out`: the row in the form out_constant(inverses != nullptr) leaves it in
template <class E>
BZ_HD void store_inverse(u64* inverses, u64* scalars, u64 i, const typename E::F::fe& out,
                         bool zero) {
  using F = typename E::F;
  if (inverses != nullptr) {
    store_row<F>(inverses, i, out, zero);
    if (scalars != nullptr) store_row<F>(scalars, i, scalar_of_element<E>(out), zero);
  } else {
    store_row<F>(scalars, i, out, zero);
  }
}
// coefficient j times the conversion constant of column j's kind; the shift, engine form
template <class E>
BZ_HD typename E::F::fe scaled_coefficient(const u8* coefficients, u32 j, const column_view& c) {
  using F = typename E::F;
  const typename F::fe conversion = E::conversion(c.nbytes == E::element_bytes);
  return coefficients != nullptr ? F::mul(E::load(coefficients + 32 * j), conversion) : conversion;
}
template <class E> BZ_HD typename E::F::fe engine_shift(const u8* shift) {
  using F = typename E::F;
  return shift != nullptr ? E::load(shift) : F::zero();
}

// fn(constant r) for r = 0 .. kLaneRows - 1, expanded at compile time: whatever fn indexes with r
// is indexed by a constant, so a lane's denominators and prefixes stay in registers
template <class Fn, u32... R>
BZ_HD void for_each_lane_row(std::integer_sequence<u32, R...>, Fn&& fn) {
  (fn(std::integral_constant<u32, R>{}), ...);
}
template <class Fn> BZ_HD void for_each_lane_row(Fn&& fn) {
  for_each_lane_row(std::make_integer_sequence<u32, kLaneRows>{}, fn);
}

//--------------------------------------------------------------------------------------------------
// device kernel
//--------------------------------------------------------------------------------------------------
template <class E>
__global__ void __launch_bounds__(kInverseThreads, 2)
    k_invert_columns(u64* inverses, u64* scalars, const inverse_views views,
                     const u8* __restrict__ coefficients, const u8* __restrict__ shift, u32 count,
                     u64 n) {
  using F = typename E::F;
  using fe = typename F::fe;
  using B = field_batch<F>;
  constexpr u32 T = kInverseThreads;
  __shared__ fe scaled[kMaxInvertedColumns];
  __shared__ fe shared_shift;
  __shared__ fe tree[2 * T];
  const u32 tid = threadIdx.x;
  if (tid < count) scaled[tid] = scaled_coefficient<E>(coefficients, tid, views.v[tid]);
  if (tid == T - 1) shared_shift = engine_shift<E>(shift);
  __syncthreads();
  const fe to_out = out_constant<E>(inverses != nullptr);
  const u64 num_tiles = (n + kInverseTile - 1) / kInverseTile;
  for (u64 tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    const u64 base = tile * kInverseTile + tid;
    fe d[kLaneRows];
    for_each_lane_row([&](auto r) { d[r] = shared_shift; });
    for (u32 j = 0; j < count; ++j) {
      const column_view c = views.v[j];
      const fe coefficient = scaled[j];
      // lazy: limbs and value grow by one product's a column, swept and reduced every fourth
      for_each_lane_row([&](auto r) {
        const u64 i = base + static_cast<u64>(r) * T;
        if (i < c.n) d[r] = F::add(d[r], F::mul(load_raw<F>(c, i), coefficient));
        if ((j & 3) == 3) d[r] = F::reduce(F::norm(d[r]));
      });
    }
    // zeros (and rows past n) become one; prefix[r] = d[0] .. d[r]
    u32 zeros = 0;
    fe prefix[kLaneRows];
    for_each_lane_row([&](auto r) {
      const u64 i = base + static_cast<u64>(r) * T;
      d[r] = F::reduce(F::norm(d[r]));
      const bool zero = i >= n || F::is_zero(d[r]);
      zeros |= (zero ? 1u : 0u) << r;
      d[r] = F::select(d[r], F::one(), zero);
      if constexpr (r == 0) {
        prefix[0] = d[0];
      } else {
        prefix[r] = F::mul(prefix[r - 1], d[r]);
      }
      // one row after the other: interleaved, the rows' zero tests hold 100 registers more
      F::pin(prefix[r]);
    });
    tree[T + tid] = prefix[kLaneRows - 1];
    __syncthreads();
    for (u32 s = T / 2; s >= 1; s >>= 1) {
      tree_product_step<B>(tree, s, tid);
      __syncthreads();
    }
    // every lane of wavefront 0 inverts the same value: uniform control flow
    if (tid < 64) {
      const fe inv = F::invert_inline(tree[1]);
      if (tid == 0) tree[1] = inv;
    }
    __syncthreads();
    for (u32 s = 1; s < T; s <<= 1) {
      tree_inverse_step<B>(tree, s, tid);
      __syncthreads();
    }
    // a lane reads its own leaf alone, and writes it alone before the next tile's first barrier
    fe inv = F::mul(tree[T + tid], to_out);
    for_each_lane_row([&](auto k) {
      constexpr u32 r = kLaneRows - 1 - k;
      const u64 i = base + static_cast<u64>(r) * T;
      fe out = inv;
      if constexpr (r > 0) {
        out = F::mul(inv, prefix[r - 1]);
        inv = F::mul(inv, d[r]);
        F::pin(inv); // as above: a row's store conversions before the next row's products
      }
      if (i < n) store_inverse<E>(inverses, scalars, i, out, ((zeros >> r) & 1) != 0);
    });
  }
}

//--------------------------------------------------------------------------------------------------
// host backend: the same arithmetic, Montgomery's trick over blocks of kHostBlock rows
//--------------------------------------------------------------------------------------------------
template <class E> void invert_host(u64* inverses, u64* scalars, const column_inversion& v) {
  using F = typename E::F;
  using fe = typename F::fe;
  const u8* coefficients = static_cast<const u8*>(v.coefficients);
  std::vector<column_view> views(v.num_columns);
  std::vector<fe> scaled(v.num_columns);
  for (u32 j = 0; j < v.num_columns; ++j) {
    views[j] = make_column_view(v.columns[j]);
    scaled[j] = scaled_coefficient<E>(coefficients, j, views[j]);
  }
  const fe shift = engine_shift<E>(static_cast<const u8*>(v.shift));
  const fe to_out = out_constant<E>(inverses != nullptr);
  fe d[kHostBlock], prefix[kHostBlock];
  bool zero[kHostBlock];
  for (u64 first = 0; first < v.n; first += kHostBlock) {
    const u32 rows = static_cast<u32>(std::min<u64>(kHostBlock, v.n - first));
    for (u32 r = 0; r < rows; ++r) {
      const u64 i = first + r;
      fe acc = shift;
      for (u32 j = 0; j < v.num_columns; ++j) {
        if (i < views[j].n) acc = fadd<F>(acc, F::mul(load_raw<F>(views[j], i), scaled[j]));
      }
      zero[r] = F::is_zero(acc);
      d[r] = zero[r] ? F::one() : acc;
      prefix[r] = r == 0 ? d[0] : F::mul(prefix[r - 1], d[r]);
    }
    fe inv = F::mul(F::invert(prefix[rows - 1]), to_out);
    for (u32 r = rows; r-- > 0;) {
      const fe out = r > 0 ? F::mul(inv, prefix[r - 1]) : inv;
      if (r > 0) inv = F::mul(inv, d[r]);
      store_inverse<E>(inverses, scalars, first + r, out, zero[r]);
    }
  }
}

//--------------------------------------------------------------------------------------------------
// device form: enqueue only, one launch
//--------------------------------------------------------------------------------------------------
template <class E>
void invert_enqueue(u64* inverses, u64* scalars, const column_inversion& v, hipStream_t stream) {
  const u64 num_tiles = (v.n + kInverseTile - 1) / kInverseTile;
  const u32 blocks = static_cast<u32>(std::min<u64>(kInverseBlocks, num_tiles));
  inverse_views views;
  std::memset(&views, 0, sizeof(views));
  for (u32 j = 0; j < v.num_columns; ++j) views.v[j] = make_column_view(v.columns[j]);
  hipLaunchKernelGGL((k_invert_columns<E>), dim3(blocks), dim3(kInverseThreads), 0, stream,
                     inverses, scalars, views, static_cast<const u8*>(v.coefficients),
                     static_cast<const u8*>(v.shift), v.num_columns, v.n);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}
} // namespace

void check_column_inversion(const void* inverses, const void* scalars, unsigned field_id,
                            const column_inversion& v) {
  BZ_RELEASE_ASSERT(v.columns != nullptr && (inverses != nullptr || scalars != nullptr),
                    "null argument to the column inversion");
  BZ_RELEASE_ASSERT(v.num_columns >= 1 && v.num_columns <= kMaxInvertedColumns,
                    "the column inversion needs 1 <= num_columns <= 32");
  BZ_RELEASE_ASSERT(v.n >= 1 && v.n <= (u64{1} << 30), "the column inversion needs 1 <= n <= 2^30");
  BZ_RELEASE_ASSERT(reinterpret_cast<uintptr_t>(inverses) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(scalars) % 8 == 0,
                    "the inverse columns must be 8-byte aligned");
  const u64 out_bytes = 32 * v.n;
  const byte_range outputs[2] = {{inverses, out_bytes}, {scalars, out_bytes}};
  BZ_RELEASE_ASSERT(!overlap(outputs[0], outputs[1]), "the outputs of the column inversion overlap");
  for (const byte_range& out : outputs) {
    for (u32 j = 0; j < v.num_columns; ++j) {
      BZ_RELEASE_ASSERT(v.columns[j].n <= v.n, "an inverted column is longer than n");
      BZ_RELEASE_ASSERT(!overlap(out, {v.columns[j].data, v.columns[j].n * v.columns[j].nbytes}),
                        "an output overlaps an input of the same call");
    }
    BZ_RELEASE_ASSERT(!overlap(out, {v.coefficients, u64{32} * v.num_columns}) &&
                          !overlap(out, {v.shift, 32}),
                      "an output overlaps an input of the same call");
  }
  BZ_RELEASE_ASSERT(field_id <= 1, "unsupported field id");
}

void invert_columns_device(void* inverses, void* scalars, unsigned field_id,
                           const column_inversion& v, hipStream_t stream) {
  with_elements(field_id, [&](auto elements) {
    invert_enqueue<decltype(elements)>(static_cast<u64*>(inverses), static_cast<u64*>(scalars), v,
                                       stream);
  });
}

void invert_columns(api_state& st, void* inverses, void* scalars, unsigned field_id,
                    const column_inversion& v) {
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      invert_host<E>(static_cast<u64*>(inverses), static_cast<u64*>(scalars), v);
      return;
    }
    // the columns up at their own width, the device form, the results down
    host_call call{st};
    const size_t out_bytes = static_cast<size_t>(32) * v.n;
    u64 *d_inverses, *d_scalars;
    u8 *d_coefficients, *d_shift;
    std::vector<sumcheck_column> on_device;
    call.output(&d_inverses, inverses, out_bytes);
    call.output(&d_scalars, scalars, out_bytes);
    call.input(&d_coefficients, v.coefficients, static_cast<size_t>(32) * v.num_columns);
    call.input(&d_shift, v.shift, 32);
    call.columns(&on_device, v.columns, v.num_columns);
    call.allocate();
    const column_inversion staged{on_device.data(), d_coefficients, d_shift, v.num_columns, v.n};
    invert_enqueue<E>(d_inverses, d_scalars, staged, call.stream());
    call.finish();
  });
}
} // namespace bz::proof
