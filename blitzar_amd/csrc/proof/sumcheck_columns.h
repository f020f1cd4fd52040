// What the provers over typed columns share (proof/sumcheck_columns.hip: the callback form;
// proof/sumcheck_transcript.hip: the chain with the built-in transcript): how a column is described
// to a kernel, how an element is fetched as the raw residue of its bytes, round 0's `Tables` over
// the columns and the round-0 kernels.  Why raw residues are enough is in the head comment of
// proof/sumcheck_columns.hip.  Everything has internal linkage: each translation unit compiles
// the kernels it launches.
#pragma once

#include "blitzar_amd/csrc/proof/sumcheck_rows.h"

namespace bz::proof {
namespace {
// how an element's bytes are fetched (the same for a whole column: uniform over a wavefront)
enum : u32 {
  kAccessBytes = 0, // any width, any address
  kAccessWords = 1, // width a multiple of 8 at an address that is one
};

struct column_view {
  const u8* data;
  u64 n;
  u32 nbytes, access, is_signed, reserved;
};

u32 access_of(const void* data, u32 nbytes) {
  return nbytes % 8 == 0 && reinterpret_cast<uintptr_t>(data) % 8 == 0 ? kAccessWords : kAccessBytes;
}

// w = the little-endian integer of the c.nbytes bytes at p
BZ_HD void load_bytes(u64* w, const column_view& c, const u8* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the aligned 32-bit words the bytes lie in (never more memory than those: nothing outside the
  // words that hold a byte of the column is touched), shifted into place and cut to the width;
  // every array index is a constant, so the words stay in registers
  const u64 address = reinterpret_cast<u64>(p);
  const u32 offset = static_cast<u32>(address & 3);
  const u32* q = reinterpret_cast<const u32*>(address - offset);
  u32 d[9];
#pragma unroll
  for (u32 k = 0; k < 9; ++k) d[k] = 4 * k < offset + c.nbytes ? q[k] : 0;
#pragma unroll
  for (u32 k = 0; k < 8; ++k) {
    u32 x = __builtin_amdgcn_alignbyte(d[k + 1], d[k], offset);
    const u32 have = c.nbytes > 4 * k ? c.nbytes - 4 * k : 0;
    if (have < 4) x &= (1u << (8 * have)) - 1;
    if (k % 2 == 0) {
      w[k / 2] = x;
    } else {
      w[k / 2] |= static_cast<u64>(x) << 32;
    }
  }
#else
  for (u32 k = 0; k < c.nbytes; ++k) w[k >> 3] |= static_cast<u64>(p[k]) << (8 * (k & 7));
#endif
}

// w = magnitude of row i < c.n of the column (little-endian words); returns its sign
BZ_HD bool load_magnitude(u64* w, const column_view& c, u64 i) {
  const u8* p = c.data + i * c.nbytes;
  if (c.access == kAccessWords) {
    const u64* q = reinterpret_cast<const u64*>(p);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
      if (8 * k < c.nbytes) w[k] = q[k];
    }
  } else {
    load_bytes(w, c, p);
  }
  if (c.is_signed == 0) return false;
  // at most 16 bytes: sign-extend to 128 bits, take the magnitude
  u64 lo = w[0], hi = w[1];
  if (c.nbytes <= 8) {
    const u32 s = 64 - 8 * c.nbytes;
    lo = static_cast<u64>(static_cast<i64>(lo << s) >> s);
    hi = static_cast<u64>(static_cast<i64>(lo) >> 63);
  } else {
    const u32 s = 128 - 8 * c.nbytes;
    hi = static_cast<u64>(static_cast<i64>(hi << s) >> s);
  }
  const bool negative = static_cast<i64>(hi) < 0;
  if (negative) {
    lo = ~lo + 1;
    hi = ~hi + (lo == 0 ? 1 : 0);
  }
  w[0] = lo;
  w[1] = hi;
  return negative;
}

// row i < c.n as the raw residue of its bytes, normalised, V < 4 (32 bytes may hold up to 16 p)
template <class F> BZ_HD typename F::fe load_raw(const column_view& c, u64 i) {
  u64 w[4] = {0, 0, 0, 0};
  const bool negative = load_magnitude(w, c, i);
  const typename F::fe v = F::reduce(F::from_words(w));
  return F::select(v, fneg<F>(v), negative);
}

// the `Tables` of round 0 (proof/sumcheck_rows.h), raw: rows past a column's end are zero; nothing
// is common to the columns of a row (every column has its own length)
struct no_row_state {};
template <class F> struct column_tables {
  const column_view* views;
  u64 mid;
  BZ_HD no_row_state row(u64) const { return {}; }
  BZ_HD void pair(u32 mle, u64 i, no_row_state, typename F::fe& a, typename F::fe& b) const {
    const column_view c = views[mle];
    a = i < c.n ? load_raw<F>(c, i) : F::zero();
    b = mid + i < c.n ? fsub<F>(load_raw<F>(c, mid + i), a) : fneg<F>(a);
  }
};

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
// round 0, round_degree D <= kFixedDegree: k_sumcheck_round_fixed's expansion (no scratch memory);
// `products`: the multipliers times their terms' conversion constants
template <class F, u32 D>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_columns_round(typename F::fe* __restrict__ partials,
                             const column_view* __restrict__ views, u64 mid,
                             const product_desc<F>* __restrict__ products, u32 num_products,
                             const u32* __restrict__ terms) {
  using fe = typename F::fe;
  __shared__ fe tree[D + 1][kRoundThreads];
  fe poly[D + 1];
#pragma unroll
  for (u32 k = 0; k <= D; ++k) poly[k] = F::zero();
  const column_tables<F> tables{views, mid};
  for (u64 i = static_cast<u64>(blockIdx.x) * kRoundThreads + threadIdx.x; i < mid;
       i += static_cast<u64>(gridDim.x) * kRoundThreads) {
    accumulate_row_fixed<F, D>(poly, tables, i, products, num_products, terms);
  }
  store_partials<F, D>(partials + static_cast<u64>(blockIdx.x) * (kMaxDegree + 1), tree, poly);
}

// round 0, round_degree 6 .. 8: product lengths at run time
template <class F>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_columns_generic(typename F::fe* __restrict__ partials,
                               const column_view* __restrict__ views, u64 mid,
                               const product_desc<F>* __restrict__ products, u32 num_products,
                               const u32* __restrict__ terms, u32 degree) {
  using fe = typename F::fe;
  __shared__ fe tree[kRoundThreads];
  fe poly[kMaxDegree + 1];
  for (u32 k = 0; k <= kMaxDegree; ++k) poly[k] = F::zero();
  const column_tables<F> tables{views, mid};
  for (u64 i = static_cast<u64>(blockIdx.x) * kRoundThreads + threadIdx.x; i < mid;
       i += static_cast<u64>(gridDim.x) * kRoundThreads) {
    accumulate_row<F>(poly, tables, i, products, num_products, terms);
  }
  for (u32 k = 0; k <= degree; ++k) {
    const fe sum = block_sum<F>(tree, poly[k]);
    if (threadIdx.x == 0) partials[static_cast<u64>(blockIdx.x) * (kMaxDegree + 1) + k] = sum;
  }
}

template <class F, u32 D>
void launch_columns_round(hipStream_t stream, u32 blocks, typename F::fe* d_partials,
                          const column_view* d_views, u64 mid, const product_desc<F>* d_products,
                          u32 num_products, const u32* d_terms, u32 degree) {
  if (degree == D) {
    hipLaunchKernelGGL((k_sumcheck_columns_round<F, D>), dim3(blocks), dim3(kRoundThreads), 0,
                       stream, d_partials, d_views, mid, d_products, num_products, d_terms);
    return;
  }
  if constexpr (D < kFixedDegree) {
    launch_columns_round<F, D + 1>(stream, blocks, d_partials, d_views, mid, d_products,
                                   num_products, d_terms, degree);
  } else {
    hipLaunchKernelGGL((k_sumcheck_columns_generic<F>), dim3(blocks), dim3(kRoundThreads), 0,
                       stream, d_partials, d_views, mid, d_products, num_products, d_terms, degree);
  }
}
} // namespace
} // namespace bz::proof
