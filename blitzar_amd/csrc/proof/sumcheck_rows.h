// What the translation units of the sumcheck provers share (proof/sumcheck.hip: the prover with the
// caller's transcript and the kernels on engine-form tables; proof/sumcheck_columns.hip: round 0
// and the first fold on typed columns; proof/sumcheck_transcript.hip: the chain with the built-in
// transcript): the two fields' element conversions and the dispatch on the field id, the shape of a
// proof (variables, round workgroups), the row arithmetic of a round and the bodies of the round
// kernels, written once over a `Tables` type that says where a row's a_j and b_j come from, the
// workgroup reductions, and the fold of one element of engine-form tables.
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "blitzar_amd/csrc/field/mont29.h"
#include "blitzar_amd/csrc/proof/scalar25.h"
#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
constexpr u32 kMaxDegree = 8; // round polynomials of degree <= 8 (9 coefficients in registers)
constexpr u32 kFixedDegree = 5; // round degrees with the row expansion fixed at compile time
constexpr u32 kRoundThreads = 128;
// workgroups of a round at most: 4 of 2 wavefronts per CU, the 2 wavefronts per SIMD the widest
// kernels get (measured against 512: 3-12 % slower, and 2048: within 3 % either way)
constexpr u32 kRoundBlocks = 1024;

// caller representation <-> engine representation (Montgomery, normalised, V < 4)
struct scalar25519_elements {
  using F = scalar25_field;
  static constexpr u32 element_bytes = 32, product_stride = 36;
  BZ_HD static F::fe load(const u8* p) { return s25::to_mont(s25::load(p)); }
  BZ_HD static void store(u8* p, const F::fe& v) { s25::store(p, s25::from_mont(v)); }
  // the same bytes as little-endian words (for destinations known to be 8-byte aligned)
  BZ_HD static void store_words(u64* w, const F::fe& v) { s25::store_words(w, s25::from_mont(v)); }
  // engine form of little-endian words: of an element's 32 bytes (`element`: what load() makes of
  // those bytes) or of an integer below 2^248, as raw * conversion(element) / R
  BZ_HD static F::fe conversion(bool element) {
    (void)element; // the caller's representation is the plain integer
    return s25::r2();
  }
  BZ_HD static F::fe convert(const u64* w, bool element) {
    return F::mul(F::from_words(w), conversion(element));
  }
};
struct grumpkin_elements {
  using F = grumpkin_fq29;
  static constexpr u32 element_bytes = 32, product_stride = 40;
  BZ_HD static F::fe load(const u8* p) {
    u64 w[4];
    std::memcpy(w, p, 32);
    return F::from_mont64(w);
  }
  BZ_HD static void store(u8* p, const F::fe& v) {
    u64 w[4];
    F::to_mont64(w, v);
    std::memcpy(p, w, 32);
  }
  BZ_HD static void store_words(u64* w, const F::fe& v) { F::to_mont64(w, v); }
  // an element is x 2^256 and takes from_mont64's constant; an integer x becomes x R^2 / R with the
  // engine's R = 2^261: the caller's Montgomery form is never made
  BZ_HD static F::fe conversion(bool element) {
    F::fe c;
#pragma unroll
    for (int i = 0; i < F::N; ++i) {
      c.v[i] = element ? grumpkin_fq29_params::c_in(i) : grumpkin_fq29_params::r2(i);
    }
    return c;
  }
  BZ_HD static F::fe convert(const u64* w, bool element) {
    return F::mul(F::from_words(w), conversion(element));
  }
};

// fn(elements) for the field's conversions (blitzar_api.h SXT_FIELD_*): the one place that knows
// which field ids exist
template <class Fn> decltype(auto) with_elements(unsigned field_id, Fn&& fn) {
  BZ_RELEASE_ASSERT(field_id <= 1, "unsupported field id");
  if (field_id == 0) return fn(scalar25519_elements{});
  return fn(grumpkin_elements{});
}

// variables of a proof over n rows, and the workgroups of a round over `mid` pairs of rows
inline u32 variables_of(u64 n) {
  u32 v = 0;
  while ((u64{1} << v) < n) ++v;
  return v == 0 ? 1 : v;
}
inline u32 round_blocks(u64 mid) {
  return static_cast<u32>(std::min<u64>(kRoundBlocks, (mid + kRoundThreads - 1) / kRoundThreads));
}

template <class F> BZ_HD typename F::fe fadd(const typename F::fe& a, const typename F::fe& b) {
  return F::reduce(F::norm(F::add(a, b)));
}
template <class F> BZ_HD typename F::fe fsub(const typename F::fe& a, const typename F::fe& b) {
  return F::reduce(F::norm(F::template sub<8>(a, b)));
}
template <class F> BZ_HD typename F::fe fneg(const typename F::fe& a) {
  return F::reduce(F::norm(F::template neg<8>(a)));
}

// product p (engine form): multiplier, terms [first_term, first_term + num_terms)
template <class F> struct product_desc {
  typename F::fe multiplier;
  u32 first_term, num_terms;
};

// the descriptor's products in engine form, checked against round_degree and num_mles
template <class E> std::vector<product_desc<typename E::F>> engine_products(const sumcheck_inputs& d) {
  using F = typename E::F;
  std::vector<product_desc<F>> products(d.num_products);
  u32 first = 0;
  for (u32 p = 0; p < d.num_products; ++p) {
    const u8* entry = static_cast<const u8*>(d.product_table) + static_cast<size_t>(E::product_stride) * p;
    u32 num_terms;
    std::memcpy(&num_terms, entry + E::element_bytes, sizeof(num_terms));
    BZ_RELEASE_ASSERT(num_terms >= 1 && num_terms <= d.round_degree,
                      "a sumcheck product must have between 1 and round_degree terms");
    products[p] = product_desc<F>{E::load(entry), first, num_terms};
    first += num_terms;
  }
  BZ_RELEASE_ASSERT(first == d.num_product_terms, "num_product_terms does not match the product table");
  for (u32 t = 0; t < d.num_product_terms; ++t) {
    BZ_RELEASE_ASSERT(d.product_terms[t] < d.num_mles, "product term refers to a missing MLE");
  }
  return products;
}

// `Tables` of a round: pair(mle, i, row(i), a, b) yields a = f_mle[i] and b = f_mle[mid + i] - a
// (rows without a partner: b = -a) of the round's `mid`; row(i) is whatever is worth working out
// once per row.
//
// engine-form tables of n rows, column-major; per row: whether it has a partner
template <class F> struct dense_tables {
  const typename F::fe* mles;
  u64 n, mid;
  BZ_HD bool row(u64 i) const { return mid + i < n; }
  BZ_HD void pair(u32 mle, u64 i, bool paired, typename F::fe& a, typename F::fe& b) const {
    const typename F::fe* column = mles + static_cast<u64>(mle) * n;
    a = column[i];
    b = paired ? fsub<F>(column[mid + i], a) : fneg<F>(a);
  }
};

// poly[0 .. degree] += sum_products mult * prod_j (a_j + b_j X) for row i
// (polynomial_utility.h:64-137 expand_products / partial_expand_products; cpu_driver.h:75-102)
template <class F, class Tables>
BZ_HD void accumulate_row(typename F::fe* poly, const Tables& tables, u64 i,
                          const product_desc<F>* products, u32 num_products, const u32* terms) {
  using fe = typename F::fe;
  const auto row = tables.row(i);
  for (u32 pi = 0; pi < num_products; ++pi) {
    const product_desc<F>& pd = products[pi];
    fe p[kMaxDegree + 1];
    for (u32 t = 0; t < pd.num_terms; ++t) {
      fe a, b;
      tables.pair(terms[pd.first_term + t], i, row, a, b);
      if (t == 0) {
        p[0] = a;
        p[1] = b;
        continue;
      }
      // p <- p * (a + b X)
      fe previous = p[0];
      p[0] = F::mul(previous, a);
      for (u32 k = 1; k <= t; ++k) {
        const fe current = p[k];
        p[k] = fadd<F>(F::mul(current, a), F::mul(previous, b));
        previous = current;
      }
      p[t + 1] = F::mul(previous, b);
    }
    for (u32 k = 0; k <= pd.num_terms; ++k) {
      poly[k] = fadd<F>(poly[k], F::mul(pd.multiplier, p[k]));
    }
  }
}

// The same sum with every product length known at compile time (round_degree D <= kFixedDegree): the
// term loops are recursions over the term index, so p[] and poly[] are only ever indexed with
// constants and live in registers.  Algebraically equal to accumulate_row, with fewer products:
// the multiplier goes into the first factor (2 products instead of length + 1) and a middle
// coefficient p[k] a + p[k - 1] b is one mul2 (one Montgomery reduction for two products).
//
// poly[K] += c.  The pin keeps the sums of the different product lengths apart: merged into one
// tail behind the branches they would index poly[] through a run-time pointer (scratch memory).
template <class F, u32 K> BZ_HD void add_coefficient(typename F::fe* poly, const typename F::fe& c) {
  poly[K] = fadd<F>(poly[K], c);
  F::pin(poly[K]);
}
// coefficients K .. 0 of p <- p * (a + b X), top coefficient already written; for the product's
// last factor (Last) every coefficient goes to poly[] as soon as it is final
template <class F, u32 K, bool Last>
BZ_HD void mul_linear(typename F::fe* poly, typename F::fe* p, const typename F::fe& a,
                      const typename F::fe& b) {
  if constexpr (K == 0) {
    p[0] = F::mul(p[0], a);
  } else {
    p[K] = F::mul2(p[K], a, p[K - 1], b);
  }
  if constexpr (Last) add_coefficient<F, K>(poly, p[K]);
  if constexpr (K > 0) mul_linear<F, K - 1, Last>(poly, p, a, b);
}
// p[0 .. T + 1] <- mult * prod_{t <= T} (a_t + b_t X), then terms T + 1 .. L - 1
template <class F, u32 L, u32 T, class Tables, class Row>
BZ_HD void expand_terms(typename F::fe* poly, typename F::fe* p, const Tables& tables, u64 i,
                        const Row& row, const typename F::fe& multiplier, const u32* terms) {
  using fe = typename F::fe;
  constexpr bool last = T + 1 == L;
  fe a, b;
  tables.pair(terms[T], i, row, a, b);
  if constexpr (T == 0) {
    p[0] = F::mul(multiplier, a);
    p[1] = F::mul(multiplier, b);
    if constexpr (last) {
      add_coefficient<F, 0>(poly, p[0]);
      add_coefficient<F, 1>(poly, p[1]);
    }
  } else {
    p[T + 1] = F::mul(p[T], b);
    if constexpr (last) add_coefficient<F, T + 1>(poly, p[T + 1]);
    mul_linear<F, T, last>(poly, p, a, b);
  }
  if constexpr (!last) expand_terms<F, L, T + 1>(poly, p, tables, i, row, multiplier, terms);
}
// the product's length picks the expansion (the same for every row: uniform over a wavefront)
template <class F, u32 D, u32 L, class Tables, class Row>
BZ_HD void accumulate_product(typename F::fe* poly, const Tables& tables, u64 i, const Row& row,
                              const product_desc<F>& pd, const u32* terms) {
  if (pd.num_terms == L) {
    typename F::fe p[L + 1];
    expand_terms<F, L, 0>(poly, p, tables, i, row, pd.multiplier, terms + pd.first_term);
    return;
  }
  if constexpr (L < D) accumulate_product<F, D, L + 1>(poly, tables, i, row, pd, terms);
}
// poly[0 .. D] += row i's contribution; every product has between 1 and D terms
template <class F, u32 D, class Tables>
BZ_HD void accumulate_row_fixed(typename F::fe* poly, const Tables& tables, u64 i,
                                const product_desc<F>* products, u32 num_products,
                                const u32* terms) {
  const auto row = tables.row(i);
  for (u32 pi = 0; pi < num_products; ++pi) {
    accumulate_product<F, D, 1>(poly, tables, i, row, products[pi], terms);
  }
}

// the workgroup's sum of `mine` over its threads, valid in thread 0
template <class F> BZ_DEV typename F::fe block_sum(typename F::fe* tree, const typename F::fe mine) {
  tree[threadIdx.x] = mine;
  __syncthreads();
  for (u32 stride = kRoundThreads / 2; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      tree[threadIdx.x] = fadd<F>(tree[threadIdx.x], tree[threadIdx.x + stride]);
    }
    __syncthreads();
  }
  const typename F::fe sum = tree[0];
  __syncthreads();
  return sum;
}
// partials[k] = the workgroup's sum of poly[k], k <= D: one tree for all coefficients (the D + 1
// sums of a stage are independent: one barrier per stage, not one per stage and coefficient)
template <class F, u32 D>
BZ_DEV void store_partials(typename F::fe* partials, typename F::fe (*tree)[kRoundThreads],
                           const typename F::fe* poly) {
#pragma unroll
  for (u32 k = 0; k <= D; ++k) tree[k][threadIdx.x] = poly[k];
  __syncthreads();
  for (u32 stride = kRoundThreads / 2; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
#pragma unroll
      for (u32 k = 0; k <= D; ++k) {
        tree[k][threadIdx.x] = fadd<F>(tree[k][threadIdx.x], tree[k][threadIdx.x + stride]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x <= D) partials[threadIdx.x] = tree[threadIdx.x][0];
}

// The bodies of the round kernels (k_sumcheck_round_fixed and k_sumcheck_round of
// proof/sumcheck.hip, k_sumcheck_columns_round and k_sumcheck_columns_generic of
// proof/sumcheck_columns.hip), which differ in their `Tables` alone:
// partials[block][k] = the block's share of coefficient k of the round polynomial.
// round_degree D <= kFixedDegree: no array is indexed at run time (no scratch memory)
template <class F, u32 D, class Tables>
BZ_DEV void round_fixed_body(typename F::fe* partials, const Tables& tables,
                             const product_desc<F>* products, u32 num_products, const u32* terms) {
  using fe = typename F::fe;
  __shared__ fe tree[D + 1][kRoundThreads];
  fe poly[D + 1];
#pragma unroll
  for (u32 k = 0; k <= D; ++k) poly[k] = F::zero();
  for (u64 i = static_cast<u64>(blockIdx.x) * kRoundThreads + threadIdx.x; i < tables.mid;
       i += static_cast<u64>(gridDim.x) * kRoundThreads) {
    accumulate_row_fixed<F, D>(poly, tables, i, products, num_products, terms);
  }
  store_partials<F, D>(partials + static_cast<u64>(blockIdx.x) * (kMaxDegree + 1), tree, poly);
}
// round_degree 6 .. 8: product lengths at run time (p[] and poly[] live in scratch memory).
// `poly`: the kernel's own array of kMaxDegree + 1 coefficients -- declared here it would be an
// inlined stack object with lifetime markers, which changes the kernel's register report
template <class F, class Tables>
BZ_DEV void round_generic_body(typename F::fe* partials, typename F::fe* poly, const Tables& tables,
                               const product_desc<F>* products, u32 num_products, const u32* terms,
                               u32 degree) {
  using fe = typename F::fe;
  __shared__ fe tree[kRoundThreads];
  for (u32 k = 0; k <= kMaxDegree; ++k) poly[k] = F::zero();
  for (u64 i = static_cast<u64>(blockIdx.x) * kRoundThreads + threadIdx.x; i < tables.mid;
       i += static_cast<u64>(gridDim.x) * kRoundThreads) {
    accumulate_row<F>(poly, tables, i, products, num_products, terms);
  }
  for (u32 k = 0; k <= degree; ++k) {
    const fe sum = block_sum<F>(tree, poly[k]);
    if (threadIdx.x == 0) partials[static_cast<u64>(blockIdx.x) * (kMaxDegree + 1) + k] = sum;
  }
}

// The fold of engine-form tables of n rows, one output element (cpu_driver.h:106-143):
// (1 - r) in[m n + i] + r in[m n + mid + i], rows without a partner: (1 - r) in[m n + i].
// `Index`: the caller's own index type, so that its address arithmetic stays what it was
template <class F, class Index>
BZ_HD typename F::fe fold_element(const typename F::fe* in, u64 n, Index mid, Index m, Index i,
                                  const typename F::fe& r, const typename F::fe& one_minus_r) {
  typename F::fe v = F::mul(in[m * n + i], one_minus_r);
  if (mid + i < n) v = fadd<F>(v, F::mul(r, in[m * n + mid + i]));
  return v;
}
// where a fold kernel's element goes: to the caller's `evaluations` (not null: the last fold of a
// chain) in the caller's representation, else to the next table
template <class E>
BZ_HD void store_folded(typename E::F::fe* out, u8* evaluations, u64 id,
                        const typename E::F::fe& v) {
  if (evaluations != nullptr) {
    E::store(evaluations + E::element_bytes * id, v);
  } else {
    out[id] = v;
  }
}

// Round 0 and the first fold from another source than engine-form tables (typed columns,
// proof/sumcheck_columns.hip).  With one, prove() never holds the tables at full size on the
// device: its working tables are the folded half and quarter.
template <class F> struct first_round_source {
  using fe = typename F::fe;
  virtual ~first_round_source() = default;
  // the proof's products (engine form, `terms` on the host), before anything below on a device
  virtual void bind(const product_desc<F>* products, u32 num_products, const u32* terms) = 0;
  // device memory stage() takes from the call's arena
  virtual size_t device_bytes() const = 0;
  // whatever round() and fold() need on the device, enqueued on `stream`
  virtual void stage(device_arena& arena, hipStream_t stream) = 0;
  // partials[block][k] as the round kernels of proof/sumcheck.hip leave them; `terms` on the device
  virtual void round(hipStream_t stream, u32 blocks, fe* partials, u64 mid, const u32* terms,
                     u32 degree) = 0;
  // out[m * mid + i] = (1 - r) f_m[i] + r f_m[mid + i], every i < mid
  virtual void fold(hipStream_t stream, fe* out, u64 mid, const fe& r, const fe& one_minus_r) = 0;
  // host backend: out[m * n + i] = f_m[i] in engine form
  virtual void load_host(fe* out, u64 n) const = 0;
};

// The prover of proof/sumcheck.hip (E: scalar25519_elements or grumpkin_elements).  `source`
// (may be null): the source of round 0 and the first fold, d.mles is then not read.
template <class E>
void prove(api_state& st, u8* polynomials, u8* evaluation_point, u8* mle_evaluations,
           const sumcheck_inputs& d, void* callback, void* context, api_state::device_lease* lease,
           const sumcheck_device_tables* device_tables, first_round_source<typename E::F>* source);
// the limits every entry point shares
void check_sumcheck_limits(const sumcheck_inputs& d);
// kernels of proof/sumcheck.hip, enqueued on `stream`: out[i] = E::load(elements + 32 i), and the
// round kernel for `degree` (partials[block][k], `blocks` workgroups)
template <class E>
void launch_sumcheck_load(hipStream_t stream, typename E::F::fe* out, const u8* elements, u64 count);
template <class F>
void launch_sumcheck_round(hipStream_t stream, u32 blocks, typename F::fe* partials,
                           const typename F::fe* mles, u64 n, u64 mid,
                           const product_desc<F>* products, u32 num_products, const u32* terms,
                           u32 degree);
} // namespace bz::proof
