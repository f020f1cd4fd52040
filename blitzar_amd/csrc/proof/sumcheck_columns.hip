// Sumcheck over typed columns (bzamd_prove_sumcheck_columns / _device_columns): the MLEs are the
// columns a service holds and commits -- little-endian integers of 1 .. 31 bytes, signed up to 16,
// or 32-byte field elements, each with its own length -- described by the MSM's descriptors.
//
// The prover is the one of proof/sumcheck.hip.  What differs is where round 0 and the first fold
// read: the columns where they lie (k_sumcheck_columns_round, k_sumcheck_columns_generic, which
// the chain of proof/sumcheck_transcript.hip launches too, through launch_sumcheck_columns_round,
// and k_sumcheck_columns_fold).  No engine-form copy of the full tables exists on the device; from
// round 1 on the kernels of proof/sumcheck.hip run on the folded half.
//
// Neither kernel converts an element.  With R the engine's Montgomery radix, a loaded element is
// the RAW residue of its bytes: x itself for an integer or a curve25519 scalar, x 2^256 for a
// Grumpkin element, where the engine form is x R.  A Montgomery product with a raw factor comes out
// short of one conversion constant c (raw c / R = engine form: R^2, or R^2 / 2^256), and sums and
// differences do not care.  So round 0 multiplies every product's multiplier by the constants of
// its terms' columns, once on the host, and then runs the row arithmetic on raw a_j and b_j; the
// fold multiplies raw rows by r c / R and (1 - r) c / R, which lands in engine form.
// The host form on the GPU backend uploads the columns at their own width and takes the same path;
// the host backend converts while it loads its tables.
#include <cstring>
#include <vector>

#include "blitzar_amd/csrc/proof/sumcheck_columns.h"

namespace bz::proof {
namespace {
// row i < c.n in engine form (the host backend's tables)
template <class E> typename E::F::fe load_element(const column_view& c, u64 i) {
  using F = typename E::F;
  u64 w[4] = {0, 0, 0, 0};
  const bool negative = load_magnitude(w, c, i);
  const typename F::fe v = E::convert(w, c.nbytes == E::element_bytes);
  return F::select(v, fneg<F>(v), negative);
}

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
// round 0 (the bodies: proof/sumcheck_rows.h); `products`: the multipliers times their terms'
// conversion constants.  round_degree D <= kFixedDegree: k_sumcheck_round_fixed's expansion
template <class F, u32 D>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_columns_round(typename F::fe* __restrict__ partials,
                             const column_view* __restrict__ views, u64 mid,
                             const product_desc<F>* __restrict__ products, u32 num_products,
                             const u32* __restrict__ terms) {
  round_fixed_body<F, D>(partials, column_tables<F>{views, mid}, products, num_products, terms);
}
// round_degree 6 .. 8: product lengths at run time
template <class F>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_columns_generic(typename F::fe* __restrict__ partials,
                               const column_view* __restrict__ views, u64 mid,
                               const product_desc<F>* __restrict__ products, u32 num_products,
                               const u32* __restrict__ terms, u32 degree) {
  typename F::fe poly[kMaxDegree + 1];
  round_generic_body<F>(partials, poly, column_tables<F>{views, mid}, products, num_products,
                        terms, degree);
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

// r and 1 - r times the conversion constant of integers and of elements
template <class F> struct fold_factors {
  typename F::fe r[2], one_minus_r[2];
};
// the first fold: out[m * mid + i] = (1 - r) f_m[i] + r f_m[mid + i] in engine form, every i < mid
template <class F>
__global__ void __launch_bounds__(256)
    k_sumcheck_columns_fold(typename F::fe* __restrict__ out, const column_view* __restrict__ views,
                            u64 mid, u32 num_mles, fold_factors<F> factors) {
  const u64 id = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= mid * num_mles) return;
  const u64 m = id / mid, i = id % mid;
  const column_view c = views[m];
  const bool element = c.nbytes == 32;
  out[id] = fold_column_element<F>(
      c, mid, i, [&] { return F::select(factors.r[0], factors.r[1], element); },
      [&] { return F::select(factors.one_minus_r[0], factors.one_minus_r[1], element); });
}

//--------------------------------------------------------------------------------------------------
// `upload`: the columns are host memory and the proof runs on a device
template <class E> class column_source final : public first_round_source<typename E::F> {
public:
  using F = typename E::F;
  using fe = typename F::fe;

  column_source(const sumcheck_column* columns, u32 num_mles, bool upload)
      : views_(num_mles), upload_(upload) {
    for (u32 j = 0; j < num_mles; ++j) views_[j] = make_column_view(columns[j]);
  }

  void bind(const product_desc<F>* products, u32 num_products, const u32* terms) override {
    products_.resize(num_products);
    conversion_scaled_products<E>(products_.data(), products, num_products, terms, views_.data());
  }

  size_t device_bytes() const override {
    size_t bytes = device_arena::padded(sizeof(column_view) * views_.size()) +
                   device_arena::padded(sizeof(product_desc<F>) * products_.size());
    if (upload_) {
      for (const column_view& c : views_) bytes += device_arena::padded(c.n * c.nbytes);
    }
    return bytes;
  }

  void stage(device_arena& arena, hipStream_t stream) override {
    if (upload_) {
      for (column_view& c : views_) {
        const size_t bytes = c.n * c.nbytes;
        u8* staged = arena.take<u8>(bytes);
        if (bytes != 0) {
          BZ_HIP_CHECK(hipMemcpyAsync(staged, c.data, bytes, hipMemcpyHostToDevice, stream));
        }
        c.data = staged;
        c.access = access_of(staged, c.nbytes);
      }
    }
    d_views_ = arena.take<column_view>(views_.size());
    BZ_HIP_CHECK(hipMemcpyAsync(d_views_, views_.data(), sizeof(column_view) * views_.size(),
                                hipMemcpyHostToDevice, stream));
    d_products_ = arena.take<product_desc<F>>(products_.size());
    BZ_HIP_CHECK(hipMemcpyAsync(d_products_, products_.data(),
                                sizeof(product_desc<F>) * products_.size(), hipMemcpyHostToDevice,
                                stream));
  }

  void round(hipStream_t stream, u32 blocks, fe* partials, u64 mid, const u32* terms,
             u32 degree) override {
    launch_sumcheck_columns_round<F>(stream, blocks, partials, d_views_, mid, d_products_,
                                     static_cast<u32>(products_.size()), terms, degree);
  }

  void fold(hipStream_t stream, fe* out, u64 mid, const fe& r, const fe& one_minus_r) override {
    const u32 num_mles = static_cast<u32>(views_.size());
    fold_factors<F> factors;
    for (int element = 0; element < 2; ++element) {
      factors.r[element] = F::mul(r, E::conversion(element != 0));
      factors.one_minus_r[element] = F::mul(one_minus_r, E::conversion(element != 0));
    }
    hipLaunchKernelGGL((k_sumcheck_columns_fold<F>), dim3(ceil_div_u32(mid * num_mles, 256)),
                       dim3(256), 0, stream, out, d_views_, mid, num_mles, factors);
  }

  void load_host(fe* out, u64 n) const override {
    for (size_t m = 0; m < views_.size(); ++m) {
      const column_view& c = views_[m];
      for (u64 i = 0; i < n; ++i) out[m * n + i] = i < c.n ? load_element<E>(c, i) : F::zero();
    }
  }

private:
  std::vector<column_view> views_;
  std::vector<product_desc<F>> products_; // multipliers times their terms' conversion constants
  column_view* d_views_ = nullptr;
  product_desc<F>* d_products_ = nullptr;
  bool upload_;
};

} // namespace

// round 0 for the chain of proof/sumcheck_transcript.hip as well
template <class F>
void launch_sumcheck_columns_round(hipStream_t stream, u32 blocks, typename F::fe* partials,
                                   const column_view* views, u64 mid,
                                   const product_desc<F>* products, u32 num_products,
                                   const u32* terms, u32 degree) {
  launch_columns_round<F, 1>(stream, blocks, partials, views, mid, products, num_products, terms,
                             degree);
}
template void launch_sumcheck_columns_round<scalar25_field>(hipStream_t, u32, scalar25_field::fe*,
                                                            const column_view*, u64,
                                                            const product_desc<scalar25_field>*,
                                                            u32, const u32*, u32);
template void launch_sumcheck_columns_round<grumpkin_fq29>(hipStream_t, u32, grumpkin_fq29::fe*,
                                                           const column_view*, u64,
                                                           const product_desc<grumpkin_fq29>*, u32,
                                                           const u32*, u32);

void prove_sumcheck_columns(api_state& st, void* polynomials, void* evaluation_point,
                            void* mle_evaluations, unsigned field_id, const sumcheck_inputs& d,
                            const sumcheck_column* columns, void* callback, void* context,
                            api_state::device_lease* lease,
                            const sumcheck_device_tables* device_tables) {
  check_sumcheck_limits(d);
  check_column_lengths(d, columns);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    column_source<E> source(columns, d.num_mles, st.backend == 2 && device_tables == nullptr);
    prove<E>(st, static_cast<u8*>(polynomials), static_cast<u8*>(evaluation_point),
             static_cast<u8*>(mle_evaluations), d, callback, context, lease, device_tables,
             &source);
  });
}
} // namespace bz::proof
