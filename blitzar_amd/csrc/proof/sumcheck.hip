// Sumcheck prover (sxt_prove_sumcheck; reference: cbindings/sumcheck.cc, sxt/cbindings/backend/
// cpu_backend.cc:73-112, sxt/proof/sumcheck/{proof_computation,cpu_driver,polynomial_utility}.h).
//
// The polynomial is  sum_p mult_p * prod_{j in terms_p} f_j(X_1 .. X_r)  over multilinear
// extensions f_j given by their n evaluations (column-major n x num_mles).  Round t fixes the top
// variable: with mid = 2^(r-1-t), every row i < mid contributes  mult_p * prod_j (a_j + b_j X),
// a_j = f_j[i], b_j = f_j[mid + i] - a_j (rows without a partner: b_j = -a_j), to the round
// polynomial; the caller's transcript callback turns the polynomial into the challenge r; the
// tables fold to (1 - r) f[i] + r f[mid + i].  Outputs are field elements in the caller's
// representation, canonical, hence identical to the reference's bytes.
//
// Fields (blitzar_api.h SXT_FIELD_*): 0 = curve25519 scalar field (32 little-endian bytes,
// proof/scalar25.h), 1 = Grumpkin base field (4 x 64-bit Montgomery limbs, field/mont29.h
// grumpkin_fq29).  Both compute on the 9 x 29-bit Montgomery representation.
//
// GPU backend: the tables live in HBM in engine form; k_sumcheck_round_fixed (round_degree <= 5: the
// row expansion is written out per product length at compile time, so partial product and round
// polynomial stay in registers) or k_sumcheck_round (round_degree 6 .. 8: run-time lengths) reduces
// every row's contribution to per-workgroup partial polynomials, k_sumcheck_finish adds those up,
// k_sumcheck_fold folds.  The host backend runs the same row arithmetic on the host.
//
// bzamd_prove_sumcheck* additionally return f_j(r_1 .. r_v): the tables folded once more by the
// last challenge.  The device form reads the caller's tables straight from HBM (k_sumcheck_load) on
// the caller's stream and never writes them.
//
// The row arithmetic lives in proof/sumcheck_rows.h.  prove() can take round 0 and the first fold
// from a first_round_source (typed columns, proof/sumcheck_columns.hip); the tables are then never
// held at full size on the device.
#include "blitzar_amd/csrc/proof/sumcheck.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "blitzar_amd/csrc/proof/sumcheck_rows.h"

namespace bz::proof {
std::atomic<u64> g_sumcheck_arena_bytes{0};

namespace {
//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
template <class E>
__global__ void __launch_bounds__(256)
    k_sumcheck_load(typename E::F::fe* __restrict__ out, const u8* __restrict__ elements, u64 count) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < count) out[i] = E::load(elements + E::element_bytes * i);
}

// the round kernels on engine-form tables (the bodies: proof/sumcheck_rows.h)
template <class F, u32 D>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_round_fixed(typename F::fe* __restrict__ partials,
                           const typename F::fe* __restrict__ mles, u64 n, u64 mid,
                           const product_desc<F>* __restrict__ products, u32 num_products,
                           const u32* __restrict__ terms) {
  round_fixed_body<F, D>(partials, dense_tables<F>{mles, n, mid}, products, num_products, terms);
}
template <class F>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_round(typename F::fe* __restrict__ partials, const typename F::fe* __restrict__ mles,
                     u64 n, u64 mid, const product_desc<F>* __restrict__ products, u32 num_products,
                     const u32* __restrict__ terms, u32 degree) {
  typename F::fe poly[kMaxDegree + 1];
  round_generic_body<F>(partials, poly, dense_tables<F>{mles, n, mid}, products, num_products,
                        terms, degree);
}

// poly[k] = sum_blocks partials[block][k]: workgroup k adds up coefficient k
template <class F>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_finish(typename F::fe* __restrict__ poly, const typename F::fe* __restrict__ partials,
                      u32 blocks) {
  using fe = typename F::fe;
  __shared__ fe tree[kRoundThreads];
  const u32 k = blockIdx.x;
  fe mine = F::zero();
  for (u32 b = threadIdx.x; b < blocks; b += kRoundThreads) {
    mine = fadd<F>(mine, partials[static_cast<u64>(b) * (kMaxDegree + 1) + k]);
  }
  const fe sum = block_sum<F>(tree, mine);
  if (threadIdx.x == 0) poly[k] = sum;
}

// out[m * mid + i] = (1 - r) in[m * n + i] + r in[m * n + mid + i]
template <class F>
__global__ void __launch_bounds__(256)
    k_sumcheck_fold(typename F::fe* __restrict__ out, const typename F::fe* __restrict__ in, u64 n,
                    u64 mid, u32 num_mles, typename F::fe r, typename F::fe one_minus_r) {
  const u64 id = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= mid * num_mles) return;
  out[id] = fold_element<F, u64>(in, n, mid, id / mid, id % mid, r, one_minus_r);
}

//--------------------------------------------------------------------------------------------------
template <class F, u32 D>
void launch_round(hipStream_t stream, u32 blocks, typename F::fe* d_partials,
                  const typename F::fe* d_mles, u64 n, u64 mid, const product_desc<F>* d_products,
                  u32 num_products, const u32* d_terms, u32 degree) {
  if (degree == D) {
    hipLaunchKernelGGL((k_sumcheck_round_fixed<F, D>), dim3(blocks), dim3(kRoundThreads), 0, stream,
                       d_partials, d_mles, n, mid, d_products, num_products, d_terms);
    return;
  }
  if constexpr (D < kFixedDegree) {
    launch_round<F, D + 1>(stream, blocks, d_partials, d_mles, n, mid, d_products, num_products,
                           d_terms, degree);
  } else {
    hipLaunchKernelGGL((k_sumcheck_round<F>), dim3(blocks), dim3(kRoundThreads), 0, stream,
                       d_partials, d_mles, n, mid, d_products, num_products, d_terms, degree);
  }
}

// the host backend's round: the same row arithmetic as the kernels
template <class F, u32 D>
void host_round(typename F::fe* poly, const typename F::fe* mles, u64 n, u64 mid,
                const product_desc<F>* products, u32 num_products, const u32* terms, u32 degree) {
  const dense_tables<F> tables{mles, n, mid};
  if (degree == D) {
    for (u64 i = 0; i < mid; ++i) {
      accumulate_row_fixed<F, D>(poly, tables, i, products, num_products, terms);
    }
    return;
  }
  if constexpr (D < kFixedDegree) {
    host_round<F, D + 1>(poly, mles, n, mid, products, num_products, terms, degree);
  } else {
    for (u64 i = 0; i < mid; ++i) accumulate_row<F>(poly, tables, i, products, num_products, terms);
  }
}

} // namespace

// the load and round kernels for the other provers over engine-form tables
// (proof/sumcheck_transcript.hip)
template <class E>
void launch_sumcheck_load(hipStream_t stream, typename E::F::fe* out, const u8* elements, u64 count) {
  hipLaunchKernelGGL((k_sumcheck_load<E>), dim3(ceil_div_u32(count, 256)), dim3(256), 0, stream, out,
                     elements, count);
}
template void launch_sumcheck_load<scalar25519_elements>(hipStream_t, scalar25_field::fe*, const u8*, u64);
template void launch_sumcheck_load<grumpkin_elements>(hipStream_t, grumpkin_fq29::fe*, const u8*, u64);
template <class F>
void launch_sumcheck_round(hipStream_t stream, u32 blocks, typename F::fe* partials,
                           const typename F::fe* mles, u64 n, u64 mid,
                           const product_desc<F>* products, u32 num_products, const u32* terms,
                           u32 degree) {
  launch_round<F, 1>(stream, blocks, partials, mles, n, mid, products, num_products, terms, degree);
}
template void launch_sumcheck_round<scalar25_field>(hipStream_t, u32, scalar25_field::fe*,
                                                    const scalar25_field::fe*, u64, u64,
                                                    const product_desc<scalar25_field>*, u32,
                                                    const u32*, u32);
template void launch_sumcheck_round<grumpkin_fq29>(hipStream_t, u32, grumpkin_fq29::fe*,
                                                   const grumpkin_fq29::fe*, u64, u64,
                                                   const product_desc<grumpkin_fq29>*, u32,
                                                   const u32*, u32);

template <class E>
void prove(api_state& st, u8* polynomials, u8* evaluation_point, u8* mle_evaluations,
           const sumcheck_inputs& d, void* callback, void* context, api_state::device_lease* lease,
           const sumcheck_device_tables* device_tables, first_round_source<typename E::F>* source) {
  using F = typename E::F;
  using fe = typename F::fe;
  using callback_t = void (*)(void* r, void* context, const void* polynomial, unsigned length);
  const u32 degree = d.round_degree;
  const u32 length = degree + 1;
  u64 n = d.n;
  const u32 num_variables = variables_of(n);

  const std::vector<product_desc<F>> products = engine_products<E>(d);

  const bool on_device = st.backend == 2;
  const u64 total = n * d.num_mles;
  std::vector<fe> h_mles, h_next;
  fe* d_mles = nullptr;
  fe* d_next = nullptr;
  fe* d_partials = nullptr;
  fe* d_poly = nullptr;
  product_desc<F>* d_products = nullptr;
  u32* d_terms = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  device_arena own; // not the device's staging arena: the lease is given up around the callback
  if (on_device) {
    if (device_tables != nullptr) {
      device = device_tables->device;
      stream = device_tables->stream;
    } else {
      device = st.primary().device;
      stream = st.primary().stream;
    }
    BZ_HIP_CHECK(hipSetDevice(device));
    const u64 half = (u64{1} << (num_variables - 1)) * d.num_mles;
    // host tables are uploaded as they are and converted on the device; device tables are
    // converted straight from the caller's memory
    const size_t raw_bytes =
        device_tables != nullptr || source != nullptr ? 0 : static_cast<size_t>(E::element_bytes) * total;
    // the tables a round reads and the tables its fold writes: full size and half, or, round 0
    // and its fold reading `source`, quarter (unused until the second fold) and half
    const u64 round_table = source != nullptr ? half / 2 : total;
    if (source != nullptr) source->bind(products.data(), d.num_products, d.product_terms);
    const size_t arena_bytes =
        device_arena::padded(raw_bytes) + device_arena::padded(sizeof(fe) * round_table) +
        device_arena::padded(sizeof(fe) * half) + (source != nullptr ? source->device_bytes() : 0) +
        device_arena::padded(sizeof(fe) * kRoundBlocks * (kMaxDegree + 1)) +
        device_arena::padded(sizeof(fe) * (kMaxDegree + 1)) +
        device_arena::padded(sizeof(product_desc<F>) * products.size()) +
        device_arena::padded(sizeof(u32) * d.num_product_terms) + 4096;
    g_sumcheck_arena_bytes.store(arena_bytes);
    own.reset(arena_bytes, stream);
    const u8* d_raw = static_cast<const u8*>(d.mles);
    if (source != nullptr) {
      source->stage(own, stream);
    } else if (device_tables == nullptr) {
      u8* staged = own.take<u8>(raw_bytes);
      BZ_HIP_CHECK(hipMemcpyAsync(staged, d.mles, raw_bytes, hipMemcpyHostToDevice, stream));
      d_raw = staged;
    }
    d_mles = own.take<fe>(round_table);
    d_next = own.take<fe>(half);
    d_partials = own.take<fe>(static_cast<size_t>(kRoundBlocks) * (kMaxDegree + 1));
    d_poly = own.take<fe>(kMaxDegree + 1);
    d_products = own.take<product_desc<F>>(products.size());
    d_terms = own.take<u32>(d.num_product_terms);
    BZ_HIP_CHECK(hipMemcpyAsync(d_products, products.data(), sizeof(product_desc<F>) * products.size(),
                                hipMemcpyHostToDevice, stream));
    BZ_HIP_CHECK(hipMemcpyAsync(d_terms, d.product_terms, sizeof(u32) * d.num_product_terms,
                                hipMemcpyHostToDevice, stream));
    if (source == nullptr) {
      hipLaunchKernelGGL((k_sumcheck_load<E>), dim3(ceil_div_u32(total, 256)), dim3(256), 0, stream,
                         d_mles, d_raw, total);
      BZ_HIP_CHECK(hipGetLastError());
      g_kernel_launches += 1;
    }
  } else {
    h_mles.resize(total);
    if (source != nullptr) {
      source->load_host(h_mles.data(), n);
    } else {
      const u8* raw = static_cast<const u8*>(d.mles);
      for (u64 i = 0; i < total; ++i) h_mles[i] = E::load(raw + E::element_bytes * i);
    }
  }

  for (u32 round = 0; round < num_variables; ++round) {
    const u64 mid = u64{1} << (num_variables - 1 - round);
    std::vector<fe> poly(kMaxDegree + 1, F::zero());
    if (on_device) {
      const u32 blocks = round_blocks(mid);
      if (source != nullptr && round == 0) {
        source->round(stream, blocks, d_partials, mid, d_terms, degree);
      } else {
        launch_round<F, 1>(stream, blocks, d_partials, d_mles, n, mid, d_products, d.num_products,
                           d_terms, degree);
      }
      BZ_HIP_CHECK(hipGetLastError());
      g_kernel_launches += 1;
      // one workgroup's partials are the round polynomial
      if (blocks > 1) {
        hipLaunchKernelGGL((k_sumcheck_finish<F>), dim3(length), dim3(kRoundThreads), 0, stream,
                           d_poly, d_partials, blocks);
        BZ_HIP_CHECK(hipGetLastError());
        g_kernel_launches += 1;
      }
      BZ_HIP_CHECK(hipMemcpyAsync(poly.data(), blocks > 1 ? d_poly : d_partials, sizeof(fe) * length,
                                  hipMemcpyDeviceToHost, stream));
      BZ_HIP_CHECK(hipStreamSynchronize(stream));
    } else {
      host_round<F, 1>(poly.data(), h_mles.data(), n, mid, products.data(), d.num_products,
                       d.product_terms, degree);
    }
    u8* out = polynomials + static_cast<size_t>(E::element_bytes) * length * round;
    for (u32 k = 0; k < length; ++k) E::store(out + E::element_bytes * k, poly[k]);
    // the caller's transcript draws the challenge (callback_sumcheck_transcript.h:27-45)
    u8* r_bytes = evaluation_point + static_cast<size_t>(E::element_bytes) * round;
    if (lease != nullptr) lease->unlock();
    reinterpret_cast<callback_t>(callback)(r_bytes, context, out, length);
    if (lease != nullptr) lease->relock();
    // the callback may have changed the thread's current device
    if (on_device) BZ_HIP_CHECK(hipSetDevice(device));
    // the fold by the last challenge leaves one row per MLE: f_j(r_1 .. r_v)
    if (round + 1 == num_variables && mle_evaluations == nullptr) break;
    const fe r = E::load(r_bytes);
    const fe one_minus_r = fsub<F>(F::one(), r);
    if (on_device) {
      if (source != nullptr && round == 0) {
        source->fold(stream, d_next, mid, r, one_minus_r);
      } else {
        hipLaunchKernelGGL((k_sumcheck_fold<F>), dim3(ceil_div_u32(mid * d.num_mles, 256)),
                           dim3(256), 0, stream, d_next, d_mles, n, mid, d.num_mles, r, one_minus_r);
      }
      BZ_HIP_CHECK(hipGetLastError());
      g_kernel_launches += 1;
      std::swap(d_mles, d_next);
    } else {
      h_next.assign(mid * d.num_mles, F::zero());
      for (u64 m = 0; m < d.num_mles; ++m) {
        for (u64 i = 0; i < mid; ++i) {
          h_next[m * mid + i] = fold_element<F, u64>(h_mles.data(), n, mid, m, i, r, one_minus_r);
        }
      }
      h_mles.swap(h_next);
    }
    n = mid;
  }
  if (mle_evaluations != nullptr) {
    if (on_device) {
      h_mles.resize(d.num_mles);
      BZ_HIP_CHECK(hipMemcpyAsync(h_mles.data(), d_mles, sizeof(fe) * d.num_mles,
                                  hipMemcpyDeviceToHost, stream));
      BZ_HIP_CHECK(hipStreamSynchronize(stream));
    }
    for (u32 m = 0; m < d.num_mles; ++m) {
      E::store(mle_evaluations + static_cast<size_t>(E::element_bytes) * m, h_mles[m]);
    }
  }
  if (on_device) {
    BZ_HIP_CHECK(hipStreamSynchronize(stream));
    own.release();
  }
}
template void prove<scalar25519_elements>(api_state&, u8*, u8*, u8*, const sumcheck_inputs&, void*,
                                          void*, api_state::device_lease*,
                                          const sumcheck_device_tables*,
                                          first_round_source<scalar25_field>*);
template void prove<grumpkin_elements>(api_state&, u8*, u8*, u8*, const sumcheck_inputs&, void*, void*,
                                       api_state::device_lease*, const sumcheck_device_tables*,
                                       first_round_source<grumpkin_fq29>*);

void check_sumcheck_limits(const sumcheck_inputs& d) {
  BZ_RELEASE_ASSERT(d.n > 0, "sumcheck needs at least one row");
  BZ_RELEASE_ASSERT(d.round_degree >= 1 && d.round_degree <= kMaxDegree,
                    "round_degree must be in [1, 8]");
  BZ_RELEASE_ASSERT(d.n <= (1u << 30), "sumcheck tables are limited to 2^30 rows");
}

void prove_sumcheck(api_state& st, void* polynomials, void* evaluation_point, void* mle_evaluations,
                    unsigned field_id, const sumcheck_inputs& d, void* callback, void* context,
                    api_state::device_lease* lease, const sumcheck_device_tables* device_tables) {
  check_sumcheck_limits(d);
  with_elements(field_id, [&](auto elements) {
    prove<decltype(elements)>(st, static_cast<u8*>(polynomials), static_cast<u8*>(evaluation_point),
                              static_cast<u8*>(mle_evaluations), d, callback, context, lease,
                              device_tables, nullptr);
  });
}
} // namespace bz::proof
