// The verifier's half of an MLE opening in front of the inner-product verifier
// (proof/verify_opening.h), for proofs that stay in HBM.
//
//   k_verify_sumcheck       one workgroup of one wavefront per proof (blockIdx): verify<E> of
//                           proof/sumcheck_transcript.hip on the proof's bytes.  The transcript, the
//                           round's message and the challenge live in LDS; the Merlin logic is
//                           proof/transcript.h over wave_sponge, the protocol transcript_begin and
//                           transcript_round of proof/sumcheck_protocol.h.  The arithmetic of a
//                           round (D + 2 additions, D products) is done by every lane alike: the
//                           wavefront is there for the sponge.  1 launch for the whole batch.
//   k_check_evaluations     one workgroup per proof: products to lanes with a stride, block_sum,
//                           lane 0 compares.  1 launch for the whole batch, behind one copy of the
//                           statement through the pinned stage ring.
//   k_decode_commitments    one lane per compressed commitment -> ed_point rows in the workspace (the
//                           identity and `valid` = 0 for a rejected encoding); then ONE engine call
//                           with projective output over those rows as caller generators.
//                           1 launch + the engine's.
#include "blitzar_amd/csrc/proof/verify_opening.h"

#include <cstring>
#include <mutex>
#include <vector>

#include "blitzar_amd/csrc/curve/ed29.h"
#include "blitzar_amd/csrc/proof/sumcheck_protocol.h"
#include "blitzar_amd/csrc/proof/sumcheck_rows.h"
#include "blitzar_amd/csrc/proof/transcript.h"

namespace bz::proof {
namespace {
//--------------------------------------------------------------------------------------------------
// the sumcheck rounds
//--------------------------------------------------------------------------------------------------
// what the wavefront keeps in LDS: wave_transcript of proof/sumcheck_transcript.hip and the two
// canonical encodings a round compares
struct alignas(8) wave_verifier {
  transcript_state t;
  u8 pad[5];
  u8 message[(kMaxDegree + 1) * 32]; // the round polynomial as the prover wrote it
  u8 x[32], r[32];
  u8 have[32], want[32]; // 2 p[0] + p[1] + .. + p[D] and the running sum, canonical
};

template <class E>
__global__ void __launch_bounds__(64)
    k_verify_sumcheck(u32* __restrict__ verdicts, u8* __restrict__ expected_sums,
                      u8* __restrict__ evaluation_points, u8* __restrict__ transcripts,
                      const u8* __restrict__ polynomials, u32 num_variables, u32 degree) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ wave_verifier w;
  const u32 lane = threadIdx.x;
  const u64 proof = blockIdx.x;
  const u32 length = degree + 1;
  u8* transcript = transcripts + sizeof(transcript_state) * proof;
  u8* expected_sum = expected_sums + 32 * proof;
  u8* point = evaluation_points + static_cast<u64>(32) * num_variables * proof;
  const u8* p = polynomials + static_cast<u64>(32) * length * num_variables * proof;

  wave_load_transcript(w.t, transcript);
  transcript_begin<wave_sponge>(&w.t, num_variables, degree);
  if (lane == 0) E::store(w.want, E::load(expected_sum));
  u32 round = 0;
  for (; round < num_variables; ++round, p += 32 * length) {
    for (u32 i = lane; i < 32 * length; i += 64) w.message[i] = p[i];
    wave_sponge::sync();
    // p(0) + p(1)
    fe sum = E::load(w.message);
    sum = fadd<F>(sum, sum);
    for (u32 k = 1; k <= degree; ++k) sum = fadd<F>(sum, E::load(w.message + 32 * k));
    if (lane == 0) E::store(w.have, sum);
    wave_sponge::sync();
    const bool same = lane >= 32 || w.have[lane] == w.want[lane];
    if (__all(same) == 0) break; // what the rounds before left stays as it is
    const fe r = transcript_round<E, wave_sponge>(w.r, w.x, &w.t, w.message, length);
    wave_sponge::sync();
    if (lane < 32) point[32 * round + lane] = w.r[lane];
    // p(r) by Horner
    fe next = E::load(w.message + 32 * degree);
    for (u32 k = degree; k-- > 0;) next = fadd<F>(F::mul(next, r), E::load(w.message + 32 * k));
    if (lane == 0) E::store(w.want, next);
  }
  wave_sponge::sync();
  if (round != 0 && lane < 32) expected_sum[lane] = w.want[lane];
  wave_store_transcript(transcript, w.t);
  if (lane == 0) verdicts[proof] = round == num_variables ? 1 : 0;
}

//--------------------------------------------------------------------------------------------------
// the final evaluation check
//--------------------------------------------------------------------------------------------------
// sum_p mult_p prod_{j in terms_p} evaluations[j] of one proof; the sum is engine form
template <class E>
BZ_HD typename E::F::fe product_value(const product_desc<typename E::F>& pd, const u32* terms,
                                      const u8* evaluations) {
  using F = typename E::F;
  typename F::fe v = pd.multiplier;
  for (u32 t = 0; t < pd.num_terms; ++t) {
    v = F::mul(v, E::load(evaluations + static_cast<u64>(E::element_bytes) * terms[pd.first_term + t]));
  }
  return v;
}
template <class E>
BZ_HD bool sums_agree(const typename E::F::fe& sum, const u8* expected_sum) {
  using F = typename E::F;
  return F::is_zero(fsub<F>(sum, E::load(expected_sum)));
}

template <class E>
__global__ void __launch_bounds__(kRoundThreads)
    k_check_evaluations(u32* __restrict__ verdicts, const u8* __restrict__ expected_sums,
                        const u8* __restrict__ evaluations, u32 num_mles,
                        const product_desc<typename E::F>* __restrict__ products, u32 num_products,
                        const u32* __restrict__ terms) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[kRoundThreads];
  const u64 proof = blockIdx.x;
  const u8* mine = evaluations + static_cast<u64>(E::element_bytes) * num_mles * proof;
  fe sum = F::zero();
  for (u32 p = threadIdx.x; p < num_products; p += kRoundThreads) {
    sum = fadd<F>(sum, product_value<E>(products[p], terms, mine));
  }
  const fe total = block_sum<F>(tree, sum);
  if (threadIdx.x == 0) {
    verdicts[proof] = sums_agree<E>(total, expected_sums + E::element_bytes * proof) ? 1 : 0;
  }
}

// The statement's products in engine form.  engine_products adds the lengths up in 32 bits and
// bounds them by a round degree, which the verifier is not given: the lengths are added up here
// first, and the bound passed on is their sum
template <class E>
std::vector<product_desc<typename E::F>> statement_products(const evaluation_statement& s) {
  BZ_RELEASE_ASSERT(s.num_mles >= 1 && s.num_products >= 1,
                    "the evaluation check needs at least one MLE and one product");
  u64 total = 0;
  for (u32 p = 0; p < s.num_products; ++p) {
    u32 num_terms;
    std::memcpy(&num_terms,
                static_cast<const u8*>(s.product_table) + static_cast<size_t>(E::product_stride) * p +
                    E::element_bytes,
                sizeof(num_terms));
    BZ_RELEASE_ASSERT(num_terms >= 1, "a sumcheck product must have at least one term");
    total += num_terms;
  }
  BZ_RELEASE_ASSERT(total == s.num_product_terms,
                    "num_product_terms does not match the product table");
  return engine_products<E>(sumcheck_inputs{nullptr, s.product_table, s.product_terms, 1, s.num_mles,
                                            s.num_products, s.num_product_terms,
                                            s.num_product_terms});
}

// the caller's workspace of the device form: the products and the terms, one block
template <class F> struct statement_layout {
  size_t products, terms, end, total;
  statement_layout(u32 num_products, u32 num_product_terms) {
    workspace_carver carve;
    products = carve.take(sizeof(product_desc<F>) * num_products);
    terms = carve.take(sizeof(u32) * num_product_terms);
    end = carve.end();
    total = carve.total();
  }
};

// pinned staging for the statement, as in proof/sumcheck_transcript.hip.  Never destroyed
std::mutex g_stage_mutex;
host_stage_ring& stage_ring() {
  static host_stage_ring* ring = new host_stage_ring;
  return *ring;
}

//--------------------------------------------------------------------------------------------------
// the commitments
//--------------------------------------------------------------------------------------------------
constexpr u32 kDecodeThreads = 256;

// out[i] = decode(commitments[i]), or the identity for an encoding ristretto29::decode rejects.
// `valid` holds 1 when the kernel starts; a wavefront that met a rejected encoding stores 0 from
// one lane -- every such store writes the same word, no wavefront reads it, and a batch without a
// rejected encoding touches it not at all
__global__ void __launch_bounds__(kDecodeThreads)
    k_decode_commitments(ed_point* __restrict__ out, u32* __restrict__ valid,
                         const u8* __restrict__ commitments, u64 n) {
  const u64 i = static_cast<u64>(blockIdx.x) * kDecodeThreads + threadIdx.x;
  bool ok = true;
  if (i < n) {
    ed_point p;
    ok = ristretto29::decode(p, commitments + 32 * i);
    out[i] = ok ? p : ed::identity();
  }
  if (__any(!ok) != 0 && (threadIdx.x & 63u) == 0) *valid = 0;
}

struct combine_layout {
  size_t points, total;
  explicit combine_layout(u64 n) {
    workspace_carver carve;
    points = carve.take(sizeof(ed_point) * n);
    total = carve.total();
  }
};
} // namespace

void verify_sumcheck_device(void* verdicts, void* expected_sums, void* evaluation_points,
                            void* transcripts, unsigned field_id, const void* round_polynomials,
                            unsigned num_variables, unsigned round_degree, unsigned num_proofs,
                            hipStream_t stream) {
  with_elements(field_id, [&](auto elements) {
    hipLaunchKernelGGL((k_verify_sumcheck<decltype(elements)>), dim3(num_proofs), dim3(64), 0, stream,
                       static_cast<u32*>(verdicts), static_cast<u8*>(expected_sums),
                       static_cast<u8*>(evaluation_points), static_cast<u8*>(transcripts),
                       static_cast<const u8*>(round_polynomials), num_variables, round_degree);
  });
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}

bool check_sumcheck_evaluations(unsigned field_id, const void* expected_sum,
                                const void* mle_evaluations, const evaluation_statement& s) {
  return with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    using F = typename E::F;
    const std::vector<product_desc<F>> products = statement_products<E>(s);
    typename F::fe sum = F::zero();
    for (const product_desc<F>& pd : products) {
      sum = fadd<F>(sum, product_value<E>(pd, s.product_terms, static_cast<const u8*>(mle_evaluations)));
    }
    return sums_agree<E>(sum, static_cast<const u8*>(expected_sum));
  });
}

u64 check_sumcheck_evaluations_workspace_bytes(unsigned field_id, unsigned num_products,
                                               unsigned num_product_terms) {
  if (field_id > 1 || num_products == 0 || num_product_terms < num_products) return 0;
  return with_elements(field_id, [&](auto elements) -> u64 {
    return statement_layout<typename decltype(elements)::F>{num_products, num_product_terms}.total;
  });
}

void check_sumcheck_evaluations_device(void* verdicts, unsigned field_id, const void* expected_sums,
                                       const void* mle_evaluations, const evaluation_statement& s,
                                       unsigned num_proofs, void* workspace, u64 workspace_bytes,
                                       hipStream_t stream) {
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    using F = typename E::F;
    const std::vector<product_desc<F>> products = statement_products<E>(s);
    const statement_layout<F> layout{s.num_products, s.num_product_terms};
    BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                      "the evaluation check's workspace is too small");
    u8* base = workspace_carver::aligned(workspace);
    auto* d_products = reinterpret_cast<product_desc<F>*>(base + layout.products);
    u32* d_terms = reinterpret_cast<u32*>(base + layout.terms);
    {
      // the block from the products to the terms, laid out in pinned memory as in the workspace
      const size_t product_bytes = sizeof(product_desc<F>) * products.size();
      const std::lock_guard<std::mutex> lock{g_stage_mutex};
      u8* staged = static_cast<u8*>(stage_ring().acquire(layout.end));
      std::memset(staged + product_bytes, 0, layout.terms - product_bytes);
      std::memcpy(staged, products.data(), product_bytes);
      std::memcpy(staged + layout.terms, s.product_terms, sizeof(u32) * s.num_product_terms);
      BZ_HIP_CHECK(hipMemcpyAsync(d_products, staged, layout.end, hipMemcpyHostToDevice, stream));
      stage_ring().release(stream);
    }
    hipLaunchKernelGGL((k_check_evaluations<E>), dim3(num_proofs), dim3(kRoundThreads), 0, stream,
                       static_cast<u32*>(verdicts), static_cast<const u8*>(expected_sums),
                       static_cast<const u8*>(mle_evaluations), s.num_mles, d_products,
                       s.num_products, d_terms);
  });
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}

bool combine_commitments(void* combined, const u8* commitments, const u8* coefficients,
                         u64 num_commitments) {
  std::vector<ed_point> points(num_commitments);
  bool valid = true;
  for (u64 j = 0; j < num_commitments; ++j) {
    if (!ristretto::decode(points[j], commitments + 32 * j)) {
      points[j] = ed::identity();
      valid = false;
    }
  }
  ed_point sum = ed::identity();
  const std::vector<host_column> cols{byte_column(coefficients, num_commitments, 32, false)};
  curve25519_vtable().msm_host(reinterpret_cast<u8*>(&sum), sizeof(ed_point), true, cols,
                               points.data(), false, num_commitments);
  std::memcpy(combined, &sum, sizeof(sum));
  return valid;
}

u64 combine_commitments_workspace_bytes(u64 num_commitments) {
  if (num_commitments == 0 || num_commitments > kMaxCombinedCommitments) return 0;
  return combine_layout{num_commitments}.total;
}

void combine_commitments_device(msm_context& ctx, void* combined, void* valid, const u8* commitments,
                                const u8* coefficients, u64 num_commitments, void* workspace,
                                u64 workspace_bytes, hipStream_t stream) {
  const combine_layout layout{num_commitments};
  BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                    "the commitment combination's workspace is too small");
  ed_point* d_points =
      reinterpret_cast<ed_point*>(workspace_carver::aligned(workspace) + layout.points);
  BZ_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(valid), 1, 1, stream));
  hipLaunchKernelGGL(k_decode_commitments,
                     dim3(static_cast<u32>((num_commitments + kDecodeThreads - 1) / kDecodeThreads)),
                     dim3(kDecodeThreads), 0, stream, d_points, static_cast<u32*>(valid), commitments,
                     num_commitments);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
  const curve_vtable& vt = curve25519_vtable();
  vt.msm(ctx, static_cast<u8*>(combined), static_cast<u32>(vt.projective_size), true,
         {byte_column(coefficients, num_commitments, 32, false)}, nullptr, d_points, stream, false);
}
} // namespace bz::proof
