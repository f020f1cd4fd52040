// Sumcheck with the library's own transcript: prfsk::reference_transcript<T>
// (sxt/proof/sumcheck/reference_transcript.h) over the caller's 203-byte Merlin state.
//
//   init:   append_message("domain-sep", "sumcheck proof v1"), append_message("n", u64 v),
//           append_message("k", u64 round_degree)
//   round:  append_message("P", the round polynomial's (D + 1) 32 bytes as written to the caller),
//           challenge_bytes("R", 32) = x, and r from x by field (prft::challenge_value,
//           sxt/proof/transcript/transcript_utility.cc):
//             curve25519 scalars: the integer x mod l (s25o::reduce32)
//             Grumpkin:           fgkb::to_bytes_le applied to x read as four limbs, i.e. the integer
//                                 x / 2^256 mod p, canonical -- and THOSE bytes are then the element
//                                 (Montgomery limbs), so the challenge's value is x / 2^512.  The
//                                 double interpretation is the reference's; the bytes are the contract.
//
// On the host this is a callback for the existing entry points (sumcheck_transcript_round) and the
// verifier.  On the device the prover never returns to the host between rounds:
//   k_sumcheck_load, then per round while more than kTailRows pairs are left (or down to the last
//   round for round degrees 6 .. 8): the round kernel of proof/sumcheck.hip, k_sumcheck_challenge
//   (adds the workgroups' partials, stores the polynomial, runs the transcript step in LDS, leaves
//   r and 1 - r in a workspace slot), k_sumcheck_fold_slot; then k_sumcheck_tail runs every
//   remaining round in one workgroup.
// Kernel launches of a proof of v variables (c: the rounds before the tail):
//   round degree <= 5:  c = max(v - 1 - log2(kTailRows), 0),  launches = 1 + 3 c + 1
//   round degree 6..8:  c = v,  launches = 1 + 3 v, less the last fold when mle_evaluations is NULL
// The Merlin logic is proof/transcript.h over wave_sponge: wavefront 0 of the workgroup runs it in
// lockstep, Keccak-f[1600] with one Keccak lane per SIMD lane.
//
// The same chain over typed columns (bzamd_prove_sumcheck_transcript_columns / _device_columns;
// the columns, their raw residues and the conversion constants c: proof/sumcheck_columns.hip).
// No engine-form copy of the full tables is made:
//   n <= 2 kTailRows at round degree <= 5:  k_sumcheck_columns_load writes the n-row engine-form
//     table (these proofs are tiny), k_sumcheck_tail runs every round;
//   otherwise round 0 is k_sumcheck_columns_round / _generic (compiled in
//     proof/sumcheck_columns.hip, launch_sumcheck_columns_round) on the columns with the
//     multipliers times their terms' c, k_sumcheck_columns_challenge (k_sumcheck_challenge that
//     also leaves
//     r c and (1 - r) c for both kinds of column in the slot: four products on one lane, not two
//     in every lane of the fold), k_sumcheck_columns_fold_slot (raw rows times those factors:
//     engine form); rounds >= 1 are the chain above on the folded half and quarter.
// Kernel launches of a proof over columns:
//   round degree <= 5, n <= 2 kTailRows:  2
//   round degree <= 5, above:             3 c + 1, c = v - 1 - log2(kTailRows)
//   round degree 6..8:                    3 v, less the last fold when mle_evaluations is NULL
#include "blitzar_amd/csrc/proof/sumcheck_transcript.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "blitzar_amd/csrc/proof/host_call.h"
#include "blitzar_amd/csrc/proof/sumcheck_columns.h"
#include "blitzar_amd/csrc/proof/sumcheck_protocol.h"
#include "blitzar_amd/csrc/proof/transcript.h"

namespace bz::proof {
namespace {
// pairs of rows from which on one workgroup finishes the proof
constexpr u32 kTailRows = 256;

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
// what wavefront 0 keeps in LDS for the transcript
struct alignas(8) wave_transcript {
  transcript_state t;
  u8 pad[5];
  u8 message[(kMaxDegree + 1) * 32]; // the round polynomial in the caller's representation
  u8 x[32], r[32];
};

BZ_DEV void load_transcript(wave_transcript& w, const u8* transcript) {
  u8* t = reinterpret_cast<u8*>(&w.t);
  for (u32 i = threadIdx.x; i < sizeof(transcript_state); i += 64) t[i] = transcript[i];
  wave_sponge::sync();
}
BZ_DEV void store_transcript(u8* transcript, const wave_transcript& w) {
  const u8* t = reinterpret_cast<const u8*>(&w.t);
  for (u32 i = threadIdx.x; i < sizeof(transcript_state); i += 64) transcript[i] = t[i];
}

// A round's transcript step, by the 64 lanes of wavefront 0: sum[0 .. length) (LDS) is the round
// polynomial; stores it and the challenge in the caller's representation, leaves r and 1 - r in
// engine form in slot[0], slot[1]; with Factors also r c and (1 - r) c in slot[2], slot[3] for the
// conversion constant c of integer columns and in slot[4], slot[5] for that of 32-byte elements
template <class E, bool Factors = false>
BZ_DEV void wave_round(wave_transcript& w, const typename E::F::fe* sum, u32 length, u8* polynomial,
                       u8* point, typename E::F::fe* slot) {
  using F = typename E::F;
  const u32 lane = threadIdx.x;
  if (lane < length) E::store(w.message + 32 * lane, sum[lane]);
  wave_sponge::sync();
  for (u32 i = lane; i < 32 * length; i += 64) polynomial[i] = w.message[i];
  const typename F::fe r = transcript_round<E, wave_sponge>(w.r, w.x, &w.t, w.message, length);
  wave_sponge::sync();
  if (lane < 32) point[lane] = w.r[lane];
  if (lane == 0) {
    slot[0] = r;
    slot[1] = fsub<F>(F::one(), r);
    if constexpr (Factors) {
      const typename F::fe one_minus_r = fsub<F>(F::one(), r);
      slot[2] = F::mul(r, E::conversion(false));
      slot[3] = F::mul(one_minus_r, E::conversion(false));
      slot[4] = F::mul(r, E::conversion(true));
      slot[5] = F::mul(one_minus_r, E::conversion(true));
    }
  }
}

// One workgroup, in the place of k_sumcheck_finish: adds the workgroups' partials, then the
// round's transcript step (round 0: the transcript's init first)
template <class E, bool Factors>
BZ_DEV void challenge_step(u8* __restrict__ polynomials, u8* __restrict__ evaluation_point,
                           typename E::F::fe* __restrict__ slot, u8* __restrict__ transcript,
                           const typename E::F::fe* __restrict__ partials, u32 blocks, u32 length,
                           u32 round, u32 num_variables) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[kRoundThreads];
  __shared__ fe sum[kMaxDegree + 1];
  __shared__ wave_transcript w;
  for (u32 k = 0; k < length; ++k) {
    fe mine = F::zero();
    for (u32 b = threadIdx.x; b < blocks; b += kRoundThreads) {
      mine = fadd<F>(mine, partials[static_cast<u64>(b) * (kMaxDegree + 1) + k]);
    }
    const fe total = block_sum<F>(tree, mine);
    if (threadIdx.x == 0) sum[k] = total;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  load_transcript(w, transcript);
  if (round == 0) transcript_begin<wave_sponge>(&w.t, num_variables, length - 1);
  wave_round<E, Factors>(w, sum, length, polynomials + static_cast<size_t>(32) * length * round,
                         evaluation_point + static_cast<size_t>(32) * round, slot);
  store_transcript(transcript, w);
}
template <class E>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_challenge(u8* __restrict__ polynomials, u8* __restrict__ evaluation_point,
                         typename E::F::fe* __restrict__ slot, u8* __restrict__ transcript,
                         const typename E::F::fe* __restrict__ partials, u32 blocks, u32 length,
                         u32 round, u32 num_variables) {
  challenge_step<E, false>(polynomials, evaluation_point, slot, transcript, partials, blocks, length,
                           round, num_variables);
}
// round 0 over typed columns: the slot takes six elements (wave_round's Factors).  A kernel of its
// own name rather than a flag on the one above: the two are told apart in a resource report
template <class E>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_columns_challenge(u8* __restrict__ polynomials, u8* __restrict__ evaluation_point,
                                 typename E::F::fe* __restrict__ slot, u8* __restrict__ transcript,
                                 const typename E::F::fe* __restrict__ partials, u32 blocks,
                                 u32 length, u32 num_variables) {
  challenge_step<E, true>(polynomials, evaluation_point, slot, transcript, partials, blocks, length, 0,
                          num_variables);
}

// k_sumcheck_fold with r and 1 - r from the slot; the last fold (`evaluations`, mid = 1) goes to
// the caller in the caller's representation
template <class E>
__global__ void __launch_bounds__(256)
    k_sumcheck_fold_slot(typename E::F::fe* __restrict__ out, u8* __restrict__ evaluations,
                         const typename E::F::fe* __restrict__ in, u64 n, u64 mid, u32 num_mles,
                         const typename E::F::fe* __restrict__ slot) {
  using F = typename E::F;
  const u64 id = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= mid * num_mles) return;
  store_folded<E>(out, evaluations, id,
                  fold_element<F, u64>(in, n, mid, id / mid, id % mid, slot[0], slot[1]));
}

// The n-row engine-form table of typed columns, for proofs k_sumcheck_tail runs alone:
// out[m * n + i] = row i of column m (raw) times its conversion constant, zero past the column's end
template <class E>
__global__ void __launch_bounds__(256)
    k_sumcheck_columns_load(typename E::F::fe* __restrict__ out,
                            const column_view* __restrict__ views, u64 n, u32 num_mles) {
  using F = typename E::F;
  const u64 id = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= n * num_mles) return;
  const u64 m = id / n, i = id % n;
  const column_view c = views[m];
  typename F::fe v = F::zero();
  if (i < c.n) v = F::mul(load_raw<F>(c, i), E::conversion(c.nbytes == E::element_bytes));
  out[id] = v;
}

// k_sumcheck_columns_fold (proof/sumcheck_columns.hip) with its factors from the slot as
// k_sumcheck_columns_challenge leaves it; the last fold (`evaluations`, mid = 1) goes to the caller
// in the caller's representation
template <class E>
__global__ void __launch_bounds__(256)
    k_sumcheck_columns_fold_slot(typename E::F::fe* __restrict__ out, u8* __restrict__ evaluations,
                                 const column_view* __restrict__ views, u64 mid, u32 num_mles,
                                 const typename E::F::fe* __restrict__ slot) {
  using F = typename E::F;
  const u64 id = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= mid * num_mles) return;
  const u64 m = id / mid, i = id % mid;
  const column_view c = views[m];
  // r c and (1 - r) c of the column's kind
  const typename F::fe* factors = slot + (c.nbytes == E::element_bytes ? 4 : 2);
  store_folded<E>(out, evaluations, id,
                  fold_column_element<F>(
                      c, mid, i, [&]() -> const typename F::fe& { return factors[0]; },
                      [&]() -> const typename F::fe& { return factors[1]; }));
}

// Rounds first_round .. v - 1 in one workgroup (2^(v - 1 - first_round) <= kTailRows pairs of
// rows): per round the workgroup sums the round polynomial, wavefront 0 runs the transcript step,
// r and 1 - r come back through LDS, the fold writes the other table (not in place: the layout
// changes from m n + i to m mid + i).  The last fold goes to `evaluations` (may be null).
template <class E, u32 D>
__global__ void __launch_bounds__(kRoundThreads)
    k_sumcheck_tail(u8* __restrict__ polynomials, u8* __restrict__ evaluation_point,
                    u8* __restrict__ evaluations, u8* __restrict__ transcript,
                    typename E::F::fe* table_in, typename E::F::fe* table_out, u64 n, u32 num_mles,
                    const product_desc<typename E::F>* __restrict__ products, u32 num_products,
                    const u32* __restrict__ terms, u32 first_round, u32 num_variables) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[D + 1][kRoundThreads];
  __shared__ fe sum[D + 1];
  __shared__ fe slot[2];
  __shared__ wave_transcript w;
  const bool wave0 = threadIdx.x < 64;
  if (wave0) {
    load_transcript(w, transcript);
    if (first_round == 0) transcript_begin<wave_sponge>(&w.t, num_variables, D);
  }
  for (u32 round = first_round; round < num_variables; ++round) {
    const u32 mid = 1u << (num_variables - 1 - round);
    fe poly[D + 1];
#pragma unroll
    for (u32 k = 0; k <= D; ++k) poly[k] = F::zero();
    const dense_tables<F> tables{table_in, n, mid};
    for (u32 i = threadIdx.x; i < mid; i += kRoundThreads) {
      accumulate_row_fixed<F, D>(poly, tables, i, products, num_products, terms);
    }
    store_partials<F, D>(sum, tree, poly);
    __syncthreads();
    if (wave0) {
      wave_round<E>(w, sum, D + 1, polynomials + static_cast<size_t>(32) * (D + 1) * round,
                    evaluation_point + static_cast<size_t>(32) * round, slot);
    }
    __syncthreads();
    const bool last = round + 1 == num_variables;
    if (last && evaluations == nullptr) break;
    const fe r = slot[0], one_minus_r = slot[1];
    for (u32 id = threadIdx.x; id < mid * num_mles; id += kRoundThreads) {
      const fe v = fold_element<F, u32>(table_in, n, mid, id / mid, id % mid, r, one_minus_r);
      // not store_folded: the choice is `last`, and sharing it changes this kernel's registers
      if (last) {
        E::store(evaluations + E::element_bytes * id, v);
      } else {
        table_out[id] = v;
      }
    }
    __syncthreads();
    fe* const folded = table_out;
    table_out = table_in;
    table_in = folded;
    n = mid;
  }
  if (wave0) store_transcript(transcript, w);
}

template <class E, u32 D>
void launch_tail(hipStream_t stream, u32 degree, u8* polynomials, u8* evaluation_point,
                 u8* evaluations, u8* transcript, typename E::F::fe* table_in,
                 typename E::F::fe* table_out, u64 n, u32 num_mles,
                 const product_desc<typename E::F>* products, u32 num_products, const u32* terms,
                 u32 first_round, u32 num_variables) {
  if (degree == D) {
    hipLaunchKernelGGL((k_sumcheck_tail<E, D>), dim3(1), dim3(kRoundThreads), 0, stream, polynomials,
                       evaluation_point, evaluations, transcript, table_in, table_out, n, num_mles,
                       products, num_products, terms, first_round, num_variables);
    return;
  }
  if constexpr (D < kFixedDegree) {
    launch_tail<E, D + 1>(stream, degree, polynomials, evaluation_point, evaluations, transcript,
                          table_in, table_out, n, num_mles, products, num_products, terms,
                          first_round, num_variables);
  }
}

//--------------------------------------------------------------------------------------------------
// the caller's workspace
//--------------------------------------------------------------------------------------------------
// whether k_sumcheck_tail runs the whole proof over typed columns (on the table
// k_sumcheck_columns_load writes)
bool tail_only(const sumcheck_inputs& d) {
  return d.round_degree <= kFixedDegree && (u64{1} << (variables_of(d.n) - 1)) <= kTailRows;
}

// Engine-form tables (not `columns`), or typed columns with the tail only: the n-row table and the
// half it folds to.  Typed columns otherwise: no table at full size, the first fold's half and the
// quarter, ping-pong.  Over columns the views, both product tables (`raw_products`: for round 0,
// the multipliers times their terms' conversion constants) and the terms are one block, uploaded
// with one copy, and the slot takes six elements; without, the views and raw products are empty.
// A function of n, num_mles, num_products, num_product_terms and round_degree alone.
template <class F> struct chain_layout {
  using fe = typename F::fe;
  size_t table, folded, partials, slot, views, raw_products, products, terms, end, total;
  chain_layout(const sumcheck_inputs& d, bool columns) {
    const u64 half = u64{1} << (variables_of(d.n) - 1);
    const bool full = !columns || tail_only(d);
    workspace_carver carve;
    table = carve.take(sizeof(fe) * (full ? d.n : half) * d.num_mles);
    folded = carve.take(sizeof(fe) * (full ? half : (half + 1) / 2) * d.num_mles);
    partials = carve.take(sizeof(fe) * kRoundBlocks * (kMaxDegree + 1));
    slot = carve.take(sizeof(fe) * (columns ? 6 : 2));
    views = carve.take(columns ? sizeof(column_view) * d.num_mles : 0);
    raw_products = carve.take(columns ? sizeof(product_desc<F>) * d.num_products : 0);
    products = carve.take(sizeof(product_desc<F>) * d.num_products);
    terms = carve.take(sizeof(u32) * d.num_product_terms);
    end = carve.end();
    total = carve.total();
  }
};

// Pinned staging for the products and terms: the copies are enqueued from memory that outlives
// the call.  A slot is reused after kSlots calls; waiting for its last copy is the only wait of
// the device form on the host.  Never destroyed (the runtime may be gone by then).
std::mutex g_stage_mutex;
host_stage_ring& stage_ring() {
  static host_stage_ring* ring = new host_stage_ring;
  return *ring;
}

// what a chain writes and where it works: memory of the current device (`mle_evaluations` may be
// null), enqueued on `stream`
struct chain_target {
  u8 *polynomials, *evaluation_point, *mle_evaluations, *transcript;
  void* workspace;
  u64 workspace_bytes;
  hipStream_t stream;
};

// Rounds first_round .. v - 1 of the chain on engine-form tables: d_mles holds n rows per MLE (the
// tables as round first_round reads them), d_next takes the next fold
template <class E>
void chain_rounds(const chain_target& to, const sumcheck_inputs& d, u32 first_round,
                  typename E::F::fe* d_mles, u64 n, typename E::F::fe* d_next,
                  typename E::F::fe* d_partials, typename E::F::fe* d_slot,
                  const product_desc<typename E::F>* d_products, const u32* d_terms) {
  using F = typename E::F;
  hipStream_t stream = to.stream;
  const u32 degree = d.round_degree;
  const u32 length = degree + 1;
  const u32 num_variables = variables_of(d.n);
  for (u32 round = first_round; round < num_variables; ++round) {
    const u64 mid = u64{1} << (num_variables - 1 - round);
    if (degree <= kFixedDegree && mid <= kTailRows) {
      launch_tail<E, 1>(stream, degree, to.polynomials, to.evaluation_point, to.mle_evaluations,
                        to.transcript, d_mles, d_next, n, d.num_mles, d_products, d.num_products,
                        d_terms, round, num_variables);
      BZ_HIP_CHECK(hipGetLastError());
      g_kernel_launches += 1;
      return;
    }
    const u32 blocks = round_blocks(mid);
    launch_sumcheck_round<F>(stream, blocks, d_partials, d_mles, n, mid, d_products, d.num_products,
                             d_terms, degree);
    BZ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_sumcheck_challenge<E>), dim3(1), dim3(kRoundThreads), 0, stream,
                       to.polynomials, to.evaluation_point, d_slot, to.transcript, d_partials,
                       blocks, length, round, num_variables);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 2;
    const bool last = round + 1 == num_variables;
    if (last && to.mle_evaluations == nullptr) return;
    hipLaunchKernelGGL((k_sumcheck_fold_slot<E>), dim3(ceil_div_u32(mid * d.num_mles, 256)),
                       dim3(256), 0, stream, d_next, last ? to.mle_evaluations : nullptr, d_mles, n,
                       mid, d.num_mles, d_slot);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
    std::swap(d_mles, d_next);
    n = mid;
  }
}

template <class E> void prove_device(const chain_target& to, const sumcheck_inputs& d) {
  using F = typename E::F;
  using fe = typename F::fe;
  hipStream_t stream = to.stream;
  const std::vector<product_desc<F>> products = engine_products<E>(d);
  const chain_layout<F> layout{d, false};
  BZ_RELEASE_ASSERT(to.workspace != nullptr && to.workspace_bytes >= layout.total,
                    "the sumcheck workspace is too small");
  u8* base = workspace_carver::aligned(to.workspace);
  fe* d_mles = reinterpret_cast<fe*>(base + layout.table);
  fe* d_next = reinterpret_cast<fe*>(base + layout.folded);
  fe* d_partials = reinterpret_cast<fe*>(base + layout.partials);
  fe* d_slot = reinterpret_cast<fe*>(base + layout.slot);
  auto* d_products = reinterpret_cast<product_desc<F>*>(base + layout.products);
  u32* d_terms = reinterpret_cast<u32*>(base + layout.terms);

  {
    const size_t product_bytes = sizeof(product_desc<F>) * products.size();
    const size_t term_bytes = sizeof(u32) * d.num_product_terms;
    const std::lock_guard<std::mutex> lock{g_stage_mutex};
    u8* staged = static_cast<u8*>(stage_ring().acquire(product_bytes + term_bytes));
    std::memcpy(staged, products.data(), product_bytes);
    std::memcpy(staged + product_bytes, d.product_terms, term_bytes);
    BZ_HIP_CHECK(hipMemcpyAsync(d_products, staged, product_bytes, hipMemcpyHostToDevice, stream));
    BZ_HIP_CHECK(hipMemcpyAsync(d_terms, staged + product_bytes, term_bytes, hipMemcpyHostToDevice,
                                stream));
    stage_ring().release(stream);
  }

  launch_sumcheck_load<E>(stream, d_mles, static_cast<const u8*>(d.mles),
                          static_cast<u64>(d.n) * d.num_mles);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
  chain_rounds<E>(to, d, 0, d_mles, d.n, d_next, d_partials, d_slot, d_products, d_terms);
}

// `columns`: d.num_mles of them, data in memory of the current device, lengths checked.  No
// engine-form copy of the full tables unless k_sumcheck_tail runs the whole proof
template <class E>
void prove_device_columns(const chain_target& to, const sumcheck_inputs& d,
                          const sumcheck_column* columns) {
  using F = typename E::F;
  using fe = typename F::fe;
  hipStream_t stream = to.stream;
  const u32 degree = d.round_degree;
  const u32 num_variables = variables_of(d.n);
  const std::vector<product_desc<F>> products = engine_products<E>(d);
  const chain_layout<F> layout{d, true};
  BZ_RELEASE_ASSERT(to.workspace != nullptr && to.workspace_bytes >= layout.total,
                    "the sumcheck workspace is too small");
  u8* base = workspace_carver::aligned(to.workspace);
  fe* d_table = reinterpret_cast<fe*>(base + layout.table);
  fe* d_folded = reinterpret_cast<fe*>(base + layout.folded);
  fe* d_partials = reinterpret_cast<fe*>(base + layout.partials);
  fe* d_slot = reinterpret_cast<fe*>(base + layout.slot);
  auto* d_views = reinterpret_cast<column_view*>(base + layout.views);
  auto* d_raw_products = reinterpret_cast<product_desc<F>*>(base + layout.raw_products);
  auto* d_products = reinterpret_cast<product_desc<F>*>(base + layout.products);
  u32* d_terms = reinterpret_cast<u32*>(base + layout.terms);

  {
    // the block from the views to the terms, laid out in pinned memory as in the workspace
    const size_t block_bytes = layout.end - layout.views;
    const std::lock_guard<std::mutex> lock{g_stage_mutex};
    u8* staged = static_cast<u8*>(stage_ring().acquire(block_bytes));
    auto* views = reinterpret_cast<column_view*>(staged);
    for (u32 j = 0; j < d.num_mles; ++j) views[j] = make_column_view(columns[j]);
    conversion_scaled_products<E>(
        reinterpret_cast<product_desc<F>*>(staged + (layout.raw_products - layout.views)),
        products.data(), d.num_products, d.product_terms, views);
    std::memcpy(staged + (layout.products - layout.views), products.data(),
                sizeof(product_desc<F>) * products.size());
    std::memcpy(staged + (layout.terms - layout.views), d.product_terms,
                sizeof(u32) * d.num_product_terms);
    BZ_HIP_CHECK(hipMemcpyAsync(d_views, staged, block_bytes, hipMemcpyHostToDevice, stream));
    stage_ring().release(stream);
  }

  if (tail_only(d)) {
    hipLaunchKernelGGL((k_sumcheck_columns_load<E>),
                       dim3(ceil_div_u32(static_cast<u64>(d.n) * d.num_mles, 256)), dim3(256), 0,
                       stream, d_table, d_views, static_cast<u64>(d.n), d.num_mles);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
    chain_rounds<E>(to, d, 0, d_table, d.n, d_folded, d_partials, d_slot, d_products, d_terms);
    return;
  }
  const u64 mid = u64{1} << (num_variables - 1);
  const u32 blocks = round_blocks(mid);
  launch_sumcheck_columns_round<F>(stream, blocks, d_partials, d_views, mid, d_raw_products,
                                   d.num_products, d_terms, degree);
  BZ_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_sumcheck_columns_challenge<E>), dim3(1), dim3(kRoundThreads), 0, stream,
                     to.polynomials, to.evaluation_point, d_slot, to.transcript, d_partials, blocks,
                     degree + 1, num_variables);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 2;
  const bool last = num_variables == 1;
  if (last && to.mle_evaluations == nullptr) return;
  hipLaunchKernelGGL((k_sumcheck_columns_fold_slot<E>), dim3(ceil_div_u32(mid * d.num_mles, 256)),
                     dim3(256), 0, stream, d_table, last ? to.mle_evaluations : nullptr, d_views,
                     mid, d.num_mles, d_slot);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
  chain_rounds<E>(to, d, 1, d_table, mid, d_folded, d_partials, d_slot, d_products, d_terms);
}

// What the GPU backend's forms on host operands declare alike before their tables or columns: the
// three results (`mle_evaluations` may be null), the transcript, which goes up before the chain and
// comes down after it, and the chain's workspace.  `to` is complete once `call` has allocated and
// must stay where it is until then.
template <class F>
void declare_target(host_call& call, chain_target& to, void* polynomials, void* evaluation_point,
                    void* mle_evaluations, void* transcript, const sumcheck_inputs& d,
                    bool columns) {
  const u32 num_variables = variables_of(d.n);
  to.workspace_bytes = chain_layout<F>{d, columns}.total;
  to.stream = call.stream();
  call.output(&to.polynomials, polynomials,
              static_cast<size_t>(32) * (d.round_degree + 1) * num_variables);
  call.output(&to.evaluation_point, evaluation_point, static_cast<size_t>(32) * num_variables);
  call.output(&to.mle_evaluations, mle_evaluations, static_cast<size_t>(32) * d.num_mles);
  call.in_out(&to.transcript, transcript, sizeof(transcript_state));
  call.scratch(&to.workspace, to.workspace_bytes);
}

struct round_context {
  void* transcript;
  unsigned field_id;
};
void round_callback(void* r, void* context, const void* polynomial, unsigned length) {
  const auto* c = static_cast<const round_context*>(context);
  sumcheck_transcript_round(r, c->transcript, c->field_id, polynomial, length);
}

template <class E>
bool verify(u8* expected_sum, u8* evaluation_point, transcript_state* t, const u8* polynomials,
            u32 num_variables, u32 degree) {
  using F = typename E::F;
  using fe = typename F::fe;
  transcript_begin<host_sponge>(t, num_variables, degree);
  fe expected = E::load(expected_sum);
  for (u32 round = 0; round < num_variables; ++round) {
    const u8* p = polynomials + static_cast<size_t>(32) * (degree + 1) * round;
    // p(0) + p(1) (polynomial_utility.h sum_polynomial_01)
    fe sum = fadd<F>(E::load(p), E::load(p));
    for (u32 k = 1; k <= degree; ++k) sum = fadd<F>(sum, E::load(p + 32 * k));
    u8 have[32], want[32];
    E::store(have, sum);
    E::store(want, expected);
    if (std::memcmp(have, want, 32) != 0) return false;
    u8 x[32];
    const fe r = transcript_round<E, host_sponge>(evaluation_point + static_cast<size_t>(32) * round,
                                                  x, t, p, degree + 1);
    // p(r) by Horner (polynomial_utility.h evaluate_polynomial)
    expected = E::load(p + 32 * degree);
    for (u32 k = degree; k-- > 0;) expected = fadd<F>(F::mul(expected, r), E::load(p + 32 * k));
    E::store(expected_sum, expected);
  }
  return true;
}
} // namespace

void sumcheck_transcript_begin(void* transcript, u64 num_variables, u64 round_degree) {
  transcript_begin<host_sponge>(static_cast<transcript_state*>(transcript), num_variables,
                                round_degree);
}

void sumcheck_transcript_round(void* r, void* transcript, unsigned field_id, const void* polynomial,
                               unsigned length) {
  with_elements(field_id, [&](auto elements) {
    u8 x[32];
    transcript_round<decltype(elements), host_sponge>(
        static_cast<u8*>(r), x, static_cast<transcript_state*>(transcript),
        static_cast<const u8*>(polynomial), length);
  });
}

void prove_sumcheck_transcript(api_state& st, void* polynomials, void* evaluation_point,
                               void* mle_evaluations, void* transcript, unsigned field_id,
                               const sumcheck_inputs& d) {
  check_sumcheck_limits(d);
  with_elements(field_id, [&](auto elements) {
    if (st.backend != 2) {
      // the host round loop with the host Merlin as its callback
      sumcheck_transcript_begin(transcript, variables_of(d.n), d.round_degree);
      round_context context{transcript, field_id};
      prove_sumcheck(st, polynomials, evaluation_point, mle_evaluations, field_id, d,
                     reinterpret_cast<void*>(&round_callback), &context);
      return;
    }
    // host tables: uploaded as they are, converted on the device
    using E = decltype(elements);
    host_call call{st};
    chain_target to;
    sumcheck_inputs on_device = d;
    declare_target<typename E::F>(call, to, polynomials, evaluation_point, mle_evaluations,
                                  transcript, d, false);
    call.input(&on_device.mles, d.mles, static_cast<size_t>(E::element_bytes) * d.n * d.num_mles);
    call.allocate();
    g_sumcheck_arena_bytes.store(call.bytes());
    prove_device<E>(to, on_device);
    call.finish();
  });
}

u64 sumcheck_transcript_workspace_bytes(unsigned field_id, const sumcheck_inputs& d) {
  check_sumcheck_limits(d);
  return with_elements(field_id, [&](auto elements) -> u64 {
    return chain_layout<typename decltype(elements)::F>{d, false}.total;
  });
}

void prove_sumcheck_transcript_device(void* polynomials, void* evaluation_point,
                                      void* mle_evaluations, void* transcript, unsigned field_id,
                                      const sumcheck_inputs& d, void* workspace, u64 workspace_bytes,
                                      hipStream_t stream) {
  check_sumcheck_limits(d);
  with_elements(field_id, [&](auto elements) {
    prove_device<decltype(elements)>(
        chain_target{static_cast<u8*>(polynomials), static_cast<u8*>(evaluation_point),
                     static_cast<u8*>(mle_evaluations), static_cast<u8*>(transcript), workspace,
                     workspace_bytes, stream},
        d);
  });
}

void prove_sumcheck_transcript_columns(api_state& st, void* polynomials, void* evaluation_point,
                                       void* mle_evaluations, void* transcript, unsigned field_id,
                                       const sumcheck_inputs& d, const sumcheck_column* columns) {
  check_sumcheck_limits(d);
  with_elements(field_id, [&](auto elements) {
    if (st.backend != 2) {
      // the host round loop over the columns with the host Merlin as its callback
      sumcheck_transcript_begin(transcript, variables_of(d.n), d.round_degree);
      round_context context{transcript, field_id};
      prove_sumcheck_columns(st, polynomials, evaluation_point, mle_evaluations, field_id, d,
                             columns, reinterpret_cast<void*>(&round_callback), &context);
      return;
    }
    check_column_lengths(d, columns);
    // host columns: uploaded at their own width
    using E = decltype(elements);
    host_call call{st};
    chain_target to;
    std::vector<sumcheck_column> on_device;
    declare_target<typename E::F>(call, to, polynomials, evaluation_point, mle_evaluations,
                                  transcript, d, true);
    call.columns(&on_device, columns, d.num_mles);
    call.allocate();
    g_sumcheck_arena_bytes.store(call.bytes());
    prove_device_columns<E>(to, d, on_device.data());
    call.finish();
  });
}

u64 sumcheck_transcript_columns_workspace_bytes(unsigned field_id, const sumcheck_inputs& d) {
  check_sumcheck_limits(d);
  return with_elements(field_id, [&](auto elements) -> u64 {
    return chain_layout<typename decltype(elements)::F>{d, true}.total;
  });
}

void prove_sumcheck_transcript_device_columns(void* polynomials, void* evaluation_point,
                                              void* mle_evaluations, void* transcript,
                                              unsigned field_id, const sumcheck_inputs& d,
                                              const sumcheck_column* columns, void* workspace,
                                              u64 workspace_bytes, hipStream_t stream) {
  check_sumcheck_limits(d);
  check_column_lengths(d, columns);
  with_elements(field_id, [&](auto elements) {
    prove_device_columns<decltype(elements)>(
        chain_target{static_cast<u8*>(polynomials), static_cast<u8*>(evaluation_point),
                     static_cast<u8*>(mle_evaluations), static_cast<u8*>(transcript), workspace,
                     workspace_bytes, stream},
        d, columns);
  });
}

bool verify_sumcheck(void* expected_sum, void* evaluation_point, void* transcript, unsigned field_id,
                     const void* round_polynomials, unsigned num_variables, unsigned round_degree) {
  BZ_RELEASE_ASSERT(num_variables > 0 && round_degree > 0,
                    "sumcheck verification needs num_variables > 0 and round_degree > 0");
  return with_elements(field_id, [&](auto elements) {
    return verify<decltype(elements)>(
        static_cast<u8*>(expected_sum), static_cast<u8*>(evaluation_point),
        static_cast<transcript_state*>(transcript), static_cast<const u8*>(round_polynomials),
        num_variables, round_degree);
  });
}
} // namespace bz::proof
