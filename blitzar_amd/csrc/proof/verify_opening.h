// The verifier's half of an MLE opening in front of the inner-product verifier
// (proof/verify_opening.hip): the sumcheck rounds of a batch of device-resident proofs, the final
// evaluation check sum_p mult_p prod_{j in terms_p} mle_evaluations[j] == expected_sum, and
// a_commit = sum_j c_j decode(C_j) from the compressed commitments the MSM wrote.
#pragma once

#include "blitzar_amd/csrc/api/state.h"

namespace bz::proof {
// bzamd_verify_sumcheck_device: `num_proofs` proofs of one shape back to back in memory of the
// current device (transcripts 203 bytes apart); proof i is verify_sumcheck on the same bytes, its
// verdict in verdicts[i].  One launch on `stream`, no workspace.  Arguments checked by the caller
// but for the field id.
void verify_sumcheck_device(void* verdicts, void* expected_sums, void* evaluation_points,
                            void* transcripts, unsigned field_id, const void* round_polynomials,
                            unsigned num_variables, unsigned round_degree, unsigned num_proofs,
                            hipStream_t stream);

// The statement of the final evaluation check: the product table and terms of
// `sumcheck_descriptor` (host memory), validated as the prover validates them, except that a
// product may have any number of terms >= 1
struct evaluation_statement {
  const void* product_table;
  const unsigned* product_terms;
  unsigned num_mles, num_products, num_product_terms;
};
// bzamd_check_sumcheck_evaluations: host operands, host arithmetic
bool check_sumcheck_evaluations(unsigned field_id, const void* expected_sum,
                                const void* mle_evaluations, const evaluation_statement& statement);
// 0 for counts the call rejects (needs no backend)
u64 check_sumcheck_evaluations_workspace_bytes(unsigned field_id, unsigned num_products,
                                               unsigned num_product_terms);
// bzamd_check_sumcheck_evaluations_device: one statement for `num_proofs` proofs; expected_sums,
// mle_evaluations (num_proofs x num_mles elements) and verdicts in memory of the current device
void check_sumcheck_evaluations_device(void* verdicts, unsigned field_id, const void* expected_sums,
                                       const void* mle_evaluations,
                                       const evaluation_statement& statement, unsigned num_proofs,
                                       void* workspace, u64 workspace_bytes, hipStream_t stream);

// bzamd_combine_commitments: host operands, the host decode and the host MSM on every backend;
// false when an encoding did not decode (it contributes the identity)
constexpr u64 kMaxCombinedCommitments = u64{1} << 28; // one pass of the engine
bool combine_commitments(void* combined, const u8* commitments, const u8* coefficients,
                         u64 num_commitments);
u64 combine_commitments_workspace_bytes(u64 num_commitments);
// bzamd_combine_commitments_device: `ctx` the engine context of the current device; the decoded
// points go to the workspace, one plain engine call with projective output follows
void combine_commitments_device(msm_context& ctx, void* combined, void* valid, const u8* commitments,
                                const u8* coefficients, u64 num_commitments, void* workspace,
                                u64 workspace_bytes, hipStream_t stream);
} // namespace bz::proof
