// The field work of a HyperKZG opening between its MSM calls (proof/univariate_opening.hip): the
// folds P_1 .. P_{l-1} of a polynomial of l variables, the evaluations of all l polynomials at up
// to four points, and the quotients of their combination B = sum_i q^i P_i by X - u_k.  Exact in
// both fields, enqueue-only in the device forms.  The definitions are those above
// bzamd_fold_polynomial in include/blitzar_amd.h.
#pragma once

#include <utility>
#include <vector>

#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
constexpr u32 kMaxOpeningVariables = 30;
constexpr u32 kMaxOpeningPoints = 4;

// P_i, 1 <= i < num_variables: (row offset in `folded`, rows)
std::vector<std::pair<u64, u64>> folded_layout(u64 n, u32 num_variables);

// the operands of one call; which are read and which written depends on the call
struct univariate_opening {
  const void* polynomial; // P_0: n x 32 bytes, element form, 8-byte aligned
  void* folded;           // P_1 .. P_{l-1} back to back, element form, 8-byte aligned
  u64 n;
  u32 num_variables;
  const void* points; // num_points x 32 bytes, element form, any alignment
  u32 num_points;
};

// bzamd_fold_polynomial: writes o.folded, `scalars` (may be null: the same rows as plain integers)
// and `evaluation` (may be null).  o.points: the num_variables challenges, o.num_points is not read.
// Host operands, blocking, st.backend; GPU backend: on devices[0], whose lease the caller holds
void fold_polynomial(api_state& st, void* scalars, void* evaluation, unsigned field_id,
                     const univariate_opening& o);
// everything is memory of the current device; enqueue-only
void fold_polynomial_device(void* scalars, void* evaluation, unsigned field_id,
                            const univariate_opening& o, hipStream_t stream);

// bzamd_evaluate_polynomials: evaluations[k * l + i] = P_i(u_k), element form
void evaluate_polynomials(api_state& st, void* evaluations, unsigned field_id,
                          const univariate_opening& o);
// 0 for arguments the call would reject
u64 evaluate_polynomials_workspace_bytes(unsigned field_id, u64 n, u32 num_variables,
                                         u32 num_points);
// the device form's checks alone (the C ABI runs them before it asks for the backend)
void check_evaluate_polynomials_device(const void* evaluations, unsigned field_id,
                                       const univariate_opening& o, const void* workspace,
                                       u64 workspace_bytes);
void evaluate_polynomials_device(void* evaluations, unsigned field_id, const univariate_opening& o,
                                 void* workspace, u64 workspace_bytes, hipStream_t stream);

// bzamd_batch_quotients: quotients[k * n + j] = h_k[j] as plain integers, remainders[k] = B(u_k)
// (may be null), element form
void batch_quotients(api_state& st, void* quotients, void* remainders, unsigned field_id,
                     const univariate_opening& o, const void* q);
u64 batch_quotients_workspace_bytes(unsigned field_id, u64 n, u32 num_variables, u32 num_points);
void check_batch_quotients_device(const void* quotients, const void* remainders, unsigned field_id,
                                  const univariate_opening& o, const void* q,
                                  const void* workspace, u64 workspace_bytes);
void batch_quotients_device(void* quotients, void* remainders, unsigned field_id,
                            const univariate_opening& o, const void* q, void* workspace,
                            u64 workspace_bytes, hipStream_t stream);
} // namespace bz::proof
