// What opening the sumcheck's claimed evaluations with one inner-product proof needs beside the two
// provers (proof/mle_opening.hip): the evaluation vector of the point, b with <column_j, b> =
// f_j(r), and a linear combination of the typed columns widened to scalars, a = sum_j c_j column_j.
#pragma once

#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
// bzamd_mle_evaluation_vector: vector[i] = prod_t (bit_{v-1-t}(i) ? r_t : 1 - r_t), i < n, with
// v = num_variables and r = evaluation_point (32-byte elements in the caller's representation, the
// vector canonical).  Host operands, blocking, st.backend; GPU backend: on devices[0], whose lease
// the caller holds
void mle_evaluation_vector(api_state& st, void* vector, unsigned field_id,
                           const void* evaluation_point, unsigned num_variables, u64 n);
// bzamd_mle_evaluation_vector_device: both are memory of the current device; enqueue-only
void mle_evaluation_vector_device(void* vector, unsigned field_id, const void* evaluation_point,
                                  unsigned num_variables, u64 n, hipStream_t stream);

// bzamd_combine_columns: combined[i] = sum_j coefficients[j] column_j[i], i < n (rows past a column's
// end are zero), and with `product` and `evaluations` both present product = sum_j coefficients[j]
// evaluations[j].  `columns`: num_columns of them, widths checked by the caller, on the host
struct column_combination {
  const sumcheck_column* columns;
  const void* coefficients; // num_columns x 32 bytes
  const void* evaluations;  // may be null: num_columns x 32 bytes
  u32 num_columns;
  u64 n;
};
// host operands, blocking, st.backend; GPU backend: the columns uploaded at their own width to
// devices[0], whose lease the caller holds
void combine_columns(api_state& st, void* combined, void* product, unsigned field_id,
                     const column_combination& c);
// everything but `c` and the columns array is memory of the current device; enqueue-only
void combine_columns_device(void* combined, void* product, unsigned field_id,
                            const column_combination& c, hipStream_t stream);

// bzamd_evaluate_columns: evaluations[j] = sum_{i < columns[j].n} column_j[i] vector[i], 32 bytes
// each, canonical, any alignment.  `vector`: n x 32 bytes, entries meaning what a 32-byte column
// element means, 8-byte aligned.  `columns`: num_columns of them, widths checked by the caller, on
// the host
struct column_evaluation {
  const sumcheck_column* columns;
  u32 num_columns;
  u64 n;
};
// host operands, blocking, st.backend; GPU backend: the vector and the columns uploaded at their
// own width to devices[0], whose lease the caller holds
void evaluate_columns(api_state& st, void* evaluations, unsigned field_id, const void* vector,
                      const column_evaluation& e);
// the device form's workspace (the workgroups' partial sums); 0 for arguments the call would reject
u64 evaluate_columns_workspace_bytes(unsigned field_id, u32 num_columns, u64 n);
// everything but `e` and the columns array is memory of the current device; enqueue-only
void evaluate_columns_device(void* evaluations, unsigned field_id, const void* vector,
                             const column_evaluation& e, void* workspace, u64 workspace_bytes,
                             hipStream_t stream);
} // namespace bz::proof
