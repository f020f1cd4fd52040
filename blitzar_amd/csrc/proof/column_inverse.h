// The column of inverses a log-derivative argument commits to and multiplies in its sumcheck
// (proof/column_inverse.hip): inverses[i] = 1 / (shift + sum_j coefficients[j] column_j[i]) over
// typed columns, zero where the denominator is zero, written in element form and in scalar form in
// one pass.  Exact in both fields, enqueue-only in the device form.  The definitions are those
// above bzamd_invert_columns in include/blitzar_amd.h.
#pragma once

#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
constexpr u32 kMaxInvertedColumns = 32; // the views of one call travel as kernel arguments

// `columns`: num_columns of them, widths checked by the caller, on the host
struct column_inversion {
  const sumcheck_column* columns;
  const void* coefficients; // may be null: every coefficient is 1; else num_columns x 32 bytes
  const void* shift;        // may be null: 0; else 32 bytes
  u32 num_columns;
  u64 n;
};
// the checks both forms share (limits, alignment, overlaps, the field id): aborts.  The C ABI runs
// them before either form below (and before it asks for the backend), which do not repeat them
void check_column_inversion(const void* inverses, const void* scalars, unsigned field_id,
                            const column_inversion& v);
// bzamd_invert_columns: host operands, blocking, st.backend; GPU backend: the columns uploaded at
// their own width to devices[0], whose lease the caller holds.  `inverses` (element form) and
// `scalars` (scalar form): n x 32 bytes each, either may be null
void invert_columns(api_state& st, void* inverses, void* scalars, unsigned field_id,
                    const column_inversion& v);
// everything but `v` and the columns array is memory of the current device; enqueue-only, one
// kernel launch
void invert_columns_device(void* inverses, void* scalars, unsigned field_id,
                           const column_inversion& v, hipStream_t stream);
} // namespace bz::proof
