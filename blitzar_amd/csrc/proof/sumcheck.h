// Sumcheck prover behind sxt_prove_sumcheck and bzamd_prove_sumcheck* (proof/sumcheck.hip).
#pragma once

#include <atomic>

#include "blitzar_amd/csrc/api/state.h"

namespace bz::proof {
// device memory the latest proof on the GPU backend asked for: everything it holds on the device
// (exported as bzamd_sumcheck_device_bytes)
extern std::atomic<u64> g_sumcheck_arena_bytes;

// the fields of `struct sumcheck_descriptor` (cbindings/blitzar_api.h:147-181)
struct sumcheck_inputs {
  const void* mles;              // n x num_mles field elements, column-major
  const void* product_table;     // num_products x {element multiplier; unsigned product_length}
  const unsigned* product_terms; // MLE indices of every product, back to back
  unsigned n, num_mles, num_products, num_product_terms, round_degree;
};
// bzamd_prove_sumcheck_device: `inputs.mles` is device memory of `device`, read in stream order on
// `stream` and never written
struct sumcheck_device_tables {
  int device;
  hipStream_t stream;
};
// Runs on st.backend; GPU backend: on devices[0], whose lease the caller holds and passes in -- it
// is given up around every call of `callback` (the caller's transcript may call back into the
// library) and the proof's tables live in device memory of the call's own.  With `device_tables`
// the proof runs on that device and stream instead and needs no lease (it touches none of the
// backend's per-device state).  `mle_evaluations` (may be null): num_mles elements, the tables
// folded by every challenge.  `callback` has the signature
// void (FIELD* r, void* context, const FIELD* polynomial, unsigned polynomial_length)
void prove_sumcheck(api_state& st, void* polynomials, void* evaluation_point, void* mle_evaluations,
                    unsigned field_id, const sumcheck_inputs& inputs, void* callback, void* context,
                    api_state::device_lease* lease = nullptr,
                    const sumcheck_device_tables* device_tables = nullptr);

// MLE j of bzamd_prove_sumcheck*_columns: `n` little-endian integers of `nbytes` (1 .. 31, two's
// complement when `is_signed`) or field elements of 32 bytes; rows n .. inputs.n - 1 are zero
struct sumcheck_column {
  const void* data;
  u64 n;
  u32 nbytes;
  bool is_signed;
};
// prove_sumcheck over typed columns (proof/sumcheck_columns.hip): `columns` (inputs.num_mles of
// them, checked by the caller) take the place of inputs.mles, which is not read.  Their data is
// host memory, or with `device_tables` memory of that device.  GPU backend: round 0 and the first
// fold read the columns where they lie, the working tables are the folded ones.
void prove_sumcheck_columns(api_state& st, void* polynomials, void* evaluation_point,
                            void* mle_evaluations, unsigned field_id, const sumcheck_inputs& inputs,
                            const sumcheck_column* columns, void* callback, void* context,
                            api_state::device_lease* lease = nullptr,
                            const sumcheck_device_tables* device_tables = nullptr);
} // namespace bz::proof
