// Inner-product argument over curve25519 (Bulletproofs protocol 2 with a public b vector), the
// next consumer of the MSM engine after the commitment calls.
// Reference: cbindings/inner_product_proof.cc:96-167, sxt/proof/inner_product/
// {proof_computation,cpu_driver,gpu_driver,fold,generator_fold,verification_computation}.cc.
#pragma once

#include <cstdint>

#include "blitzar_amd/csrc/api/state.h"

namespace bz::proof {
// Both run under the api lock of `st` (taken by the caller) on st.backend.
//   l_vector / r_vector: ceil(log2 n) compressed ristretto points each; transcript: 203 bytes,
//   updated in place; a_vector / b_vector: n scalars of 32 bytes; generators are the built-in ones
//   [offset, offset + np) with Q = generator offset + np, np = 2^ceil(log2 n).
void prove_inner_product(api_state& st, u8* l_vector, u8* r_vector, u8* ap_value, void* transcript,
                         u64 n, u64 generators_offset, const u8* a_vector, const u8* b_vector);
bool verify_inner_product(api_state& st, void* transcript, u64 n, u64 generators_offset,
                          const u8* b_vector, const u8* product, const void* a_commit,
                          const u8* l_vector, const u8* r_vector, const u8* ap_value);

// The device form (include/blitzar_amd.h: bzamd_prove_inner_product_device).  DEVICE pointers on
// the current device; `generators`: np + 1 elements in ABI layout, the last one Q, or nullptr for
// the built-in ones from `generators_offset`; `ctx`: the engine context of the current device.
// Only enqueues on `stream`.  The workspace size depends on np alone (0 for n = 0 or n > 2^30).
u64 inner_product_workspace_bytes(u64 n);
void prove_inner_product_device(msm_context& ctx, u8* l_vector, u8* r_vector, u8* ap_value,
                                void* transcript, u64 n, u64 generators_offset,
                                const void* generators, const u8* a_vector, const u8* b_vector,
                                void* workspace, u64 workspace_bytes, hipStream_t stream);

// The verifier's device form (include/blitzar_amd.h: bzamd_verify_inner_product_device): `verdict`
// one u32 (1 accepted, 0 rejected), `product` / `ap_value` 32 bytes, `a_commit` one element in ABI
// layout, the proof where the prover's device form leaves it; everything else as above.
u64 inner_product_verify_workspace_bytes(u64 n);
void verify_inner_product_device(msm_context& ctx, void* verdict, void* transcript, u64 n,
                                 u64 generators_offset, const void* generators, const u8* b_vector,
                                 const u8* product, const void* a_commit, const u8* l_vector,
                                 const u8* r_vector, const u8* ap_value, void* workspace,
                                 u64 workspace_bytes, hipStream_t stream);

// num_proofs proofs of one length over one generator set in one chain
// (include/blitzar_amd.h: bzamd_verify_inner_product_batch_device): proof i lies at 4 i in
// `verdicts`, 203 i in `transcripts`, 32 n i in `b_vectors`, 32 i in `products` / `ap_values`,
// i elements in `a_commits` and 32 ceil_log2(n) i in `l_vectors` / `r_vectors`; the single form is
// the batch of one.  The size is 0 outside 1 <= n <= 2^30, 1 <= num_proofs, num_proofs np <= 2^28.
u64 inner_product_verify_batch_workspace_bytes(u64 n, u64 num_proofs);
void verify_inner_product_batch_device(msm_context& ctx, void* verdicts, void* transcripts, u64 n,
                                       u64 num_proofs, u64 generators_offset,
                                       const void* generators, const u8* b_vectors,
                                       const u8* products, const void* a_commits,
                                       const u8* l_vectors, const u8* r_vectors,
                                       const u8* ap_values, void* workspace, u64 workspace_bytes,
                                       hipStream_t stream);

// services of api/capi.hip the prover needs
// generators [offset, offset + n) as raw extended coordinates on the host (cache + derivation)
void host_builtin_generators_unlocked(api_state& st, ed_point* out, u64 n, u64 offset);
// canonical commitment of ONE 32-byte column against HOST generators in ABI layout (the backend's
// normal Pedersen path, sharding included); the api lock is held by the caller
void commit_column_unlocked(api_state& st, u8* out32, const u8* scalars, u64 n,
                            const ed_point* generators);
} // namespace bz::proof
