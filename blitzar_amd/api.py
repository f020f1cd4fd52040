"""ctypes binding of libblitzar_amd.so -- the host-side mirror of the reference's C API.

Function names, argument order and error behaviour follow `cbindings/blitzar_api.h` of the
reference (declared for this repo in include/blitzar_api.h); the `bzamd_*` functions are the
device-resident extensions of include/blitzar_amd.h.  This module is plumbing for tests and
bench.py: the product is the C-ABI shared library, not this wrapper.  It never computes anything
itself and raises ImportError-like failures loudly when the HIP library is missing.
"""
import ctypes
import os

import numpy as np

SXT_CPU_BACKEND = 1
SXT_GPU_BACKEND = 2
SXT_CURVE_RISTRETTO255 = 0
SXT_CURVE_BLS_381 = 1
SXT_CURVE_BN_254 = 2
SXT_CURVE_GRUMPKIN = 3

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLITZAR_AMD_LIB selects another build of the same library (kernel-variant A/B runs)
LIB_PATH = os.environ.get("BLITZAR_AMD_LIB") or os.path.join(_HERE, "lib", "libblitzar_amd.so")

# per curve: (C-ABI generator stride, commitment bytes, projective element bytes)
CURVE_LAYOUT = {
    SXT_CURVE_RISTRETTO255: (160, 32, 160),
    SXT_CURVE_BLS_381: (104, 48, 144),
    SXT_CURVE_BN_254: (72, 72, 96),
    SXT_CURVE_GRUMPKIN: (72, 72, 96),
}


class sxt_config(ctypes.Structure):
    _fields_ = [("backend", ctypes.c_int), ("num_precomputed_generators", ctypes.c_uint64)]


class sxt_sequence_descriptor(ctypes.Structure):
    _fields_ = [("element_nbytes", ctypes.c_uint8), ("n", ctypes.c_uint64),
                ("data", ctypes.c_void_p), ("is_signed", ctypes.c_int)]


assert ctypes.sizeof(sxt_sequence_descriptor) == 32
assert ctypes.sizeof(sxt_config) == 16

_lib = None


def load():
    """Load the HIP library; fails loudly (no CPU fallback module exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m blitzar_amd.build` "
            "(or __graft_entry__.build()); there is no fallback implementation")
    lib = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, cu = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint
    lib.sxt_init.argtypes = [ctypes.POINTER(sxt_config)]
    lib.sxt_init.restype = ctypes.c_int
    lib.sxt_curve25519_compute_pedersen_commitments.argtypes = [
        vp, u32, ctypes.POINTER(sxt_sequence_descriptor), u64]
    for name in ("sxt_curve25519_compute_pedersen_commitments_with_generators",
                 "sxt_bls12_381_g1_compute_pedersen_commitments_with_generators",
                 "sxt_bn254_g1_uncompressed_compute_pedersen_commitments_with_generators",
                 "sxt_grumpkin_uncompressed_compute_pedersen_commitments_with_generators"):
        getattr(lib, name).argtypes = [vp, u32, ctypes.POINTER(sxt_sequence_descriptor), vp]
        getattr(lib, name).restype = None
    lib.sxt_ristretto255_get_generators.argtypes = [vp, u64, u64]
    lib.sxt_ristretto255_get_generators.restype = ctypes.c_int
    lib.sxt_curve25519_get_one_commit.argtypes = [vp, u64]
    lib.sxt_curve25519_get_one_commit.restype = ctypes.c_int
    lib.sxt_multiexp_handle_new.argtypes = [cu, vp, cu]
    lib.sxt_multiexp_handle_new.restype = vp
    lib.sxt_multiexp_handle_new_from_file.argtypes = [cu, ctypes.c_char_p]
    lib.sxt_multiexp_handle_new_from_file.restype = vp
    lib.sxt_multiexp_handle_write_to_file.argtypes = [vp, ctypes.c_char_p]
    lib.sxt_multiexp_handle_write_to_file.restype = None
    lib.sxt_multiexp_handle_free.argtypes = [vp]
    lib.sxt_multiexp_handle_free.restype = None
    lib.sxt_fixed_multiexponentiation.argtypes = [vp, vp, cu, cu, cu, vp]
    lib.sxt_fixed_multiexponentiation.restype = None
    lib.sxt_fixed_packed_multiexponentiation.argtypes = [vp, vp, vp, cu, cu, vp]
    lib.sxt_fixed_packed_multiexponentiation.restype = None
    lib.sxt_fixed_vlen_multiexponentiation.argtypes = [vp, vp, vp, vp, cu, vp]
    lib.sxt_fixed_vlen_multiexponentiation.restype = None
    lib.bzamd_version.restype = ctypes.c_char_p
    lib.bzamd_device_count.restype = ctypes.c_int
    lib.bzamd_active_backend.restype = ctypes.c_int
    lib.bzamd_kernel_launch_count.restype = ctypes.c_uint64
    lib.bzamd_concurrent_calls_high_water.restype = ctypes.c_uint32
    lib.bzamd_slow_instruction_fetch.restype = ctypes.c_int
    lib.bzamd_probe_mad_rate.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
    lib.bzamd_probe_mad_rate.restype = ctypes.c_int
    lib.bzamd_set_row_pipeline_chunks.argtypes = [u32]
    lib.bzamd_set_row_pipeline_chunks.restype = None
    lib.bzamd_reset_for_testing.restype = None
    lib.bzamd_set_tuning.argtypes = [u32, u64, u64]
    lib.bzamd_set_tuning.restype = None
    lib.bzamd_set_segments.argtypes = [u32, u32]
    lib.bzamd_set_segments.restype = None
    lib.bzamd_stage_timing_begin.argtypes = [u64]
    lib.bzamd_stage_timing_begin.restype = None
    lib.bzamd_pipeline_next.argtypes = []
    lib.bzamd_pipeline_next.restype = None
    lib.bzamd_pipeline_flush.argtypes = [ctypes.c_void_p]
    lib.bzamd_pipeline_flush.restype = None
    lib.bzamd_stage_timing_begin_masked.argtypes = [u64, u32]
    lib.bzamd_stage_timing_begin_masked.restype = None
    lib.bzamd_stage_timing_begin_sampled.argtypes = [u64, u32, u32]
    lib.bzamd_stage_timing_begin_sampled.restype = None
    lib.bzamd_stage_timing_collect.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.bzamd_stage_timing_collect.restype = ctypes.c_uint64
    lib.bzamd_msm_device.argtypes = [cu, vp, u32, ctypes.POINTER(sxt_sequence_descriptor), vp, vp]
    lib.bzamd_msm_device.restype = None
    lib.bzamd_msm_device_projective.argtypes = [cu, vp, u32,
                                                ctypes.POINTER(sxt_sequence_descriptor), vp, vp]
    lib.bzamd_msm_device_projective.restype = None
    lib.bzamd_msm_projective.argtypes = [cu, vp, u32, ctypes.POINTER(sxt_sequence_descriptor), vp]
    lib.bzamd_msm_projective.restype = None
    lib.bzamd_fold_encode.argtypes = [cu, vp, vp, u32, u32]
    lib.bzamd_fold_encode.restype = None
    lib.bzamd_fold_encode_device.argtypes = [cu, vp, vp, u32, u32, vp]
    lib.bzamd_fold_encode_device.restype = None
    lib.bzamd_generators_new_device.argtypes = [cu, vp, u64, vp]
    lib.bzamd_generators_new_device.restype = vp
    lib.bzamd_generators_new_host.argtypes = [cu, vp, u64]
    lib.bzamd_generators_new_host.restype = vp
    lib.bzamd_generators_free.argtypes = [vp]
    lib.bzamd_generators_free.restype = None
    lib.bzamd_compute_commitments_with_generator_offsets.argtypes = [
        cu, vp, u32, ctypes.POINTER(sxt_sequence_descriptor), vp, u64, ctypes.POINTER(u64)]
    lib.bzamd_compute_commitments_with_generator_offsets.restype = None
    lib.bzamd_curve25519_compute_commitments_with_offsets.argtypes = [
        vp, u32, ctypes.POINTER(sxt_sequence_descriptor), ctypes.POINTER(u64)]
    lib.bzamd_curve25519_compute_commitments_with_offsets.restype = None
    lib.bzamd_msm_device_offsets.argtypes = [cu, vp, u32, ctypes.POINTER(sxt_sequence_descriptor),
                                             vp, u64, ctypes.POINTER(u64), vp]
    lib.bzamd_msm_device_offsets.restype = None
    lib.bzamd_msm_device_resident_offsets.argtypes = [
        vp, u32, ctypes.POINTER(sxt_sequence_descriptor), vp, ctypes.POINTER(u64), vp]
    lib.bzamd_msm_device_resident_offsets.restype = None
    lib.bzamd_msm_device_resident.argtypes = [vp, u32, ctypes.POINTER(sxt_sequence_descriptor),
                                              vp, vp]
    lib.bzamd_msm_device_resident.restype = None
    lib.bzamd_generator_multiples_device.argtypes = [cu, vp, vp, u64, vp]
    lib.bzamd_generator_multiples_device.restype = None
    lib.bzamd_ristretto255_generators_device.argtypes = [vp, u64, u64, vp]
    lib.bzamd_ristretto255_generators_device.restype = None
    lib.bzamd_fixed_packed_multiexponentiation_device.argtypes = [vp, vp, vp, vp, cu, cu, vp, vp]
    lib.bzamd_fixed_packed_multiexponentiation_device.restype = None
    lib.sxt_curve25519_prove_inner_product.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp]
    lib.sxt_curve25519_prove_inner_product.restype = None
    lib.sxt_curve25519_verify_inner_product.argtypes = [vp, u64, u64, vp, vp, vp, vp, vp, vp]
    lib.sxt_curve25519_verify_inner_product.restype = ctypes.c_int
    # (an older build selected with BLITZAR_AMD_LIB lacks these two: tools/inner_product_bench.py
    # measures against one; calling them there raises AttributeError)
    if hasattr(lib, "bzamd_prove_inner_product_device"):
        lib.bzamd_inner_product_workspace_bytes.argtypes = [u64]
        lib.bzamd_inner_product_workspace_bytes.restype = u64
        lib.bzamd_prove_inner_product_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, vp, vp,
                                                         u64, vp]
        lib.bzamd_prove_inner_product_device.restype = None
    if hasattr(lib, "bzamd_verify_inner_product_device"):
        lib.bzamd_inner_product_verify_workspace_bytes.argtypes = [u64]
        lib.bzamd_inner_product_verify_workspace_bytes.restype = u64
        lib.bzamd_verify_inner_product_device.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp, vp, vp,
                                                          vp, vp, u64, vp]
        lib.bzamd_verify_inner_product_device.restype = None
    if hasattr(lib, "bzamd_verify_inner_product_batch_device"):
        lib.bzamd_inner_product_verify_batch_workspace_bytes.argtypes = [u64, u64]
        lib.bzamd_inner_product_verify_batch_workspace_bytes.restype = u64
        lib.bzamd_verify_inner_product_batch_device.argtypes = [vp, vp, u64, u64, u64, vp, vp, vp,
                                                                vp, vp, vp, vp, vp, u64, vp]
        lib.bzamd_verify_inner_product_batch_device.restype = None
    lib.bzamd_transcript_init.argtypes = [vp, ctypes.c_char_p, u64]
    lib.bzamd_transcript_init.restype = None
    lib.bzamd_num_devices.restype = ctypes.c_int
    lib.bzamd_set_window_bits.argtypes = [u32]
    lib.bzamd_set_window_bits.restype = None
    lib.bzamd_generator_cache_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 2
    lib.bzamd_generator_cache_stats.restype = None
    lib.bzamd_set_call_tables.argtypes = [ctypes.c_int]
    lib.bzamd_set_call_tables.restype = ctypes.c_uint64
    lib.bzamd_set_max_rows_per_pass.argtypes = [u64]
    lib.bzamd_set_max_rows_per_pass.restype = None
    lib.bzamd_device_id.argtypes = [ctypes.c_int]
    lib.bzamd_device_id.restype = ctypes.c_int
    lib.bzamd_multi_device_columns_per_device.argtypes = [u32]
    lib.bzamd_multi_device_columns_per_device.restype = u32
    lib.bzamd_multi_device_exchange.restype = ctypes.c_char_p
    lib.bzamd_msm_multi_device.argtypes = [cu, ctypes.POINTER(vp), u32,
                                           ctypes.POINTER(sxt_sequence_descriptor),
                                           ctypes.POINTER(vp)]
    lib.bzamd_msm_multi_device.restype = None
    lib.bzamd_set_shard_min_bytes.argtypes = [u64]
    lib.bzamd_set_shard_min_bytes.restype = None
    lib.bzamd_accumulate_form.restype = ctypes.c_int
    lib.bzamd_sumcheck_device_bytes.restype = ctypes.c_uint64
    lib.bzamd_sumcheck_transcript_begin.argtypes = [vp, u64, u64]
    lib.bzamd_sumcheck_transcript_begin.restype = None
    lib.bzamd_sumcheck_transcript_round.argtypes = [vp, vp, vp, cu]
    lib.bzamd_sumcheck_transcript_round.restype = None
    lib.bzamd_prove_sumcheck_transcript.argtypes = [vp, vp, vp, vp, cu, vp]
    lib.bzamd_prove_sumcheck_transcript.restype = None
    lib.bzamd_sumcheck_transcript_workspace_bytes.argtypes = [cu, vp]
    lib.bzamd_sumcheck_transcript_workspace_bytes.restype = u64
    lib.bzamd_prove_sumcheck_transcript_device.argtypes = [vp, vp, vp, vp, cu, vp, vp, u64, vp]
    lib.bzamd_prove_sumcheck_transcript_device.restype = None
    lib.bzamd_verify_sumcheck.argtypes = [vp, vp, vp, cu, vp, cu, cu]
    lib.bzamd_verify_sumcheck.restype = ctypes.c_int
    # (an older build selected with BLITZAR_AMD_LIB lacks these three)
    if hasattr(lib, "bzamd_prove_sumcheck_transcript_device_columns"):
        lib.bzamd_prove_sumcheck_transcript_columns.argtypes = [vp, vp, vp, vp, cu, vp]
        lib.bzamd_prove_sumcheck_transcript_columns.restype = None
        lib.bzamd_sumcheck_transcript_columns_workspace_bytes.argtypes = [cu, vp]
        lib.bzamd_sumcheck_transcript_columns_workspace_bytes.restype = u64
        lib.bzamd_prove_sumcheck_transcript_device_columns.argtypes = [vp, vp, vp, vp, cu, vp, vp,
                                                                       u64, vp]
        lib.bzamd_prove_sumcheck_transcript_device_columns.restype = None
    if hasattr(lib, "bzamd_combine_columns_device"):
        lib.bzamd_mle_evaluation_vector.argtypes = [vp, cu, vp, cu, u64]
        lib.bzamd_mle_evaluation_vector.restype = None
        lib.bzamd_mle_evaluation_vector_device.argtypes = [vp, cu, vp, cu, u64, vp]
        lib.bzamd_mle_evaluation_vector_device.restype = None
        lib.bzamd_combine_columns.argtypes = [vp, vp, cu, vp]
        lib.bzamd_combine_columns.restype = None
        lib.bzamd_combine_columns_device.argtypes = [vp, vp, cu, vp, vp]
        lib.bzamd_combine_columns_device.restype = None
    if hasattr(lib, "bzamd_invert_columns_device"):
        lib.bzamd_invert_columns.argtypes = [vp, vp, cu, vp]
        lib.bzamd_invert_columns.restype = None
        lib.bzamd_invert_columns_device.argtypes = [vp, vp, cu, vp, vp]
        lib.bzamd_invert_columns_device.restype = None
    if hasattr(lib, "bzamd_count_multiplicities_device"):
        lib.bzamd_count_multiplicities_workspace_bytes.argtypes = [u64]
        lib.bzamd_count_multiplicities_workspace_bytes.restype = u64
        lib.bzamd_count_multiplicities.argtypes = [vp, vp, cu, vp]
        lib.bzamd_count_multiplicities.restype = None
        lib.bzamd_count_multiplicities_device.argtypes = [vp, vp, cu, vp, vp, u64, vp]
        lib.bzamd_count_multiplicities_device.restype = None
        lib.bzamd_multiplicity_first_slot.argtypes = [cu, vp, u64]
        lib.bzamd_multiplicity_first_slot.restype = u64
    if hasattr(lib, "bzamd_sum_by_key_device"):
        lib.bzamd_sum_by_key_workspace_bytes.argtypes = [u64, cu]
        lib.bzamd_sum_by_key_workspace_bytes.restype = u64
        lib.bzamd_sum_by_key.argtypes = [vp, vp, vp, vp, vp, cu, vp]
        lib.bzamd_sum_by_key.restype = None
        lib.bzamd_sum_by_key_device.argtypes = [vp, vp, vp, vp, vp, cu, vp, vp, u64, vp]
        lib.bzamd_sum_by_key_device.restype = None
    if hasattr(lib, "bzamd_select_rows_device"):
        lib.bzamd_select_rows_workspace_bytes.argtypes = [u64]
        lib.bzamd_select_rows_workspace_bytes.restype = u64
        lib.bzamd_select_rows.argtypes = [vp, vp, vp]
        lib.bzamd_select_rows.restype = None
        lib.bzamd_select_rows_device.argtypes = [vp, vp, vp, vp, u64, vp]
        lib.bzamd_select_rows_device.restype = None
        lib.bzamd_select_rows_packed_width.argtypes = [ctypes.c_int]
        lib.bzamd_select_rows_packed_width.restype = ctypes.c_int
        lib.bzamd_take_rows.argtypes = [vp]
        lib.bzamd_take_rows.restype = None
        lib.bzamd_take_rows_device.argtypes = [vp, vp]
        lib.bzamd_take_rows_device.restype = None
    if hasattr(lib, "bzamd_decompose_words_device"):
        lib.bzamd_decompose_words.argtypes = [vp, vp, vp, cu, vp]
        lib.bzamd_decompose_words.restype = None
        lib.bzamd_decompose_words_device.argtypes = [vp, vp, vp, cu, vp, vp]
        lib.bzamd_decompose_words_device.restype = None
        lib.bzamd_map_words.argtypes = [vp, vp]
        lib.bzamd_map_words.restype = None
        lib.bzamd_map_words_device.argtypes = [vp, vp, vp]
        lib.bzamd_map_words_device.restype = None
    if hasattr(lib, "bzamd_evaluate_columns_device"):
        lib.bzamd_evaluate_columns.argtypes = [vp, cu, vp, vp]
        lib.bzamd_evaluate_columns.restype = None
        lib.bzamd_evaluate_columns_workspace_bytes.argtypes = [cu, cu, u64]
        lib.bzamd_evaluate_columns_workspace_bytes.restype = u64
        lib.bzamd_evaluate_columns_device.argtypes = [vp, cu, vp, vp, vp, u64, vp]
        lib.bzamd_evaluate_columns_device.restype = None
    if hasattr(lib, "bzamd_batch_quotients_device"):
        lib.bzamd_fold_polynomial.argtypes = [vp, vp, vp, cu, vp, u64, vp, cu]
        lib.bzamd_fold_polynomial.restype = None
        lib.bzamd_fold_polynomial_device.argtypes = [vp, vp, vp, cu, vp, u64, vp, cu, vp]
        lib.bzamd_fold_polynomial_device.restype = None
        lib.bzamd_evaluate_polynomials.argtypes = [vp, cu, vp, vp, u64, cu, vp, cu]
        lib.bzamd_evaluate_polynomials.restype = None
        lib.bzamd_evaluate_polynomials_workspace_bytes.argtypes = [cu, u64, cu, cu]
        lib.bzamd_evaluate_polynomials_workspace_bytes.restype = u64
        lib.bzamd_evaluate_polynomials_device.argtypes = [vp, cu, vp, vp, u64, cu, vp, cu, vp, u64,
                                                          vp]
        lib.bzamd_evaluate_polynomials_device.restype = None
        lib.bzamd_batch_quotients.argtypes = [vp, vp, cu, vp, vp, u64, cu, vp, vp, cu]
        lib.bzamd_batch_quotients.restype = None
        lib.bzamd_batch_quotients_workspace_bytes.argtypes = [cu, u64, cu, cu]
        lib.bzamd_batch_quotients_workspace_bytes.restype = u64
        lib.bzamd_batch_quotients_device.argtypes = [vp, vp, cu, vp, vp, u64, cu, vp, vp, cu, vp,
                                                     u64, vp]
        lib.bzamd_batch_quotients_device.restype = None
    if hasattr(lib, "bzamd_combine_commitments_device"):
        lib.bzamd_verify_sumcheck_device.argtypes = [vp, vp, vp, vp, cu, vp, cu, cu, cu, vp]
        lib.bzamd_verify_sumcheck_device.restype = None
        lib.bzamd_check_sumcheck_evaluations.argtypes = [cu, vp, vp, cu, vp, vp, cu, cu]
        lib.bzamd_check_sumcheck_evaluations.restype = ctypes.c_int
        lib.bzamd_check_sumcheck_evaluations_workspace_bytes.argtypes = [cu, cu, cu]
        lib.bzamd_check_sumcheck_evaluations_workspace_bytes.restype = u64
        lib.bzamd_check_sumcheck_evaluations_device.argtypes = [vp, cu, vp, vp, cu, vp, vp, cu, cu,
                                                                cu, vp, u64, vp]
        lib.bzamd_check_sumcheck_evaluations_device.restype = None
        lib.bzamd_combine_commitments.argtypes = [vp, vp, vp, u64]
        lib.bzamd_combine_commitments.restype = ctypes.c_int
        lib.bzamd_combine_commitments_workspace_bytes.argtypes = [u64]
        lib.bzamd_combine_commitments_workspace_bytes.restype = u64
        lib.bzamd_combine_commitments_device.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp]
        lib.bzamd_combine_commitments_device.restype = None
    # (an older build selected with BLITZAR_AMD_LIB lacks these two)
    if hasattr(lib, "bzamd_prepare_tiles_converted"):
        lib.bzamd_prepare_tiles_converted.argtypes = []
        lib.bzamd_prepare_tiles_converted.restype = u64
        lib.bzamd_caller_table_reset.argtypes = []
        lib.bzamd_caller_table_reset.restype = None
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def init(backend, num_precomputed_generators=0):
    cfg = sxt_config(backend, num_precomputed_generators)
    return load().sxt_init(ctypes.byref(cfg))


def reset_for_testing():
    load().bzamd_reset_for_testing()


def make_descriptors(columns):
    """columns: iterable of (numpy array of shape [n, nbytes] or 1-D integer array, is_signed).

    Returns (ctypes array, keep-alive list).  1-D integer arrays use their itemsize as
    element_nbytes (little-endian host assumed)."""
    cols = list(columns)
    descs = (sxt_sequence_descriptor * max(1, len(cols)))()
    keep = []
    for i, (arr, is_signed) in enumerate(cols):
        arr = np.ascontiguousarray(arr)
        if arr.ndim == 1:
            nbytes, n = arr.dtype.itemsize, arr.shape[0]
        else:
            assert arr.dtype == np.uint8
            n, nbytes = arr.shape
        keep.append(arr)
        descs[i] = sxt_sequence_descriptor(nbytes, n, arr.ctypes.data if n > 0 else None,
                                           1 if is_signed else 0)
    return descs, keep


def compute_pedersen_commitments(curve_id, columns, generators=None, offset_generators=0):
    """Drop-in Pedersen call with host buffers.  `generators`: uint8 array in the C-ABI layout of
    the curve, or None for the built-in ristretto generators."""
    lib = load()
    descs, keep = make_descriptors(columns)
    num = len(keep)
    out = np.zeros((num, CURVE_LAYOUT[curve_id][1]), dtype=np.uint8)
    if curve_id == SXT_CURVE_RISTRETTO255 and generators is None:
        lib.sxt_curve25519_compute_pedersen_commitments(_ptr(out), num, descs, offset_generators)
        return out
    fn = {
        SXT_CURVE_RISTRETTO255: lib.sxt_curve25519_compute_pedersen_commitments_with_generators,
        SXT_CURVE_BLS_381: lib.sxt_bls12_381_g1_compute_pedersen_commitments_with_generators,
        SXT_CURVE_BN_254:
            lib.sxt_bn254_g1_uncompressed_compute_pedersen_commitments_with_generators,
        SXT_CURVE_GRUMPKIN:
            lib.sxt_grumpkin_uncompressed_compute_pedersen_commitments_with_generators,
    }[curve_id]
    gens = np.ascontiguousarray(generators)
    fn(_ptr(out), num, descs, _ptr(gens))
    return out


def offsets_array(offsets, num_columns):
    """per-column generator offsets -> (ctypes u64 pointer or None, keep-alive array)"""
    if offsets is None:
        return None, None
    arr = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    assert arr.shape[0] == num_columns, "one generator offset per column"
    return arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), arr


def compute_commitments_with_generator_offsets(curve_id, columns, generators, offsets):
    """commitments[i] = sum_j scalar_ij * G[offsets[i] + j] with host buffers (either backend).
    `generators`: uint8 array in the C-ABI layout of the curve (its rows are the sequence G), or None
    for the built-in ristretto generators; `offsets`: one per column, or None (all 0)."""
    lib = load()
    descs, keep = make_descriptors(columns)
    num = len(keep)
    out = np.zeros((num, CURVE_LAYOUT[curve_id][1]), dtype=np.uint8)
    offs, _keep_offs = offsets_array(offsets, num)
    if generators is None:
        assert curve_id == SXT_CURVE_RISTRETTO255, "built-in generators are ristretto255 only"
        lib.bzamd_curve25519_compute_commitments_with_offsets(_ptr(out), num, descs, offs)
        return out
    gens = np.ascontiguousarray(generators)
    lib.bzamd_compute_commitments_with_generator_offsets(curve_id, _ptr(out), num, descs,
                                                         _ptr(gens), gens.shape[0], offs)
    return out


def msm_projective(curve_id, columns, generators):
    """raw projective MSM results (host operands), one element per column"""
    lib = load()
    descs, keep = make_descriptors(columns)
    out = np.zeros((len(keep), CURVE_LAYOUT[curve_id][2]), dtype=np.uint8)
    gens = np.ascontiguousarray(generators)
    lib.bzamd_msm_projective(curve_id, _ptr(out), len(keep), descs, _ptr(gens))
    return out


def fold_encode(curve_id, partials):
    """partials: uint8 [num_partials, num_outputs, projective bytes] -> canonical [num_outputs, .]"""
    p = np.ascontiguousarray(partials, dtype=np.uint8)
    num_partials, num_outputs = p.shape[0], p.shape[1]
    out = np.zeros((num_outputs, CURVE_LAYOUT[curve_id][1]), dtype=np.uint8)
    load().bzamd_fold_encode(curve_id, _ptr(out), _ptr(p), num_partials, num_outputs)
    return out


def get_generators(n, offset=0):
    out = np.zeros((n, 20), dtype=np.uint64)
    rc = load().sxt_ristretto255_get_generators(_ptr(out) if n > 0 else None, n, offset)
    assert rc == 0
    return out


def get_one_commit(n):
    out = np.zeros(20, dtype=np.uint64)
    rc = load().sxt_curve25519_get_one_commit(_ptr(out), n)
    assert rc == 0
    return out


def transcript_new(label):
    """a fresh Merlin transcript (203 bytes) with the application label"""
    raw = label.encode() if isinstance(label, str) else bytes(label)
    out = np.zeros(203, dtype=np.uint8)
    load().bzamd_transcript_init(_ptr(out), raw, len(raw))
    return out


def _rounds(n):
    return max(int(n) - 1, 0).bit_length()


def prove_inner_product(transcript, n, generators_offset, a_vector, b_vector):
    """sxt_curve25519_prove_inner_product -> (l [rounds, 32], r [rounds, 32], ap [32], transcript)"""
    t = np.ascontiguousarray(transcript, dtype=np.uint8).copy()
    a = np.ascontiguousarray(a_vector, dtype=np.uint8).reshape(n, 32)
    b = np.ascontiguousarray(b_vector, dtype=np.uint8).reshape(n, 32)
    rounds = _rounds(n)
    l = np.zeros((max(rounds, 1), 32), dtype=np.uint8)
    r = np.zeros((max(rounds, 1), 32), dtype=np.uint8)
    ap = np.zeros(32, dtype=np.uint8)
    load().sxt_curve25519_prove_inner_product(_ptr(l), _ptr(r), _ptr(ap), _ptr(t), n,
                                              generators_offset, _ptr(a), _ptr(b))
    return l[:rounds], r[:rounds], ap, t


def inner_product_workspace_bytes(n):
    """bytes of device workspace bzamd_prove_inner_product_device needs for n elements (0 for
    n = 0 or n > 2^30); needs no backend"""
    return load().bzamd_inner_product_workspace_bytes(n)


def prove_inner_product_device(n, generators_offset, a_device_ptr, b_device_ptr, l_device_ptr,
                               r_device_ptr, ap_device_ptr, transcript_device_ptr,
                               workspace_device_ptr, workspace_bytes, generators_device_ptr=None,
                               stream=None):
    """bzamd_prove_inner_product_device: every operand is a raw device pointer (e.g.
    tensor.data_ptr()) on the current device; `generators_device_ptr` None: the built-in
    generators from `generators_offset`.  Only enqueues on `stream`."""
    load().bzamd_prove_inner_product_device(l_device_ptr, r_device_ptr, ap_device_ptr,
                                            transcript_device_ptr, n, generators_offset,
                                            generators_device_ptr, a_device_ptr, b_device_ptr,
                                            workspace_device_ptr, workspace_bytes, stream)


def inner_product_verify_workspace_bytes(n):
    """bytes of device workspace bzamd_verify_inner_product_device needs for n elements (0 for
    n = 0 or n > 2^30); needs no backend"""
    return load().bzamd_inner_product_verify_workspace_bytes(n)


def verify_inner_product_device(n, generators_offset, b_device_ptr, product_device_ptr,
                                a_commit_device_ptr, l_device_ptr, r_device_ptr, ap_device_ptr,
                                transcript_device_ptr, verdict_device_ptr, workspace_device_ptr,
                                workspace_bytes, generators_device_ptr=None, stream=None):
    """bzamd_verify_inner_product_device: every operand is a raw device pointer (e.g.
    tensor.data_ptr()) on the current device; the verdict is one uint32 there (1 accepted, 0
    rejected); `generators_device_ptr` None: the built-in generators from `generators_offset`.
    Only enqueues on `stream`."""
    load().bzamd_verify_inner_product_device(verdict_device_ptr, transcript_device_ptr, n,
                                             generators_offset, generators_device_ptr,
                                             b_device_ptr, product_device_ptr, a_commit_device_ptr,
                                             l_device_ptr, r_device_ptr, ap_device_ptr,
                                             workspace_device_ptr, workspace_bytes, stream)


def inner_product_verify_batch_workspace_bytes(n, num_proofs):
    """bytes of device workspace bzamd_verify_inner_product_batch_device needs for num_proofs
    proofs of n elements (0 outside the limits); needs no backend"""
    return load().bzamd_inner_product_verify_batch_workspace_bytes(n, num_proofs)


def verify_inner_product_batch_device(n, num_proofs, generators_offset, b_device_ptr,
                                      product_device_ptr, a_commit_device_ptr, l_device_ptr,
                                      r_device_ptr, ap_device_ptr, transcript_device_ptr,
                                      verdict_device_ptr, workspace_device_ptr, workspace_bytes,
                                      generators_device_ptr=None, stream=None):
    """bzamd_verify_inner_product_batch_device: num_proofs proofs of one length n over one generator
    set, back to back in every operand (include/blitzar_amd.h has the layout); every operand is a
    raw device pointer on the current device, the verdicts are num_proofs uint32 there;
    `generators_device_ptr` None: the built-in generators from `generators_offset`.  Only enqueues
    on `stream`."""
    load().bzamd_verify_inner_product_batch_device(
        verdict_device_ptr, transcript_device_ptr, n, num_proofs, generators_offset,
        generators_device_ptr, b_device_ptr, product_device_ptr, a_commit_device_ptr, l_device_ptr,
        r_device_ptr, ap_device_ptr, workspace_device_ptr, workspace_bytes, stream)


def verify_inner_product(transcript, n, generators_offset, b_vector, product, a_commit, l_vector,
                         r_vector, ap_value):
    """sxt_curve25519_verify_inner_product -> (bool, transcript after)"""
    t = np.ascontiguousarray(transcript, dtype=np.uint8).copy()
    b = np.ascontiguousarray(b_vector, dtype=np.uint8).reshape(n, 32)
    lv = np.ascontiguousarray(l_vector, dtype=np.uint8).reshape(-1, 32)
    rv = np.ascontiguousarray(r_vector, dtype=np.uint8).reshape(-1, 32)
    if lv.shape[0] == 0:
        lv = rv = np.zeros((1, 32), np.uint8)
    rc = load().sxt_curve25519_verify_inner_product(
        _ptr(t), n, generators_offset, _ptr(b), _ptr(np.ascontiguousarray(product, np.uint8)),
        _ptr(np.ascontiguousarray(a_commit, np.uint64)), _ptr(lv), _ptr(rv),
        _ptr(np.ascontiguousarray(ap_value, np.uint8)))
    return bool(rc), t


class sumcheck_descriptor(ctypes.Structure):
    _fields_ = [("mles", ctypes.c_void_p), ("product_table", ctypes.c_void_p),
                ("product_terms", ctypes.c_void_p), ("n", ctypes.c_uint),
                ("num_mles", ctypes.c_uint), ("num_products", ctypes.c_uint),
                ("num_product_terms", ctypes.c_uint), ("round_degree", ctypes.c_uint)]


SUMCHECK_CALLBACK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_uint)
SUMCHECK_PRODUCT_STRIDE = {0: 36, 1: 40}  # std::pair<FIELD, unsigned> of the reference


def _sumcheck_call(symbol, field_id, mles_ptr, num_mles, product_table, product_terms, n,
                   round_degree, callback, with_evaluations, stream=None, context=None):
    table = np.ascontiguousarray(product_table, dtype=np.uint8)
    terms = np.ascontiguousarray(product_terms, dtype=np.uint32)
    num_variables = max((int(n) - 1).bit_length(), 1)
    polys = np.zeros((num_variables, round_degree + 1, 32), dtype=np.uint8)
    point = np.zeros((num_variables, 32), dtype=np.uint8)
    d = sumcheck_descriptor(mles_ptr, table.ctypes.data, terms.ctypes.data, n, num_mles,
                            table.size // SUMCHECK_PRODUCT_STRIDE[field_id], terms.size,
                            round_degree)
    cb = callback if isinstance(callback, SUMCHECK_CALLBACK) else SUMCHECK_CALLBACK(callback)
    vp = ctypes.c_void_p
    fn = getattr(load(), symbol)
    fn.restype = None
    tail = [ctypes.c_uint, ctypes.POINTER(sumcheck_descriptor), SUMCHECK_CALLBACK, vp]
    if not with_evaluations:
        fn.argtypes = [vp, vp] + tail
        fn(_ptr(polys), _ptr(point), field_id, ctypes.byref(d), cb, context)
        return polys, point
    evaluations = np.zeros((num_mles, 32), dtype=np.uint8)
    if symbol == "bzamd_prove_sumcheck_device":
        fn.argtypes = [vp, vp, vp] + tail + [vp]
        fn(_ptr(polys), _ptr(point), _ptr(evaluations), field_id, ctypes.byref(d), cb, context,
           stream)
    else:
        fn.argtypes = [vp, vp, vp] + tail
        fn(_ptr(polys), _ptr(point), _ptr(evaluations), field_id, ctypes.byref(d), cb, context)
    return polys, point, evaluations


def prove_sumcheck(field_id, mles, product_table, product_terms, n, round_degree, callback,
                   context=None):
    """sxt_prove_sumcheck.  mles: uint8 [num_mles, n, 32]; product_table: raw bytes of
    num_products x {32-byte multiplier; unsigned length}; callback(r_ptr, ctx, poly_ptr, length).
    -> (polynomials [num_variables, round_degree + 1, 32], evaluation_point [num_variables, 32])"""
    m = np.ascontiguousarray(mles, dtype=np.uint8)
    return _sumcheck_call("sxt_prove_sumcheck", field_id, m.ctypes.data, m.shape[0], product_table,
                          product_terms, n, round_degree, callback, False, context=context)


def prove_sumcheck_with_evaluations(field_id, mles, product_table, product_terms, n, round_degree,
                                    callback, context=None):
    """bzamd_prove_sumcheck: prove_sumcheck plus mle_evaluations [num_mles, 32], the value of every
    MLE at the evaluation point -> (polynomials, evaluation_point, mle_evaluations)"""
    m = np.ascontiguousarray(mles, dtype=np.uint8)
    return _sumcheck_call("bzamd_prove_sumcheck", field_id, m.ctypes.data, m.shape[0],
                          product_table, product_terms, n, round_degree, callback, True,
                          context=context)


def prove_sumcheck_device(field_id, mles_device_ptr, num_mles, product_table, product_terms, n,
                          round_degree, callback, stream=None, context=None):
    """bzamd_prove_sumcheck_device: the tables ([num_mles, n, 32] bytes) are device memory of the
    current device at `mles_device_ptr`, `stream` a hipStream_t as an integer (None: the default
    stream); everything else on the host -> (polynomials, evaluation_point, mle_evaluations)"""
    return _sumcheck_call("bzamd_prove_sumcheck_device", field_id, int(mles_device_ptr), num_mles,
                          product_table, product_terms, n, round_degree, callback, True,
                          None if stream is None else ctypes.c_void_p(int(stream)), context=context)


#--------------------------------------------------------------------------------------------------
# sumcheck with the library's own transcript (the reference's reference_transcript)
#--------------------------------------------------------------------------------------------------
class bzamd_sumcheck_transcript_context(ctypes.Structure):
    _fields_ = [("transcript", ctypes.c_void_p), ("field_id", ctypes.c_uint)]


def __getattr__(name):
    # SUMCHECK_TRANSCRIPT_ROUND: bzamd_sumcheck_transcript_round as a SUMCHECK_CALLBACK, for the
    # `callback` of the entry points above with a bzamd_sumcheck_transcript_context (by reference)
    # as their `context`; made on first use, the library is not loaded on import
    if name == "SUMCHECK_TRANSCRIPT_ROUND":
        cb = ctypes.cast(load().bzamd_sumcheck_transcript_round, SUMCHECK_CALLBACK)
        globals()[name] = cb
        return cb
    raise AttributeError(name)


def sumcheck_transcript_begin(transcript, num_variables, round_degree):
    """bzamd_sumcheck_transcript_begin, in place on a uint8 [203] array"""
    assert transcript.dtype == np.uint8 and transcript.size == 203
    load().bzamd_sumcheck_transcript_begin(_ptr(transcript), num_variables, round_degree)


def _transcript_descriptor(field_id, mles_ptr, num_mles, product_table, product_terms, n,
                           round_degree):
    table = np.ascontiguousarray(product_table, dtype=np.uint8)
    terms = np.ascontiguousarray(product_terms, dtype=np.uint32)
    d = sumcheck_descriptor(mles_ptr, table.ctypes.data, terms.ctypes.data, n, num_mles,
                            table.size // SUMCHECK_PRODUCT_STRIDE[field_id], terms.size,
                            round_degree)
    return d, (table, terms)


def prove_sumcheck_transcript(field_id, mles, product_table, product_terms, n, round_degree,
                              transcript, with_evaluations=True):
    """bzamd_prove_sumcheck_transcript (host operands, either backend)
    -> (polynomials, evaluation_point, mle_evaluations or None, transcript after)"""
    m = np.ascontiguousarray(mles, dtype=np.uint8)
    d, _keep = _transcript_descriptor(field_id, m.ctypes.data, m.shape[0], product_table,
                                      product_terms, n, round_degree)
    num_variables = max((int(n) - 1).bit_length(), 1)
    polys = np.zeros((num_variables, round_degree + 1, 32), dtype=np.uint8)
    point = np.zeros((num_variables, 32), dtype=np.uint8)
    evaluations = np.zeros((m.shape[0], 32), dtype=np.uint8) if with_evaluations else None
    t = np.ascontiguousarray(transcript, dtype=np.uint8).copy()
    load().bzamd_prove_sumcheck_transcript(_ptr(polys), _ptr(point), _ptr(evaluations), _ptr(t),
                                           field_id, ctypes.byref(d))
    return polys, point, evaluations, t


def sumcheck_transcript_workspace_bytes(field_id, n, num_mles, num_products, num_product_terms,
                                        round_degree):
    d = sumcheck_descriptor(None, None, None, n, num_mles, num_products, num_product_terms,
                            round_degree)
    return load().bzamd_sumcheck_transcript_workspace_bytes(field_id, ctypes.byref(d))


def prove_sumcheck_transcript_device(field_id, mles_device_ptr, num_mles, product_table,
                                     product_terms, n, round_degree, polynomials_ptr,
                                     evaluation_point_ptr, mle_evaluations_ptr, transcript_ptr,
                                     workspace_ptr, workspace_bytes, stream=None):
    """bzamd_prove_sumcheck_transcript_device: enqueue only.  Every *_ptr is memory of the current
    device as an integer (torch: tensor.data_ptr()), mle_evaluations_ptr may be None; `stream` a
    hipStream_t as an integer (None: the default stream).  Results are in the caller's device
    memory once the stream has run."""
    d, _keep = _transcript_descriptor(field_id, int(mles_device_ptr), num_mles, product_table,
                                      product_terms, n, round_degree)
    load().bzamd_prove_sumcheck_transcript_device(
        int(polynomials_ptr), int(evaluation_point_ptr),
        None if mle_evaluations_ptr is None else int(mle_evaluations_ptr), int(transcript_ptr),
        field_id, ctypes.byref(d), int(workspace_ptr), workspace_bytes,
        None if stream is None else ctypes.c_void_p(int(stream)))


def verify_sumcheck(field_id, claimed_sum, round_polynomials, transcript):
    """bzamd_verify_sumcheck.  round_polynomials: uint8 [num_variables, round_degree + 1, 32]
    -> (ok, expected_sum after, evaluation_point, transcript after)"""
    polys = np.ascontiguousarray(round_polynomials, dtype=np.uint8)
    num_variables, length = polys.shape[0], polys.shape[1]
    expected = np.ascontiguousarray(claimed_sum, dtype=np.uint8).copy()
    point = np.zeros((num_variables, 32), dtype=np.uint8)
    t = np.ascontiguousarray(transcript, dtype=np.uint8).copy()
    ok = load().bzamd_verify_sumcheck(_ptr(expected), _ptr(point), _ptr(t), field_id, _ptr(polys),
                                      num_variables, length - 1)
    return bool(ok), expected, point, t


def _stream(stream):
    return None if stream is None else ctypes.c_void_p(int(stream))


def verify_sumcheck_device(field_id, num_variables, round_degree, num_proofs,
                           round_polynomials_ptr, expected_sums_ptr, evaluation_points_ptr,
                           transcripts_ptr, verdicts_ptr, stream=None):
    """bzamd_verify_sumcheck_device: enqueue only.  `num_proofs` proofs of one shape back to back;
    every *_ptr is memory of the current device as an integer (torch: tensor.data_ptr()): per proof
    num_variables x (round_degree + 1) x 32 bytes of polynomials, 32 of expected sum (in / out),
    num_variables x 32 of evaluation point (out), 203 of transcript (in / out) and one uint32
    verdict (out)."""
    load().bzamd_verify_sumcheck_device(int(verdicts_ptr), int(expected_sums_ptr),
                                        int(evaluation_points_ptr), int(transcripts_ptr), field_id,
                                        int(round_polynomials_ptr), num_variables, round_degree,
                                        num_proofs, _stream(stream))


def _statement(field_id, product_table, product_terms):
    table = np.ascontiguousarray(product_table, dtype=np.uint8)
    terms = np.ascontiguousarray(product_terms, dtype=np.uint32)
    return table, terms, table.size // SUMCHECK_PRODUCT_STRIDE[field_id]


def check_sumcheck_evaluations(field_id, expected_sum, mle_evaluations, product_table,
                               product_terms):
    """bzamd_check_sumcheck_evaluations (host operands) -> bool.  mle_evaluations: uint8
    [num_mles, 32]; the table and the terms as the prover takes them"""
    table, terms, num_products = _statement(field_id, product_table, product_terms)
    evaluations = np.ascontiguousarray(mle_evaluations, dtype=np.uint8).reshape(-1, 32)
    expected = np.ascontiguousarray(expected_sum, dtype=np.uint8)
    return bool(load().bzamd_check_sumcheck_evaluations(
        field_id, _ptr(expected), _ptr(evaluations), evaluations.shape[0], _ptr(table), _ptr(terms),
        num_products, terms.size))


def check_sumcheck_evaluations_workspace_bytes(field_id, num_products, num_product_terms):
    """bytes of device workspace bzamd_check_sumcheck_evaluations_device needs (0 for counts the
    call rejects); needs no backend"""
    return load().bzamd_check_sumcheck_evaluations_workspace_bytes(field_id, num_products,
                                                                   num_product_terms)


def check_sumcheck_evaluations_device(field_id, num_mles, product_table, product_terms, num_proofs,
                                      expected_sums_ptr, mle_evaluations_ptr, verdicts_ptr,
                                      workspace_ptr, workspace_bytes, stream=None):
    """bzamd_check_sumcheck_evaluations_device: enqueue only.  One statement (host arrays) for
    `num_proofs` proofs; every *_ptr is memory of the current device as an integer: num_proofs x 32
    bytes of expected sums, num_proofs x num_mles x 32 of evaluations, num_proofs uint32 verdicts."""
    table, terms, num_products = _statement(field_id, product_table, product_terms)
    load().bzamd_check_sumcheck_evaluations_device(
        int(verdicts_ptr), field_id, int(expected_sums_ptr), int(mle_evaluations_ptr), num_mles,
        _ptr(table), _ptr(terms), num_products, terms.size, num_proofs, int(workspace_ptr),
        workspace_bytes, _stream(stream))


def combine_commitments(commitments, coefficients):
    """bzamd_combine_commitments (host operands): commitments uint8 [K, 32] compressed, coefficients
    uint8 [K, 32] -> (every encoding decoded, sum_j c_j C_j as one sxt_ristretto255, uint64 [20])"""
    c = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(-1, 32)
    k = np.ascontiguousarray(coefficients, dtype=np.uint8).reshape(-1, 32)
    assert c.shape == k.shape
    out = np.zeros(20, dtype=np.uint64)
    ok = load().bzamd_combine_commitments(_ptr(out), _ptr(c), _ptr(k), c.shape[0])
    return bool(ok), out


def combine_commitments_workspace_bytes(num_commitments):
    """bytes of device workspace bzamd_combine_commitments_device needs (0 for 0 or more than 2^28
    commitments); needs no backend"""
    return load().bzamd_combine_commitments_workspace_bytes(num_commitments)


def combine_commitments_device(num_commitments, commitments_ptr, coefficients_ptr, combined_ptr,
                               valid_ptr, workspace_ptr, workspace_bytes, stream=None):
    """bzamd_combine_commitments_device: enqueue only.  Every *_ptr is memory of the current device
    as an integer: num_commitments x 32 bytes of encodings and of coefficients, 160 bytes of
    `combined` (one sxt_ristretto255), one uint32 `valid`."""
    load().bzamd_combine_commitments_device(int(combined_ptr), int(valid_ptr), int(commitments_ptr),
                                            int(coefficients_ptr), num_commitments,
                                            int(workspace_ptr), workspace_bytes, _stream(stream))


class bzamd_sumcheck_columns(ctypes.Structure):
    _fields_ = [("mles", ctypes.POINTER(sxt_sequence_descriptor)),
                ("product_table", ctypes.c_void_p), ("product_terms", ctypes.c_void_p),
                ("n", ctypes.c_uint), ("num_mles", ctypes.c_uint), ("num_products", ctypes.c_uint),
                ("num_product_terms", ctypes.c_uint), ("round_degree", ctypes.c_uint)]


def _sumcheck_columns_call(symbol, field_id, descs, num_mles, product_table, product_terms, n,
                           round_degree, callback, stream=None):
    table = np.ascontiguousarray(product_table, dtype=np.uint8)
    terms = np.ascontiguousarray(product_terms, dtype=np.uint32)
    num_variables = max((int(n) - 1).bit_length(), 1)
    polys = np.zeros((num_variables, round_degree + 1, 32), dtype=np.uint8)
    point = np.zeros((num_variables, 32), dtype=np.uint8)
    evaluations = np.zeros((num_mles, 32), dtype=np.uint8)
    c = bzamd_sumcheck_columns(descs, table.ctypes.data, terms.ctypes.data, n, num_mles,
                               table.size // SUMCHECK_PRODUCT_STRIDE[field_id], terms.size,
                               round_degree)
    cb = SUMCHECK_CALLBACK(callback)
    vp = ctypes.c_void_p
    fn = getattr(load(), symbol)
    fn.restype = None
    fn.argtypes = [vp, vp, vp, ctypes.c_uint, ctypes.POINTER(bzamd_sumcheck_columns),
                   SUMCHECK_CALLBACK, vp]
    args = [_ptr(polys), _ptr(point), _ptr(evaluations), field_id, ctypes.byref(c), cb, None]
    if symbol == "bzamd_prove_sumcheck_device_columns":
        fn.argtypes = fn.argtypes + [vp]
        args.append(stream)
    fn(*args)
    return polys, point, evaluations


def _column_pairs(columns):
    pairs = []
    for c in columns:
        if isinstance(c, tuple):
            pairs.append((np.ascontiguousarray(c[0]), bool(c[1])))
        else:
            c = np.ascontiguousarray(c)
            pairs.append((c, c.ndim == 1 and np.issubdtype(c.dtype, np.signedinteger)))
    return pairs


def _device_descriptors(descriptors):
    ds = list(descriptors)
    descs = (sxt_sequence_descriptor * max(1, len(ds)))()
    for i, (ptr, rows, nbytes, signed) in enumerate(ds):
        descs[i] = sxt_sequence_descriptor(nbytes, rows, int(ptr) if rows > 0 else None,
                                           1 if signed else 0)
    return descs, len(ds)


def prove_sumcheck_columns(field_id, columns, product_table, product_terms, n, round_degree,
                           callback):
    """bzamd_prove_sumcheck_columns.  columns: one per MLE, a 1-D numpy integer array (its itemsize
    is the width, a signed dtype a signed column) or a uint8 [rows, nbytes] array (unsigned
    integers of nbytes, field elements for nbytes = 32), or an (array, is_signed) pair that says
    it outright; at most n rows each, the rest is zero
    -> (polynomials, evaluation_point, mle_evaluations)"""
    descs, keep = make_descriptors(_column_pairs(columns))
    return _sumcheck_columns_call("bzamd_prove_sumcheck_columns", field_id, descs, len(keep),
                                  product_table, product_terms, n, round_degree, callback)


def prove_sumcheck_device_columns(field_id, descriptors, product_table, product_terms, n,
                                  round_degree, callback, stream=None):
    """bzamd_prove_sumcheck_device_columns.  descriptors: one (device_ptr, n_j, nbytes, signed) per
    MLE, memory of the current device; `stream` a hipStream_t as an integer (None: the default
    stream); everything else on the host -> (polynomials, evaluation_point, mle_evaluations)"""
    descs, num_mles = _device_descriptors(descriptors)
    return _sumcheck_columns_call("bzamd_prove_sumcheck_device_columns", field_id, descs, num_mles,
                                  product_table, product_terms, n, round_degree, callback,
                                  None if stream is None else ctypes.c_void_p(int(stream)))


def _transcript_columns(field_id, descs, num_mles, product_table, product_terms, n, round_degree):
    table = np.ascontiguousarray(product_table, dtype=np.uint8)
    terms = np.ascontiguousarray(product_terms, dtype=np.uint32)
    c = bzamd_sumcheck_columns(descs, table.ctypes.data, terms.ctypes.data, n, num_mles,
                               table.size // SUMCHECK_PRODUCT_STRIDE[field_id], terms.size,
                               round_degree)
    return c, (table, terms)


def prove_sumcheck_transcript_columns(field_id, columns, product_table, product_terms, n,
                                      round_degree, transcript, with_evaluations=True):
    """bzamd_prove_sumcheck_transcript_columns (host operands, either backend).  columns: as
    prove_sumcheck_columns; transcript: uint8 [203], or None to pass a null pointer
    -> (polynomials, evaluation_point, mle_evaluations or None, transcript after)"""
    descs, keep = make_descriptors(_column_pairs(columns))
    c, _keep = _transcript_columns(field_id, descs, len(keep), product_table, product_terms, n,
                                   round_degree)
    num_variables = max((int(n) - 1).bit_length(), 1)
    polys = np.zeros((num_variables, round_degree + 1, 32), dtype=np.uint8)
    point = np.zeros((num_variables, 32), dtype=np.uint8)
    evaluations = np.zeros((len(keep), 32), dtype=np.uint8) if with_evaluations else None
    t = None if transcript is None else np.ascontiguousarray(transcript, dtype=np.uint8).copy()
    load().bzamd_prove_sumcheck_transcript_columns(_ptr(polys), _ptr(point), _ptr(evaluations),
                                                   _ptr(t), field_id, ctypes.byref(c))
    return polys, point, evaluations, t


def sumcheck_transcript_columns_workspace_bytes(field_id, n, num_mles, num_products,
                                                num_product_terms, round_degree):
    """bzamd_sumcheck_transcript_columns_workspace_bytes: needs no backend and no descriptors"""
    c = bzamd_sumcheck_columns(None, None, None, n, num_mles, num_products, num_product_terms,
                               round_degree)
    return load().bzamd_sumcheck_transcript_columns_workspace_bytes(field_id, ctypes.byref(c))


def prove_sumcheck_transcript_device_columns(field_id, descriptors, product_table, product_terms, n,
                                             round_degree, polynomials_ptr, evaluation_point_ptr,
                                             mle_evaluations_ptr, transcript_ptr, workspace_ptr,
                                             workspace_bytes, stream=None):
    """bzamd_prove_sumcheck_transcript_device_columns: enqueue only.  descriptors: one (device_ptr,
    n_j, nbytes, signed) per MLE, or a ready sxt_sequence_descriptor array (the one the MSM took);
    every *_ptr is memory of the current device as an integer, mle_evaluations_ptr may be None;
    `stream` a hipStream_t as an integer (None: the default stream).  Results are in the caller's
    device memory once the stream has run."""
    if isinstance(descriptors, ctypes.Array):
        descs, num_mles = descriptors, len(descriptors)
    else:
        descs, num_mles = _device_descriptors(descriptors)
    c, _keep = _transcript_columns(field_id, descs, num_mles, product_table, product_terms, n,
                                   round_degree)
    load().bzamd_prove_sumcheck_transcript_device_columns(
        int(polynomials_ptr), int(evaluation_point_ptr),
        None if mle_evaluations_ptr is None else int(mle_evaluations_ptr),
        None if transcript_ptr is None else int(transcript_ptr), field_id, ctypes.byref(c),
        int(workspace_ptr), workspace_bytes,
        None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_column_combination(ctypes.Structure):
    _fields_ = [("columns", ctypes.POINTER(sxt_sequence_descriptor)),
                ("coefficients", ctypes.c_void_p), ("evaluations", ctypes.c_void_p),
                ("num_columns", ctypes.c_uint), ("n", ctypes.c_uint64)]


def mle_evaluation_vector(field_id, evaluation_point, n, num_variables=None):
    """bzamd_mle_evaluation_vector (host operands, either backend).  evaluation_point: uint8
    [num_variables, 32] (num_variables defaults to its rows) -> uint8 [n, 32]:
    vector[i] = prod_t (bit_{v-1-t}(i) ? r_t : 1 - r_t)"""
    point = np.ascontiguousarray(evaluation_point, dtype=np.uint8)
    if num_variables is None:
        num_variables = point.size // 32
    vector = np.zeros((max(int(n), 1), 32), dtype=np.uint8)
    load().bzamd_mle_evaluation_vector(_ptr(vector), field_id, _ptr(point), num_variables, n)
    return vector[:n]


def mle_evaluation_vector_device(field_id, vector_ptr, evaluation_point_ptr, num_variables, n,
                                 stream=None):
    """bzamd_mle_evaluation_vector_device: enqueue only.  Both pointers are memory of the current
    device as integers (None: a null pointer); `stream` a hipStream_t as an integer (None: the
    default stream)."""
    load().bzamd_mle_evaluation_vector_device(
        None if vector_ptr is None else int(vector_ptr), field_id,
        None if evaluation_point_ptr is None else int(evaluation_point_ptr), num_variables, n,
        None if stream is None else ctypes.c_void_p(int(stream)))


def combine_columns(field_id, columns, coefficients, n, evaluations=None, product=None):
    """bzamd_combine_columns (host operands, either backend).  columns: as prove_sumcheck_columns;
    coefficients, evaluations: uint8 [num_columns, 32]; product: a uint8 [32] buffer the call may
    write (None: a null pointer) -> (combined uint8 [n, 32], product)"""
    descs, keep = make_descriptors(_column_pairs(columns))
    coefficients = np.ascontiguousarray(coefficients, dtype=np.uint8)
    if evaluations is not None:
        evaluations = np.ascontiguousarray(evaluations, dtype=np.uint8)
    combined = np.zeros((max(int(n), 1), 32), dtype=np.uint8)
    c = bzamd_column_combination(descs, coefficients.ctypes.data,
                                 None if evaluations is None else evaluations.ctypes.data,
                                 len(keep), n)
    load().bzamd_combine_columns(_ptr(combined), _ptr(product), field_id, ctypes.byref(c))
    return combined[:n], product


def combine_columns_device(field_id, descriptors, coefficients_ptr, n, combined_ptr,
                           evaluations_ptr=None, product_ptr=None, stream=None):
    """bzamd_combine_columns_device: enqueue only.  descriptors: one (device_ptr, n_j, nbytes,
    signed) per column, or a ready sxt_sequence_descriptor array (the one the MSM took); every
    *_ptr is memory of the current device as an integer; `stream` a hipStream_t as an integer
    (None: the default stream)."""
    if isinstance(descriptors, ctypes.Array):
        descs, num_columns = descriptors, len(descriptors)
    else:
        descs, num_columns = _device_descriptors(descriptors)
    c = bzamd_column_combination(descs, int(coefficients_ptr),
                                 None if evaluations_ptr is None else int(evaluations_ptr),
                                 num_columns, n)
    load().bzamd_combine_columns_device(
        int(combined_ptr), None if product_ptr is None else int(product_ptr), field_id,
        ctypes.byref(c), None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_column_inversion(ctypes.Structure):
    _fields_ = [("columns", ctypes.POINTER(sxt_sequence_descriptor)),
                ("coefficients", ctypes.c_void_p), ("shift", ctypes.c_void_p),
                ("num_columns", ctypes.c_uint), ("n", ctypes.c_uint64)]


def invert_columns(field_id, columns, n, coefficients=None, shift=None, want_scalars=False):
    """bzamd_invert_columns (host operands, either backend).  columns: as combine_columns;
    coefficients: uint8 [num_columns, 32] (None: every coefficient is 1); shift: uint8 [32] (None:
    0) -> inverses uint8 [n, 32] in element form, 1 / (shift + sum_j coefficients[j] column_j[i])
    with 0 for a zero denominator; want_scalars: (inverses, scalars), the same rows in scalar
    form"""
    descs, keep = make_descriptors(_column_pairs(columns))
    if coefficients is not None:
        coefficients = np.ascontiguousarray(coefficients, dtype=np.uint8)
    if shift is not None:
        shift = np.ascontiguousarray(shift, dtype=np.uint8)
    inverses = np.zeros((max(int(n), 1), 32), dtype=np.uint8)
    scalars = np.zeros((max(int(n), 1), 32), dtype=np.uint8) if want_scalars else None
    v = bzamd_column_inversion(descs, None if coefficients is None else coefficients.ctypes.data,
                               None if shift is None else shift.ctypes.data, len(keep), n)
    load().bzamd_invert_columns(_ptr(inverses), _ptr(scalars), field_id, ctypes.byref(v))
    return (inverses[:n], scalars[:n]) if want_scalars else inverses[:n]


def invert_columns_device(field_id, inverses_ptr, scalars_ptr, descriptors, coefficients_ptr,
                          shift_ptr, n, stream=None):
    """bzamd_invert_columns_device: enqueue only, one kernel launch.  descriptors: one (device_ptr,
    n_j, nbytes, signed) per column, or a ready sxt_sequence_descriptor array (the one the MSM
    took); every *_ptr is memory of the current device as an integer (None: a null pointer);
    `stream` a hipStream_t as an integer (None: the default stream)."""
    if isinstance(descriptors, ctypes.Array):
        descs, num_columns = descriptors, len(descriptors)
    else:
        descs, num_columns = _device_descriptors(descriptors)
    v = bzamd_column_inversion(descs, None if coefficients_ptr is None else int(coefficients_ptr),
                               None if shift_ptr is None else int(shift_ptr), num_columns, n)
    load().bzamd_invert_columns_device(
        None if inverses_ptr is None else int(inverses_ptr),
        None if scalars_ptr is None else int(scalars_ptr), field_id, ctypes.byref(v),
        None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_multiplicity_count(ctypes.Structure):
    _fields_ = [("table", sxt_sequence_descriptor), ("lookups", sxt_sequence_descriptor)]


def count_multiplicities_workspace_bytes(table_rows):
    """bzamd_count_multiplicities_workspace_bytes: no backend needed; 0 outside the limits"""
    return load().bzamd_count_multiplicities_workspace_bytes(table_rows)


def multiplicity_first_slot(field_id, element, table_rows):
    """bzamd_multiplicity_first_slot: the slot at which the probe for a key starts (a diagnostic;
    the hash is not part of the ABI).  element: uint8 [32], element form, may be unreduced"""
    element = np.ascontiguousarray(element, dtype=np.uint8)
    return load().bzamd_multiplicity_first_slot(field_id, _ptr(element), table_rows)


def count_multiplicities(field_id, table, lookups, want_misses=True):
    """bzamd_count_multiplicities (host operands, either backend).  table, lookups: one column each
    as in combine_columns (an array or an (array, is_signed) pair); table may be (None, m): the
    range table 0 .. m - 1 -> (multiplicities uint64 [m], misses), or the multiplicities alone
    with want_misses False (a null pointer)"""
    if isinstance(table, tuple) and table[0] is None:
        table_desc, keep_table = sxt_sequence_descriptor(8, int(table[1]), None, 0), None
    else:
        descs, keep_table = make_descriptors(_column_pairs([table]))
        table_desc = descs[0]
    descs, keep_lookups = make_descriptors(_column_pairs([lookups]))
    multiplicities = np.zeros(max(int(table_desc.n), 1), dtype=np.uint64)
    misses = ctypes.c_uint64(0)
    c = bzamd_multiplicity_count(table_desc, descs[0])
    load().bzamd_count_multiplicities(_ptr(multiplicities),
                                      ctypes.byref(misses) if want_misses else None, field_id,
                                      ctypes.byref(c))
    del keep_table, keep_lookups
    multiplicities = multiplicities[:table_desc.n]
    return (multiplicities, int(misses.value)) if want_misses else multiplicities


def count_multiplicities_device(field_id, multiplicities_ptr, misses_ptr, table, lookups,
                                workspace_ptr, workspace_bytes, stream=None):
    """bzamd_count_multiplicities_device: enqueue only, three kernel launches (the range table:
    two).  table, lookups: one (device_ptr, rows, nbytes, signed) each; a table with device_ptr
    None is the range table 0 .. rows - 1; every *_ptr is memory of the current device as an
    integer (None: a null pointer); `stream` a hipStream_t as an integer (None: the default
    stream)."""
    def descriptor(column):
        ptr, rows, nbytes, signed = column
        return sxt_sequence_descriptor(nbytes, rows, None if ptr is None else int(ptr),
                                       1 if signed else 0)
    c = bzamd_multiplicity_count(descriptor(table), descriptor(lookups))
    load().bzamd_count_multiplicities_device(
        None if multiplicities_ptr is None else int(multiplicities_ptr),
        None if misses_ptr is None else int(misses_ptr), field_id, ctypes.byref(c),
        None if workspace_ptr is None else int(workspace_ptr), workspace_bytes,
        None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_key_sums(ctypes.Structure):
    _fields_ = [("table", sxt_sequence_descriptor), ("lookups", sxt_sequence_descriptor),
                ("values", ctypes.POINTER(sxt_sequence_descriptor)),
                ("num_values", ctypes.c_uint)]


def sum_by_key_workspace_bytes(table_rows, num_values):
    """bzamd_sum_by_key_workspace_bytes: no backend needed; 0 outside the limits"""
    return load().bzamd_sum_by_key_workspace_bytes(table_rows, num_values)


def sum_by_key(field_id, table, lookups, values=(), want=("sums", "scalars", "counts", "misses",
                                                          "matches")):
    """bzamd_sum_by_key (host operands, either backend).  table, lookups: as in
    count_multiplicities (table may be (None, m): the range table); values: value columns as in
    combine_columns, at most lookups' rows each; want: the outputs asked for, the others are null
    pointers -> a dict of those: sums, scalars uint8 [num_values, m, 32]; counts uint64 [m];
    misses an int; matches uint32 [n]"""
    if isinstance(table, tuple) and table[0] is None:
        table_desc, keep_table = sxt_sequence_descriptor(8, int(table[1]), None, 0), None
    else:
        descs, keep_table = make_descriptors(_column_pairs([table]))
        table_desc = descs[0]
    lookup_descs, keep_lookups = make_descriptors(_column_pairs([lookups]))
    value_descs, keep_values = make_descriptors(_column_pairs(values))
    m, n, count = int(table_desc.n), int(lookup_descs[0].n), len(keep_values)
    out = {"sums": np.zeros((count, max(m, 1), 32), dtype=np.uint8),
           "scalars": np.zeros((count, max(m, 1), 32), dtype=np.uint8),
           "counts": np.zeros(max(m, 1), dtype=np.uint64),
           "misses": np.zeros(1, dtype=np.uint64),
           "matches": np.zeros(max(n, 1), dtype=np.uint32)}
    out = {name: array for name, array in out.items() if name in want}
    k = bzamd_key_sums(table_desc, lookup_descs[0], value_descs if count else None, count)
    load().bzamd_sum_by_key(*(_ptr(out.get(name)) for name in ("sums", "scalars", "counts",
                                                               "misses", "matches")),
                            field_id, ctypes.byref(k))
    del keep_table, keep_lookups, keep_values
    shaped = {"sums": lambda a: a[:, :m], "scalars": lambda a: a[:, :m], "counts": lambda a: a[:m],
              "misses": lambda a: int(a[0]), "matches": lambda a: a[:n]}
    return {name: shaped[name](array) for name, array in out.items()}


def sum_by_key_device(field_id, sums_ptr, scalars_ptr, counts_ptr, misses_ptr, matches_ptr, table,
                      lookups, values, workspace_ptr, workspace_bytes, stream=None):
    """bzamd_sum_by_key_device: enqueue only, four kernel launches (the range table: three).
    table, lookups: one (device_ptr, rows, nbytes, signed) each; a table with device_ptr None is
    the range table 0 .. rows - 1; values: a list of such tuples; every *_ptr is memory of the
    current device as an integer (None: a null pointer); `stream` a hipStream_t as an integer
    (None: the default stream)."""
    def descriptor(column):
        ptr, rows, nbytes, signed = column
        return sxt_sequence_descriptor(nbytes, rows, None if ptr is None else int(ptr),
                                       1 if signed else 0)
    value_descs, count = _device_descriptors(values)
    k = bzamd_key_sums(descriptor(table), descriptor(lookups), value_descs if count else None,
                       count)
    pointers = [None if p is None else int(p)
                for p in (sums_ptr, scalars_ptr, counts_ptr, misses_ptr, matches_ptr)]
    load().bzamd_sum_by_key_device(
        *pointers, field_id, ctypes.byref(k),
        None if workspace_ptr is None else int(workspace_ptr), workspace_bytes,
        None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_row_selection(ctypes.Structure):
    _fields_ = [("selector", sxt_sequence_descriptor), ("reject", ctypes.c_uint64),
                ("invert", ctypes.c_int),
                ("columns", ctypes.POINTER(sxt_sequence_descriptor)),
                ("selected", ctypes.POINTER(ctypes.c_void_p)), ("num_columns", ctypes.c_uint),
                ("capacity", ctypes.c_uint64), ("zero_tail", ctypes.c_int)]


class bzamd_row_take(ctypes.Structure):
    _fields_ = [("indices", ctypes.c_void_p), ("num_rows", ctypes.c_uint64),
                ("columns", ctypes.POINTER(sxt_sequence_descriptor)),
                ("taken", ctypes.POINTER(ctypes.c_void_p)), ("num_columns", ctypes.c_uint)]


def _pointer_array(pointers):
    ps = [None if p is None else int(p) for p in pointers]
    return (ctypes.c_void_p * max(1, len(ps)))(*ps)


def select_rows_workspace_bytes(n):
    """bzamd_select_rows_workspace_bytes: no backend needed; 0 outside the limits"""
    return load().bzamd_select_rows_workspace_bytes(n)


def select_rows_packed_width(width=-1):
    """bzamd_select_rows_packed_width: columns of at most `width` bytes a row are packed in LDS by
    the device form's second launch (0: none); negative: only ask -> the width in force before"""
    return load().bzamd_select_rows_packed_width(width)


def select_rows(selector, columns=(), reject=0, invert=False, capacity=None, zero_tail=False,
                want_indices=True):
    """bzamd_select_rows (host operands, either backend).  selector: one column of 1 .. 8 bytes a
    row and columns: up to 16 columns, as in combine_columns; capacity: None is the selector's rows
    -> (count, indices uint32 or None, [uint8 [rows, nbytes] per column]) with rows = capacity
    with zero_tail, min(count, capacity) without"""
    selector_descs, keep_selector = make_descriptors(_column_pairs([selector]))
    descs, keep = make_descriptors(_column_pairs(columns))
    n, num = int(selector_descs[0].n), len(keep)
    capacity = n if capacity is None else capacity
    indices = np.zeros(max(capacity, 1), dtype=np.uint32) if want_indices else None
    selected = [np.zeros((max(capacity, 1), int(descs[j].element_nbytes)), dtype=np.uint8)
                for j in range(num)]
    outputs = _pointer_array(a.ctypes.data for a in selected)
    count = ctypes.c_uint64(0)
    s = bzamd_row_selection(selector_descs[0], reject, 1 if invert else 0, descs if num else None,
                            outputs if num else None, num, capacity, 1 if zero_tail else 0)
    load().bzamd_select_rows(ctypes.byref(count), _ptr(indices), ctypes.byref(s))
    del keep_selector, keep
    rows = capacity if zero_tail else min(int(count.value), capacity)
    return (int(count.value), None if indices is None else indices[:rows],
            [a[:rows] for a in selected])


def select_rows_device(count_ptr, indices_ptr, selector, columns, selected_ptrs, capacity,
                       workspace_ptr, workspace_bytes, reject=0, invert=False, zero_tail=False,
                       stream=None):
    """bzamd_select_rows_device: enqueue only, two kernel launches.  selector: one
    (device_ptr, rows, nbytes, signed); columns: a list of such tuples; selected_ptrs: one output
    pointer per column; every pointer is memory of the current device as an integer (None: a null
    pointer); `stream` a hipStream_t as an integer (None: the default stream)."""
    selector_descs, _ = _device_descriptors([selector])
    descs, num = _device_descriptors(columns)
    outputs = _pointer_array(selected_ptrs)
    s = bzamd_row_selection(selector_descs[0], reject, 1 if invert else 0, descs if num else None,
                            outputs if num else None, num, capacity, 1 if zero_tail else 0)
    load().bzamd_select_rows_device(
        None if count_ptr is None else int(count_ptr),
        None if indices_ptr is None else int(indices_ptr), ctypes.byref(s),
        None if workspace_ptr is None else int(workspace_ptr), workspace_bytes,
        None if stream is None else ctypes.c_void_p(int(stream)))


def take_rows(indices, columns):
    """bzamd_take_rows (host operands, either backend).  indices: uint32 [num_rows]; columns: 1 ..
    16 columns as in combine_columns, of any lengths -> [uint8 [num_rows, nbytes] per column]:
    row r is row indices[r] of the column, zero bytes where that is past its end"""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    descs, keep = make_descriptors(_column_pairs(columns))
    num = len(keep)
    taken = [np.zeros((max(len(indices), 1), int(descs[j].element_nbytes)), dtype=np.uint8)
             for j in range(num)]
    outputs = _pointer_array(a.ctypes.data for a in taken)
    t = bzamd_row_take(indices.ctypes.data, len(indices), descs, outputs, num)
    load().bzamd_take_rows(ctypes.byref(t))
    del keep
    return [a[:len(indices)] for a in taken]


def take_rows_device(indices_ptr, num_rows, columns, taken_ptrs, stream=None):
    """bzamd_take_rows_device: enqueue only, one kernel launch.  columns: a list of
    (device_ptr, rows, nbytes, signed); taken_ptrs: one output pointer per column; every pointer
    is memory of the current device as an integer (None: a null pointer); `stream` a hipStream_t
    as an integer (None: the default stream)."""
    descs, num = _device_descriptors(columns)
    outputs = _pointer_array(taken_ptrs)
    t = bzamd_row_take(None if indices_ptr is None else int(indices_ptr), num_rows, descs, outputs,
                       num)
    load().bzamd_take_rows_device(ctypes.byref(t),
                                  None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_word_decomposition(ctypes.Structure):
    _fields_ = [("column", sxt_sequence_descriptor), ("shift", ctypes.c_void_p),
                ("num_words", ctypes.c_uint), ("plane_stride", ctypes.c_uint64)]


class bzamd_word_map(ctypes.Structure):
    _fields_ = [("words", ctypes.c_void_p), ("table", ctypes.c_void_p),
                ("num_planes", ctypes.c_uint), ("n", ctypes.c_uint64),
                ("plane_stride", ctypes.c_uint64), ("mapped_stride", ctypes.c_uint64)]


def decompose_words(field_id, column, num_words, shift=None, want_words=True):
    """bzamd_decompose_words (host operands, either backend).  column: as in combine_columns (an
    array or an (array, is_signed) pair); shift: uint8 [32] in element form (None: 0)
    -> (words uint8 [num_words, n], counts uint64 [256], overflow): words[k, i] is byte k of the
    key of shift + column[i]; want_words False: a null pointer, words is None"""
    descs, keep = make_descriptors(_column_pairs([column]))
    n = int(descs[0].n)
    if shift is not None:
        shift = np.ascontiguousarray(shift, dtype=np.uint8)
    words = np.zeros((num_words, max(n, 1)), dtype=np.uint8) if want_words else None
    counts = np.zeros(256, dtype=np.uint64)
    overflow = ctypes.c_uint64(0)
    d = bzamd_word_decomposition(descs[0], None if shift is None else shift.ctypes.data, num_words,
                                 max(n, 1))
    load().bzamd_decompose_words(_ptr(words), _ptr(counts), ctypes.byref(overflow), field_id,
                                 ctypes.byref(d))
    del keep
    return (None if words is None else words[:, :n]), counts, int(overflow.value)


def decompose_words_device(field_id, words_ptr, counts_ptr, overflow_ptr, column, num_words,
                           plane_stride, shift_ptr=None, stream=None):
    """bzamd_decompose_words_device: enqueue only, two kernel launches.  column: (device_ptr, rows,
    nbytes, signed); every *_ptr is memory of the current device as an integer (None: a null
    pointer); `stream` a hipStream_t as an integer (None: the default stream)."""
    ptr, rows, nbytes, signed = column
    d = bzamd_word_decomposition(
        sxt_sequence_descriptor(nbytes, rows, None if ptr is None else int(ptr), 1 if signed else 0),
        None if shift_ptr is None else int(shift_ptr), num_words, plane_stride)
    load().bzamd_decompose_words_device(
        None if words_ptr is None else int(words_ptr),
        None if counts_ptr is None else int(counts_ptr),
        None if overflow_ptr is None else int(overflow_ptr), field_id, ctypes.byref(d),
        None if stream is None else ctypes.c_void_p(int(stream)))


def map_words(words, table):
    """bzamd_map_words (host operands, either backend).  words: uint8 [num_planes, n]; table:
    uint8 [256, 32] -> uint8 [num_planes, n, 32]: mapped[k, i] = table[words[k, i]]"""
    words = np.ascontiguousarray(words, dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.uint8)
    num_planes, n = words.shape
    mapped = np.zeros((num_planes, n, 32), dtype=np.uint8)
    m = bzamd_word_map(words.ctypes.data, table.ctypes.data, num_planes, n, n, 32 * n)
    load().bzamd_map_words(_ptr(mapped), ctypes.byref(m))
    return mapped


def map_words_device(mapped_ptr, words_ptr, table_ptr, num_planes, n, plane_stride, mapped_stride,
                     stream=None):
    """bzamd_map_words_device: enqueue only, one kernel launch.  Every *_ptr is memory of the
    current device as an integer (None: a null pointer); `stream` a hipStream_t as an integer
    (None: the default stream)."""
    m = bzamd_word_map(None if words_ptr is None else int(words_ptr),
                       None if table_ptr is None else int(table_ptr), num_planes, n, plane_stride,
                       mapped_stride)
    load().bzamd_map_words_device(None if mapped_ptr is None else int(mapped_ptr), ctypes.byref(m),
                                  None if stream is None else ctypes.c_void_p(int(stream)))


class bzamd_column_evaluation(ctypes.Structure):
    _fields_ = [("columns", ctypes.POINTER(sxt_sequence_descriptor)),
                ("num_columns", ctypes.c_uint), ("n", ctypes.c_uint64)]


def evaluate_columns(field_id, columns, vector, n):
    """bzamd_evaluate_columns (host operands, either backend).  columns: as prove_sumcheck_columns;
    vector: uint8 [n, 32], what mle_evaluation_vector returns
    -> uint8 [num_columns, 32]: evaluations[j] = sum_i column_j[i] * vector[i]"""
    descs, keep = make_descriptors(_column_pairs(columns))
    vector = np.ascontiguousarray(vector, dtype=np.uint8)
    evaluations = np.zeros((max(len(keep), 1), 32), dtype=np.uint8)
    e = bzamd_column_evaluation(descs, len(keep), n)
    load().bzamd_evaluate_columns(_ptr(evaluations), field_id, _ptr(vector), ctypes.byref(e))
    return evaluations[:len(keep)]


def evaluate_columns_workspace_bytes(field_id, num_columns, n):
    """bzamd_evaluate_columns_workspace_bytes: needs no backend"""
    return load().bzamd_evaluate_columns_workspace_bytes(field_id, num_columns, n)


def evaluate_columns_device(field_id, descriptors, vector_ptr, n, evaluations_ptr, workspace_ptr,
                            workspace_bytes, stream=None):
    """bzamd_evaluate_columns_device: enqueue only.  descriptors: one (device_ptr, n_j, nbytes,
    signed) per column, or a ready sxt_sequence_descriptor array (the one the MSM took); every
    *_ptr is memory of the current device as an integer (None: a null pointer); `stream` a
    hipStream_t as an integer (None: the default stream)."""
    if isinstance(descriptors, ctypes.Array):
        descs, num_columns = descriptors, len(descriptors)
    else:
        descs, num_columns = _device_descriptors(descriptors)
    e = bzamd_column_evaluation(descs, num_columns, n)
    load().bzamd_evaluate_columns_device(
        None if evaluations_ptr is None else int(evaluations_ptr), field_id,
        None if vector_ptr is None else int(vector_ptr), ctypes.byref(e),
        None if workspace_ptr is None else int(workspace_ptr), workspace_bytes,
        None if stream is None else ctypes.c_void_p(int(stream)))


def folded_layout(n, num_variables):
    """[(offset, length)] in rows of P_1 .. P_{num_variables - 1} inside `folded`: len_0 = n,
    len_i = ceil(len_{i-1} / 2), off_1 = 0, off_{i+1} = off_i + len_i"""
    out, offset, length = [], 0, int(n)
    for _ in range(1, num_variables):
        length = (length + 1) // 2
        out.append((offset, length))
        offset += length
    return out


def _folded_rows(n, num_variables):
    return sum(length for _, length in folded_layout(n, num_variables))


def _device_ptr(p):
    return None if p is None else int(p)


def _stream(stream):
    return None if stream is None else ctypes.c_void_p(int(stream))


def fold_polynomial(field_id, polynomial, point, n=None, num_variables=None, scalars=True,
                    evaluation=True):
    """bzamd_fold_polynomial (host operands, either backend).  polynomial: uint8 [n, 32]; point:
    uint8 [num_variables, 32]; scalars, evaluation: True for a fresh buffer, a uint8 buffer the
    call may write, or None for a null pointer
    -> (folded uint8 [rows, 32], scalars uint8 [rows, 32] or None, evaluation uint8 [32] or None)
    with rows = sum of folded_layout's lengths"""
    polynomial = np.ascontiguousarray(polynomial, dtype=np.uint8)
    point = np.ascontiguousarray(point, dtype=np.uint8)
    n = polynomial.size // 32 if n is None else n
    num_variables = point.size // 32 if num_variables is None else num_variables
    rows = _folded_rows(n, num_variables) if 1 <= num_variables <= 30 and n >= 1 else 0
    folded = np.zeros((max(rows, 1), 32), dtype=np.uint8)
    if scalars is True:
        scalars = np.zeros((max(rows, 1), 32), dtype=np.uint8)
    if evaluation is True:
        evaluation = np.zeros(32, dtype=np.uint8)
    load().bzamd_fold_polynomial(_ptr(folded), _ptr(scalars), _ptr(evaluation), field_id,
                                 _ptr(polynomial), n, _ptr(point), num_variables)
    return folded[:rows], None if scalars is None else scalars[:rows], evaluation


def fold_polynomial_device(field_id, folded_ptr, scalars_ptr, evaluation_ptr, polynomial_ptr, n,
                           point_ptr, num_variables, stream=None):
    """bzamd_fold_polynomial_device: enqueue only.  Every *_ptr is memory of the current device as
    an integer (None: a null pointer); `stream` a hipStream_t as an integer (None: the default
    stream)."""
    load().bzamd_fold_polynomial_device(
        _device_ptr(folded_ptr), _device_ptr(scalars_ptr), _device_ptr(evaluation_ptr), field_id,
        _device_ptr(polynomial_ptr), n, _device_ptr(point_ptr), num_variables, _stream(stream))


def evaluate_polynomials(field_id, polynomial, folded, points, num_variables, n=None):
    """bzamd_evaluate_polynomials (host operands, either backend).  polynomial: uint8 [n, 32];
    folded: what fold_polynomial returns; points: uint8 [num_points, 32]
    -> uint8 [num_points, num_variables, 32]: P_i(u_k) at [k, i]"""
    polynomial = np.ascontiguousarray(polynomial, dtype=np.uint8)
    folded = np.ascontiguousarray(folded, dtype=np.uint8)
    points = np.ascontiguousarray(points, dtype=np.uint8)
    n = polynomial.size // 32 if n is None else n
    num_points = points.size // 32
    evaluations = np.zeros((max(num_points, 1), max(num_variables, 1), 32), dtype=np.uint8)
    load().bzamd_evaluate_polynomials(_ptr(evaluations), field_id, _ptr(polynomial),
                                      _ptr(folded) if folded.size else None, n, num_variables,
                                      _ptr(points), num_points)
    return evaluations[:num_points, :num_variables]


def evaluate_polynomials_workspace_bytes(field_id, n, num_variables, num_points):
    """bzamd_evaluate_polynomials_workspace_bytes: needs no backend"""
    return load().bzamd_evaluate_polynomials_workspace_bytes(field_id, n, num_variables, num_points)


def evaluate_polynomials_device(field_id, evaluations_ptr, polynomial_ptr, folded_ptr, n,
                                num_variables, points_ptr, num_points, workspace_ptr,
                                workspace_bytes, stream=None):
    """bzamd_evaluate_polynomials_device: enqueue only; pointers and stream as
    fold_polynomial_device"""
    load().bzamd_evaluate_polynomials_device(
        _device_ptr(evaluations_ptr), field_id, _device_ptr(polynomial_ptr),
        _device_ptr(folded_ptr), n, num_variables, _device_ptr(points_ptr), num_points,
        _device_ptr(workspace_ptr), workspace_bytes, _stream(stream))


def batch_quotients(field_id, polynomial, folded, q, points, num_variables, n=None,
                    remainders=True):
    """bzamd_batch_quotients (host operands, either backend).  q: uint8 [32]; remainders: True for
    a fresh buffer, a uint8 buffer the call may write, or None for a null pointer
    -> (quotients uint8 [num_points, n, 32] in scalar form, remainders uint8 [num_points, 32] or
    None)"""
    polynomial = np.ascontiguousarray(polynomial, dtype=np.uint8)
    folded = np.ascontiguousarray(folded, dtype=np.uint8)
    points = np.ascontiguousarray(points, dtype=np.uint8)
    q = np.ascontiguousarray(q, dtype=np.uint8)
    n = polynomial.size // 32 if n is None else n
    num_points = points.size // 32
    quotients = np.zeros((max(num_points, 1), max(int(n), 1), 32), dtype=np.uint8)
    if remainders is True:
        remainders = np.zeros((max(num_points, 1), 32), dtype=np.uint8)
    load().bzamd_batch_quotients(_ptr(quotients), _ptr(remainders), field_id, _ptr(polynomial),
                                 _ptr(folded) if folded.size else None, n, num_variables, _ptr(q),
                                 _ptr(points), num_points)
    return quotients[:num_points, :n], remainders


def batch_quotients_workspace_bytes(field_id, n, num_variables, num_points):
    """bzamd_batch_quotients_workspace_bytes: needs no backend"""
    return load().bzamd_batch_quotients_workspace_bytes(field_id, n, num_variables, num_points)


def batch_quotients_device(field_id, quotients_ptr, remainders_ptr, polynomial_ptr, folded_ptr, n,
                           num_variables, q_ptr, points_ptr, num_points, workspace_ptr,
                           workspace_bytes, stream=None):
    """bzamd_batch_quotients_device: enqueue only; pointers and stream as fold_polynomial_device"""
    load().bzamd_batch_quotients_device(
        _device_ptr(quotients_ptr), _device_ptr(remainders_ptr), field_id,
        _device_ptr(polynomial_ptr), _device_ptr(folded_ptr), n, num_variables,
        _device_ptr(q_ptr), _device_ptr(points_ptr), num_points, _device_ptr(workspace_ptr),
        workspace_bytes, _stream(stream))


class MultiexpHandle:
    """sxt_multiexp_handle wrapper (fixed generators)."""

    def __init__(self, curve_id, generators_projective=None, filename=None):
        lib = load()
        self.curve_id = curve_id
        if filename is not None:
            self._h = lib.sxt_multiexp_handle_new_from_file(curve_id, filename.encode())
        else:
            g = np.ascontiguousarray(generators_projective)
            psize = CURVE_LAYOUT[curve_id][2]
            assert g.nbytes % psize == 0
            self._h = lib.sxt_multiexp_handle_new(curve_id, _ptr(g), g.nbytes // psize)

    def write_to_file(self, filename):
        load().sxt_multiexp_handle_write_to_file(self._h, filename.encode())

    def _out(self, num_outputs):
        return np.zeros((num_outputs, CURVE_LAYOUT[self.curve_id][2]), dtype=np.uint8)

    def multiexponentiation(self, element_num_bytes, num_outputs, n, scalars):
        s = np.ascontiguousarray(scalars, dtype=np.uint8)
        out = self._out(num_outputs)
        load().sxt_fixed_multiexponentiation(_ptr(out), self._h, element_num_bytes, num_outputs, n,
                                             _ptr(s))
        return out

    def packed_multiexponentiation(self, bit_table, n, scalars):
        bt = np.ascontiguousarray(bit_table, dtype=np.uint32)
        s = np.ascontiguousarray(scalars, dtype=np.uint8)
        out = self._out(len(bt))
        load().sxt_fixed_packed_multiexponentiation(_ptr(out), self._h, _ptr(bt), len(bt), n,
                                                    _ptr(s))
        return out

    def vlen_multiexponentiation(self, bit_table, lengths, scalars):
        bt = np.ascontiguousarray(bit_table, dtype=np.uint32)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        s = np.ascontiguousarray(scalars, dtype=np.uint8)
        out = self._out(len(bt))
        load().sxt_fixed_vlen_multiexponentiation(_ptr(out), self._h, _ptr(bt), _ptr(ln), len(bt),
                                                  _ptr(s))
        return out

    def close(self):
        if self._h:
            load().sxt_multiexp_handle_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
