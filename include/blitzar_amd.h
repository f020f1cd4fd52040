/* MI355X-native extensions next to the drop-in Blitzar ABI (include/blitzar_api.h).
 *
 * The reference API only accepts host buffers and re-uploads scalars and generators on every
 * call (sxt/multiexp/bucket_method/accumulation.h:68-71, bucket_method2/sum.h:103-107).  These
 * entry points are what SURVEY.md section 8(f) row 1 asks for: the same computation on operands that are
 * already resident in HBM, enqueued on a caller stream.  They are also what `bench.py` times
 * ("inputs already resident in HBM when the timed region starts").
 *
 * All pointers marked DEVICE must be valid on the current HIP device.  `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  Calls are asynchronous unless stated otherwise.
 *
 * Concurrency: the engine keeps one workspace per device.  Calls on one device are executed in the
 * order they were enqueued, whatever streams they arrive on (a call on another stream first waits
 * for everything enqueued so far on the stream of the previous call; do not destroy a stream the
 * engine may still have to wait for), and the host side of every call takes the device context's
 * lock, so several host threads may enqueue.  What can overlap is the tail of one call with the
 * next call (bzamd_pipeline_next below).  The blocking sxt_* entry points serialise on one
 * process-wide lock.
 */
#ifndef BLITZAR_AMD_BLITZAR_AMD_H
#define BLITZAR_AMD_BLITZAR_AMD_H

#include <stdint.h>

#include "blitzar_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* library / device introspection */
const char* bzamd_version(void);
int bzamd_device_count(void);
/* 0 = not initialised, SXT_CPU_BACKEND, SXT_GPU_BACKEND */
int bzamd_active_backend(void);
/* HIP devices the GPU backend drives from this process (0 before sxt_init / on the cpu backend).
 * sxt_init takes every visible device (the current one first), capped by the environment variable
 * BLITZAR_AMD_NUM_DEVICES; a blocking sxt_* call shards its columns / outputs (or the rows of a
 * single long column) over them, one host thread per device.  BLITZAR_AMD_FORCE_SHARDS=k makes k
 * logical devices out of the current physical one (testing the sharded paths on a one-GPU box). */
int bzamd_num_devices(void);
/* calls with fewer scalar bytes than this stay on one device (default 1 MiB) */
void bzamd_set_shard_min_bytes(uint64_t bytes);
/* A blocking call with host operands that stays on one device is cut into row chunks when that pays:
 * chunk k is committed to projective partials while chunk k + 1 crosses PCIe, one fold adds the
 * partials up (exact group addition: the same commitments).  0 = the cost model decides (default);
 * k = k chunks wherever the longest sequence has that many rows (tests). */
void bzamd_set_row_pipeline_chunks(uint32_t chunks);
/* rows of a sequence one pass of the engine takes (default 2^28, at most 2^31 - 1: the engine
 * indexes the rows of a pass with 31 bits).  A longer sequence -- the ABI's n is a uint64_t -- runs
 * in ceil(n / rows) passes over row ranges whose projective partial results are folded; the
 * canonical result is the same.  Tests lower it. */
void bzamd_set_max_rows_per_pass(uint64_t rows);
/* A fresh Merlin transcript with the application's domain-separation label: the 203 bytes a
 * caller hands to sxt_curve25519_prove_inner_product / _verify_inner_product (the reference leaves
 * their construction to the caller's Merlin implementation; Rust callers transmute
 * merlin::Transcript, prft::transcript{label} in C++). */
void bzamd_transcript_init(struct sxt_transcript* transcript, const char* label,
                           uint64_t label_len);
/* addition formula k_accumulate runs for curve25519 caller generators: 1 = Z = 1 addends (7 field
 * products, generators normalised per call by a batched inversion), 0 = projective (8 products) */
int bzamd_accumulate_form(void);
/* number of gfx950 kernel launches issued by this process so far (tests use it to prove that the
 * HIP path, not a host path, produced a result) */
uint64_t bzamd_kernel_launch_count(void);
/* the most blocking sxt_* calls that ever held devices of the GPU backend at the same time (calls
 * take per-device leases, not a process-wide lock: two host threads on a two-device backend run
 * side by side; tests use this to prove it) */
uint32_t bzamd_concurrent_calls_high_water(void);
/* 1 if the current device fetches code beyond its instruction cache more slowly than it executes it
 * (probed once per device; such devices run the bucket reduction of calls with few columns through
 * k_reduce_compact), 0 if not, -1 without an initialised GPU backend */
int bzamd_slow_instruction_fetch(void);
/* Issue rate of v_mad_u64_u32 -- the field products' one wide primitive, the binding bound of the
 * bucket accumulation -- on the current device, measured now: every SIMD holds 6 waves of 8
 * independent chains for about `target_ms` milliseconds, the fastest ~3 ms launch of the second half
 * of that load is what is reported.
 *   out[0] wave-instructions per second over the whole device
 *   out[1] effective shader clock in Hz (s_memtime ticks of the longest wave / wall time)
 *   out[2] shader cycles per wave-instruction and SIMD
 *   out[3] milliseconds of load the probe ran
 * Returns 0, or -1 without the GPU backend.  bench.py normalises `roofline.alu` with it. */
int bzamd_probe_mad_rate(double target_ms, double* out);
/* BLITZAR_AMD_GENERATOR_CACHE=1 (read by sxt_init; off by default): the blocking
 * sxt_*_compute_pedersen_commitments_with_generators entry points keep a caller's host generators on
 * the device across calls.  Key = (host pointer, count, curve) + a hash of a 1-in-256 sample of the
 * rows; the second call with the same key registers the set (one extra upload), later calls whose key
 * and sample still match upload scalars only (the reference re-uploads on every call:
 * sxt/multiexp/bucket_method/accumulation.h:68-71).  CAVEAT: rewriting rows the sample misses, in
 * place, is not noticed -- hence opt-in.  Counters: calls served from the cache / sets registered. */
void bzamd_generator_cache_stats(uint64_t* hits, uint64_t* builds);

/* drop the backend singleton so that sxt_init may be called again (reference:
 * cbn::reset_backend_for_testing, cbindings/backend.cc:111) */
void bzamd_reset_for_testing(void);

/* Engine knobs of the current device's MSM context (GPU backend; 0 keeps the current value):
 * cap on the window width c (2..16), and the batching limits for many-column jobs (tasks = column
 * windows per launch, device workspace bytes per batch).  Results never depend on them. */
void bzamd_set_tuning(uint32_t max_window_bits, uint64_t max_tasks_per_batch,
                      uint64_t max_workspace_bytes);
/* Every column takes window width `window_bits` (2..16) wherever its bit width allows, instead of
 * the width the cost model would choose from its length (0 restores the model).  For tests: the
 * c = 16 code paths at sizes a CPU reference finishes in seconds. */
void bzamd_set_window_bits(uint32_t window_bits);
/* Per-call window tables: a call of many columns over the same caller generators (the reference's
 * bucket_method2 regime, sxt/multiexp/bucket_method2/multiexponentiation.h:48-121) builds the
 * 2^(c w) multiples of its generators once, inside the call, and runs every column as ONE task with
 * one bucket set.  mode 0 = the cost model decides (default), 1 = never, 6..16 = a table of that
 * window width for every call with caller generators (tests, A/B runs), negative = change nothing.
 * Returns the number of tables built so far on the backend's contexts.  Results never depend on it.
 * Env: BLITZAR_AMD_CALL_TABLES=0, BLITZAR_AMD_CALL_TABLE_BITS=c, BLITZAR_AMD_CALL_TABLE_OVERLAP=0. */
uint64_t bzamd_set_call_tables(int mode);
/* Caller tables: bzamd_msm_device* over caller generators keeps the converted generators of the
 * two generator pointers used last on a device, and a later call at the same pointer converts only
 * the tiles of 64 generators whose bytes changed (every byte is read and compared by digest on
 * every call).  Env: BLITZAR_AMD_CALLER_TABLE=0 converts everything on every call.
 * bzamd_prepare_tiles_converted: tiles converted into the tables so far on the backend's contexts
 * (synchronises their devices).  bzamd_caller_table_reset: free the tables.  For tests and tools;
 * results never depend on either. */
uint64_t bzamd_prepare_tiles_converted(void);
void bzamd_caller_table_reset(void);
/* Work per lane of the two bucket kernels, as log2 (0, the default, lets every launch choose from
 * its size): sorted entries per accumulation lane (2^3..2^10; 32 for a single column so that its
 * lanes fill the machine, up to 128 when hundreds of columns do -- every segment leaves one partial
 * sum to fold) and buckets per bucket-reduction lane (2^1..2^8; 8 for a single column: shortest
 * dependent chain, up to 64 for many: least total work).  Results never depend on them. */
void bzamd_set_segments(uint32_t log2_entries_per_accumulate_lane,
                        uint32_t log2_buckets_per_reduce_lane);

/* Per-stage device timing of the next `max_calls` MSM calls issued on the current device, measured
 * with HIP events on the launch stream.  `bzamd_stage_timing_collect` blocks until those calls
 * finished, writes the accumulated milliseconds of the six stages
 * {prepare_addends, recode, bucket_sort, accumulate, reduce, combine} to out_ms[6] and returns the
 * number of calls recorded.  Every recorded stage puts an event pair on the stream, i.e. two bubbles
 * of a few microseconds per call: `_masked` records only the stages whose bit is set in
 * `stage_mask` (bit 3 = accumulate), the others read 0. */
void bzamd_stage_timing_begin(uint64_t max_calls);
void bzamd_stage_timing_begin_masked(uint64_t max_calls, uint32_t stage_mask);
/* ... recording one MSM in `sample_every` only (an event pair costs the stream two bubbles per
 * recorded stage: a sample keeps a timed region honest); `max_calls` and the count
 * bzamd_stage_timing_collect returns are then of RECORDED calls */
void bzamd_stage_timing_begin_sampled(uint64_t max_calls, uint32_t stage_mask, uint32_t sample_every);
uint64_t bzamd_stage_timing_collect(double* out_ms);

/* Throughput mode for a sequence of device-resident MSM calls.  A call with few columns is four
 * stages with complementary bottlenecks: a front of short HBM-bound kernels (generator conversion,
 * recoding, bucket sort), the integer-issue-bound bucket accumulation, and two latency chains that
 * leave the machine nearly idle -- the bucket reduction at one wavefront per SIMD and the final
 * stage at ONE workgroup per column (~250 dependent doublings, the encoding's 250 squarings).
 * bzamd_pipeline_next() makes the NEXT MSM enqueued through a device entry point of this header
 * (bzamd_msm_device*, bzamd_fixed_packed_multiexponentiation_device) on the current device run its
 * two tail stages on internal streams of the engine, beside the front and the accumulation of call
 * k + 1, which stay on the caller's `stream` (the calls must have the same shape to overlap: the
 * engine otherwise simply waits).  The operands are consumed in stream order, as without the mode.
 * The commitments of such a call are complete on `stream` only once TWO later
 * such calls on the device have been enqueued on it, or after bzamd_pipeline_flush(stream): do not
 * read them earlier.  Calls with 64 or more columns ignore the request (their tails fill the
 * machine).  A pipelined sequence lives on ONE stream and one caller thread per device (the NULL
 * stream or a stream of the caller's own: the engine's internal streams are non-blocking streams
 * of the lowest priority, they synchronise with nobody implicitly).
 * (Measured on MI355X, 2^20 curve25519 rows: see DESIGN.md section 9.) */
void bzamd_pipeline_next(void);
void bzamd_pipeline_flush(void* stream);

/* Variable-base MSM on device-resident operands.
 *   commitments  DEVICE  num_sequences canonical encodings (32 / 48 / 72 / 72 bytes each)
 *   descriptors  HOST    array whose `data` members are DEVICE pointers
 *   generators   DEVICE  C-ABI layout of the curve (sxt_ristretto255[160] / bls 104-byte stride /
 *                        sxt_bn254_g1[72] / sxt_grumpkin[72]), max_i n_i entries
 * Same validation/abort behaviour as the sxt_*_compute_pedersen_commitments_with_generators calls. */
void bzamd_msm_device(unsigned curve_id, void* commitments, uint32_t num_sequences,
                      const struct sxt_sequence_descriptor* descriptors, const void* generators,
                      void* stream);

/* Multi-device MSM inside ONE process on device-resident operands (the
 * reference's gpu backend drives every visible device from one process too,
 * sxt/execution/device/for_each.cc:56-82, but bounces partial results through pinned host memory).
 * The backend drives D = bzamd_num_devices() devices; device slot d is HIP device bzamd_device_id(d)
 * (slot 0 = the device that was current at sxt_init).  The columns are cut into contiguous ranges
 * of per = bzamd_multi_device_columns_per_device(num_sequences) = ceil(num_sequences / D) columns:
 * column i belongs to slot i / per, and descriptors[i].data is a DEVICE pointer on THAT device;
 * generators[d] = the generator set (C-ABI layout) as a DEVICE pointer on slot d (may be NULL for a
 * slot that owns no column).  Every device commits its columns; ONE all-gather of the encodings --
 * ncclAllGather on the communicators the library creates with ncclCommInitAll on first use, RCCL
 * over the xGMI links; librccl is loaded on that first use only -- leaves ALL num_sequences
 * commitments on EVERY device, copied to commitments[d] (DEVICE pointer on slot d, NULL = not
 * wanted there).  Blocking.  Logical devices that share a physical one
 * (BLITZAR_AMD_FORCE_SHARDS; RCCL refuses duplicate devices within a communicator) exchange with
 * peer copies instead: bzamd_multi_device_exchange() says which ("rccl" / "peer-copies"). */
int bzamd_device_id(int slot);
uint32_t bzamd_multi_device_columns_per_device(uint32_t num_sequences);
const char* bzamd_multi_device_exchange(void);
void bzamd_msm_multi_device(unsigned curve_id, void* const* commitments, uint32_t num_sequences,
                            const struct sxt_sequence_descriptor* descriptors,
                            const void* const* generators);

/* Row-sharded MSM support (one column split by rows across GPUs):
 * the partial result of a shard as a raw projective element (sxt_ristretto255 160 B /
 * sxt_bls12_381_g1_p2 144 B / sxt_bn254_g1_p2, sxt_grumpkin_p2 96 B per column), and the fold
 *   commitments[k] = canonical encoding of  sum_r partials[r * num_outputs + k]
 * that every rank applies after the all-gather of the partials (RCCL has no user-defined
 * reduction; group addition is exact, so the canonical result equals the unsharded one). */
void bzamd_msm_device_projective(unsigned curve_id, void* res, uint32_t num_sequences,
                                 const struct sxt_sequence_descriptor* descriptors,
                                 const void* generators, void* stream);
/* HOST operands, either backend (blocking) */
void bzamd_msm_projective(unsigned curve_id, void* res, uint32_t num_sequences,
                          const struct sxt_sequence_descriptor* descriptors,
                          const void* generators);
/* HOST operands (no backend needed: G - 1 point additions and one encoding per output) */
void bzamd_fold_encode(unsigned curve_id, void* commitments, const void* partials,
                       uint32_t num_partials, uint32_t num_outputs);
/* DEVICE operands (async) */
void bzamd_fold_encode_device(unsigned curve_id, void* commitments, const void* partials,
                              uint32_t num_partials, uint32_t num_outputs, void* stream);

/* Resident generator set: generators converted once into the engine's addend layout and kept in
 * HBM across calls. */
struct bzamd_generators;
/* from DEVICE generators in C-ABI layout (blocking) */
struct bzamd_generators* bzamd_generators_new_device(unsigned curve_id, const void* generators,
                                                     uint64_t n, void* stream);
/* from HOST generators in C-ABI layout (blocking) */
struct bzamd_generators* bzamd_generators_new_host(unsigned curve_id, const void* generators,
                                                   uint64_t n);
void bzamd_generators_free(struct bzamd_generators* gens);
void bzamd_msm_device_resident(void* commitments, uint32_t num_sequences,
                               const struct sxt_sequence_descriptor* descriptors,
                               const struct bzamd_generators* gens, void* stream);

/* Per-column generator offsets: independent MSMs over different windows of ONE generator sequence
 * G in one call,
 *   commitments[i] = sum_j scalar_ij * G[generator_offsets[i] + j]
 * (appending rows to tables of different lengths; batched MSMs with non-shared bases laid out back
 * to back).  generator_offsets == NULL means every offset is 0: the bytes of the corresponding call
 * without offsets.  A column with generator_offsets[i] + n_i > num_generators aborts, like a bad
 * descriptor.  Only the generators in [min offset_i, max offset_i + n_i) are uploaded or converted.
 * Descriptors, encodings and generator layouts as in the calls without offsets. */
/* HOST operands, blocking, cpu and gpu backends (as sxt_*_compute_pedersen_commitments_with_generators) */
void bzamd_compute_commitments_with_generator_offsets(unsigned curve_id, void* commitments,
                                                      uint32_t num_sequences,
                                                      const struct sxt_sequence_descriptor* descriptors,
                                                      const void* generators, uint64_t num_generators,
                                                      const uint64_t* generator_offsets);
/* built-in ristretto generators (as sxt_curve25519_compute_pedersen_commitments; the sequence has
 * no end) */
void bzamd_curve25519_compute_commitments_with_offsets(struct sxt_ristretto255_compressed* commitments,
                                                       uint32_t num_sequences,
                                                       const struct sxt_sequence_descriptor* descriptors,
                                                       const uint64_t* generator_offsets);
/* DEVICE operands (as bzamd_msm_device), generator_offsets on the HOST, async */
void bzamd_msm_device_offsets(unsigned curve_id, void* commitments, uint32_t num_sequences,
                              const struct sxt_sequence_descriptor* descriptors,
                              const void* generators, uint64_t num_generators,
                              const uint64_t* generator_offsets, void* stream);
/* resident set (as bzamd_msm_device_resident; num_generators = the set's), async */
void bzamd_msm_device_resident_offsets(void* commitments, uint32_t num_sequences,
                                       const struct sxt_sequence_descriptor* descriptors,
                                       const struct bzamd_generators* gens,
                                       const uint64_t* generator_offsets, void* stream);

/* DEVICE built-in ristretto generators g_first .. g_first+n-1 as sxt_ristretto255 (async) */
void bzamd_ristretto255_generators_device(struct sxt_ristretto255* generators, uint64_t first,
                                          uint64_t n, void* stream);

/* DEVICE generators[i] = (i + 1) * base in the curve's C-ABI generator layout, base = one DEVICE
 * generator in the same layout (async).  Synthetic generator sets with known discrete logarithms
 * for benchmarks and full-size parity checks. */
void bzamd_generator_multiples_device(unsigned curve_id, void* generators, const void* base,
                                      uint64_t n, void* stream);

/* Fixed-base (handle) MSM with DEVICE scalars and DEVICE results; same packing rules as
 * sxt_fixed_packed_multiexponentiation / sxt_fixed_vlen_multiexponentiation
 * (output_lengths may be NULL = all rows). */
void bzamd_fixed_packed_multiexponentiation_device(void* res, const struct sxt_multiexp_handle* handle,
                                                   const unsigned* output_bit_table,
                                                   const unsigned* output_lengths,
                                                   unsigned num_outputs, unsigned n,
                                                   const uint8_t* scalars, void* stream);

/* Sumcheck prover (sxt_prove_sumcheck) that also returns what the caller sends the verifier next,
 * and its form on device-resident tables.  `polynomials`, `evaluation_point`, the descriptor and
 * the transcript callback are those of sxt_prove_sumcheck, and with the same inputs the same bytes
 * are written to them; limits and aborts are the same (round_degree <= 8, n <= 2^30).
 * `mle_evaluations` (may be NULL): num_mles field elements in the caller's representation,
 * canonical: mle_evaluations[j] = f_j(r_1 .. r_v), the value of MLE j at the evaluation point.
 * With v = max(ceil_log2(n), 1), T_0 = the tables padded with zero rows to 2^v, mid_t = 2^(v-1-t) and
 *   T_{t+1}[j][i] = (1 - r_t) T_t[j][i] + r_t T_t[j][mid_t + i],
 * it is T_v[j][0]: the fold the prover does between rounds, applied once more with the last
 * challenge (n = 1: (1 - r_0) f_j[0]). */
/* HOST operands, blocking, cpu and gpu backends */
void bzamd_prove_sumcheck(void* polynomials, void* evaluation_point, void* mle_evaluations,
                          unsigned field_id, const struct sumcheck_descriptor* descriptor,
                          void* transcript_callback, void* transcript_context);
/* descriptor->mles is a DEVICE pointer on the current HIP device; everything else is HOST.  gpu
 * backend only.  Blocking (the transcript callback runs on the host every round).  The tables are
 * read in stream order after the work already enqueued on `stream` and are not modified; when the
 * call returns, all reads of them are complete.  The kernels run on `stream`, the working tables
 * live in device memory of the call's own, and no device of the backend is held: the callback may
 * call back into the library. */
void bzamd_prove_sumcheck_device(void* polynomials, void* evaluation_point, void* mle_evaluations,
                                 unsigned field_id, const struct sumcheck_descriptor* descriptor,
                                 void* transcript_callback, void* transcript_context, void* stream);

/* Sumcheck over typed columns: the MLEs are described by the descriptors the MSM entry points
 * take, so a service proves over the columns it has just committed, as they are.  MLE j has
 * mles[j].n <= n rows (longer aborts); rows mles[j].n .. n - 1 are zero (n = 0 with data = NULL is
 * a zero column).  element_nbytes 1 .. 31: little-endian integers, two's complement when
 * is_signed (a negative v is the field's p - |v|); for SXT_FIELD_GRUMPKIN the library converts the
 * integer into Montgomery form.  element_nbytes 32: field elements in the representation
 * sxt_prove_sumcheck takes for the field.  Descriptors are validated by the MSM's rule
 * (element_nbytes in [1, 32], signed only up to 16 bytes).  Everything else -- outputs, product
 * table, limits, callback -- is as in bzamd_prove_sumcheck, and the outputs are the bytes
 * sxt_prove_sumcheck writes for the columns widened to 32 bytes and padded with zero rows to n. */
struct bzamd_sumcheck_columns {
  const struct sxt_sequence_descriptor* mles; /* num_mles descriptors, one per MLE */
  const void* product_table;                  /* as sumcheck_descriptor */
  const unsigned* product_terms;
  unsigned n, num_mles, num_products, num_product_terms, round_degree;
};
/* mles[j].data on the HOST; blocking, cpu and gpu backends.  The gpu backend uploads the columns
 * at their own width. */
void bzamd_prove_sumcheck_columns(void* polynomials, void* evaluation_point, void* mle_evaluations,
                                  unsigned field_id, const struct bzamd_sumcheck_columns* columns,
                                  void* transcript_callback, void* transcript_context);
/* mles[j].data are DEVICE pointers on the current HIP device; everything else, the descriptors
 * included, is HOST.  The rules of bzamd_prove_sumcheck_device hold: gpu backend only, kernels on
 * `stream`, the columns read in stream order and never written, no device of the backend held
 * (the callback may call back into the library), mle_evaluations may be NULL.  Round 0 and the
 * first fold read the columns where they lie; the call's device memory holds the folded tables
 * only (27 bytes per padded row and MLE). */
void bzamd_prove_sumcheck_device_columns(void* polynomials, void* evaluation_point,
                                         void* mle_evaluations, unsigned field_id,
                                         const struct bzamd_sumcheck_columns* columns,
                                         void* transcript_callback, void* transcript_context,
                                         void* stream);
/* Device memory the latest sumcheck call of the process on the gpu backend allocated, in bytes:
 * working tables, staged operands and round buffers (0 before the first one). */
uint64_t bzamd_sumcheck_device_bytes(void);


/* Sumcheck with the library's own transcript: the reference's prfsk::reference_transcript over the
 * caller's 203-byte Merlin state, used in place; its state after a call is part of the contract.
 *   init, for v = max(ceil_log2(n), 1) variables and round degree D:
 *     append_message("domain-sep", "sumcheck proof v1"), append_message("n", u64 LE v),
 *     append_message("k", u64 LE D)
 *   every round: append_message("P", the (D + 1) 32 bytes of the round polynomial as written to
 *     `polynomials`), x = challenge_bytes("R", 32), and the challenge from x by field:
 *     SXT_FIELD_SCALAR255: the little-endian integer x mod l; SXT_FIELD_GRUMPKIN: the bytes the
 *     reference makes of x (the canonical integer x / 2^256 mod p), taken as the element.
 *
 * The transcript as a callback for sxt_prove_sumcheck / bzamd_prove_sumcheck*: call
 * bzamd_sumcheck_transcript_begin once, then pass bzamd_sumcheck_transcript_round as
 * transcript_callback and a bzamd_sumcheck_transcript_context as transcript_context. */
struct bzamd_sumcheck_transcript_context {
  struct sxt_transcript* transcript;
  unsigned field_id;
};
void bzamd_sumcheck_transcript_begin(struct sxt_transcript* transcript, uint64_t num_variables,
                                     uint64_t round_degree);
void bzamd_sumcheck_transcript_round(void* r, void* context, const void* polynomial, unsigned length);

/* bzamd_prove_sumcheck with that transcript built in (init included).  HOST operands, blocking,
 * cpu and gpu backends; outputs as bzamd_prove_sumcheck.  The gpu backend runs the device form
 * below on uploaded operands and synchronises once, at the end. */
void bzamd_prove_sumcheck_transcript(void* polynomials, void* evaluation_point, void* mle_evaluations,
                                     struct sxt_transcript* transcript, unsigned field_id,
                                     const struct sumcheck_descriptor* descriptor);

/* The prover that never returns to the host between rounds.  DEVICE pointers on the current HIP
 * device: descriptor->mles (read only), polynomials, evaluation_point, mle_evaluations (may be
 * NULL), transcript (203 bytes, in / out) and workspace (bzamd_sumcheck_transcript_workspace_bytes
 * of the same field and descriptor, at least; less aborts).  HOST: the descriptor, the product
 * table and the terms, which are read before the call returns.  gpu backend only.  The call only
 * enqueues on `stream`: no synchronise, no allocation, no callback; outputs, transcript and
 * workspace are the caller's to reuse once the work enqueued by the call has completed.  Limits
 * and aborts are those of bzamd_prove_sumcheck_device. */
uint64_t bzamd_sumcheck_transcript_workspace_bytes(unsigned field_id,
                                                   const struct sumcheck_descriptor* descriptor);
void bzamd_prove_sumcheck_transcript_device(void* polynomials, void* evaluation_point,
                                            void* mle_evaluations, void* transcript,
                                            unsigned field_id,
                                            const struct sumcheck_descriptor* descriptor,
                                            void* workspace, uint64_t workspace_bytes, void* stream);

/* Both over typed columns: commit the columns with bzamd_msm_device, then prove over the same
 * descriptors on the same stream, with no host round trip and no widened copy.  The three entry
 * points write the bytes, and leave the transcript state, that bzamd_prove_sumcheck_transcript /
 * _transcript_device produce for the columns widened to 32-byte elements and padded with zero rows
 * to n.  Descriptors, limits and aborts are those of bzamd_prove_sumcheck_columns; a null
 * transcript aborts. */
/* HOST operands (mles[j].data included), blocking, cpu and gpu backends.  The gpu backend uploads
 * the columns at their own width, runs the device form below and synchronises once, at the end. */
void bzamd_prove_sumcheck_transcript_columns(void* polynomials, void* evaluation_point,
                                             void* mle_evaluations,
                                             struct sxt_transcript* transcript, unsigned field_id,
                                             const struct bzamd_sumcheck_columns* columns);
/* DEVICE pointers on the current HIP device: mles[j].data (any address; read in stream order,
 * never written), polynomials, evaluation_point, mle_evaluations (may be NULL), transcript (203
 * bytes, in / out) and workspace (bzamd_sumcheck_transcript_columns_workspace_bytes of the same
 * field and counts, at least; less aborts; any alignment).  HOST: the struct, the descriptors, the
 * product table and the terms, which are read before the call returns.  gpu backend only.  The
 * call only enqueues on `stream`: no synchronise, no allocation, no callback.  Round 0 and the
 * first fold read the columns where they lie: the workspace holds the folded half and quarter (27
 * bytes per padded row and MLE, against 54 of the 32-byte form), or for n <= 512 at round degree
 * <= 5 the n-row table.  The workspace size needs no backend and depends on field_id, n, num_mles,
 * num_products, num_product_terms and round_degree only (mles and the tables may be NULL). */
uint64_t bzamd_sumcheck_transcript_columns_workspace_bytes(
    unsigned field_id, const struct bzamd_sumcheck_columns* columns);
void bzamd_prove_sumcheck_transcript_device_columns(void* polynomials, void* evaluation_point,
                                                    void* mle_evaluations, void* transcript,
                                                    unsigned field_id,
                                                    const struct bzamd_sumcheck_columns* columns,
                                                    void* workspace, uint64_t workspace_bytes,
                                                    void* stream);

/* The matching verifier (the reference's prfsk::verify_sumcheck_no_evaluation with that
 * transcript): host arithmetic only, needs no backend.  round_polynomials: num_variables x
 * (round_degree + 1) elements.  Every round checks 2 p[0] + p[1] + .. + p[D] == expected_sum, draws
 * r into evaluation_point and sets expected_sum = p(r).  expected_sum: in = the claimed sum, out =
 * the value the caller's final evaluation must equal.  Returns 1, or 0 at the first round whose
 * check fails: outputs and transcript are then as the rounds before it left them. */
int bzamd_verify_sumcheck(void* expected_sum, void* evaluation_point, struct sxt_transcript* transcript,
                          unsigned field_id, const void* round_polynomials, unsigned num_variables,
                          unsigned round_degree);

/* The same verifier on device-resident proofs: num_proofs independent proofs of one shape, laid out
 * back to back at byte granularity.  DEVICE pointers on the current HIP device, per proof:
 * round_polynomials num_variables x (round_degree + 1) x 32 bytes (read in stream order, never
 * written), expected_sums 32 bytes (in / out), evaluation_points num_variables x 32 bytes (out),
 * transcripts 203 bytes (in / out, used in place; proof i's transcript is at byte 203 i) and
 * verdicts one uint32_t (out).  Proof i is exactly bzamd_verify_sumcheck on the same bytes:
 * verdicts[i] is 1, or 0 at the first failing round -- the proof's expected_sum, the rows of its
 * evaluation point already written and its transcript are then as the rounds before it left them,
 * later rows of the point are not written.  One wavefront per proof, one kernel launch for the
 * batch, no workspace.  gpu backend only.  The call only enqueues on `stream`: no synchronise, no
 * allocation, no callback.  Aborts before anything is launched: NULL pointers, num_variables == 0,
 * round_degree == 0 or > 8, num_proofs == 0, an unsupported field id. */
void bzamd_verify_sumcheck_device(void* verdicts, void* expected_sums, void* evaluation_points,
                                  void* transcripts, unsigned field_id,
                                  const void* round_polynomials, unsigned num_variables,
                                  unsigned round_degree, unsigned num_proofs, void* stream);

/* The check the rounds' verifier leaves to its caller: 1 iff
 *   sum_p mult_p prod_{j in terms_p} mle_evaluations[j] == expected_sum
 * on canonical values (unreduced 32-byte inputs are taken as given), else 0.  expected_sum is what
 * bzamd_verify_sumcheck* left, mle_evaluations the num_mles elements the prover returned.
 * product_table and product_terms are those of `sumcheck_descriptor` ({multiplier; unsigned
 * length} entries of 36 bytes for field 0, 40 for field 1), validated as the prover validates
 * them, except that no round degree bounds a product: it needs at least one term.  Aborts: NULL
 * pointers, num_mles == 0, num_products == 0, a product without terms, a term >= num_mles,
 * num_product_terms that is not the sum of the lengths, an unsupported field id.
 * HOST operands, host arithmetic, needs no backend. */
int bzamd_check_sumcheck_evaluations(unsigned field_id, const void* expected_sum,
                                     const void* mle_evaluations, unsigned num_mles,
                                     const void* product_table, const unsigned* product_terms,
                                     unsigned num_products, unsigned num_product_terms);
/* The device form for num_proofs proofs of one statement.  DEVICE pointers on the current HIP
 * device: expected_sums (num_proofs x 32 bytes), mle_evaluations (num_proofs x num_mles x 32 bytes;
 * both read in stream order, never written), verdicts (num_proofs x uint32_t, out) and workspace
 * (at least bzamd_check_sumcheck_evaluations_workspace_bytes of the same field and counts; less
 * aborts; any alignment; a later call on the same stream may reuse it).  HOST: the product table
 * and the terms, which are read before the call returns.  One workgroup per proof, one kernel
 * launch behind one copy of the statement.  gpu backend only.  The call only enqueues on `stream`.
 * The workspace size needs no backend and is 0 for arguments the call would reject. */
uint64_t bzamd_check_sumcheck_evaluations_workspace_bytes(unsigned field_id, unsigned num_products,
                                                          unsigned num_product_terms);
void bzamd_check_sumcheck_evaluations_device(void* verdicts, unsigned field_id,
                                             const void* expected_sums, const void* mle_evaluations,
                                             unsigned num_mles, const void* product_table,
                                             const unsigned* product_terms, unsigned num_products,
                                             unsigned num_product_terms, unsigned num_proofs,
                                             void* workspace, uint64_t workspace_bytes, void* stream);

/* combined = sum_j coefficients[j] * decode(commitments[j]): the a_commit that
 * bzamd_verify_inner_product_device and sxt_curve25519_verify_inner_product take, from the
 * compressed commitments bzamd_msm_device(SXT_CURVE_RISTRETTO255, ..) writes and the scalars the
 * caller gave bzamd_combine_columns* (num_commitments x 32 bytes, unreduced values included).
 * `combined` is one sxt_ristretto255 of any Z.  An encoding the ristretto decoder rejects
 * contributes the identity and makes the result 0; otherwise it is 1.
 * 1 <= num_commitments <= 2^28; NULL pointers abort.  HOST operands, blocking, any backend. */
int bzamd_combine_commitments(struct sxt_ristretto255* combined,
                              const struct sxt_ristretto255_compressed* commitments,
                              const void* coefficients, uint64_t num_commitments);
/* The device form.  DEVICE pointers on the current HIP device: commitments, coefficients (read in
 * stream order, never written), combined (one sxt_ristretto255, out), valid (one uint32_t, out: 1,
 * or 0 when an encoding did not decode -- the same kernels run either way) and workspace (at least
 * bzamd_combine_commitments_workspace_bytes(num_commitments), 160 bytes a commitment; less aborts;
 * any alignment).  A decode kernel, one lane per commitment, then one engine call with projective
 * output (a pending bzamd_pipeline_next is not consumed).  gpu backend only.  The call only
 * enqueues on `stream`.  The workspace size needs no backend and is 0 outside the limits. */
uint64_t bzamd_combine_commitments_workspace_bytes(uint64_t num_commitments);
void bzamd_combine_commitments_device(void* combined, void* valid, const void* commitments,
                                      const void* coefficients, uint64_t num_commitments,
                                      void* workspace, uint64_t workspace_bytes, void* stream);

/* The inner-product prover on device-resident vectors: sxt_curve25519_prove_inner_product as a
 * chain of kernels that never returns to the host between rounds.  DEVICE pointers on the current
 * HIP device: l_vector, r_vector (ceil_log2(n) x 32 bytes each; may be NULL for n = 1), ap_value
 * (32 bytes), transcript (203 bytes, in / out, used in place), a_vector, b_vector (n x 32 bytes
 * each, read in stream order, never written), generators (NULL: the built-in generators
 * [generators_offset, generators_offset + np], derived on the device, Q = generator
 * generators_offset + np, np = 2^ceil_log2(n); otherwise np + 1 sxt_ristretto255 elements, the
 * last one Q, read only, and generators_offset is ignored) and workspace (at least
 * bzamd_inner_product_workspace_bytes(n); less aborts).  gpu backend only.  The call only
 * enqueues on `stream`: no synchronise, no callback, no allocation but the MSM engine's own
 * buffers, which grow as for bzamd_msm_device; outputs, transcript and workspace are the caller's
 * to reuse once the work enqueued by the call has completed, and a later call on the same stream
 * may use the same workspace.  Same inputs, same bytes and transcript state as
 * sxt_curve25519_prove_inner_product (n = 1: the transcript's init and ap = a[0] verbatim;
 * unreduced scalars included); same limits and aborts (null arguments, n = 0, n > 2^30).
 *
 * bzamd_inner_product_workspace_bytes depends on np alone, needs no backend, and returns 0 for
 * n = 0 and n > 2^30. */
uint64_t bzamd_inner_product_workspace_bytes(uint64_t n);
void bzamd_prove_inner_product_device(void* l_vector, void* r_vector, void* ap_value,
                                      void* transcript, uint64_t n, uint64_t generators_offset,
                                      const void* generators, const void* a_vector,
                                      const void* b_vector, void* workspace,
                                      uint64_t workspace_bytes, void* stream);

/* The inner-product verifier on a device-resident proof: sxt_curve25519_verify_inner_product as
 * one chain of kernels.  DEVICE pointers on the current HIP device: verdict (one uint32_t, written
 * 1 for an accepted proof and 0 for a rejected one), transcript (203 bytes, in / out, used in
 * place), b_vector (n x 32 bytes, no alignment needed), product, ap_value (32 bytes each),
 * a_commit (one sxt_ristretto255, any Z), l_vector, r_vector (ceil_log2(n) x 32 bytes each, where
 * bzamd_prove_inner_product_device left them; may be NULL for n = 1), generators (as for the
 * prover: NULL for the built-in ones, or np + 1 resident elements, the last one Q) and workspace
 * (at least bzamd_inner_product_verify_workspace_bytes(n); less aborts).  None of the inputs is
 * written.  gpu backend only.  The call only enqueues on `stream`: no synchronise, no callback,
 * no allocation but the MSM engine's own buffers; a later call on the same stream may use the same
 * workspace.  Same inputs, same verdict and transcript state as
 * sxt_curve25519_verify_inner_product (unreduced b, product and ap are taken as given; an L or R
 * that does not decode gives verdict 0 and the whole chain still runs); same limits and aborts.
 *
 * bzamd_inner_product_verify_workspace_bytes depends on np alone, needs no backend, and returns 0
 * for n = 0 and n > 2^30. */
uint64_t bzamd_inner_product_verify_workspace_bytes(uint64_t n);
void bzamd_verify_inner_product_device(void* verdict, void* transcript, uint64_t n,
                                       uint64_t generators_offset, const void* generators,
                                       const void* b_vector, const void* product,
                                       const void* a_commit, const void* l_vector,
                                       const void* r_vector, const void* ap_value,
                                       void* workspace, uint64_t workspace_bytes, void* stream);

/* num_proofs independent inner-product proofs of ONE length n over ONE generator set, verified in
 * one chain of kernels whose launch count outside the MSM engine does not depend on num_proofs:
 * the generators (NULL: the built-in ones from generators_offset; otherwise np + 1 resident
 * sxt_ristretto255 elements, the last one Q) are derived or copied once for the batch, and one
 * engine call takes two columns per proof.  With rounds = ceil_log2(n) and np = 2^rounds, every
 * pointer is DEVICE memory on the current HIP device, the proofs lie back to back at byte
 * granularity, and no pointer needs any alignment.  Proof i:
 *
 *   operand               offset          size                          access
 *   verdicts              4 i             one uint32_t                  out
 *   transcripts           203 i           203 bytes                     in / out, used in place
 *   b_vectors             32 n i          n x 32 bytes (n, not np)      read
 *   products              32 i            32 bytes                      read
 *   ap_values             32 i            32 bytes                      read
 *   a_commits             i elements      one sxt_ristretto255, any Z   read
 *   l_vectors, r_vectors  32 rounds i     rounds x 32 bytes each        read
 *
 * (l_vectors and r_vectors may be NULL for n = 1).  This is where bzamd_prove_inner_product_device
 * leaves a proof when it is handed the matching offsets.
 *
 * Proof i is exactly bzamd_verify_inner_product_device, and therefore
 * sxt_curve25519_verify_inner_product, on the same bytes: the same verdict and the same 203 bytes
 * of transcript afterwards; unreduced b, product and ap are taken as given; an L or R that does not
 * decode gives verdict 0 for that proof only, and what is launched never depends on any proof's
 * contents.  Proofs do not influence each other, and no input is written.  The chain compares
 *   (e_Q - product) Q + <e, g>   with   a_commit + sum_j x_j^2 L_j + x_j^-2 R_j,
 * the reference's equation with the per-proof points moved to one side so that [Q | g] is shared;
 * the two sides have equal ristretto encodings exactly when the reference's have, provided a_commit
 * is a ristretto element (a point of the even subgroup, as every decoded or computed commitment
 * is) -- which the single form assumes as well.
 *
 * gpu backend only.  The call only enqueues on `stream`: no synchronise, no callback, no allocation
 * but the MSM engine's own grow-only buffers (the engine cuts a call of more columns than a launch
 * grid takes into batches of its own); a pending bzamd_pipeline_next is not consumed; a later call
 * on the same stream may use the same workspace.
 *
 * Limits: 1 <= n <= 2^30, num_proofs >= 1, num_proofs x np <= 2^28.  Aborts before anything is
 * launched: a NULL pointer (except generators, and l_vectors / r_vectors at n = 1), n or
 * num_proofs outside the limits, a workspace smaller than
 * bzamd_inner_product_verify_batch_workspace_bytes(n, num_proofs), which needs no backend, depends
 * on n through np alone and returns 0 outside the limits. */
uint64_t bzamd_inner_product_verify_batch_workspace_bytes(uint64_t n, uint64_t num_proofs);
void bzamd_verify_inner_product_batch_device(void* verdicts, void* transcripts, uint64_t n,
                                             uint64_t num_proofs, uint64_t generators_offset,
                                             const void* generators, const void* b_vectors,
                                             const void* products, const void* a_commits,
                                             const void* l_vectors, const void* r_vectors,
                                             const void* ap_values, void* workspace,
                                             uint64_t workspace_bytes, void* stream);

/* From the sumcheck's outputs to the inner-product argument's inputs: the two vectors with which
 * one inner-product proof opens every claimed evaluation mle_evaluations[j] = f_j(r).  Both are
 * exact field arithmetic; elements are 32 bytes in the representation sxt_prove_sumcheck takes for
 * the field (field_id 0 or 1; anything else aborts) and are written canonical.
 *
 * The evaluation vector of a point: with v = num_variables and r_0 .. r_{v-1} = evaluation_point,
 *   vector[i] = prod_{t < v} (bit_{v-1-t}(i) ? r_t : 1 - r_t),   i < n,
 * the bit order of the fold above bzamd_prove_sumcheck (round 0 binds the top bit), so that
 * sum_i T_0[j][i] vector[i] = T_v[j][0] = mle_evaluations[j] exactly; n = 1, v = 1 gives 1 - r_0.
 * 1 <= num_variables <= 30 and 1 <= n <= 2^num_variables (num_variables may exceed ceil_log2(n));
 * `vector` must be 8-byte aligned; null pointers abort. */
/* HOST operands, blocking, cpu and gpu backends (the gpu backend uploads the point, runs the device
 * form and downloads the vector) */
void bzamd_mle_evaluation_vector(void* vector, unsigned field_id, const void* evaluation_point,
                                 unsigned num_variables, uint64_t n);
/* DEVICE pointers on the current HIP device: vector (n x 32 bytes) and evaluation_point
 * (num_variables x 32 bytes, read in stream order: the call may follow the sumcheck chain that
 * writes it with no synchronise in between).  gpu backend only.  The call only enqueues on
 * `stream`: no synchronise, no allocation, no callback, no workspace. */
void bzamd_mle_evaluation_vector_device(void* vector, unsigned field_id,
                                        const void* evaluation_point, unsigned num_variables,
                                        uint64_t n, void* stream);

/* A linear combination of typed columns, widened to scalars:
 *   combined[i] = sum_j coefficients[j] * column_j[i],   i < n,
 * n x 32 bytes.  The columns are the MSM's / sumcheck's descriptors and mean what they mean in
 * bzamd_prove_sumcheck_columns: columns[j].n <= n rows (longer aborts), rows past a column's end
 * are zero (n = 0 with data = NULL is a zero column); element_nbytes 1 .. 31 little-endian
 * integers, two's complement when is_signed; element_nbytes 32 the field's elements, unreduced
 * values included; validated by the same rule.  When `product` and `evaluations` are both
 * non-NULL, product = sum_j coefficients[j] * evaluations[j] (32 bytes): the inner product the
 * proof claims when evaluations are the sumcheck's mle_evaluations.  When either is NULL nothing
 * is written there.  1 <= n <= 2^30, 1 <= num_columns (no upper limit); `combined` must be 8-byte
 * aligned and must not overlap a column. */
struct bzamd_column_combination {
  const struct sxt_sequence_descriptor* columns; /* num_columns descriptors */
  const void* coefficients;                      /* num_columns x 32 bytes */
  const void* evaluations;                       /* may be NULL: num_columns x 32 bytes */
  unsigned num_columns;
  uint64_t n;
};
/* HOST operands (columns[j].data included), blocking, cpu and gpu backends.  The gpu backend
 * uploads the columns at their own width, runs the device form and synchronises once. */
void bzamd_combine_columns(void* combined, void* product, unsigned field_id,
                           const struct bzamd_column_combination* c);
/* DEVICE pointers on the current HIP device: combined, product (may be NULL), coefficients,
 * evaluations (may be NULL) and every columns[j].data (any address; read in stream order, never
 * written).  HOST: the struct and the descriptors, which are read before the call returns.  gpu
 * backend only.  The call only enqueues on `stream`: no synchronise, no allocation, no callback,
 * no workspace (the descriptors travel as kernel arguments, 32 columns to a launch; further
 * launches add to `combined`). */
void bzamd_combine_columns_device(void* combined, void* product, unsigned field_id,
                                  const struct bzamd_column_combination* c, void* stream);

/* The column of inverses a log-derivative argument (lookup, membership, join, group-by) commits to
 * and multiplies in its sumcheck:
 *   denominator[i] = shift + sum_j coefficients[j] * column_j[i]        i < n
 *   inverses[i]    = denominator[i]^-1, and 0 where denominator[i] = 0
 * A zero denominator disturbs no other row.  The columns mean what they mean in
 * bzamd_combine_columns and are validated by the same rule: columns[j].n <= n rows (longer aborts),
 * rows past a column's end are zero (their denominator is `shift` plus the other columns), n = 0
 * with data = NULL is a zero column; element_nbytes 1 .. 31 little-endian integers, two's
 * complement when is_signed (up to 16 bytes); element_nbytes 32 the field's elements, unreduced
 * values included; data at any address.  `coefficients` (NULL: every coefficient is 1) and `shift`
 * (NULL: 0) are in element form, need no alignment and may be unreduced.  `inverses` (n x 32 bytes)
 * is written in element form, canonical; `scalars` (n x 32 bytes) takes the same rows in scalar
 * form, what bzamd_msm_device reads as a 32-byte column (the two forms are defined above
 * bzamd_fold_polynomial: field 0 the same bytes, field 1 Montgomery words and plain integers).
 * Either output may be NULL, not both; both must be 8-byte aligned.
 * 1 <= n <= 2^30, 1 <= num_columns <= 32: the descriptors of a call travel as kernel arguments; a
 * caller with more columns combines them with bzamd_combine_columns_device first and inverts that
 * one 32-byte column.  field_id 0 or 1.  Aborts, before anything is launched: a null v, columns or
 * both outputs null, a bad descriptor, a column longer than n, a limit exceeded, a misaligned
 * output, an output that overlaps an input or the other output, an unsupported field id. */
struct bzamd_column_inversion {
  const struct sxt_sequence_descriptor* columns; /* num_columns descriptors */
  const void* coefficients; /* may be NULL: every coefficient is 1; else num_columns x 32 bytes */
  const void* shift;        /* may be NULL: 0; else 32 bytes */
  unsigned num_columns;
  uint64_t n;
};
/* HOST operands (columns[j].data included), blocking, cpu and gpu backends.  The cpu backend shares
 * one inversion among 256 rows; the gpu backend uploads the columns at their own width, runs the
 * device form, synchronises once and downloads the outputs. */
void bzamd_invert_columns(void* inverses, void* scalars, unsigned field_id,
                          const struct bzamd_column_inversion* v);
/* DEVICE pointers on the current HIP device: inverses, scalars, coefficients, shift and every
 * columns[j].data (read in stream order, never written).  HOST: the struct and the descriptors,
 * which are read before the call returns.  gpu backend only (anything else aborts).  The call only
 * enqueues on `stream`: no synchronise, no allocation, no callback, no workspace.  ONE kernel
 * launch, whatever n, num_columns and the data are. */
void bzamd_invert_columns_device(void* inverses, void* scalars, unsigned field_id,
                                 const struct bzamd_column_inversion* v, void* stream);

/* The multiplicity column of a log-derivative argument: how often each row of a table column is
 * looked up by the rows of a lookup column, so that
 *   sum_t multiplicities[t] / (alpha + T[t]) = sum_i 1 / (alpha + L[i])      whenever misses = 0.
 * The key of a row is its value in the field as the canonical integer in [0, p).  Both columns are
 * the MSM's / sumcheck's descriptors and mean what they mean in bzamd_combine_columns, validated by
 * the same rule: element_nbytes 1 .. 31 little-endian integers, two's complement when is_signed (up
 * to 16 bytes); element_nbytes 32 the field's elements, unreduced values included; data at any
 * address.  Two rows are equal when their keys are: an i8 -1, an i64 -1 and the 32-byte element
 * p - 1 are one key, x and x + p in a 32-byte column are one key, and in field 1 a 32-byte row
 * (Montgomery words) and a narrow row compare by value, not by bytes.  The table (m = table.n rows)
 * and the lookups (n = lookups.n rows) may differ in width and signedness.  Tuples are the caller's
 * to fold: bzamd_combine_columns_device with the powers of beta makes the one 32-byte column that
 * bzamd_invert_columns_device inverts, and the same column goes here.
 *   multiplicities: m x 8 bytes, little-endian uint64_t, 8-byte aligned.  With first(t) the least
 *     t' whose key equals that of row t:
 *       multiplicities[t] = #{i < n : key(lookups[i]) = key(table[t])}   when first(t) = t,
 *       multiplicities[t] = 0                                            otherwise
 *     (duplicates in the table give their count to the first occurrence, so the identity holds for
 *     any table).  What bzamd_msm_device, the sumcheck provers and bzamd_combine_columns_device
 *     read as an 8-byte unsigned column.
 *   misses (may be NULL; one uint64_t, 8-byte aligned): the number of lookup rows whose key is in
 *     no table row.  The identity holds exactly when it is 0.
 * No input is written.
 * The range table: table.data == NULL with table.n = m >= 1, table.element_nbytes = 8 and
 * table.is_signed = 0 means T[t] = t (any other width or signedness with a NULL table aborts).  A
 * lookup row hits row `key` when key < m and misses otherwise; negative narrow values are p - |x|
 * and miss.  This form needs no workspace (`workspace` may be NULL).
 * Limits: 1 <= m <= 2^28, 0 <= n <= 2^30 (lookups.n = 0 with data = NULL writes m zeros and
 * misses = 0); field_id 0 or 1.  Aborts, before anything is launched: a null multiplicities or c,
 * a bad descriptor, a limit exceeded, a misaligned output, an output that overlaps an input, the
 * other output or the workspace, a workspace that is too small, an unsupported field id, the
 * device form on the cpu backend. */
struct bzamd_multiplicity_count {
  struct sxt_sequence_descriptor table;   /* m = table.n rows */
  struct sxt_sequence_descriptor lookups; /* n = lookups.n rows */
};
/* What the device form's workspace takes for a table with data: S slots of 4 bytes, S the least
 * power of two >= 2 table_rows (1 row: 2 slots, 2 rows: 4, 3 rows: 8; there is no minimum), and
 * 256 bytes for the pointer's alignment.  Needs no backend; 0 outside 1 <= table_rows <= 2^28. */
uint64_t bzamd_count_multiplicities_workspace_bytes(uint64_t table_rows);
/* HOST operands (table.data and lookups.data included), blocking, cpu and gpu backends.  The cpu
 * backend counts row by row; the gpu backend uploads both columns at their own width, runs the
 * device form on memory of the call's own, synchronises once and downloads the outputs. */
void bzamd_count_multiplicities(void* multiplicities, uint64_t* misses, unsigned field_id,
                                const struct bzamd_multiplicity_count* c);
/* DEVICE pointers on the current HIP device: multiplicities, misses, workspace, table.data and
 * lookups.data (read in stream order, never written).  HOST: the struct, which is read before the
 * call returns.  gpu backend only (anything else aborts).  The call only enqueues on `stream`: no
 * synchronise, no allocation, no callback.  THREE kernel launches (the range table: TWO), whatever
 * m, n and the data are.  workspace: at least bzamd_count_multiplicities_workspace_bytes(m) bytes
 * at any address, contents ignored; a later call on the same stream may use the same workspace. */
void bzamd_count_multiplicities_device(void* multiplicities, void* misses, unsigned field_id,
                                       const struct bzamd_multiplicity_count* c, void* workspace,
                                       uint64_t workspace_bytes, void* stream);
/* A diagnostic, like bzamd_accumulate_form: the slot, below S, at which the probe for a key starts
 * in the device form's table of table_rows rows, so that tests can build clusters and wrap-arounds
 * without restating the hash.  element: 32 bytes in element form, may be unreduced.  Host
 * arithmetic, needs no backend; UINT64_MAX outside the limits (table_rows, field_id) or for a NULL
 * element.  The hash is NOT part of the ABI and may change between versions. */
uint64_t bzamd_multiplicity_first_slot(unsigned field_id, const void* element, uint64_t table_rows);

/* Sums of value columns by key: the result columns of a group-by, and the match index of a join.
 * Per key of the table, the sum of each value column over the input rows that carry the key and
 * their number, so that for every value column v
 *   sum_t sums_v[t] / (alpha + T[t]) = sum_i value_v[i] / (alpha + L[i])      whenever misses = 0.
 * Keys, the equality of rows, first(t), the range table (table.data == NULL), `misses` and the
 * limits 1 <= m <= 2^28, 0 <= n <= 2^30 are those above bzamd_count_multiplicities.  The value
 * columns mean what they mean in bzamd_combine_columns and are validated by the same rule:
 * element_nbytes 1 .. 31 little-endian integers, two's complement when is_signed (up to 16 bytes);
 * element_nbytes 32 the field's elements, unreduced values included, Montgomery words in field 1;
 * data at any address; values[v].n <= n rows (longer aborts), rows past a column's end are zero.
 * The value of a row is its value in the field: a negative x is p - |x|.
 *   sums:    num_values x m x 32 bytes, column v at sums + 32 m v, element form, canonical:
 *              sums_v[t] = sum over {i < n : key(L[i]) = key(T[t])} of value_v[i]  mod p
 *            when first(t) = t; 0 otherwise, and 0 for a key nobody looks up.
 *   scalars: the same shape, the same rows in scalar form, what bzamd_msm_device reads as a
 *            32-byte column (the two forms are defined above bzamd_fold_polynomial).
 *   counts:  m x 8 bytes: exactly the `multiplicities` of bzamd_count_multiplicities for the same
 *            table and lookups.
 *   misses:  one uint64_t, as in bzamd_count_multiplicities.
 *   matches: n x 4 bytes, little-endian uint32_t, 4-byte aligned: matches[i] = first(t) of the
 *            table row that L[i] hits, 0xFFFFFFFF for a miss; with the range table the key itself
 *            when it is below m.
 * Any output may be NULL: with num_values = 0 both sums and scalars must be; with num_values >= 1
 * at least one of them must not be; at least one output must not be.  Lookups that miss contribute
 * nowhere.  No input is written.  The result is the same bits from run to run.
 * 0 <= num_values <= 8; field_id 0 or 1.  Aborts, before anything is launched: a null k, a null
 * values with num_values > 0, a bad descriptor, a value column longer than n, a limit exceeded, a
 * misaligned output (8 bytes; matches 4), an output that overlaps an input, another output or the
 * workspace, a workspace that is too small, an unsupported field id, the device form on the cpu
 * backend. */
struct bzamd_key_sums {
  struct sxt_sequence_descriptor table;   /* m = table.n rows; data NULL: the range table T[t] = t */
  struct sxt_sequence_descriptor lookups; /* n = lookups.n rows: the key of every input row */
  const struct sxt_sequence_descriptor* values; /* num_values descriptors, values[v].n <= n */
  unsigned num_values;                    /* 0 .. 8 */
};
/* What the device form's workspace takes: the slots of bzamd_count_multiplicities_workspace_bytes
 * padded to a multiple of 256, 64 bytes per table row and value column (eight 64-bit accumulators,
 * what the widest column needs), and 256 bytes for the pointer's alignment.  Needs no backend;
 * 0 outside 1 <= table_rows <= 2^28, num_values <= 8. */
uint64_t bzamd_sum_by_key_workspace_bytes(uint64_t table_rows, unsigned num_values);
/* HOST operands (every descriptor's data included), blocking, cpu and gpu backends.  The cpu backend
 * goes row by row with one field addition per row and value column; the gpu backend uploads the
 * columns at their own width, runs the device form on memory of the call's own, synchronises once
 * and downloads the outputs. */
void bzamd_sum_by_key(void* sums, void* scalars, void* counts, uint64_t* misses, void* matches,
                      unsigned field_id, const struct bzamd_key_sums* k);
/* DEVICE pointers on the current HIP device: the five outputs, workspace, table.data, lookups.data
 * and every values[v].data (read in stream order, never written).  HOST: the struct and the value
 * descriptors, which are read before the call returns.  gpu backend only (anything else aborts).
 * The call only enqueues on `stream`: no synchronise, no allocation, no callback.  FOUR kernel
 * launches (the range table: THREE), whatever m, n, num_values and the data are.  workspace: at
 * least bzamd_sum_by_key_workspace_bytes(m, num_values) bytes at any address, contents ignored (the
 * range table with num_values = 0 needs none: NULL); a later call on the same stream may use the
 * same workspace. */
void bzamd_sum_by_key_device(void* sums, void* scalars, void* counts, void* misses, void* matches,
                             unsigned field_id, const struct bzamd_key_sums* k, void* workspace,
                             uint64_t workspace_bytes, void* stream);

/* Selection of rows: the stable compaction of typed columns by a selector column, and the gather
 * by row index that goes with it.  A WHERE keeps the rows of its result columns whose flag is set;
 * a group-by needs the dense table of distinct keys (the rows at which the `multiplicities` of
 * bzamd_count_multiplicities with the key column as table and lookups are non-zero); a join drops
 * the misses of the `matches` of bzamd_sum_by_key and fetches the table's columns at the hits.
 * Neither call does field arithmetic: rows are copied at their own width, for either field and
 * either form.
 *   kept(i):  (bits(selector[i]) != reject) != invert, i < n = selector.n, where bits is the row's
 *             element_nbytes (1 .. 8) bytes as a little-endian unsigned integer, zero-extended to
 *             64 bits; is_signed does not enter.  A u8 flag column with reject = 0 is a WHERE; the
 *             u64 counts with reject = 0 give first occurrences; the u32 matches with
 *             reject = 0xFFFFFFFF give the hits, with invert = 1 the misses (anti-join).
 *   rank(i):  the number of kept rows before i.
 *   count:    (may be NULL) one uint64_t, 8-byte aligned: the number of kept rows, exact even when
 *             it exceeds capacity.
 *   selected: num_columns output pointers, 8-byte aligned each: kept row i of columns[j] goes to
 *             bytes rank(i) * w_j ..+ w_j of selected[j], w_j = columns[j].element_nbytes
 *             (1 .. 32), whenever rank(i) < capacity.  A byte copy.  The columns are validated by
 *             the rule of bzamd_combine_columns; data at any address; columns[j].n <= n (longer
 *             aborts); a kept row at or past columns[j].n is written as zero bytes; n = 0 with
 *             data = NULL is a zero column.  Each output is what every columns call reads as a
 *             column of w_j-byte rows.
 *   indices:  (may be NULL) capacity x 4 bytes, little-endian uint32_t, 4-byte aligned:
 *             indices[rank(i)] = i for kept rows with rank(i) < capacity.
 *   zero_tail = 1: rows min(count, capacity) .. capacity of every output column are written as
 *             zero bytes and those of indices as 0xFFFFFFFF, so that the commitment, sumcheck and
 *             combination of an output over `capacity` rows equal those of its `count` rows, and a
 *             chain stays enqueue-only with a length the host knows beforehand.
 *   zero_tail = 0: nothing at or past min(count, capacity) is written.
 * At least one of count, indices and a column must be asked for.  With capacity = 0 the output
 * pointers may be NULL.  0 <= n <= 2^30 (n = 0 with data = NULL: count = 0, and the tail rule still
 * applies); 0 <= capacity <= 2^30, which may exceed n; 0 <= num_columns <= 16.  In-place compaction
 * is NOT supported.  No input is written.  The result is the same bits from run to run.
 * Aborts, before anything is launched: a null s, a null columns or selected with num_columns > 0,
 * a bad descriptor, a selector wider than 8 bytes, a column longer than n, a limit exceeded, no
 * output asked for, a null output pointer with capacity > 0, a misaligned output (8 bytes; indices
 * 4), an output that overlaps an input, another output or the workspace, a workspace that is too
 * small, the device form on the cpu backend. */
struct bzamd_row_selection {
  struct sxt_sequence_descriptor selector;       /* n = selector.n rows, element_nbytes 1 .. 8 */
  uint64_t reject;                               /* compared with the row's bits, zero-extended */
  int invert;                                    /* 0: keep rows != reject; 1: keep rows == reject */
  const struct sxt_sequence_descriptor* columns; /* num_columns descriptors, columns[j].n <= n */
  void* const* selected;                         /* num_columns output pointers (host array) */
  unsigned num_columns;                          /* 0 .. 16 */
  uint64_t capacity;                             /* rows every output column (and indices) can hold */
  int zero_tail;                                 /* 1: rows min(count, capacity) .. capacity are zeroed */
};
/* What the device form's workspace takes: one 32-bit count per span of rows (at most 2048 spans of
 * whole tiles of 1024 rows; n = 0 has one) and 256 bytes for the pointer's alignment.  Needs no
 * backend; 0 outside n <= 2^30. */
uint64_t bzamd_select_rows_workspace_bytes(uint64_t n);
/* HOST operands (every descriptor's data and every selected[j] included), blocking, cpu and gpu
 * backends.  The cpu backend goes row by row; the gpu backend uploads the columns at their own
 * width, runs the device form on memory of the call's own, synchronises once and downloads the
 * outputs. */
void bzamd_select_rows(uint64_t* count, void* indices, const struct bzamd_row_selection* s);
/* DEVICE pointers on the current HIP device: count, indices, every selected[j], workspace,
 * selector.data and every columns[j].data (read in stream order, never written).  HOST: the struct,
 * the descriptors and the array of output pointers, which are read before the call returns.  gpu
 * backend only (anything else aborts).  The call only enqueues on `stream`: no synchronise, no
 * allocation, no callback.  TWO kernel launches, whatever n, the columns and the data are, and no
 * workgroup waits on another.  workspace: at least bzamd_select_rows_workspace_bytes(n) bytes at
 * any address, contents ignored; a later call on the same stream may use the same workspace. */
void bzamd_select_rows_device(void* count, void* indices, const struct bzamd_row_selection* s,
                              void* workspace, uint64_t workspace_bytes, void* stream);

/* A diagnostic, like bzamd_accumulate_form: how the second launch of bzamd_select_rows_device
 * stores.  Columns of at most `width` bytes a row (0 .. 32; larger counts as 32) have a tile's kept
 * rows packed in LDS and written as whole 16-byte pieces; wider columns are stored one row a lane.
 * 0 stores every column one row a lane.  The results are the same bytes either way.  A negative
 * width changes nothing.  Returns the width in force before; process-wide, needs no backend. */
int bzamd_select_rows_packed_width(int width);

/* The gather: row r of taken[j] is row indices[r] of columns[j],
 *   taken[j][r * w_j ..+ w_j] = columns[j][indices[r]]   when indices[r] < columns[j].n,
 * and zero bytes otherwise: one rule for the 0xFFFFFFFF of `matches`, the zero tail of `indices`
 * and short columns.  A byte copy at widths 1 .. 32; the columns may have any lengths and are
 * validated by the rule of bzamd_combine_columns.  indices: num_rows x uint32_t, 4-byte aligned;
 * outputs 8-byte aligned; 1 <= num_rows <= 2^30; 1 <= num_columns <= 16.  Aborts, before anything
 * is launched: a null t, indices, columns, taken or output pointer, a bad descriptor, a limit
 * exceeded, misalignment, an output that overlaps an input or another output, the device form on
 * the cpu backend.  No input is written. */
struct bzamd_row_take {
  const void* indices;                           /* num_rows x uint32_t, 4-byte aligned */
  uint64_t num_rows;                             /* 1 .. 2^30 */
  const struct sxt_sequence_descriptor* columns; /* num_columns source columns, any lengths */
  void* const* taken;                            /* num_columns output pointers (host array) */
  unsigned num_columns;                          /* 1 .. 16 */
};
/* HOST operands, blocking, cpu and gpu backends (the gpu backend uploads the indices and the
 * columns, runs the device form, synchronises once and downloads the outputs). */
void bzamd_take_rows(const struct bzamd_row_take* t);
/* DEVICE pointers on the current HIP device: indices, every taken[j] and every columns[j].data
 * (read in stream order, never written).  HOST: the struct, the descriptors and the array of
 * output pointers.  gpu backend only.  Enqueue only: no synchronise, no allocation, no callback, no
 * workspace.  ONE kernel launch, whatever num_rows, the columns and the data are. */
void bzamd_take_rows_device(const struct bzamd_row_take* t, void* stream);

/* The word columns of a range check.  A value is in range when its byte words are: every word is
 * looked up in the table 0 .. 255, and the prover commits to the word columns, the 256 word counts
 * and one inverse column 1 / (alpha + word) per word column.
 *   key(i) = the canonical integer in [0, p) of shift + column[i],   i < n = column.n.
 * The column is the MSM's / sumcheck's descriptor and means what it means in
 * bzamd_count_multiplicities, validated by the same rule: element_nbytes 1 .. 31 little-endian
 * integers, two's complement when is_signed (up to 16 bytes; a negative row is p - |x|);
 * element_nbytes 32 the field's elements, unreduced values included (x and x + p have one key),
 * Montgomery words in field 1; data at any address.  `shift` (NULL: 0; else 32 bytes in element
 * form at any address, may be unreduced) lets a signed column be checked without a 32-byte
 * intermediate: with shift = 2^63 every i64 has a key below 2^64.
 *   words:    num_words planes of n bytes, words[k * plane_stride + i] = byte k of key(i),
 *             k < num_words, i < n.  The planes may start at any address; bytes between n and
 *             plane_stride are not written.  Each plane is an ordinary 1-byte unsigned column for
 *             bzamd_msm_device, the sumcheck provers and every columns call.
 *   counts:   256 x 8 bytes, little-endian uint64_t, 8-byte aligned: counts[v] = the number of
 *             pairs (k, i), k < num_words, i < n, whose byte is v; their sum is num_words * n.
 *             What the columns calls read as an 8-byte unsigned column of 256 rows: the
 *             multiplicity column of the lookup of ALL planes in the table 0 .. 255.
 *   overflow: one uint64_t, 8-byte aligned: the number of rows with key(i) >= 2^(8 num_words),
 *             always 0 for num_words = 32.  Words of those rows are the low bytes all the same.
 *             The range check holds exactly when overflow = 0.
 * words, counts and overflow may each be NULL, not all three.  No input is written.
 * Limits: 0 <= n <= 2^30 (n = 0 with data = NULL writes 256 zeros and overflow = 0),
 * 1 <= num_words <= 32, plane_stride >= n, field_id 0 or 1.  Aborts, before anything is launched: a
 * null d, all outputs null, a bad descriptor, a limit exceeded, plane_stride < n, a misaligned
 * counts or overflow, an output that overlaps an input or another output (the planes' range is
 * (num_words - 1) * plane_stride + n bytes), an unsupported field id, the device form on the cpu
 * backend. */
struct bzamd_word_decomposition {
  struct sxt_sequence_descriptor column; /* n = column.n rows */
  const void* shift;                     /* may be NULL: 0; else 32 bytes, element form */
  unsigned num_words;                    /* 1 .. 32 */
  uint64_t plane_stride;                 /* bytes from plane k to plane k + 1; >= n */
};
/* HOST operands (column.data included), blocking, cpu and gpu backends.  The cpu backend goes row
 * by row; the gpu backend uploads the column at its own width, runs the device form on memory of
 * the call's own, synchronises once and downloads the outputs plane by plane. */
void bzamd_decompose_words(void* words, uint64_t* counts, uint64_t* overflow, unsigned field_id,
                           const struct bzamd_word_decomposition* d);
/* DEVICE pointers on the current HIP device: words, counts, overflow, shift and column.data (read
 * in stream order, never written).  HOST: the struct, which is read before the call returns.  gpu
 * backend only (anything else aborts).  The call only enqueues on `stream`: no synchronise, no
 * allocation, no callback, no workspace.  TWO kernel launches, whatever n, num_words and the data
 * are. */
void bzamd_decompose_words_device(void* words, void* counts, void* overflow, unsigned field_id,
                                  const struct bzamd_word_decomposition* d, void* stream);

/* The columns a word plane maps to through a table of 256 rows of 32 bytes:
 *   mapped[k * mapped_stride + 32 i ..+32] = table[words_k[i]],   k < num_planes, i < n,
 * with words_k[i] = words[k * plane_stride + i].  A byte copy: it works for either field and
 * either form.  With the `inverses` table of bzamd_invert_columns_device over the one-byte column
 * 0 .. 255 and shift = alpha, the outputs are the inverse-word columns 1 / (alpha + word) in
 * element form, for the price of moving their bytes instead of one field inversion a row; with its
 * `scalars` table they are what bzamd_msm_device reads as 32-byte columns.
 * 1 <= n <= 2^30, 1 <= num_planes <= 32, plane_stride >= n, mapped_stride >= 32 n and a multiple
 * of 8, `mapped` 8-byte aligned; words and table at any address.  Aborts, before anything is
 * launched: a null mapped, m, words or table, a limit exceeded, a bad stride, a misaligned mapped,
 * an output that overlaps an input (the mapped range is (num_planes - 1) * mapped_stride + 32 n
 * bytes), the device form on the cpu backend.  No input is written. */
struct bzamd_word_map {
  const void* words;        /* num_planes planes of n bytes, plane k at words + k * plane_stride */
  const void* table;        /* 256 x 32 bytes */
  unsigned num_planes;      /* 1 .. 32 */
  uint64_t n, plane_stride; /* plane_stride >= n */
  uint64_t mapped_stride;   /* bytes from mapped column k to k + 1; >= 32 n, a multiple of 8 */
};
/* HOST operands, blocking, cpu and gpu backends (the gpu backend uploads the planes and the table,
 * runs the device form, synchronises once and downloads the columns one by one). */
void bzamd_map_words(void* mapped, const struct bzamd_word_map* m);
/* DEVICE pointers on the current HIP device: mapped, words and table (read in stream order, never
 * written).  HOST: the struct.  gpu backend only.  Enqueue only: no synchronise, no allocation, no
 * callback, no workspace.  ONE kernel launch, whatever n, num_planes and the data are. */
void bzamd_map_words_device(void* mapped, const struct bzamd_word_map* m, void* stream);

/* The MLE evaluations of typed columns, given the evaluation vector of the point:
 *   evaluations[j] = sum_{i < columns[j].n} column_j[i] * vector[i],
 * num_columns x 32 bytes, written canonical (no alignment needed).  With the vector of
 * bzamd_mle_evaluation_vector this is the identity above, sum_i T_0[j][i] vector[i] =
 * mle_evaluations[j], for any column, whether or not the sumcheck multiplied it: the evaluations
 * bzamd_combine_columns takes.  The columns mean what they mean in bzamd_combine_columns and are
 * validated by the same rule: columns[j].n <= n rows (longer aborts), rows past a column's end
 * contribute nothing, n = 0 with data = NULL is a zero column (evaluation 0).  `vector`: n x 32
 * bytes, an entry meaning what a 32-byte column element means (field 0 the little-endian integer
 * mod l, field 1 Montgomery form x 2^256; unreduced entries are taken as given), 8-byte aligned
 * (what bzamd_mle_evaluation_vector* writes; anything else aborts).  1 <= n <= 2^30,
 * 1 <= num_columns (no upper limit); null evaluations, vector, e or columns abort.  None of the
 * inputs is written. */
struct bzamd_column_evaluation {
  const struct sxt_sequence_descriptor* columns; /* num_columns descriptors */
  unsigned num_columns;
  uint64_t n;                                    /* rows of `vector` */
};
/* HOST operands (columns[j].data included), blocking, cpu and gpu backends.  The gpu backend
 * uploads the vector and the columns at their own width, runs the device form on memory of the
 * call's own and synchronises once. */
void bzamd_evaluate_columns(void* evaluations, unsigned field_id, const void* vector,
                            const struct bzamd_column_evaluation* e);
/* What the device form needs as workspace: the partial sums of its workgroups.  Needs no backend;
 * 0 for an unsupported field, num_columns = 0, n = 0 and n > 2^30. */
uint64_t bzamd_evaluate_columns_workspace_bytes(unsigned field_id, unsigned num_columns, uint64_t n);
/* DEVICE pointers on the current HIP device: evaluations, vector, every columns[j].data (any
 * address) and workspace (any alignment; at least bzamd_evaluate_columns_workspace_bytes of the
 * same arguments, less aborts).  HOST: the struct and the descriptors, which are read before the
 * call returns.  gpu backend only.  The call only enqueues on `stream`: no synchronise, no
 * allocation, no callback.  `vector` and the columns are read in stream order, so the call may
 * follow bzamd_mle_evaluation_vector_device on the same stream with no synchronise in between, and
 * a bzamd_combine_columns_device on the same stream may read `evaluations` right after it; a later
 * call on the same stream may use the same workspace.  The descriptors travel as kernel arguments,
 * 8 columns to a launch, and one more launch finishes every column. */
void bzamd_evaluate_columns_device(void* evaluations, unsigned field_id, const void* vector,
                                   const struct bzamd_column_evaluation* e, void* workspace,
                                   uint64_t workspace_bytes, void* stream);

/* Univariate openings: the field work of a HyperKZG prover between its MSM calls, for a polynomial
 * of l = num_variables variables given by its n evaluations (the combined column of
 * bzamd_combine_columns, say).  Exact field arithmetic in both fields (field_id 0 or 1; anything
 * else aborts).  The transcript and the commitment key stay with the caller.
 *
 * Element form: 32 bytes in the representation sxt_prove_sumcheck takes for the field (field 0 the
 * little-endian integer mod l, field 1 four little-endian 64-bit words of x 2^256 mod p); inputs
 * may be unreduced, outputs are canonical.  Scalar form: the canonical value as a plain 32-byte
 * little-endian integer, what an MSM descriptor with element_nbytes 32 reads (field 0: the same
 * bytes as element form).
 *
 * Sizes: 1 <= l <= 30 and 1 <= n <= 2^l.  P_0 = polynomial has n rows and rows past the end are
 * zero.  len_0 = n, len_i = ceil(len_{i-1} / 2); off_1 = 0, off_{i+1} = off_i + len_i.  `folded`
 * holds P_1 .. P_{l-1} back to back, P_i at row off_i with len_i rows: off_l <= n + l rows in all,
 * none for l = 1 (folded may then be NULL).
 *
 * Fold.  With x_0 .. x_{l-1} = point, for i = 1 .. l - 1 and j < len_i
 *   P_i[j] = P_{i-1}[2j] + x_{l-i} (P_{i-1}[2j+1] - P_{i-1}[2j]),
 * P_{i-1}[2j+1] being 0 when 2j + 1 = len_{i-1}.  `folded` is written in element form; `scalars`
 * (may be NULL) takes the same rows in scalar form, the input of the commitments to P_1 .. P_{l-1};
 * `evaluation` (may be NULL; 32 bytes, element form) takes the same step once more, with x_0 on
 * P_{l-1}: x_0 binds the top bit of the row index and x_{l-1} the lowest, so that evaluation =
 * sum_i P_0[i] vector[i] with the vector of bzamd_mle_evaluation_vector for the same point, exactly
 * (l = 1, n = 1: (1 - x_0) P_0[0]).
 *
 * Evaluate.  Points u_0 .. u_{t-1}, 1 <= t = num_points <= 4 (HyperKZG: r, -r, r^2):
 *   evaluations[k l + i] = sum_{j < len_i} P_i[j] u_k^j,   element form, u^0 = 1 for u = 0 too.
 *
 * Batch and divide.  One element q and the same points:
 *   B[m]   = sum_{i < l, m < len_i} q^i P_i[m],        m < n,
 *   h_k[j] = sum_{m = j+1}^{n-1} B[m] u_k^(m-j-1),     j < n   (h_k[n-1] = 0 is written),
 * `quotients`: t x n rows in scalar form, h_k at row k n; `remainders` (may be NULL): t elements,
 * element form, B(u_k).  B(X) = (X - u_k) h_k(X) + remainders[k], and remainders[k] =
 * sum_i q^i evaluations[k l + i].
 *
 * polynomial, folded, scalars and quotients must be 8-byte aligned; point, points, q, evaluation,
 * evaluations, remainders and workspace need no alignment.  Aborts, before anything is launched: a
 * null pointer other than those named as optional, l outside [1, 30], n outside [1, 2^l],
 * num_points outside [1, 4], a misaligned array, a workspace that is too small, and an output that
 * overlaps an input of the same call. */
/* HOST operands, blocking, cpu and gpu backends.  The gpu backend uploads the operands, runs the
 * device form on memory of the call's own, synchronises once and downloads the results. */
void bzamd_fold_polynomial(void* folded, void* scalars, void* evaluation, unsigned field_id,
                           const void* polynomial, uint64_t n, const void* point,
                           unsigned num_variables);
/* DEVICE pointers on the current HIP device, all of them.  gpu backend only.  The call only
 * enqueues on `stream`: no synchronise, no allocation, no callback, no workspace.  The operands
 * are read in stream order, so the call may follow the producer of `polynomial` and `point` on the
 * same stream with no synchronise in between.  ceil(l / 10) kernel launches, whatever n is. */
void bzamd_fold_polynomial_device(void* folded, void* scalars, void* evaluation, unsigned field_id,
                                  const void* polynomial, uint64_t n, const void* point,
                                  unsigned num_variables, void* stream);

void bzamd_evaluate_polynomials(void* evaluations, unsigned field_id, const void* polynomial,
                                const void* folded, uint64_t n, unsigned num_variables,
                                const void* points, unsigned num_points);
/* What the device form needs as workspace: one partial sum per point and chunk of rows, at most
 * 2080 x 36 x num_points + 512 bytes whatever n is.  Needs no backend; 0 for an unsupported field
 * and for sizes outside the limits above. */
uint64_t bzamd_evaluate_polynomials_workspace_bytes(unsigned field_id, uint64_t n,
                                                    unsigned num_variables, unsigned num_points);
/* DEVICE pointers, as bzamd_fold_polynomial_device, which it may follow on the same stream with no
 * synchronise in between; workspace: at least bzamd_evaluate_polynomials_workspace_bytes of the
 * same arguments, and a later call on the same stream may use the same one.  Two kernel launches. */
void bzamd_evaluate_polynomials_device(void* evaluations, unsigned field_id, const void* polynomial,
                                       const void* folded, uint64_t n, unsigned num_variables,
                                       const void* points, unsigned num_points, void* workspace,
                                       uint64_t workspace_bytes, void* stream);

void bzamd_batch_quotients(void* quotients, void* remainders, unsigned field_id,
                           const void* polynomial, const void* folded, uint64_t n,
                           unsigned num_variables, const void* q, const void* points,
                           unsigned num_points);
/* What the device form needs as workspace: B is made on the fly and never stored, so it is a sum
 * and a carry per point and chunk of rows, at most 2 x 1024 x 36 x num_points + 768 bytes whatever
 * n is.  Needs no backend; 0 for an unsupported field and for sizes outside the limits above. */
uint64_t bzamd_batch_quotients_workspace_bytes(unsigned field_id, uint64_t n,
                                               unsigned num_variables, unsigned num_points);
/* DEVICE pointers, as bzamd_evaluate_polynomials_device.  Three kernel launches, whatever n is. */
void bzamd_batch_quotients_device(void* quotients, void* remainders, unsigned field_id,
                                  const void* polynomial, const void* folded, uint64_t n,
                                  unsigned num_variables, const void* q, const void* points,
                                  unsigned num_points, void* workspace, uint64_t workspace_bytes,
                                  void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* BLITZAR_AMD_BLITZAR_AMD_H */
