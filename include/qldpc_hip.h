/*
 * qldpc_hip.h -- C ABI of the MI355X (gfx950) qLDPC decoding / Monte-Carlo library.
 *
 * This is the drop-in boundary for the hot path of michelebanfi/qLDPC-branched-off: the reference's
 * numba @njit kernels (src/decoding/kernels.py, src/noise/kernels.py) are what these entry points
 * replace; the reference's Python wrappers (src/decoding/{sparse,dense,osd}.py, src/noise/simulation.py,
 * src/simulation/engine.py) keep their names and call through ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.
 *   - every function returns int: 0 = QLDPC_OK, negative = error; text via qldpc_last_error()
 *     (thread-local).  Kernels never "raise": non-convergence is an output value, as in the reference.
 *   - the caller owns every buffer; the library owns only opaque handles and its device workspaces.
 *   - *_dev variants take DEVICE pointers (hipMalloc'ed or torch CUDA tensors' data_ptr()) and a
 *     hipStream_t passed as void* (NULL = default stream); they enqueue work and do not synchronise
 *     (alpha tables are cached per graph handle: a schedule is uploaded the first time it is seen, asynchronously).
 *     The variants without _dev take HOST pointers, copy in/out and return when results are ready.
 *   - every entry point selects its handle's device for the duration of the call and restores the caller's
 *     current device before returning.
 *   - a graph handle owns device workspaces shared by every decode / OSD call on it; calls on different streams
 *     are ordered through an event (the later one waits for the earlier one's kernels), so concurrent streams are
 *     safe but serialise per graph handle.  Use one handle per stream for real concurrency.
 *   - there is NO CPU fallback: without a gfx950 device every compute entry point fails with
 *     QLDPC_ERR_NO_DEVICE.
 *   - matrices over GF(2) are CSR with sorted column indices (int32 indptr[m+1], indices[nnz]).
 *   - batched arrays are shot-major: syndromes[B][m], errors[B][n], llr[B][n].
 *
 * Changelog (qldpc_version)
 *   100  the C ABI of the BP+OSD decoder and the Monte-Carlo plans
 *   101  Relay-BP: qldpc_relay_decode_batch[_dev], qldpc_circuit_plan_use_relay; tally slots QLDPC_TALLY_LEGS_Z / _X
 *        additive, same version: OSD-CS, qldpc_osdcs_batch[_dev] and qldpc_circuit_plan_use_osd_cs
 *        additive, same version: qldpc_minsum_decode_path (which decoder form a call takes), QLDPC_PATH_* and QLDPC_DETAIL_*
 *        additive, same version (the suites pin 101): sliding-window decoding, qldpc_window_decoder_*, qldpc_window_decode_batch[_dev],
 *        qldpc_circuit_plan_use_window
 *        additive, same version: layered-schedule min-sum, qldpc_layered_decoder_*, qldpc_layered_decode_batch[_dev], qldpc_check_layers,
 *        qldpc_circuit_plan_use_layered, QLDPC_FLAG_LAYERED_* and QLDPC_LAYERED_FORM_*
 *        additive, same version: BP with guided decimation, qldpc_decim_decode_batch[_dev], qldpc_circuit_plan_use_decimation; the tally slots
 *        QLDPC_TALLY_LEGS_Z / _X also carry its rounds
 *        additive, same version: single-precision (f32) min-sum, qldpc_minsum32_decoder_*, qldpc_minsum32_decode_batch[_dev],
 *        qldpc_circuit_plan_use_f32, QLDPC_FLAG_F32_* and QLDPC_F32_FORM_*
 *        additive, same version: qldpc_osd0_last_path (which OSD-0 kernel the last call on a handle took), QLDPC_OSD_PATH_* and QLDPC_OSD_DETAIL_*
 *        additive, same version (the suites pin 101): circuit plans that sample a detector error model, qldpc_dem_desc and
 *        qldpc_circuit_plan_create_dem
 *        additive, same version: recorded detection events in place of a plan's sampler, qldpc_circuit_plan_set_event_layout,
 *        qldpc_circuit_plan_decode_events[_dev] and qldpc_circuit_plan_unpack_events
 *        additive, same version: qldpc_minsum_decode_path names the resident kernel's instantiation, QLDPC_DETAIL_RES_CDEG8 and QLDPC_DETAIL_RES_CPT2
 *        additive, same version (the suites pin 101): fixed-weight fault sampling on a circuit plan, qldpc_circuit_plan_use_fixed_weight,
 *        QLDPC_FIXED_WEIGHT_MAX and QLDPC_FIXED_WEIGHT_MAX_LOCS
 *        additive, same version: BP+LSD, qldpc_lsd_batch[_dev], qldpc_circuit_plan_use_lsd and qldpc_circuit_plan_lsd_counts
 *        additive, same version: min-sum with a per-shot prior and correlated two-sector decoding, qldpc_shotprior_decode_batch[_dev] and
 *        qldpc_circuit_plan_use_correlated
 *        additive, same version: heralded-erasure noise and erasure-aware decoding on a circuit plan, qldpc_erasure_priors[_dev],
 *        qldpc_circuit_plan_use_erasure_noise, _use_erasure_aware and _sample_erasures, QLDPC_ERASURE_H_INF
 *        additive, same version: per-class, biased Pauli noise on a circuit plan, qldpc_noise_model and qldpc_circuit_plan_use_noise_model
 *        additive, same version: soft-readout noise and soft-information decoding on a circuit plan, qldpc_soft_priors[_dev],
 *        qldpc_circuit_plan_use_soft_readout, _use_soft_aware and _sample_soft, QLDPC_SOFT_MAX_LEVELS
 *        additive, same version: LSD cluster statistics and the confidence of a trial, qldpc_lsd_stats_batch[_dev],
 *        qldpc_circuit_plan_use_confidence, _confidence_read, _run_scores and _decode_events_scored[_dev], QLDPC_CONF_*
 */
#ifndef QLDPC_HIP_H
#define QLDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLDPC_OK 0
#define QLDPC_ERR_INVALID (-1)    /* bad argument (NULL, negative size, unsorted CSR, ...) */
#define QLDPC_ERR_NO_DEVICE (-2)  /* no usable gfx950 device / HIP runtime error at init     */
#define QLDPC_ERR_HIP (-3)        /* a HIP runtime call failed                              */
#define QLDPC_ERR_UNSUPPORTED (-4)

/* alpha schedule of the normalised min-sum (selection rules live in the Python wrappers,
 * src/decoding/sparse.py:18-29):  CONST: alpha_k = alpha_val (kernels.py:275);
 * DYNAMIC: alpha_k = 1 - 2^-(k+1) (kernels.py:273);  SEQ: alpha_k = seq[min(k,len-1)] (kernels.py:402-405). */
#define QLDPC_ALPHA_CONST 0
#define QLDPC_ALPHA_DYNAMIC 1
#define QLDPC_ALPHA_SEQ 2

/* decode flags */
#define QLDPC_FLAG_FIXED_ITERS 0x1   /* execute all max_iter iterations for every shot; outputs are still
                                        frozen at each shot's first converged iteration (identical results) */
#define QLDPC_FLAG_KERNEL_STREAM 0x10   /* force the HBM-streaming kernel (any graph size)            */
#define QLDPC_FLAG_KERNEL_RESIDENT 0x20 /* force the LDS/register-resident kernels (small graphs only) */
#define QLDPC_FLAG_KERNEL_GENERIC 0x40  /* resident family: use the generic (irregular-degree) kernel even for regular graphs */
#define QLDPC_FLAG_MC_UNFUSED 0x80      /* Monte-Carlo plans: separate sample / decode / judge launches instead of the fused kernel */
/* size-class selectors of the product library (parity tests force every class on small inputs; results are identical whichever runs) */
#define QLDPC_FLAG_OSD_LDS 0x20000      /* OSD-0: the row-transform kernel even for small matrices (m <= 128, n <= 1024), which otherwise take the
                                           literal one-wave-per-shot elimination */
#define QLDPC_FLAG_WG_VGLOBAL 0x100     /* workgroup-per-shot decoder: posteriors in HBM/L2 even when they fit LDS (the large-graph form) */
#define QLDPC_FLAG_WG_GENERIC 0x200     /* workgroup-per-shot decoder: the any-input kernel even for host-verified clean inputs */
#define QLDPC_FLAG_OSD_REFORDER 0x80000 /* OSD-0, m <= 1024: every shot through the kernel that follows the reference's row choice at each pivot (by default
                                          only the shots whose right-hand side lies outside the column space take it; the others cannot tell) */
#define QLDPC_FLAG_OSD_UG 0x400         /* OSD-0: row transform in HBM/L2 even when it fits LDS (the m > 1024 form) */
#define QLDPC_FLAG_OSD_GLOBAL 0x800     /* OSD-0: the literal global-memory elimination (general fallback) */
#define QLDPC_FLAG_WG_TABLES 0x200000   /* workgroup-per-shot decoder: the form with its index tables in HBM/L2 (csrc/minsum_wg.hip; what the *_dev entry points always run)
                                          even when the prior is known on the host and the LDS-resident form (csrc/minsum_wg2.hip) applies */
#define QLDPC_FLAG_WG_ROWMAJOR 0x8000   /* workgroup-per-shot decoder: natural row / column order instead of the degree-sorted assignment */
#define QLDPC_FLAG_CLOCK_PROBE 0x4000   /* plans: workgroups stamp s_memtime / s_memrealtime around their work (see *_plan_clock) */
/* layered decoder (qldpc_layered_decoder_create): form selectors for tools/ and the parity tests; results never depend on them */
#define QLDPC_FLAG_LAYERED_BLOCK_256 0x400000    /* threads per workgroup (default: by the edges of an average layer); at most one of the three */
#define QLDPC_FLAG_LAYERED_BLOCK_512 0x800000
#define QLDPC_FLAG_LAYERED_BLOCK_1024 0x1000000
#define QLDPC_FLAG_LAYERED_GLOBAL_IDX 0x2000000  /* column indices in HBM/L2 even when they fit LDS */
#define QLDPC_FLAG_LAYERED_VGLOBAL 0x4000000     /* posteriors in HBM/L2 even when they fit LDS */
/* f32 decoder (qldpc_minsum32_decoder_create): form selectors for tools/ and the parity tests; results never depend on them */
#define QLDPC_FLAG_F32_GENERIC 0x1000            /* the any-input kernel even for host-verified clean inputs */
#define QLDPC_FLAG_F32_BLOCK_256 0x2000          /* threads per workgroup (default: by size and the occupancy query); at most one of the three */
#define QLDPC_FLAG_F32_BLOCK_512 0x10000
#define QLDPC_FLAG_F32_BLOCK_1024 0x8000000
/* measured-and-rejected kernels: libqldpc_hip_experiments.so only (make -C csrc experiments; same ABI, loaded by the parity tests).  The product
 * library answers these with QLDPC_ERR_UNSUPPORTED.  Numbers: profiles/r02_osd_experiments.txt, r02_bp_lane_mapping.txt, r03_wave_kernel.txt */
#define QLDPC_FLAG_WG_EDGE_LANES 0x2     /* workgroup-per-shot decoder: check pass with 16 lanes per check and shuffle reductions (SURVEY 7-6 option B) */
#define QLDPC_FLAG_WG_IDXLOAD 0x40000    /* workgroup-per-shot decoder: reload the row's column indices every iteration (m <= 1024 keeps them in registers) */
#define QLDPC_FLAG_OSD_QUEUE 0x100000     /* OSD-0, 897 <= m <= 1024: the free-pivot kernel with a look-ahead queue of reduced columns (csrc/osd_gjq.hip) */

/* tally slots written by the *_sample_decode_tally entry points (int64[QLDPC_TALLY_SLOTS]);
 * replaces the Python tally loop of src/simulation/engine.py:450-457 */
#define QLDPC_TALLY_SLOTS 16
#define QLDPC_TALLY_TRIALS 0
#define QLDPC_TALLY_Z_ERR 1       /* code capacity: logical errors of the single decoded sector */
#define QLDPC_TALLY_X_ERR 2
#define QLDPC_TALLY_TOTAL_ERR 3
#define QLDPC_TALLY_BP_CONV_Z 4
#define QLDPC_TALLY_BP_CONV_X 5
#define QLDPC_TALLY_OSD_Z 6
#define QLDPC_TALLY_OSD_X 7
#define QLDPC_TALLY_ITERS_Z 8     /* sum over shots of (final_iter + 1) = iterations executed under reference semantics */
#define QLDPC_TALLY_ITERS_X 9
#define QLDPC_TALLY_ZERO_SYND_Z 10
#define QLDPC_TALLY_ZERO_SYND_X 11
#define QLDPC_TALLY_UNSAT_Z 12    /* decoder output (after OSD if enabled) does not reproduce the syndrome */
#define QLDPC_TALLY_UNSAT_X 13
#define QLDPC_TALLY_LEGS_Z 14     /* Relay-BP: legs; decimation: rounds -- summed over the trials of a circuit plan (0 on every other path) */
#define QLDPC_TALLY_LEGS_X 15

typedef struct qldpc_graph qldpc_graph; /* Tanner graph: host CSR + CSC (ascending check order) + device copies */

const char *qldpc_last_error(void);
int qldpc_version(void);
/* number of usable HIP devices (0 when none; never fails) */
int qldpc_device_count(void);
/* Process-wide kernel-selection switches for tools/ and the parity tests.  Results never depend on them (every selectable path is checked
 * against the same fixtures); the defaults are what bench.py measures.  New here (the reference has no counterpart).
 *   "mc_first_iteration"  reference-semantics Monte-Carlo plans: 1 (default) = bit-sliced first iteration (csrc/mc_first.hip) + the full decoder
 *                         on the shots it lists, 0 = the full decoder for every shot
 *   "mc_first_bits"       shots per lane of that kernel: 8 (default), 16, 32
 *   "osd_presort"         read at an OSD-0 launch: how many columns of the |llr| order the free-pivot OSD-0 kernels sort up front (default -1 = automatic, about m; the rest is
 *                         ordered only when a sweep gets that far; 0 = everything up front)
 *   "mc_tail_overlap"     read at plan creation: 1 (default) = whole batches on the plan's own streams so that the latency-bound pieces of one batch run
 *                         beside the next batch's first kernel (3 streams for large batches under reference semantics, 8 for batches <= 32768; fixed-work
 *                         plans with large batches keep the caller's stream), 2 = only OSD-0 + judge on a side stream, 0 = everything on the caller's stream
 *   "mc_big_lanes"        streams whole batches rotate over under reference semantics with large batches: 2 .. 8 (default 3)
 *   "mc_list_shots"       shots per workgroup of the full decoder on listed shots: 0 (default: the kernel's own 7), 1 .. 16
 *   "regular_own_edges"   read at a launch of the regular min-sum kernel: 1 (default) = on clean inputs and a (6,3)-regular graph the thread of a check is the
 *                         variable thread of two of its own columns (csrc/regular_own.h), 0 = the body without ownership on every graph
 *   "regular_own_search"  read by qldpc_graph_create: 1 (default) = of the valid assignments of those columns the one whose gathers the LDS bank model of
 *                         csrc/regular_own.h prices lowest, 0 = the first matching found
 *   "regular_place"       read at a fixed-work launch of that form: 1 (default) = every thread takes the LDS addresses of its posteriors and messages from the placement of
 *                         csrc/regular_place.h (edge colouring: the gathers and the message stores free of bank conflicts), built at the handle's first
 *                         launch with a workgroup shape; 0 = the linear layout, through the same kernel
 *   "regular_wave_classes" read with "regular_place" 1: 1 (default) = that table is built from the assignment that owns the fewest `last` edges and deals the
 *                         threads of a workgroup so that whole waves share one class of them; such a wave runs the fixed-work loop without selects.
 *                         0 = the assignment of "regular_own_search" in thread order, every wave on the loop with selects.  No output word depends on it
 *   "regular_kernel", "wave_cpl", "wave_rst", "wave_grid"  experiments build only: the wave-private decoder (csrc/minsum_wave.hip); the
 *                         product library accepts 0 and answers anything else with QLDPC_ERR_UNSUPPORTED */
int qldpc_set_option(const char *name, int value);
/* A stream of `device` for the `stream` arguments below (a host without PyTorch that drives several plans -- one per device, or several on one
 * device -- gives each its own; NULL there means the device's default stream).  New here: the reference's counterpart is the worker process
 * of its pool (src/simulation/engine.py:433-435).  qldpc_stream_sync blocks until everything enqueued on it has finished. */
int qldpc_stream_create(int device, void **stream);
int qldpc_stream_sync(int device, void *stream);
int qldpc_stream_destroy(int device, void *stream);

/* Build a Tanner-graph handle on `device`.  Validates the CSR (monotone indptr, 0 <= col < n, strictly
 * increasing columns per row) and derives the CSC view with per-column ASCENDING check order, which is what
 * reproduces the reference's scatter-add order R_sum[col] += msg (kernels.py:316).  Immutable afterwards. */
int qldpc_graph_create(int m, int n, const int32_t *indptr, const int32_t *indices, int device, qldpc_graph **out);
void qldpc_graph_destroy(qldpc_graph *g);
int qldpc_graph_dims(const qldpc_graph *g, int *m, int *n, int *nnz);

/* a1 + a2: minsum_decoder_full (src/decoding/kernels.py:234-366) and minsum_decoder_full_autoregressive
 * (kernels.py:369-485), batched over B independent syndromes.  B = 1 backs performMinSum_Symmetric_Sparse
 * (src/decoding/sparse.py:5-54).  Outputs per shot: candidateError int8[n], converged, values f64[n],
 * final_iter (max_iter-1 when not converged).  alpha_seq may be NULL unless alpha_mode == SEQ. * The host-pointer form accepts out_llr == NULL: the posteriors (8n of the 9n + 5 result bytes per shot) are then not copied back.
 */
int qldpc_minsum_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior,
                              int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len,
                              double damping, double clip_llr, int flags,
                              int8_t *out_err, double *out_llr, uint8_t *out_conv, int32_t *out_iter);
int qldpc_minsum_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior,
                                  int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len,
                                  double damping, double clip_llr, int flags,
                                  int8_t *d_out_err, double *d_out_llr, uint8_t *d_out_conv, int32_t *d_out_iter,
                                  void *stream);

/* Which decoder form qldpc_minsum_decode_batch (host prior != NULL) resp. qldpc_minsum_decode_batch_dev (prior == NULL) runs for these arguments.
 * Launches no kernel, but builds and caches the same tables the decode call would: with a host prior the handle has not seen it may upload the tables
 * of the LDS-resident form, and on the fifth distinct prior it waits for the device (hipDeviceSynchronize) and drops the four cached sets first, exactly
 * as the decode call does.  Returns what the decode call would return for arguments it refuses (QLDPC_ERR_UNSUPPORTED).  The query and the launchers
 * share one selection function, and results never depend on the form.  New here (the reference has no counterpart).
 *   path    QLDPC_PATH_*: REGULAR csrc/minsum_regular.hip, RESIDENT minsum_resident.hip, WG2 minsum_wg2.hip (workgroup per shot, every table in LDS),
 *           WG minsum_wg.hip (workgroup per shot, tables in HBM / L2), STREAM minsum_stream.hip, WAVE minsum_wave.hip (experiments build only)
 *   detail  QLDPC_DETAIL_* bits of the two workgroup forms; for QLDPC_PATH_RESIDENT the kernel instantiation (QLDPC_DETAIL_RES_* and
 *           QLDPC_DETAIL_DAMPING); 0 for the others */
#define QLDPC_PATH_REGULAR 0
#define QLDPC_PATH_RESIDENT 1
#define QLDPC_PATH_WG2 2
#define QLDPC_PATH_WG 3
#define QLDPC_PATH_STREAM 4
#define QLDPC_PATH_WAVE 5
#define QLDPC_DETAIL_LEAN 0x1            /* the clean-input kernel (WG2: always) */
#define QLDPC_DETAIL_REG_INDICES 0x2     /* a thread keeps its row's column indices in registers (WG2: always) */
#define QLDPC_DETAIL_VGLOBAL 0x4         /* posteriors in global memory, by size or by QLDPC_FLAG_WG_VGLOBAL */
#define QLDPC_DETAIL_DAMPING 0x8         /* damping != 1: the previous messages in a global-memory slab */
#define QLDPC_DETAIL_BLOCK_1024 0x10     /* 1024 threads per workgroup (else 512; WG2: always) */
#define QLDPC_DETAIL_DEG1 0x20           /* the graph has degree-1 checks: the kernel instance that carries their +-inf messages */
#define QLDPC_DETAIL_NAN_DEG1_ONLY 0x40  /* no column meets two degree-1 checks: only they can make a NaN, and only their waves test for it */
#define QLDPC_DETAIL_RES_CDEG8 0x80      /* resident kernel: the (8,4) instance (a row of degree 7 or 8, or a column of degree 4), else (6,3) */
#define QLDPC_DETAIL_RES_CPT2 0x100      /* resident kernel: a thread owns two rows and four columns (team beyond 256 threads), else one and two */
int qldpc_minsum_decode_path(const qldpc_graph *g, const double *prior, int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq,
                             int alpha_len, double damping, double clip_llr, int flags, int *path, int *detail);

/* a3: minsum_core_sparse (kernels.py:138-169): one check-node pass; Q[B][nnz], syndrome_sign[B][m] (+-1.0)
 * -> R[B][nnz], R_sum[B][n].  B = 1 is the reference call. */
int qldpc_minsum_check_pass(const qldpc_graph *g, int64_t B, const double *Q, const double *syndrome_sign, double alpha,
                            double *R, double *R_sum);
/* a5: bp_core (kernels.py:171-193) on the same CSR edge layout: tanh-product rule, clip_val = 0.9999999 */
int qldpc_bp_check_pass(const qldpc_graph *g, int64_t B, const double *Q, const double *syndrome_sign, double clip_val,
                        double *R, double *R_sum);
/* a5 driver: performBeliefPropagationFast (src/decoding/dense.py:75-96), batched */
int qldpc_bp_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, int max_iter,
                          int8_t *out_err, double *out_llr, uint8_t *out_conv, int32_t *out_iter);

/* Relay-BP (Mueller et al. 2025): normalised min-sum (constant alpha, messages clipped to +-clip_llr) with a per-variable memory
 * term, run in legs.  The variable pass of a leg writes V_j = sum_R + ((1 - gamma_j) * prior_j + gamma_j * V_j)
 * (a V_j that is not finite, as the +-inf messages of degree-1 checks make it, enters that term as 0.0).  Leg 0 runs t0
 * iterations from V = prior with gamma_j = gamma0; leg r = 1..max_legs runs tr iterations from the previous leg's final marginals
 * with gamma_j = gamma_min + (gamma_max - gamma_min) * (w / 2^16), w = the top 16 bits of word (j & 3) of
 * Philox4x32-10(ctr = {lo32(shot), hi32(shot), j >> 2, 0x52000000 | tag << 20 | r}, key = {lo32(seed), hi32(seed)}), shot = shot_begin + b.
 * Every converged leg is a solution of weight sum_{j: e_j = 1} floor(prior_j * 2^20 + 0.5) (int64; the product clamped to +-2^40);
 * the lightest one is kept (the earlier leg wins ties); the decoder stops after stop_after solutions or after leg max_legs.
 * Outputs per shot: err int8[n] (the best solution, else the last leg's hard decision), conv (>= 1 solution), legs (1..1 + max_legs),
 * iters (sum over legs of the iteration counts: it if the leg converged at it, else its length), solutions (converged legs).
 * Arguments: prior finite; alpha, clip_llr finite > 0; gammas finite with gamma_min <= gamma_max; t0, tr >= 1; 0 <= max_legs < 2^20;
 * stop_after >= 1; tag in 0..15; B = 0 is a no-op.  QLDPC_ERR_UNSUPPORTED for graphs with a row degree above 56 or whose check
 * state does not fit in LDS.  Results depend only on (seed, shot, tag, inputs): not on batch splits or the grid. */
int qldpc_relay_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, double alpha, double clip_llr,
                             double gamma0, double gamma_min, double gamma_max, int t0, int tr, int max_legs, int stop_after, uint64_t seed,
                             int64_t shot_begin, int tag, int8_t *err, uint8_t *conv, int32_t *legs, int32_t *iters, int32_t *solutions);
/* same on device pointers; only enqueues on `stream`.  Precondition: every d_prior entry is finite (not checked: it lives on the device). */
int qldpc_relay_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior, double alpha,
                                 double clip_llr, double gamma0, double gamma_min, double gamma_max, int t0, int tr, int max_legs,
                                 int stop_after, uint64_t seed, int64_t shot_begin, int tag, int8_t *d_err, uint8_t *d_conv, int32_t *d_legs,
                                 int32_t *d_iters, int32_t *d_solutions, void *stream);

/* BP with guided decimation (BPGD; Yao, Laird, Gokduman, Pfister et al. 2024).  New here: the reference has no counterpart.  Constant-alpha
 * normalised min-sum in rounds of t_round iterations; after a round that did not converge the most reliable undecided columns are frozen to
 * their hard decision by replacing their prior with +-fix_llr.  No elimination, no random numbers.
 * Arguments: prior[n] finite (checked in the host entry; a precondition of the _dev entry); alpha, clip_llr, fix_llr finite and > 0;
 * t_round >= 1; 0 <= max_rounds < 2^20; 1 <= per_round <= 64; B = 0 is a no-op.  Per shot:
 *   1. bias_j = prior_j and V_j = prior_j; no column is fixed.
 *   2. Round r = 0 .. max_rounds runs exactly one leg of Relay-BP (qldpc_relay_decode_batch) with T = t_round, gamma_j = 0 and bias_j in
 *      place of prior_j: the check state is rebuilt at the round's first pass (it = 0) from Q = V; from it = 1 on Q = V - R with a NaN
 *      becoming 0.0 and the result clipped to +-clip_llr; the minima, signs and alpha * min of the flooding decoder; s_j = 0.0 + the sum of
 *      R in ascending check order; V_j = s_j + bias_j (each one correctly rounded f64 operation, nothing contracted).  Convergence
 *      (H (V < 0) = s over every row) is tested at it >= 1 on V; the round's iteration count is it if it converged at it, else T.
 *   3. If the round converged, stop: conv = 1.
 *   4. Otherwise, if r == max_rounds or no column is unfixed, stop: conv = 0.
 *   5. Otherwise decimate: the unfixed columns are keyed by a_j = |V_j| (a NaN counts as 0, +inf is the largest) and ordered by a_j
 *      descending, then by ORIGINAL column index ascending; the first min(per_round, #unfixed) of them become fixed, each with
 *      bias_j = (V_j < 0) ? -fix_llr : +fix_llr and V_j = bias_j.  Everything else in V stays, and the next round starts from there.
 *   6. Outputs: err[j] = V_j < 0; llr = V (f64[n], the posteriors qldpc_osd0_batch / qldpc_osdcs_batch read; may be NULL in the host entry);
 *      conv uint8; iters = the sum of the rounds' iteration counts; rounds = rounds run, 1 .. 1 + max_rounds; fixed = columns fixed.
 *      rounds and fixed may be NULL.
 *   7. max_rounds = 0 is qldpc_relay_decode_batch(max_legs = 0, gamma0 = 0, t0 = t_round) bit for bit: constant-alpha min-sum.
 * A frozen column is not immune: its marginal is s_j +- fix_llr, and |s_j| <= (column degree) * alpha * clip_llr on a graph without
 * degree-1 checks, so fix_llr above that bound keeps its hard decision for good.
 * QLDPC_ERR_UNSUPPORTED for a graph Relay-BP refuses (a row degree above 56, no slot tables, its own LDS count) and for one whose state does
 * not fit in 160 KB of LDS by BPGD's own count: 24 bytes per check, two bit planes (fixed, sign) of ceil(n / 32) 32-bit words, each padded to
 * 16 bytes, 16 bytes of flags and 384 bytes of per-wave selection candidates; 8 bytes per column on top keep the posteriors in LDS, else
 * they live in global memory.  Relay-BP counts 2 bytes per column (its memory draws, n rounded up to 4) and 32 bytes of flags in place of the
 * planes and candidates, so the two counts differ in either direction: at m = 300 BPGD keeps the posteriors in LDS up to n = 18938,
 * Relay-BP up to n = 15660; at n = 64 BPGD accepts m <= 6808, Relay-BP m <= 6820.  QLDPC_ERR_INVALID for the arguments above.  Results
 * depend only on the inputs: not on batch splits, the grid or the order of the shots. */
int qldpc_decim_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, double alpha, double clip_llr,
                             int t_round, int max_rounds, int per_round, double fix_llr, int8_t *err, double *llr, uint8_t *conv,
                             int32_t *iters, int32_t *rounds, int32_t *fixed);
/* same on device pointers (d_rounds / d_fixed may be NULL, d_llr not); only enqueues on `stream`.  Precondition: every d_prior entry is finite. */
int qldpc_decim_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior, double alpha,
                                 double clip_llr, int t_round, int max_rounds, int per_round, double fix_llr, int8_t *d_err, double *d_llr,
                                 uint8_t *d_conv, int32_t *d_iters, int32_t *d_rounds, int32_t *d_fixed, void *stream);

/* Min-sum with a prior that differs per shot, and the reweighting step of correlated two-sector decoding.  New here: the reference has no
 * counterpart.  Soft measurement information, heralded erasures and any re-weighting scheme enter through `prior`; the link tables let the
 * correction of ANOTHER decoding problem (src_err: sector 0 of a circuit plan) raise the probability of columns of this one.
 * Per-shot prior.  For shot b and column j of a graph with n columns:
 *     P[b][j] = min( prior[b * prior_stride + j],
 *                    min{ link_llr[l] : link_ptr[j] <= l < link_ptr[j + 1], src_err[b * n_src + link_src[l]] == 1 } )
 *   prior_stride is 0 (one prior[n] for every shot) or n (prior[B][n]).  src_err is int8[B][n_src]; link_ptr int32[n + 1] with link_ptr[0] = 0,
 *   monotone; link_src int32[link_ptr[n]], 0 <= link_src < n_src, strictly ascending inside a column's run; link_llr f64[link_ptr[n]].  src_err and
 *   the three tables are all NULL (then P is the prior as given and n_src is not used) or all given.  Every prior and link_llr value must be
 *   finite, of any sign: the host-pointer entry checks it, for the _dev entry it is a precondition (as the table rules are).  A minimum of finite
 *   doubles involves no rounding and no order, so the result does not depend on the order in which a run is walked.
 * Decode.  Shot b is decoded exactly as one round of qldpc_decim_decode_batch with nothing frozen: V = P[b], then one leg of max_iter iterations
 *   with bias_j = P[b][j], the constant alpha and the messages clipped to +-clip_llr (steps 1 and 2 there: same operations, same order).  With
 *   prior_stride = 0 and no tables the outputs equal qldpc_decim_decode_batch(max_rounds = 0, t_round = max_iter) word for word.
 * Outputs per shot: err int8[n] = V < 0; llr f64[n] = V (may be NULL); conv; iters (the iteration at which V reproduced the syndrome, else
 *   max_iter); prior_out f64[n] = the P[b] the shot was decoded with (may be NULL).
 * Arguments: alpha, clip_llr finite and > 0; max_iter >= 1; B = 0 is a no-op.  QLDPC_ERR_INVALID for these, a prior_stride other than 0 or n, a
 *   value that is not finite or a table that breaks a rule above (the error text names the offending index); nothing is written then.
 * QLDPC_ERR_UNSUPPORTED, before any launch, for a graph without slot tables (n >= 65535 or a row degree >= 256), with a row degree above 56, or
 *   whose check state does not fit in 160 KB of LDS: 24 bytes per check and 16 bytes of flags.  On top, with link tables, 8 bytes per column keep V
 *   in LDS and 8 more keep P there (mode 1); when both do not fit P lives in a per-workgroup slab in global memory (mode 2), and when V alone does
 *   not fit either, both do (mode 3).  Without tables there is no P to keep: the bias reads the prior where it is.  Results never depend on the mode,
 *   on batch splits, the grid or the order of the shots. */
int qldpc_shotprior_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, int64_t prior_stride,
                                 int32_t n_src, const int8_t *src_err, const int32_t *link_ptr, const int32_t *link_src,
                                 const double *link_llr, double alpha, double clip_llr, int max_iter, int8_t *err, double *llr,
                                 uint8_t *conv, int32_t *iters, double *prior_out);
/* same on device pointers (d_llr / d_prior_out may be NULL); only enqueues on `stream`.  Preconditions: finite d_prior and d_link_llr, tables that
 * keep the rules above. */
int qldpc_shotprior_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior, int64_t prior_stride,
                                     int32_t n_src, const int8_t *d_src_err, const int32_t *d_link_ptr, const int32_t *d_link_src,
                                     const double *d_link_llr, double alpha, double clip_llr, int max_iter, int8_t *d_err, double *d_llr,
                                     uint8_t *d_conv, int32_t *d_iters, double *d_prior_out, void *stream);

/* a6: GF(2) syndrome SpMV  s = H e (kernels.py:222-231, 352-359; H_csr.dot(e)%2 in alpha.py:128): vectors[B][n] -> out[B][m] */
int qldpc_gf2_spmv_batch(const qldpc_graph *g, int64_t B, const int8_t *vectors, int8_t *out);
/* same on device pointers; only enqueues on `stream` (hipStream_t) */
int qldpc_gf2_spmv_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_vectors, int8_t *d_out, void *stream);

/* a7: gf2_elimination (kernels.py:5-34): Gauss-Jordan on B byte matrices A[B][m][n] (0/1), b[B][m], in place.
 * pivot_rows/pivot_cols: int64[B][min(m,n)], num_pivots int32[B].  One workgroup per matrix with 5 m + 8 nwords + 40 bytes of LDS scratch:
 * QLDPC_ERR_UNSUPPORTED above 150 KiB (m > 30710 at one row word), for this entry point and the packed one. */
int qldpc_gf2_eliminate(int64_t B, int m, int n, uint8_t *A, uint8_t *b, int64_t *pivot_rows, int64_t *pivot_cols,
                        int32_t *num_pivots);
/* a8: gf2_elimination_packed_core (kernels.py:48-96) on rows packed little-endian into uint64 words
 * (layout of _pack_rows_uint64, kernels.py:36-46): A[B][m][nwords], in place. */
int qldpc_gf2_eliminate_packed(int64_t B, int m, int n, int nwords, uint64_t *A, uint8_t *b, int64_t *pivot_rows,
                               int64_t *pivot_cols, int32_t *num_pivots);
/* a9: performOSD_enhanced with order = 0 (src/decoding/osd.py:5-29), batched over B shots of one graph.
 * ordering (int32[B][n], may be NULL): column order to eliminate in; NULL = ascending |llr| with ties broken by
 * ascending index (np.argsort's default kind leaves ties implementation-defined, osd.py:12). solution int8[B][n]. */
int qldpc_osd0_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard,
                     const int32_t *ordering, int flags, int8_t *solution);
/* same on device pointers; only enqueues on `stream`.  d_select / d_select_count (both NULL = all B shots): device list of the shots to
 * solve and its device-resident length, e.g. the shots qldpc_minsum_decode_batch_dev left unconverged -- the decode -> OSD-0 hand-over of
 * src/simulation/engine.py:96-97 without a host round trip.  Shots not listed keep whatever d_solution holds. */
int qldpc_osd0_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard,
                         const int32_t *d_ordering, const int32_t *d_select, const int32_t *d_select_count, int flags, int8_t *d_solution,
                         void *stream);
/* Which OSD-0 kernel the last OSD-0 launch on this handle took: qldpc_osd0_batch[_dev], or the OSD-0 stage of a plan or window decoder that owns the
 * handle.  Launches nothing; the values are those of the plan (csrc/osd_plan.h) the launch code executed, written by that code once it has
 * enqueued the plan's kernels, so the query cannot drift from what ran.  Results never depend on the form.  With several threads on one handle it
 * reports whichever call enqueued last.  New here (the reference has no counterpart); for tests and tools.
 *   path    QLDPC_OSD_PATH_*: the kernel that was given every listed shot.  NONE: nothing was launched (no call yet, m == 0 or n == 0, or the call
 *           was refused); SMALL csrc/osd_small.hip (one wave per shot, m <= 128 and n <= 1024); GJ csrc/osd_gj.hip (free pivot rows, row transform in
 *           LDS, m <= 1024); GJG csrc/osd_gjg.hip (the same with the transform in HBM / L2, m <= 4096); REFORDER_LDS / REFORDER_UG osd0_lds_kernel of
 *           csrc/gf2.hip (the reference's row choice at every pivot; transform in LDS / in HBM / L2) on every shot, as QLDPC_FLAG_OSD_REFORDER asks for
 *           or when a heavy column leaves the free-pivot kernels no room in LDS; GLOBAL osd0_kernel of csrc/gf2.hip (literal elimination in HBM)
 *   detail  bits 0-1 (QLDPC_OSD_DETAIL_MODE_MASK): the reference-order form the launch planned, 0 none, 1 transform in LDS, 2 in HBM / L2;
 *           QLDPC_OSD_DETAIL_REDO: a second kernel was queued behind GJ / GJG for the shots they list (right-hand side outside the column space):
 *           the reference-order form of bits 0-1, or with mode 0 the GLOBAL kernel on every shot */
#define QLDPC_OSD_PATH_NONE (-1)
#define QLDPC_OSD_PATH_SMALL 0
#define QLDPC_OSD_PATH_GJ 1
#define QLDPC_OSD_PATH_GJG 2
#define QLDPC_OSD_PATH_REFORDER_LDS 3
#define QLDPC_OSD_PATH_REFORDER_UG 4
#define QLDPC_OSD_PATH_GLOBAL 5
#define QLDPC_OSD_DETAIL_MODE_MASK 0x3
#define QLDPC_OSD_DETAIL_REDO 0x4
int qldpc_osd0_last_path(const qldpc_graph *g, int *path, int *detail);
/* Phase counters of the OSD-0 kernels and of the workgroup BP kernel on the current device (uint64[32]; layout in csrc/clocks.h).  Only the diagnostic build
 * (make -C csrc timers) counts; the product build carries no clock reads and returns QLDPC_ERR_UNSUPPORTED. */
int qldpc_osd_timers_read(uint64_t *out32, int reset);
/* f1: performOSD_enhanced(H, syndrome, llr, hard, order, max_combinations) (src/decoding/osd.py:5-77), batched.  The OSD-0 solution is
 * returned whenever it reproduces the syndrome (osd.py:27-29); otherwise the <= C(order+10, <= order) flip sets over the least
 * reliable non-pivot positions are scored with recompute_solution / compute_metric (src/decoding/kernels.py:195-219) and the
 * reference's selection rule.  max_combinations <= 0: no limit (Python None).  order <= 10; at most 65536 flip sets per shot
 * (QLDPC_ERR_UNSUPPORTED beyond, use max_combinations).  Ties of |llr|: ascending index (see qldpc_osd0_batch). */
int qldpc_osdw_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard,
                     const int32_t *ordering, int order, int64_t max_combinations, int8_t *solution);
/* OSD-CS: OSD-0 followed by a combination sweep (Roffe et al. 2020), batched over B shots of one graph.  Per shot, with the BP posteriors
 * llr and their hard decision hard (the OSD-0 hand-over) and per-column weights w[n] (finite, the same for every shot):
 *   q_j = floor(w_j * 2^20 + 0.5) (the product clamped to +-2^40) as int64; the cost of x is W(x) = sum_{j : x_j = 1} q_j, exact.
 *   1. order: columns by ascending |llr|, NaN as +inf, ties by ascending index (qldpc_osd0_batch with ordering = NULL);
 *   2. pivots: S = the columns independent of the columns before them in that order, rank = |S|; T = the other n - rank columns in the
 *      same order, T[0] the least reliable;
 *   3. candidates: corrections c with H c = s + H hard, fixed by t = c_T (c_S the unique solution on S).  Candidate 0 is t = {} (its
 *      solution hard ^ c is qldpc_osd0_batch's, bit for bit); candidates 1 .. n - rank are t = {T[i]} for EVERY i; then the pairs
 *      t = {T[a], T[b]}, a < b < order, in lexicographic order of (a, b);
 *   4. selection: the candidate of least W(hard ^ c); ties go to the earlier candidate (so OSD-0 wins every tie);
 *   5. s + H hard outside the column space of H (only a caller's own syndrome can be): exactly qldpc_osd0_batch's answer;
 *   6. flips int32[B][2]: the original column indices of the winner's t (pair: T[a], T[b]), padded with -1; (-1, -1) = OSD-0 kept.
 * 0 <= order <= 64 (order <= 1: no pairs).  m <= 1024 and n <= 65535, else QLDPC_ERR_UNSUPPORTED.  solution int8[B][n]. */
int qldpc_osdcs_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard,
                      const double *weights, int order, int8_t *solution, int32_t *flips);
/* same on device pointers; only enqueues on `stream` (weights are not checked for finiteness here).  d_select / d_select_count as in
 * qldpc_osd0_batch_dev: shots not listed keep whatever d_solution and d_flips hold.  d_solution may alias d_hard. */
int qldpc_osdcs_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard,
                          const double *d_weights, int order, const int32_t *d_select, const int32_t *d_select_count,
                          int8_t *d_solution, int32_t *d_flips, void *stream);
/* BP+LSD: localized statistics decoding (Hillmann et al. 2024) as a post-processor of the OSD hand-over, batched over B shots of one graph.  New
 * here (the reference has no counterpart).  It grows clusters around the unsatisfied checks and solves each on its own small system, so what it
 * needs of a workgroup is set by the cap max_rows and not by m.  Per shot the inputs are syndromes int8[m], llr f64[n] and hard int8[n]; the
 * parameters are bits_per_step (1..64) and max_rows (1..1024).  The key of a column is key(j) = (|llr_j| with NaN as +inf, j), compared
 * lexicographically: qldpc_osd0_batch's order with ordering = NULL.
 *   0. b = s + H hard (mod 2).  b = 0: the solution is hard, flag 0, no rounds.
 *   1. State: A, an ordered list of added columns, empty at first; R, the set of cluster rows, {r : b_r = 1} at first.  The clusters are the
 *      connected components of the bipartite graph on (R, A) with H's edges; each seed row is alone at first.  Every row of an added column is
 *      in R, so a cluster K is VALID iff b restricted to K lies in the span of the columns of A inside K.
 *   2. Round t = 1, 2, ..., on the state at the start of the round: for every invalid cluster K, cand(K) = {j not in A : column j has a row in
 *      K}.  An empty cand(K) ends the shot with flag 2 (the residual is outside the reachable column space).  Otherwise K picks its
 *      min(bits_per_step, |cand(K)|) smallest keys, and N_t is the union of the picks.  If |R u rows(N_t)| > max_rows the shot ends with flag 1
 *      (capped).  Else N_t is appended to A in ascending key order, R takes its rows, and clusters and validity are evaluated again.  The loop
 *      stops when every cluster is valid.
 *   3. Pivots are the columns of A independent of the ones before them in A; c is the unique vector on the pivots with H c = b; the solution is
 *      hard ^ c.  info int32[B][4] = {flag, rounds, |R|, |A|}, the last three 0 when the flag is not 0.
 *   4. Shots with flag 1 or 2 get exactly qldpc_osd0_batch's answer (the OSD-0 kernels run on them behind the cluster kernel).
 * The outcome is a function of sets and of the (round, key) order only: no thread or lane order enters it (tests/lsd_model.py is the model).
 * With bits_per_step = 1 a flag-0 answer was qldpc_osd0_batch's on every recorded circ144 case; larger steps take fewer rounds and may differ.
 * QLDPC_ERR_INVALID for parameters outside their ranges; QLDPC_ERR_UNSUPPORTED for n >= 65535, m > 65535, a layout at max_rows beyond
 * 160 KiB of LDS (csrc/lsd_plan.h), or a matrix qldpc_osd0_batch refuses (step 4 hands shots over to it: its scratch, 5 m + 8 ceil(n / 64)
 * + 40 bytes, passes 150 KiB beyond 30 710 rows at n <= 64 and beyond about 29 070 rows at n = 65 534, csrc/osd_plan.h).  The refusal is decided once, before anything is launched, whether or not a shot would have been
 * handed over: no kernel runs and no output byte is written.  solution int8[B][n]. */
int qldpc_lsd_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard, int bits_per_step,
                    int max_rows, int8_t *solution, int32_t *info);
/* same on device pointers; only enqueues on `stream`.  d_select / d_select_count as in qldpc_osd0_batch_dev: shots not listed keep whatever
 * d_solution and d_info hold.  d_solution may alias d_hard. */
int qldpc_lsd_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard, int bits_per_step,
                        int max_rows, const int32_t *d_select, const int32_t *d_select_count, int8_t *d_solution, int32_t *d_info,
                        void *stream);
/* qldpc_lsd_batch, and the statistics of the clusters each shot ends with: the soft output of BP+LSD (Lee et al., "Efficient post-selection for
 * general quantum LDPC codes", 2025).  New here.  For a shot that ends with flag 0 the clusters are the connected components of (R, A) at
 * termination.  Cluster i has a_i columns of A, r_i rows, and W_i = the sum of weight[j] over its columns; weight is uint16[n], the same for every
 * shot, and may be NULL.  stats uint64[B][8] =
 *   [0] the number of clusters   [1] sum a_i (= info[3])   [2] sum a_i^2   [3] max a_i   [4] sum W_i   [5] sum W_i^2   [6] max W_i   [7] max r_i
 * A shot with zero residual has eight zeros.  A shot that ends with flag 1 or 2 has all eight words 2^64 - 1: "no statement", which ranks behind
 * every statement.  With weight == NULL the words 4 .. 6 are 0.  Nothing overflows: n < 65535 and weight <= 65535 give sum W < 2^32, so
 * sum W_i^2 <= (sum W)^2 < 2^64.  The words are sums and maxima over sets: no thread or lane order enters them (tests/lsd_stats_model.py is the
 * model).  The default weight of a prior is min(65535, rint(|prior_j| * 256)) with NaN as 65535 (quantise_weights of the Python binding): a
 * cluster's W is then its prior weight in units of 1 / 256.  solution and info are qldpc_lsd_batch's, and so are the refusals, with stats == NULL
 * as one more QLDPC_ERR_INVALID. */
int qldpc_lsd_stats_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard, int bits_per_step,
                          int max_rows, const uint16_t *weight, int8_t *solution, int32_t *info, uint64_t *stats);
/* same on device pointers; only enqueues on `stream`.  Shots not listed keep whatever d_solution, d_info and d_stats hold. */
int qldpc_lsd_stats_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard,
                              int bits_per_step, int max_rows, const int32_t *d_select, const int32_t *d_select_count, const uint16_t *d_weight,
                              int8_t *d_solution, int32_t *d_info, uint64_t *d_stats, void *stream);

/* Sliding-window decoding over the row layers of a space-time decoding matrix: min-sum + OSD-0 on W layers at a time, the first C layers
 * of every window committed.  New here (the reference decodes the whole matrix).  The window graphs do not grow with the number of layers,
 * so an experiment of any length runs on the kernels a W-layer matrix takes.
 * Inputs: H = the graph g (m x n), layer_rows (must divide m; Lyr = m / layer_rows), prior[n] (finite, the same for every shot),
 * window = W >= 1, commit = C with 1 <= C <= W, and max_iter, the alpha mode and clip_llr of qldpc_minsum_decode_batch (damping is 1).
 *   1. column layers: tau(j) = the smallest row / layer_rows over the rows of column j; a column without rows has tau = 0;
 *   2. layer span: a column whose rows span more than two consecutive layers (last layer - first layer > 1) is rejected at creation
 *      with QLDPC_ERR_INVALID;
 *   3. windows: window k starts at layer a_k = k C and covers the layers [a_k, min(a_k + W, Lyr)); the last window is the first one with
 *      a_k + W >= Lyr;
 *   4. window graph: the rows of the covered layers and the columns with tau in the covered range, in ascending original index; entries
 *      in rows beyond the window are dropped (only columns of the window's top layer can lose entries); the window prior is the prior of
 *      those columns.  Windows whose CSR and prior slice are equal share one graph handle (compared, not assumed);
 *   5. per shot, running syndrome r = s; for window k in order: (a) qldpc_minsum_decode_batch of the window graph on r restricted to
 *      its rows (the reference's early exit); (b) if it did not converge, qldpc_osd0_batch (ordering = NULL) on its posteriors, including
 *      OSD-0's defined answer for a right-hand side outside the column space -- an earlier commit that differs from the true faults can
 *      leave such a residual; (c) commit the columns with tau in [a_k, a_k + C), in the last window all of its columns: err[j] = the
 *      window's decision; (d) r ^= H[:, committed] e_committed over the FULL columns (at most one layer above the commit region);
 *   6. outputs per shot: err int8[n]; conv = windows in which min-sum converged; iters = sum over windows of (final_iter + 1), what the
 *      circuit plan's judge counts per decode; osd = windows sent to OSD-0; unsat = 1 iff H err != s;
 *   7. with W >= Lyr there is one window, the whole graph: err is qldpc_minsum_decode_batch + qldpc_osd0_batch bit for bit.
 * QLDPC_ERR_UNSUPPORTED for a window without columns.  flags: the QLDPC_FLAG_* selectors of the decode and OSD-0 calls (results never
 * depend on them).  The decoder owns its window graphs and device workspaces; calls on one decoder serialise (a mutex while enqueuing, an
 * event between streams).  qldpc_window_decoder_info: number of windows, of distinct graph handles, rows and columns of the largest window,
 * and how many windows take the LDS-resident workgroup decoder (QLDPC_PATH_WG2); any output may be NULL. */
typedef struct qldpc_window_decoder qldpc_window_decoder;
int qldpc_window_decoder_create(const qldpc_graph *g, int layer_rows, int window, int commit, const double *prior, int max_iter,
                                int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len, double clip_llr, int flags,
                                qldpc_window_decoder **out);
void qldpc_window_decoder_destroy(qldpc_window_decoder *wd);
int qldpc_window_decoder_info(const qldpc_window_decoder *wd, int *windows, int *graphs, int *max_rows, int *max_cols, int *wg2_windows);
/* host pointers: syndromes int8[B][m] -> err int8[B][n], conv / iters / osd int32[B], unsat uint8[B]; returns when they are complete */
int qldpc_window_decode_batch(qldpc_window_decoder *wd, int64_t B, const int8_t *syndromes, int8_t *err, int32_t *conv, int32_t *iters,
                              int32_t *osd, uint8_t *unsat);
/* same on device pointers; only enqueues on `stream` (the first call for a larger B than any before allocates workspaces) */
int qldpc_window_decode_batch_dev(qldpc_window_decoder *wd, int64_t B, const int8_t *d_syndromes, int8_t *d_err, int32_t *d_conv,
                                  int32_t *d_iters, int32_t *d_osd, uint8_t *d_unsat, void *stream);

/* Normalised min-sum with a LAYERED (serial) schedule.  New here: the reference and every other decoder of this library use the flooding
 * schedule.  Inputs: the graph g (m x n), prior[n] (any values, as in qldpc_minsum_decode_batch), row_layer int32[m] or NULL, max_iter >= 1,
 * the alpha mode, value and sequence of qldpc_minsum_decode_batch, clip_llr > 0.  There is no damping argument: damping is 1.
 *   Layers.  row_layer == NULL: rows are taken in ascending index and a row gets the smallest layer number >= 0 that no earlier row sharing a
 *     column with it holds; a row without entries gets layer 0 (qldpc_check_layers returns this colouring).  A caller's row_layer must be
 *     >= 0 everywhere and two rows of one layer must share no column: otherwise creation returns QLDPC_ERR_INVALID and qldpc_last_error names
 *     the two rows.  Layers run in ascending number, empty numbers are skipped.  row_layer[i] = i is the literal serial schedule.
 *   State.  V = prior; every check-to-variable message R_ij = 0.0.
 *   Iteration k = 0 .. max_iter - 1, alpha_k as in qldpc_minsum_decode_batch.  For every layer in order, for every check i of it with at
 *     least one entry, over its columns j in ascending order:
 *       Q_ij = V_j - R_ij;  a NaN becomes 0.0;  then clip to +-clip_llr (the reference's rules, src/decoding/kernels.py:325-333);
 *       the sign of Q is + for Q >= 0;  sign_prod = the syndrome sign (+1 for s_i = 0, -1 for s_i = 1) times the product of the signs;
 *       min1, min2 over |Q| by the reference's strict-< scan (min2 is the second smallest of the multiset), min1_pos = the FIRST position
 *       of the minimum in ascending column order;  a degree-1 check has min2 = +inf;
 *       R_ij = alpha_k * (sign_prod * sign_ij) * (min2 if j is at min1_pos else min1);   V_j = Q_ij + R_ij.
 *     Every operation is one correctly rounded f64 operation (the multiply and the add are not contracted into an FMA).
 *     After the last layer e_j = (V_j < 0); if H e = s (over every row, those without entries included) the shot stops: converged,
 *     final_iter = k.
 *   Outputs per shot, exactly those of qldpc_minsum_decode_batch: err int8[n], llr f64[n] (= V), conv, final_iter (max_iter - 1 when not
 *     converged), so qldpc_osd0_batch and qldpc_osdcs_batch take them unchanged.
 *   Results do not depend on batch splits, the grid or any flag; the order of the checks inside a layer cannot matter by construction.
 * Limits (QLDPC_ERR_UNSUPPORTED): 1 <= m, n < 2^24; row degree <= 56; 29 bytes per row with entries + 4 per layer + 48 must fit 163 328 bytes of LDS
 * (160 KB less 512 the kernel keeps for itself; about 5600 rows).  The posteriors and the column indices (u16, n <= 65535) live in LDS when they fit beside that, else in HBM/L2.
 * flags: QLDPC_FLAG_LAYERED_* (other bits are ignored).  The decoder owns its tables; it keeps a pointer to g, which must outlive it.  Calls on
 * one decoder serialise (a mutex while enqueuing, an event between streams).
 * qldpc_layered_decoder_info: number of layers (with at least one non-empty row), rows and edges of the largest layer, LDS bytes of a
 * workgroup, and the form that runs: threads per workgroup | QLDPC_LAYERED_FORM_* bits; any output may be NULL.
 * qldpc_layered_decoder_layers: the row_layer in use, int32[m]. */
#define QLDPC_LAYERED_FORM_BLOCK_MASK 0xFFFF
#define QLDPC_LAYERED_FORM_VGLOBAL 0x10000       /* posteriors in a per-workgroup slab in HBM/L2 */
#define QLDPC_LAYERED_FORM_LDS_INDICES 0x20000   /* column indices as u16 in LDS */
typedef struct qldpc_layered_decoder qldpc_layered_decoder;
int qldpc_check_layers(const qldpc_graph *g, int32_t *row_layer, int *layers);
int qldpc_layered_decoder_create(const qldpc_graph *g, const int32_t *row_layer, const double *prior, int max_iter, int alpha_mode,
                                 double alpha_val, const double *alpha_seq, int alpha_len, double clip_llr, int flags,
                                 qldpc_layered_decoder **out);
void qldpc_layered_decoder_destroy(qldpc_layered_decoder *ld);
int qldpc_layered_decoder_info(const qldpc_layered_decoder *ld, int *layers, int *max_layer_rows, int *max_layer_edges, int *lds_bytes,
                               int *form);
int qldpc_layered_decoder_layers(const qldpc_layered_decoder *ld, int32_t *row_layer);
/* host pointers: syndromes int8[B][m] -> err int8[B][n], llr f64[B][n], conv uint8[B], iter int32[B]; returns when they are complete.  B = 0: a no-op */
int qldpc_layered_decode_batch(qldpc_layered_decoder *ld, int64_t B, const int8_t *syndromes, int8_t *err, double *llr, uint8_t *conv,
                               int32_t *iter);
/* same on device pointers; only enqueues on `stream` */
int qldpc_layered_decode_batch_dev(qldpc_layered_decoder *ld, int64_t B, const int8_t *d_syndromes, int8_t *d_err, double *d_llr,
                                   uint8_t *d_conv, int32_t *d_iter, void *stream);

/* Normalised min-sum (flooding schedule) in SINGLE PRECISION.  New here: an opt-in fast mode; f64 stays the default everywhere.  The algorithm is
 * that of qldpc_minsum_decode_batch (src/decoding/kernels.py:234-366 of the reference) with damping 1 and no damping arithmetic, and every
 * floating-point operation is one correctly rounded f32 operation (nothing is contracted into an FMA; f32 subnormals are kept, not flushed).
 * Rounding is amplified by the iteration, so on ordinary inputs the results differ from the f64 decoder's in some shots -- mostly the hard
 * decisions of shots that do not converge; tests/minsum32_model.py is the numpy model the library equals bit for bit, and the f64 decoder is
 * equalled only on inputs where no f32 operation rounds.  Compare logical error rates, not shots (tools/kbench_f32.py).
 *   Inputs.  prior32_j = (float)prior_j (round to nearest even; +-inf and NaN pass through).  clip32 = (float)clip_llr must be finite and > 0
 *     AFTER rounding (QLDPC_ERR_INVALID otherwise).  alpha_k is computed in f64 exactly as qldpc_minsum_decode_batch computes it (QLDPC_ALPHA_*),
 *     then rounded to f32.  max_iter >= 1.  There is no damping argument.
 *   Iteration 0.  Q_ij = prior32_j, unclipped, as in the reference.
 *   Check pass, for every check i with at least one entry, over its columns j in ascending order:
 *       the sign of Q is + for Q >= 0 (so a NaN counts as -);  sign_prod = the syndrome sign times the product of the signs;
 *       min1, min2 over |Q| by the reference's strict-< scan (min2 is the second smallest of the multiset; a NaN never enters), min1_pos = the
 *       FIRST position of the minimum;  a degree-1 check has min2 = +inf;
 *       R_ij = +-(alpha_k * mag), mag = min2 if j is at min1_pos else min1: ONE f32 multiply, then the sign sign_prod * sign_ij.
 *   Variable pass.  s_j = 0.0f + R_ij over the checks of j in ASCENDING check order, one f32 add each;  V_j = s_j + prior32_j;
 *       Q_ij = V_j - R_ij;  a NaN becomes 0.0f;  then clip to +-clip32.
 *     (With a non-finite prior the f64 decoder also reproduces the NaN of the reference's 0.0 * Q_old damping term; this decoder has no such term:
 *     a prior of +-inf gives Q = +-clip32 and a NaN prior Q = 0 from iteration 1 on.)
 *   Stop.  e_j = (V_j < 0); if H e = s over every row (those without entries included) the shot stops: converged, final_iter = k.
 *   Outputs per shot, exactly those of qldpc_minsum_decode_batch: err int8[n], llr f64[n] = the f32 V widened (exact), conv, final_iter
 *     (max_iter - 1 when not converged), so qldpc_osd0_batch, qldpc_osdcs_batch and a circuit plan's OSD stage take them unchanged.
 *   Results do not depend on batch splits, the grid or any flag.
 * Limits (QLDPC_ERR_UNSUPPORTED, the limit in qldpc_last_error): 1 <= m < 2^24, 1 <= n < 65535, row degree <= 56, and 4 bytes per column + 17 per
 * row + 48 must fit the 163 840 bytes of LDS of a CU ([[288,12,18]] x 18 cycles, 2880 x 26 209: 153 824).
 * flags: QLDPC_FLAG_F32_* (other bits are ignored).  The decoder owns its tables; it keeps a pointer to g, which must outlive it.  Calls on one
 * decoder serialise (a mutex while enqueuing, an event between streams).
 * qldpc_minsum32_decoder_info: LDS bytes of a workgroup, threads per workgroup, workgroups resident per CU (the runtime's occupancy query for
 * this kernel, size and LDS) and QLDPC_F32_FORM_* bits; any output may be NULL. */
#define QLDPC_F32_FORM_CLEAN 0x1                 /* the clean-input kernel: no degree-1 check, |prior32| and clip32 <= 2^100, 0 < alpha32 <= 1024 */
typedef struct qldpc_minsum32_decoder qldpc_minsum32_decoder;
int qldpc_minsum32_decoder_create(const qldpc_graph *g, const double *prior, int max_iter, int alpha_mode, double alpha_val,
                                  const double *alpha_seq, int alpha_len, double clip_llr, int flags, qldpc_minsum32_decoder **out);
void qldpc_minsum32_decoder_destroy(qldpc_minsum32_decoder *dec);
int qldpc_minsum32_decoder_info(const qldpc_minsum32_decoder *dec, int *lds_bytes, int *threads, int *wg_per_cu, int *form);
/* host pointers: syndromes int8[B][m] -> err int8[B][n], llr f64[B][n], conv uint8[B], iter int32[B]; returns when they are complete.  B = 0: a no-op */
int qldpc_minsum32_decode_batch(qldpc_minsum32_decoder *dec, int64_t B, const int8_t *syndromes, int8_t *err, double *llr, uint8_t *conv,
                                int32_t *iter);
/* same on device pointers; only enqueues on `stream` */
int qldpc_minsum32_decode_batch_dev(qldpc_minsum32_decoder *dec, int64_t B, const int8_t *d_syndromes, int8_t *d_err, double *d_llr,
                                    uint8_t *d_conv, int32_t *d_iter, void *stream);

/* a10: generate_noisy_circuit_jit (src/noise/kernels.py:175-353), batched over B draws of explicit random
 * arrays rv/rp/rt [B][n_locs]; out_* [B][cap]; out_len int64[B]. */
int qldpc_noisy_circuit_batch(int64_t B, int64_t len, const int32_t *ops, const int32_t *q1, const int32_t *q2, double p,
                              int64_t n_locs, const double *rv, const int32_t *rp, const int32_t *rt, int64_t cap,
                              int32_t *out_ops, int32_t *out_q1, int32_t *out_q2, int64_t *out_len);
/* a11: simulate_circuit_Z_jit / simulate_circuit_X_jit (noise/kernels.py:13-91 / 94-172), batched over B op
 * lists ops[B][cap] with lengths len[B]; hist int8[B][max_syn], state int8[B][total_qubits], counts int64[B][2]. */
int qldpc_frame_sim_batch(int sector_is_x, int64_t B, int64_t cap, const int64_t *len, const int32_t *ops,
                          const int32_t *q1, const int32_t *q2, int total_qubits, int max_syn, int8_t *hist, int8_t *state,
                          int64_t *counts);
/* a12: sparsify_syndrome_jit (noise/kernels.py:356-380), batched: hist[B][stride] -> out[B][stride] */
int qldpc_sparsify_batch(int64_t B, int64_t stride, const int8_t *hist, const int64_t *syn_count, const int32_t *positions,
                         const int32_t *ptrs, int num_checks, int8_t *out);

/* Code-capacity Monte-Carlo (BASELINE configs 1-4), fused on the device: for global shots
 * [shot_begin, shot_begin+count): sample e ~ Bernoulli(p)^n (law of src/decoding/alpha.py:127-128, Philox4x32-10
 * stream keyed (seed, shot)), s = H e, decode (a1), OSD-0 on non-converged shots if use_osd, logical failure iff
 * L (e xor e_hat) != 0 (rule of src/simulation/engine.py:99-100), tally.  L: dense k x n bytes (host).
 * Host-synchronous: tally (host int64[16]) is complete on return.  Results are independent of how the shot range
 * is split across calls / devices. */
int qldpc_cc_sample_decode_tally(const qldpc_graph *g, int k, const uint8_t *L, double p, uint64_t seed,
                                 int64_t shot_begin, int64_t count, int max_iter, int alpha_mode, double alpha_val,
                                 const double *alpha_seq, int alpha_len, double damping, double clip_llr, int use_osd,
                                 int flags, int64_t *tally);

/* MC plan handle: same pipeline, asynchronous, for benchmarking and multi-stream use.  qldpc_cc_plan_run cuts its shot range into pieces of
 * `batch` shots, each enqueued as one pass of the pipeline accumulating into the plan's device tally; the plan owns device buffers for `batch`
 * shots per piece in flight (up to 8 pieces for batch <= 32768, up to 3 under reference semantics above that, else 1); qldpc_cc_plan_read
 * synchronises and returns (and optionally clears) the tally.  `batch` is taken literally.  A piece costs the host three enqueues (decode,
 * OSD-0, judge; ~10 us each), so small pieces bound the rate from the host side: `min_launch` > batch (an argument of THIS plan, 0 = none) lets
 * the plan cut at that granule instead, with buffers sized for it -- the tallies do not depend on the cut (the random stream is keyed by the
 * global shot index), only the memory bound `batch` expressed is given up. */
typedef struct qldpc_cc_plan qldpc_cc_plan;
int qldpc_cc_plan_create(const qldpc_graph *g, int k, const uint8_t *L, double p, int max_iter, int alpha_mode,
                         double alpha_val, const double *alpha_seq, int alpha_len, double damping, double clip_llr,
                         int use_osd, int flags, int64_t batch, int64_t min_launch, qldpc_cc_plan **out);
/* _run only enqueues: on `stream`, or (option mc_tail_overlap >= 1: reference-semantics plans and plans with batch <= 32768) on streams the plan owns,
 * which start behind everything `stream` held when _run was called; several batches are then in flight at once.  _read waits for `stream` and for
 * the plan's own streams, then copies the tally: it is the only way results leave the plan. */
int qldpc_cc_plan_run(qldpc_cc_plan *plan, uint64_t seed, int64_t shot_begin, int64_t count, void *stream);
int qldpc_cc_plan_read(qldpc_cc_plan *plan, void *stream, int clear, int64_t *tally);
/* time of the decode kernel launches enqueued since the last call, measured with hipEvents on the launch
 * stream (ms, summed) and their count; used by bench.py for the roofline line.  With batches in flight on several streams the spans overlap (their
 * sum exceeds the wall time and each contains its neighbours' work): bench.py takes kernel times from a plan created with mc_tail_overlap = 2. */
int qldpc_cc_plan_kernel_time(qldpc_cc_plan *plan, double *ms_total, int64_t *launches);
/* the part of that total spent in the bit-sliced first-iteration kernel of the reference-semantics pipeline (csrc/mc_first.hip; 0 for plans
 * that do not use it).  Call before qldpc_cc_plan_kernel_time, which resets both sums. */
int qldpc_cc_plan_first_iteration_time(qldpc_cc_plan *plan, double *ms_first);
/* shader clock (MHz) held under the last decode launch (plans created with QLDPC_FLAG_CLOCK_PROBE; fused regular kernel only):
 * median over workgroups of delta(s_memtime) / delta(s_memrealtime) x 100 MHz.  Synchronises `stream`. */
int qldpc_cc_plan_clock(qldpc_cc_plan *plan, void *stream, double *mhz);
void qldpc_cc_plan_destroy(qldpc_cc_plan *plan);

/* ---- circuit-level Monte-Carlo (BASELINE config 5) ------------------------------------------------------------
 * Compiled syndrome-extraction circuit in the wire format of the reference's CompiledCircuit (src/noise/compiled.py:116-173;
 * op codes src/noise/constants.py:8-14).  All pointers are host pointers, copied at plan creation. */
typedef struct {
    int64_t base_len, suffix_len;                       /* noisy part (cycle * num_cycles) and noiseless suffix (cycle * 2) */
    const int32_t *base_ops, *base_q1, *base_q2, *suffix_ops, *suffix_q1, *suffix_q2;
    int32_t total_qubits, num_x_checks, num_z_checks, n_data, k, reserved;
    const int32_t *x_syn_positions, *x_syn_ptrs;        /* CSR: X check -> indices of its MeasX outcomes (compiled.py:72-103) */
    const int32_t *z_syn_positions, *z_syn_ptrs;
    const int32_t *data_qubit_indices;                  /* [n_data] */
    const uint8_t *Lx, *Lz;                             /* logical operators, dense k x n_data */
} qldpc_circuit_desc;

/* Single-fault signatures of one sector: the batched form of the per-fault simulations in src/noise/builder.py:37-66
 * (_simulate_Z_from_spec / _simulate_X_from_spec).  Entry e = 2 * base_op_index + slot (slot 1 = CNOT target). */
int qldpc_circuit_fault_signatures(const qldpc_circuit_desc *circuit, int sector_is_x, int32_t *ptr, uint16_t *idx, int64_t idx_cap,
                                   uint64_t *logmask, int64_t *idx_needed);

/* ---- f4: the trial loops of the alpha / beta estimators, batched ------------------------------------------------------------
 * Replaces the per-trial Python loops of estimate_alpha_alvarado (src/decoding/alpha.py:119-137),
 * estimate_alpha_alvarado_autoregressive (alpha.py:206-255, one call per iteration index) and estimate_scopt_beta
 * (src/decoding/scopt.py:80-134).  errors: int8[B][n], drawn by the caller (the reference draws them from the caller's numpy
 * Generator); syndromes, decoder state, samples and histograms live on the device.
 *   QLDPC_STATS_CHECK_MESSAGES  samples = R_flat of one check pass with alpha = 1 taken after `iters` decoder iterations that
 *                               use alpha_k of the given alpha mode (iters = 0 is alpha.py:119-137); class = error[col[edge]].
 *   QLDPC_STATS_POSTERIOR       samples = the posterior `values` the decoder stops with (early exit, at most `iters`
 *                               iterations; scopt.py:88-131); class = error[j].
 * range[0..1] = min / max over the finite samples of both classes (alpha.py:29-31), finite[c] = number of finite samples of
 * class c (alpha.py:23-27).  qldpc_msgstats_histogram then bins them with np.histogram's rule for the given strictly increasing
 * edges (bins + 1 values): edges[i] <= x < edges[i+1], last bin closed; hist0 / hist1: int64[bins]. */
#define QLDPC_STATS_CHECK_MESSAGES 0
#define QLDPC_STATS_POSTERIOR 1
typedef struct qldpc_msgstats qldpc_msgstats;
int qldpc_msgstats_create(const qldpc_graph *g, int64_t B, const int8_t *errors, const double *prior, int kind, int iters,
                          int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len, double damping, double clip_llr,
                          double *range, int64_t *finite, qldpc_msgstats **out);
int qldpc_msgstats_histogram(qldpc_msgstats *stats, const double *edges, int bins, int64_t *hist0, int64_t *hist1);
void qldpc_msgstats_destroy(qldpc_msgstats *stats);

typedef struct qldpc_circuit_plan qldpc_circuit_plan;
/* a13 + a14: run_trial_fast (src/noise/simulation.py:21-107) + _run_single_trial_fast and the tally
 * (src/simulation/engine.py:68-122, 450-457), batched.  gz / gx: Tanner graphs of HdecZ / HdecX; prior_*: LLRs of
 * engine.py:210-212; logmask_*[j]: bit r set iff logical row r of H*_full has a one in column j (engine.py:99,119).
 * Trials are addressed by a global index (Philox streams), so any split over calls / devices gives the same tally. */
int qldpc_circuit_plan_create(const qldpc_circuit_desc *circuit, const qldpc_graph *gz, const qldpc_graph *gx, const double *prior_z,
                              const double *prior_x, const uint64_t *logmask_z, const uint64_t *logmask_x, double p, int max_iter,
                              int alpha_mode, double alpha_val_z, double alpha_val_x, const double *alpha_seq_z, int alpha_len_z,
                              const double *alpha_seq_x, int alpha_len_x, double damping, double clip_llr, int use_osd, int flags,
                              int64_t batch, qldpc_circuit_plan **out);
int qldpc_circuit_plan_run(qldpc_circuit_plan *plan, uint64_t seed, int64_t trial_begin, int64_t count, void *stream);
/* Same pass, and additionally the per-trial verdicts in trial order: outcome[i] bit0 = z_err, bit1 = x_err of trial
 * trial_begin + i (host buffer, `count` bytes; the call synchronises `stream`).  This is what the reference's in-order
 * early stop needs (src/simulation/engine.py:441-464: stop at the trial where the target-th logical error occurs). */
int qldpc_circuit_plan_run_outcomes(qldpc_circuit_plan *plan, uint64_t seed, int64_t trial_begin, int64_t count, void *stream,
                                    uint8_t *outcome);
int qldpc_circuit_plan_read(qldpc_circuit_plan *plan, void *stream, int clear, int64_t *tally);
/* hipEvent time (ms, summed over the batches enqueued since the last call) of each phase of the per-trial pipeline of
 * src/simulation/engine.py:68-122, and the number of batches.  The phases of a batch run back to back on the caller's stream (sample, sector Z,
 * sector X, judge), so their spans do not overlap. */
#define QLDPC_CIRCUIT_PHASES 6
#define QLDPC_PHASE_SAMPLE 0   /* run_trial_fast, engine.py:75 */
#define QLDPC_PHASE_BP_Z 1     /* engine.py:84-94 */
#define QLDPC_PHASE_OSD_Z 2    /* engine.py:96-97 */
#define QLDPC_PHASE_BP_X 3     /* engine.py:103-113 */
#define QLDPC_PHASE_OSD_X 4    /* engine.py:115-116 */
#define QLDPC_PHASE_JUDGE 5    /* engine.py:99-100,119-122 + tally */
int qldpc_circuit_plan_phase_times(qldpc_circuit_plan *plan, double *ms /* [QLDPC_CIRCUIT_PHASES] */, int64_t *batches);
/* shader clock (MHz) held under the sector-Z decode kernel [0] and OSD-0 kernel [1] of the last batch (plans created with
 * QLDPC_FLAG_CLOCK_PROBE): median over workgroups of delta(s_memtime) / delta(s_memrealtime) x 100 MHz.  Synchronises `stream`. */
int qldpc_circuit_plan_clock(qldpc_circuit_plan *plan, void *stream, double *mhz /* [2] */);
/* the sampler alone = batched run_trial_fast: sparse_z int8[count][#MeasX], true_z int8[count][k], sparse_x, true_x (host) */
int qldpc_circuit_plan_sample(qldpc_circuit_plan *plan, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *sparse_z,
                              int8_t *true_z, int8_t *sparse_x, int8_t *true_x);
void qldpc_circuit_plan_destroy(qldpc_circuit_plan *plan);
/* Switches the plan's decoder to Relay-BP (one-way): both sectors are decoded by qldpc_relay_decode_batch's kernel with the plan's
 * priors, the seed of the run call and the global trial index as `shot` (tag 0 for sector Z, 1 for sector X); no OSD stage follows.
 * The tally keeps its meaning: bp_conv = Relay-BP converged, iters = sum of Relay-BP iterations, OSD slots 0, legs in
 * QLDPC_TALLY_LEGS_Z / _X.  Arguments as in qldpc_relay_decode_batch. */
int qldpc_circuit_plan_use_relay(qldpc_circuit_plan *plan, double alpha, double gamma0, double gamma_min, double gamma_max, int t0, int tr,
                                 int max_legs, int stop_after);
/* Switches the plan's OSD stage to OSD-CS of `order` (one-way; qldpc_osdcs_batch with the plan's priors as the weights): the same
 * unconverged trials, the same phase brackets, the same tally slots.  QLDPC_ERR_INVALID on a plan created with use_osd = 0 or switched to
 * Relay-BP (and qldpc_circuit_plan_use_relay after this call returns QLDPC_ERR_INVALID); QLDPC_ERR_UNSUPPORTED when a sector's matrix is
 * outside the range of qldpc_osdcs_batch. */
int qldpc_circuit_plan_use_osd_cs(qldpc_circuit_plan *plan, int order);
/* Switches the plan's OSD stage to BP+LSD (qldpc_lsd_batch with these parameters): the same unconverged trials, the same phase brackets, the
 * same tally slots.  It goes with flooding, the layered schedule, guided decimation, f32, correlated decoding, erasure-aware decoding and
 * soft-aware decoding in either order (it reads the posteriors and the hard decision as that path left them; behind correlated decoding sector X's
 * links are read against sector Z's correction as this stage left it), and may be called again with new parameters.  QLDPC_ERR_INVALID on a plan created with use_osd = 0, switched to Relay-BP, to windows or to OSD-CS (and
 * qldpc_circuit_plan_use_relay / _use_window / _use_osd_cs after this call return QLDPC_ERR_INVALID), or for parameters outside their ranges;
 * QLDPC_ERR_UNSUPPORTED when a sector's matrix is one qldpc_lsd_batch refuses at this max_rows. */
int qldpc_circuit_plan_use_lsd(qldpc_circuit_plan *plan, int bits_per_step, int max_rows);
/* The shots the plan's LSD stage has ended with flag 0 / 1 / 2 since the last clear: counts int64[2][3], counts[sector][flag] (sector 1 stays 0 on
 * a one-sector plan; all 0 on a plan that was never switched).  The cluster kernel accumulates them on the device; the three of a sector add up to
 * the sector's OSD tally slot over the same batches.  Synchronises `stream`. */
int qldpc_circuit_plan_lsd_counts(qldpc_circuit_plan *plan, void *stream, int clear, int64_t *counts);
/* The confidence of a trial on a plan whose OSD stage is BP+LSD: one uint64 score per trial from the cluster statistics of its two sectors
 * (qldpc_lsd_stats_batch), small = trustworthy, and a histogram of (score, outcome) for post-selection.  New here.
 *   kind                   word of the statistics   how the sectors combine
 *   QLDPC_CONF_COLS_1      1  sum a_i               sum, saturating at 2^64 - 2
 *   QLDPC_CONF_COLS_2      2  sum a_i^2             sum, saturating at 2^64 - 2 (the squared norm: only the order matters, so no root is taken)
 *   QLDPC_CONF_COLS_INF    3  max a_i               max
 *   QLDPC_CONF_LLR_1       4  sum W_i               sum, saturating at 2^64 - 2
 *   QLDPC_CONF_LLR_2       5  sum W_i^2             sum, saturating at 2^64 - 2
 *   QLDPC_CONF_LLR_INF     6  max W_i               max
 * A sector whose BP converged contributes 0; if LSD made no statement in either sector (flag 1 or 2) the score is 2^64 - 1.
 * edges uint64[nbins - 1], strictly increasing, 1 <= nbins <= QLDPC_CONF_MAX_BINS (NULL with nbins = 1): bin = the number of edges <= score, and every
 * trial of _run / _run_outcomes / _run_scores adds 1 to hist[bin][outcome], outcome = bit0 z_err | bit1 x_err as in _run_outcomes.  weight_z /
 * weight_x: uint16[n] of the sector (copied; weight_x is ignored on a one-sector plan); NULL is legal for the COLS kinds only.
 * Legal once qldpc_circuit_plan_use_lsd has been called, before or after the path switches LSD goes with, and again with new arguments, which clears
 * the histogram.  QLDPC_ERR_INVALID otherwise (a plan with use_osd = 0, on OSD-0, OSD-CS, Relay-BP or windows), and for a kind, nbins, edges or
 * weights outside the above.  The tally, the verdicts and the LSD counts of the plan do not change. */
#define QLDPC_CONF_COLS_1 0
#define QLDPC_CONF_COLS_2 1
#define QLDPC_CONF_COLS_INF 2
#define QLDPC_CONF_LLR_1 3
#define QLDPC_CONF_LLR_2 4
#define QLDPC_CONF_LLR_INF 5
#define QLDPC_CONF_MAX_BINS 4096
int qldpc_circuit_plan_use_confidence(qldpc_circuit_plan *plan, int kind, int nbins, const uint64_t *edges, const uint16_t *weight_z,
                                      const uint16_t *weight_x);
/* hist uint64[nbins][4] (host) of the trials since the last clear.  Synchronises `stream`.  QLDPC_ERR_INVALID on a plan without a confidence. */
int qldpc_circuit_plan_confidence_read(qldpc_circuit_plan *plan, void *stream, int clear, uint64_t *hist);
/* qldpc_circuit_plan_run_outcomes, and score[i] of trial trial_begin + i (host, uint64[count]).  A trial's score is a function of (seed, trial index)
 * alone: it depends neither on the plan's batch nor on how a range is split over calls.  QLDPC_ERR_INVALID on a plan without a confidence. */
int qldpc_circuit_plan_run_scores(qldpc_circuit_plan *plan, uint64_t seed, int64_t trial_begin, int64_t count, void *stream, uint8_t *outcome,
                                  uint64_t *score);
/* Switches the BP + OSD-0 stage of both sectors to sliding-window decoding (one-way): a qldpc_window_decoder per sector with the plan's
 * prior, alpha schedule, max_iter and clip_llr, layer_rows = the sector's number of checks (num_x_checks for sector Z, num_z_checks for
 * sector X: one layer per syndrome cycle).  Sampler, judge and tally are unchanged; bp_conv_* counts the trials in which every window
 * converged, osd_* the trials with at least one OSD-0 window, iters_* and unsat_* as before.  The phase times keep their brackets: BP_* sums
 * gather + min-sum over the windows, OSD_* collect + OSD-0 + commit.  QLDPC_ERR_INVALID on a plan created with use_osd = 0 or damping != 1,
 * switched to Relay-BP or OSD-CS, or already windowed (and qldpc_circuit_plan_use_relay / _use_osd_cs after this call return
 * QLDPC_ERR_INVALID); otherwise what qldpc_window_decoder_create returns. */
int qldpc_circuit_plan_use_window(qldpc_circuit_plan *plan, int window, int commit);
/* Switches the BP launch of both sectors to the layered schedule: a qldpc_layered_decoder per sector with the plan's prior, alpha schedule,
 * max_iter (>= 1) and clip_llr; row_layer_z / row_layer_x as in qldpc_layered_decoder_create (NULL = the greedy colouring).  Only the launch
 * inside the BP bracket changes: sampler, unconverged list, the OSD-0 / OSD-CS stage, judge and tally slots are untouched, and
 * qldpc_circuit_plan_use_osd_cs may come before or after.  A second call replaces the layers.  QLDPC_ERR_INVALID on a plan with damping != 1
 * or switched to Relay-BP or to windows (and qldpc_circuit_plan_use_relay / _use_window after this call return QLDPC_ERR_INVALID); otherwise
 * what qldpc_layered_decoder_create returns. */
int qldpc_circuit_plan_use_layered(qldpc_circuit_plan *plan, const int32_t *row_layer_z, const int32_t *row_layer_x);
/* Switches the BP launch of both sectors to BP with guided decimation (qldpc_decim_decode_batch's kernel) with the plan's priors and clip_llr and
 * the arguments given here.  Only the launch inside the BP bracket changes: it writes the plan's hard decisions, posteriors, converged flags and
 * iteration counts, so sampler, unconverged list, the OSD-0 / OSD-CS stage and judge are untouched, and qldpc_circuit_plan_use_osd_cs may come
 * before or after.  The plan's own max_iter and alpha table are NOT used by the switched bracket.  The tally keeps its meaning: bp_conv =
 * decimation converged, iters = the sum of its iterations, and QLDPC_TALLY_LEGS_Z / _X sum the rounds.  A second call replaces the
 * arguments.  QLDPC_ERR_INVALID for arguments qldpc_decim_decode_batch refuses, priors that are not finite, damping != 1, a plan switched to
 * Relay-BP or to windows or whose BP stage runs the layered schedule (and qldpc_circuit_plan_use_relay / _use_window / _use_layered after this
 * call return QLDPC_ERR_INVALID); QLDPC_ERR_UNSUPPORTED when a sector's matrix is one qldpc_decim_decode_batch refuses. */
int qldpc_circuit_plan_use_decimation(qldpc_circuit_plan *plan, double alpha, int t_round, int max_rounds, int per_round, double fix_llr);
/* Switches the BP launch of both sectors to two-pass correlated decoding (qldpc_shotprior_decode_batch's kernel) with the constant `alpha` and the
 * plan's max_iter and clip_llr (its alpha table is NOT used).  Sector 0 is decoded with its own prior and no tables.  Sector 1 is then decoded with
 * prior = base_x (f64[n_x]; NULL: the plan's sector-1 prior) at stride 0, src_err = sector 0's correction as its OSD stage left it, and the link
 * tables given here: link_ptr int32[n_x + 1] (NULL with n_links = 0: no links, the same kernel with nothing to raise), link_src int32[n_links]
 * naming sector-0 columns, link_llr f64[n_links], under the rules of qldpc_shotprior_decode_batch.  Only the launch inside the BP bracket changes:
 * sampler, unconverged list, the OSD-0 / OSD-CS / LSD stage, judge and tally slots are untouched (QLDPC_TALLY_LEGS_* stay 0), recorded events
 * (qldpc_circuit_plan_decode_events) decode the same way, and qldpc_circuit_plan_use_osd_cs / _use_lsd may come before or after.  OSD-CS scores its
 * candidates with the plan's sector prior, not the per-shot one.  A second call replaces the arguments.  QLDPC_ERR_INVALID for a one-sector plan,
 * arguments or tables qldpc_shotprior_decode_batch refuses, priors that are not finite, damping != 1, or a plan switched to another path (and every
 * other path switch after this call returns QLDPC_ERR_INVALID); QLDPC_ERR_UNSUPPORTED when a sector's matrix is one qldpc_shotprior_decode_batch
 * refuses. */
int qldpc_circuit_plan_use_correlated(qldpc_circuit_plan *plan, double alpha, const double *base_x, int64_t n_links, const int32_t *link_ptr,
                                      const int32_t *link_src, const double *link_llr);
/* Switches the BP launch of both sectors to the single-precision decoder (one-way): a qldpc_minsum32_decoder per sector with the plan's prior, alpha
 * table, max_iter (>= 1) and clip_llr.  Only the launch inside the BP bracket changes: it writes the plan's hard decisions, posteriors (f64, the f32
 * values widened), converged flags and iteration counts, so sampler, unconverged list, the OSD-0 / OSD-CS stage, judge and tally slots are untouched,
 * and qldpc_circuit_plan_use_osd_cs may come before or after.  QLDPC_ERR_INVALID on a plan with damping != 1, switched to Relay-BP or to windows, or
 * whose BP stage runs the layered schedule or guided decimation (and qldpc_circuit_plan_use_relay / _use_window / _use_layered / _use_decimation
 * after this call return QLDPC_ERR_INVALID); otherwise what qldpc_minsum32_decoder_create returns. */
int qldpc_circuit_plan_use_f32(qldpc_circuit_plan *plan);

/* ---- a circuit plan that samples a detector error model (DEM).  New here: the reference has no counterpart. -------------------------------
 * A DEM is a list of independent error mechanisms, each with a probability, the detectors it flips and the logical observables it flips.  It has one
 * or two SECTORS: decoding problems with their own detectors, graph, prior and logicals, decoded independently (as Z and X of a circuit plan; sector 0
 * takes every "Z" slot of the tally, the phases and the outcome bits, sector 1 every "X" slot).  One mechanism may touch both sectors -- that is how a
 * Y-type fault correlates them -- so there is one mechanism table, projected per sector.  All pointers are host pointers, copied at plan creation.
 *
 * The law of the sampler, a pure function of (seed, global trial index): for trial g = trial_begin + t, mechanism l has Philox block q = l >> 2 and word
 * w = l & 3 of o = Philox4x32-10(counter = (lo32(g), hi32(g), q, 3), key = (lo32(seed), hi32(seed))), and fires iff o[w] < thr_l = floor(p_l * 2^32)
 * (uint32; p_l = 0 never fires).  Counter word 3 is the domain: 0 = the code-capacity samplers, 1 and 2 = the circuit sampler, 3 = this one,
 * 0x52...... = Relay-BP.  A firing mechanism XORs its detectors into the sectors' syndromes and its logmask into the sectors' true logical flips. */
typedef struct {
    int64_t n_mech;
    const double *prob;            /* [n_mech], 0 <= p < 1 */
    int32_t n_sectors;             /* 1 or 2 */
    int32_t k[2];                  /* logical observables per sector, 0..64 */
    int32_t n_det[2];              /* detectors per sector = rows of that sector's graph, 1..65535 */
    int32_t layer_rows[2];         /* rows per layer for sliding windows; 0 = the plan refuses qldpc_circuit_plan_use_window */
    const int32_t *det_ptr[2];     /* [n_mech + 1] per sector */
    const uint16_t *det_idx[2];    /* detector indices, strictly ascending inside a mechanism */
    const uint64_t *logmask[2];    /* [n_mech] per sector, bit r = observable r */
} qldpc_dem_desc;
/* Creates an ordinary qldpc_circuit_plan whose sampler draws from `dem`: _run, _run_outcomes, _read, _sample, _phase_times, _clock, _destroy and every
 * qldpc_circuit_plan_use_* work on it unchanged and under the same rules.  The graphs, priors and column logical masks (logmask0 / logmask1: uint64 per
 * column of g0 / g1) are the DECODER's view and are given explicitly, as in qldpc_circuit_plan_create; the mechanisms are the truth that is sampled,
 * and the two need not have the same columns.  g1, prior1, logmask1 are NULL iff n_sectors == 1 (the index-1 entries of the descriptor's arrays are
 * then ignored).  qldpc_circuit_plan_use_window takes layer_rows[s] as the rows of a syndrome cycle and returns QLDPC_ERR_INVALID when it is 0 or does
 * not divide the rows.  qldpc_circuit_plan_sample writes true_z as int8[count][k[0]] and true_x as int8[count][k[1]].
 *   One sector: sector 1 has no buffers, no decode, no OSD and no phase brackets, and the judge runs sector 0 alone: every X tally slot stays 0,
 *   outcome bit 1 is 0, total_err = z_err, and qldpc_circuit_plan_sample leaves sparse_x / true_x untouched (they may be NULL).
 * QLDPC_ERR_INVALID, with qldpc_last_error naming the sector or the mechanism: NULL tables, a non-monotone det_ptr, a detector index out of range or
 * not ascending, p outside [0, 1) or NaN, a logmask bit at or above k[s], g_s->m != n_det[s], n_sectors outside {1, 2}. */
int qldpc_circuit_plan_create_dem(const qldpc_dem_desc *dem, const qldpc_graph *g0, const qldpc_graph *g1, /* g1 NULL iff n_sectors == 1 */
                                  const double *prior0, const double *prior1, const uint64_t *logmask0, const uint64_t *logmask1, int max_iter,
                                  int alpha_mode, double alpha_val0, double alpha_val1, const double *alpha_seq0, int alpha_len0,
                                  const double *alpha_seq1, int alpha_len1, double damping, double clip_llr, int use_osd, int flags, int64_t batch,
                                  qldpc_circuit_plan **out);

/* ---- fixed-weight fault sampling: the plan's sampler draws exactly `weight` faults per trial.  New here: the reference has no counterpart. ---------
 * The sampler axis of a plan, beside its decode path and its OSD stage: it is not one of the qldpc_circuit_plan_use_* decode switches, goes with every
 * one of them in either call order, and is two-way.  The plan's own sampler draws each of its N fault locations (circuit: the base ops; detector error
 * model: the mechanisms) independently with one probability p, so the number of faults is Binomial(N, p) and, given that number, the faulty set is
 * uniform.  The fixed-weight sampler draws that conditional law for one weight w: the failure fraction f_w it measures does not depend on p, and
 * LER(p) = sum_w C(N, w) p^w (1 - p)^(N - w) f_w (simulation/strata.py sweeps w on ONE plan).
 *
 * The law, a pure function of (seed, global trial index g = trial_begin + t, w): the faulty set S is built by Floyd's algorithm, for i = 0 .. w - 1:
 *   j = N - w + i;
 *   o_i = word (i & 3) of Philox4x32-10(counter = (lo32(g), hi32(g), i >> 2, 4), key = (lo32(seed), hi32(seed)));
 *   t = the high 32 bits of the 64-bit product o_i * (j + 1);
 *   S gets j if t is already in S, t otherwise.
 * Counter word 3 is the domain: 4 is new (0 = the code-capacity samplers, 1 and 2 = the circuit sampler, 3 = the DEM sampler, 0x52...... = Relay-BP).
 * S is a uniformly distributed w-subset of 0 .. N - 1 (Bentley and Floyd 1987) up to the 2^-32 granularity of t: the probability of a value of t
 * differs from 1 / (j + 1) by at most 2^-32, a relative bias of at most N / 2^32 per step (4e-6 for the 17 280 locations of the [[144,12,12]] circuit).
 * A member l of S then does what a faulty location does today: on a circuit plan it draws its Pauli component from domain 2, counter (g, l), exactly as
 * the independent sampler does (measurements and preparations have one component) and XORs the same fault signatures; on a DEM plan mechanism l XORs
 * its detectors and logical masks.  XOR is order-free, so the result does not depend on grid, block size, lane mapping or how a range is cut into batches.
 *
 * weight >= 0: from now on the plan's sampler draws exactly `weight` faulty locations per trial (law above);
 * weight == -1: back to the independent draws the plan was created with.  Two-way, any number of times.
 * qldpc_circuit_plan_run, _run_outcomes and _sample honour it; _decode_events* and _unpack_events do not sample and are untouched.
 * QLDPC_ERR_INVALID: weight < -1, weight > QLDPC_FIXED_WEIGHT_MAX (binomial mass beyond is of no use) or weight > N; a DEM plan whose mechanisms
 * do not all have the same threshold floor(p_l * 2^32) (qldpc_last_error names the first mechanism that differs from mechanism 0: a non-uniform model
 * has no weight strata of this kind).  QLDPC_ERR_UNSUPPORTED: N > QLDPC_FIXED_WEIGHT_MAX_LOCS (the membership bit set of S lives in LDS, 64 KiB).
 * A refused call leaves the plan as it was. */
#define QLDPC_FIXED_WEIGHT_MAX 4096
#define QLDPC_FIXED_WEIGHT_MAX_LOCS 524288
int qldpc_circuit_plan_use_fixed_weight(qldpc_circuit_plan *plan, int weight);

/* ---- heralded-erasure noise and erasure-aware decoding.  New here: the reference has no counterpart.  Circuit plans only. -------------------------
 * A second noise process beside the plan's Pauli faults: a location is ERASED with the rate of its class, the hardware reports which ones were (the
 * herald record), and an erased location is fully depolarised.  A decoder that reads the heralds treats such a location as a coin flip.
 *
 * Erasure draws, a pure function of (seed, global trial index g = trial_begin + t): rate[ty] in [0, 1) per location class, ty one of the six op
 * codes 1..6 of a base circuit (CNOT, PrepX, PrepZ, MeasX, MeasZ, IDLE; rate[0] is not read); ethr[ty] = floor(rate[ty] * 2^32) (uint32; a rate of
 * 0 never fires).  Location l is erased iff word (l & 3) of Philox4x32-10(counter = (lo32(g), hi32(g), l >> 2, 5), key = (lo32(seed), hi32(seed))) is
 * below ethr[type(l)].  Counter word 3 is the domain: 5 and 6 are new (0 = the code-capacity samplers, 1 and 2 = the circuit sampler, 3 = the DEM
 * sampler, 4 = the fixed-weight sampler, 0x52...... = Relay-BP).
 * Pauli of an erased location: r = word 0 of Philox4x32-10(counter = (lo32(g), hi32(g), l, 6), same key).  Its component mask (bit 0 = X on slot 0,
 * bit 1 = X on slot 1, bit 2 = Z on slot 0, bit 3 = Z on slot 1; slot 0 = the gate's first qubit, slot 1 = a CNOT's target) is
 *     CNOT            r & 15                    the sixteen two-qubit Paulis, identity included
 *     IDLE            {0, 1, 5, 4}[r & 3]       I, X, Y, Z
 *     MeasX / PrepX   (r & 1) ? 4 : 0
 *     MeasZ / PrepZ   (r & 1) ? 1 : 0
 * and the fault signatures of its components are XORed into the sectors' syndromes and true logical flips exactly as an ordinary fault's are.  All
 * moduli are powers of two: no bias.  The ordinary faults (domains 1 and 2) are drawn as without erasures, in addition: a uniform Pauli composed
 * with anything is uniform, so this is the same physical channel, and with every rate 0 the syndromes and truths are the plain sampler's bit for bit.
 * Herald record: uint32[B][ceil(n_locs / 32)], bit (l & 31) of word (l >> 5) set iff location l is erased.
 *
 * Decoder tables, per sector (simulation/erasure.py builds them on the host), for a sector with n columns:
 *   loc_ptr int32[n_locs + 1], loc_col int32[loc_ptr[n_locs]] (columns, strictly ascending inside a location's run), loc_h uint8[loc_ptr[n_locs]]:
 *     what an erasure of location l does to the columns -- h = QLDPC_ERASURE_H_INF: the column flips with probability 1/2 given the herald;
 *     h = 1: with probability 1/4 (1 - 2q = 2^-1; one of the three projections of an erased CNOT).
 *   lut_ptr int32[n + 1], lut f64[lut_ptr[n]]: column j has c_j + 1 entries, c_j = the number of its h = 1 contributions (at most 65535);
 *     lut[lut_ptr[j]] is the column's prior without heralds, entry H >= 1 the prior LLR of (1 - (1 - 2 p_j) 2^-H) / 2.  Every entry is finite.
 * Per-shot prior: H = the sum of h over column j's contributions whose location is erased in shot b;
 *     prior[b][j] = 0.0 if one of them is QLDPC_ERASURE_H_INF, else lut[lut_ptr[j] + H].
 *   H is an integer sum: the value does not depend on the order in which the locations are met, and the device takes no logarithm.  A shot without
 *   heralds gets lut[lut_ptr[j]] bit for bit. */
#define QLDPC_ERASURE_H_INF 255
/* The prior kernel alone: heralds erased uint32[B][ceil(n_locs / 32)] (bits at or above n_locs are ignored) and one sector's tables -> prior f64[B][n].
 * Host pointers, staged on the calling thread's current device.  QLDPC_ERR_INVALID for a table that breaks a rule above (the error text names the
 * offending index); QLDPC_ERR_UNSUPPORTED when a 16-bit counter and a bit per column do not fit in 160 KB of LDS (n above about 77 000). */
int qldpc_erasure_priors(int64_t B, int32_t n_locs, const uint32_t *erased, const int32_t *loc_ptr, const int32_t *loc_col, const uint8_t *loc_h,
                         int32_t n, const int32_t *lut_ptr, const double *lut, double *prior);
/* same on device pointers of the current device; only enqueues on `stream`.  Precondition: tables that keep the rules above (a column outside
 * 0 .. n - 1 is skipped and H is held inside the column's run, so nothing outside the arrays is addressed either way). */
int qldpc_erasure_priors_dev(int64_t B, int32_t n_locs, const uint32_t *d_erased, const int32_t *d_loc_ptr, const int32_t *d_loc_col,
                             const uint8_t *d_loc_h, int32_t n, const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, void *stream);
/* The sampler axis of a plan (beside qldpc_circuit_plan_use_fixed_weight): from now on the plan's sampler draws the erasures above at rate[op code]
 * on top of its ordinary faults; rate == NULL switches them off again.  Two-way, any number of times; not a decode switch, so it goes with every
 * path and OSD stage in either call order.  _run, _run_outcomes, _sample and _sample_erasures honour it; a plan that is not on the erasure-aware
 * path decodes the syndromes as it always does (it does not read the heralds).  QLDPC_ERR_INVALID: a rate outside [0, 1) or NaN (the text names the
 * class), a plan created from a detector error model, or a plan with a fixed weight in force -- and qldpc_circuit_plan_use_fixed_weight(w >= 0)
 * returns QLDPC_ERR_INVALID while erasure noise is on.  QLDPC_ERR_UNSUPPORTED: one bit per location does not fit in LDS.  A refused call leaves the
 * plan as it was. */
int qldpc_circuit_plan_use_erasure_noise(qldpc_circuit_plan *plan, const double rate[7]);
/* A decode path, "erasure-aware decoding": the BP launch of both sectors becomes qldpc_shotprior_decode_batch's kernel with the constant `alpha`, the
 * plan's max_iter and clip_llr, no link tables, and prior[batch][n] (stride n) computed per batch from the sampler's herald record and the sector's
 * tables given here (host pointers, copied; the rules above, and lut[lut_ptr[j]] must equal the plan's prior of column j bit for bit).  While erasure
 * noise is off -- and for recorded events, which carry no heralds -- every herald is zero and the path decodes with the plan's prior (stride 0): the
 * same answers as qldpc_circuit_plan_use_correlated with no links.  The rules of that path apply: damping = 1, OSD-0, OSD-CS or LSD may follow in
 * either call order, no other path, a second call replaces the arguments; OSD-CS scores its candidates with the plan's sector prior, not the
 * per-shot one.  QLDPC_ERR_INVALID for these, for a plan created from a detector error model, for arguments qldpc_shotprior_decode_batch refuses and
 * for tables that break a rule (the text names the sector and the index); QLDPC_ERR_UNSUPPORTED when a sector's matrix is one
 * qldpc_shotprior_decode_batch or qldpc_erasure_priors refuses.  A refused call leaves the plan as it was. */
int qldpc_circuit_plan_use_erasure_aware(qldpc_circuit_plan *plan, double alpha, const int32_t *loc_ptr_z, const int32_t *loc_col_z,
                                         const uint8_t *loc_h_z, const int32_t *lut_ptr_z, const double *lut_z, const int32_t *loc_ptr_x,
                                         const int32_t *loc_col_x, const uint8_t *loc_h_x, const int32_t *lut_ptr_x, const double *lut_x);
/* qldpc_circuit_plan_sample plus erased uint32[count][ceil(n_locs / 32)] (all zero while erasure noise is off) and, where prior_z / prior_x are
 * not NULL (both or neither; needs the erasure-aware path), the per-shot priors f64[count][n_z] / f64[count][n_x] the plan would decode with. */
int qldpc_circuit_plan_sample_erasures(qldpc_circuit_plan *plan, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *sparse_z,
                                       int8_t *true_z, int8_t *sparse_x, int8_t *true_x, uint32_t *erased, double *prior_z, double *prior_x);

/* ---- per-class, biased Pauli noise.  New here: the reference has one rate p and uniform Paulis.  Circuit plans only. ------------------------------
 * The plan's own sampler fires every location at the plan's p and draws an IDLE's Pauli as r % 3 and a CNOT's as r % 15.  A noise model gives every
 * location class a rate of its own and, optionally, the Paulis of a faulty IDLE and of a faulty CNOT weights of their own (measurement five times as
 * noisy as a gate, Z-biased idles, ...).  The decoder's priors are the caller's: simulation/noise_model.py computes the matched ones on the host.
 *
 * Which locations fire, a pure function of (seed, global trial index g = trial_begin + t): rate[ty] in [0, 1) per location class, ty one of the six
 * op codes 1..6 of a base circuit (CNOT, PrepX, PrepZ, MeasX, MeasZ, IDLE; rate[0] is not read); thr[ty] = floor(rate[ty] * 2^32) (uint32; a rate of
 * 0 never fires).  Location l is faulty iff word (l & 3) of Philox4x32-10(counter = (lo32(g), hi32(g), l >> 2, 1), key = (lo32(seed), hi32(seed))) is
 * below thr[type(l)]: the words and the domain of the plain sampler, only the threshold depends on the class.
 * Which Pauli a faulty location takes: a measurement or preparation keeps its one component.  IDLE and CNOT read r = word 0 of
 * Philox4x32-10(counter = (lo32(g), hi32(g), l, 2), same key), as the plain sampler does, and pick index i of their component table (IDLE: X, Y, Z;
 * CNOT: the fifteen two-qubit Paulis in the order of noise/kernels.py:283-343; both are the plain sampler's tables):
 *     weights NULL        i = r % K                                   (K = 3 or 15: the plain sampler's choice)
 *     weights w[K]        i = #{ j < K - 1 : r >= cut[j] },           cut[j] = (uint64) floor(ldexp(S_j / S_{K-1}, 32)),
 *                         S_j = w_0 + ... + w_j, the running f64 sum in index order.
 *   The compare is a 64-bit one: cut[j] may be 2^32 (then no r reaches it).  Index i is drawn for cut[i-1] <= r < cut[i] (cut[-1] = 0, cut[K-1] = 2^32):
 *   a weight of 0 gives an empty interval, so that Pauli is never drawn -- a zero last weight included -- and every probability is within 2^-32 of
 *   w_i / S_{K-1}.  The host computes the cuts; the kernel takes them, and the seven thresholds, by value.
 * With every rate equal to the plan's p and both weight tables NULL the samples are the plain sampler's bit for bit. */
typedef struct {
    double rate[7];        /* per op code 1..6 of a base circuit (CNOT, PrepX, PrepZ, MeasX, MeasZ, IDLE); rate[0] is not read */
    const double *idle_w;  /* [3]  weights of X, Y, Z on a faulty IDLE (order of c_idle_comp), or NULL = r % 3 */
    const double *cnot_w;  /* [15] weights of the fifteen Paulis of a faulty CNOT (order of c_cnot_comp = noise/kernels.py:283-343), or NULL = r % 15 */
} qldpc_noise_model;
/* The sampler axis of a plan (beside qldpc_circuit_plan_use_fixed_weight and _use_erasure_noise): from now on the plan's sampler draws its Pauli
 * faults by `model` (copied); model == NULL switches back to the plan's own p and uniform Paulis.  Two-way, any number of times; not a decode switch,
 * so it goes with every path and OSD stage in either call order.  _run, _run_outcomes, _sample and _sample_erasures honour it (the herald record of
 * _sample_erasures stays all zero); _decode_events* and _unpack_events do not sample and are untouched.  A plan that is never switched, or is
 * switched off again, enqueues exactly what it enqueued before.
 * QLDPC_ERR_INVALID: a rate outside [0, 1) or NaN (the text names the class); a weight that is negative or not finite, or a weight table whose sum is
 * 0 (the text names the table and the index); a plan created from a detector error model; a plan with a fixed weight in force (that law needs one p);
 * a plan with erasure noise on -- and qldpc_circuit_plan_use_fixed_weight(w >= 0) and qldpc_circuit_plan_use_erasure_noise(non-NULL) return
 * QLDPC_ERR_INVALID while a model is on.  Composing a noise model with heralded erasures is deliberately out of scope: the erasure sampler draws its
 * ordinary faults at one p.  A refused call leaves the plan as it was. */
int qldpc_circuit_plan_use_noise_model(qldpc_circuit_plan *plan, const qldpc_noise_model *model);

/* ---- soft-readout noise and soft-information decoding.  New here: the reference has no counterpart.  Circuit plans only. ---------------------------
 * Every measurement of the plan's sampler is a hard bit.  A real readout is an analog signal: thresholded it gives the bit, and its distance from the
 * threshold says how far to trust it.  A readout channel has K confidence levels (1 <= K <= QLDPC_SOFT_MAX_LEVELS): the readout of a measurement
 * lands in level lv on the WRONG side with probability proportional to flip_mass[lv] and on the right side with keep_mass[lv].  The masses are
 * non-negative and finite and their sum is positive.  A decoder that reads the levels gives every measurement its own flip probability.
 *
 * Cuts: S_b = the running f64 sum of the 2K masses in bin order -- the flipped bins 0 .. K-1 first, then the kept bins K .. 2K-1 --
 *     cut[b] = (uint64) floor(ldexp(S_b / S_{2K-1}, 32)) for b <= 2K-2, cut[-1] = 0, cut[2K-1] = 2^32
 *   (the law qldpc_noise_model uses for weighted Paulis; compares are 64-bit: a cut may be 2^32, which no word reaches).
 * Level flip probabilities, from the integers, so that the decoder's belief is exactly the sampler's law:
 *     q_lv = (cut[lv] - cut[lv-1]) / ((cut[lv] - cut[lv-1]) + (cut[K+lv] - cut[K+lv-1]));
 *   a level whose two integer masses are both 0 is refused.  Marginal flip rate: qbar = cut[K-1] / 2^32.
 *
 * Readout draws, a pure function of (seed, global trial index g = trial_begin + t): the plan's ordinary faults (domains 1 and 2) are drawn first,
 * word for word as without soft readout.  On top of them every location l of class MeasX or MeasZ reads
 *     u = word (l & 3) of Philox4x32-10(counter = (lo32(g), hi32(g), l >> 2, 7), key = (lo32(seed), hi32(seed)))        (domain 7 is new)
 *     bin = #{ i <= 2K-2 : u >= cut[i] };   bin < K: flipped at level bin;   else: kept at level bin - K.
 * A flipped readout XORs the location's slot-0 signature exactly as that class's measurement fault does (component 4 for MeasX, 1 for MeasZ).
 * Level record: uint8[B][n_meas], entry k = the level of the k-th MeasX / MeasZ location in ascending l.  It holds the level only, never whether
 * the readout flipped.  With soft readout off the samples are the plain sampler's bit for bit.
 *
 * Decoder tables, per sector (simulation/soft.py builds them on the host), for a sector with n columns:
 *   meas_col int32[n_meas]: the column measurement k's readout flip lands on, -1 = it touches no column of this sector;
 *   meas_w int32[n_meas]: for a column with measurements k_0 < ... < k_{c-1}, meas_w[k_r] = K^r (mixed radix; not read where meas_col is -1);
 *   lut_ptr int32[n + 1], lut f64[lut_ptr[n]]: column j's run has K^c entries, 1 for a column without measurements and at most 65536;
 *     entry (lv_0 .. lv_{c-1}) is the prior LLR of (1 - (1 - 2 p_j) prod_r (1 - 2 q_{lv_r})) / 2.  Every entry is finite.
 * Per-shot prior: I_j = sum of level[b][k] * meas_w[k] over the measurements k with meas_col[k] = j;  prior[b][j] = lut[lut_ptr[j] + I_j].
 *   I_j is an integer sum: the value does not depend on the order in which the measurements are met, and the device takes no logarithm. */
#define QLDPC_SOFT_MAX_LEVELS 16
/* The prior kernel alone: level uint8[B][n_meas] and one sector's tables -> prior f64[B][n].  Host pointers, staged on the calling thread's current
 * device.  QLDPC_ERR_INVALID for a table that breaks a rule above (the error text names the offending index) and for a level that is not below
 * `levels` (the text names the shot and the measurement); QLDPC_ERR_UNSUPPORTED when a 16-bit counter per column does not fit in 160 KB of LDS:
 * the bound is n <= 81920. */
int qldpc_soft_priors(int64_t B, int32_t levels, int32_t n_meas, const uint8_t *level, const int32_t *meas_col, const int32_t *meas_w, int32_t n,
                      const int32_t *lut_ptr, const double *lut, double *prior);
/* same on device pointers of the current device; only enqueues on `stream`.  Precondition: tables and levels that keep the rules above (a level is
 * clamped to levels - 1, a column outside 0 .. n - 1 is skipped and I_j is held inside the column's run, so nothing outside the arrays is addressed
 * either way). */
int qldpc_soft_priors_dev(int64_t B, int32_t levels, int32_t n_meas, const uint8_t *d_levels, const int32_t *d_meas_col, const int32_t *d_meas_w,
                          int32_t n, const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, void *stream);
/* The sampler axis of a plan (beside qldpc_circuit_plan_use_fixed_weight, _use_erasure_noise and _use_noise_model): from now on the
 * plan's sampler draws the readouts above on top of its ordinary faults; flip_mass == NULL switches them off again.  Two-way, any number of times;
 * not a decode switch, so it goes with every path and OSD stage in either call order.  _run, _run_outcomes, _sample, _sample_erasures (whose herald
 * record stays all zero) and _sample_soft honour it; a plan that is not on the soft-aware path decodes the syndromes as it always does (it does not
 * read the levels).  A plan that is never switched, or is switched off again, enqueues exactly what it enqueued before.
 * QLDPC_ERR_INVALID, plan unchanged: levels outside 1..16; a mass that is negative or not finite, a sum of 0, a level without mass (the text names
 * the index); a plan created from a detector error model; a plan on the soft-aware path whose tables were built for another number of levels; a
 * fixed weight, erasure noise or a noise model in force -- and qldpc_circuit_plan_use_fixed_weight(w >= 0), _use_erasure_noise(non-NULL) and
 * _use_noise_model(non-NULL) return QLDPC_ERR_INVALID while soft readout is on.  Composing them is deliberately out of scope. */
int qldpc_circuit_plan_use_soft_readout(qldpc_circuit_plan *plan, int32_t levels, const double *flip_mass, const double *keep_mass);
/* A decode path, "soft-aware decoding": the BP launch of both sectors becomes qldpc_shotprior_decode_batch's kernel with the constant `alpha`, the
 * plan's max_iter and clip_llr, no link tables, and prior[batch][n] (stride n) computed per batch, inside the QLDPC_PHASE_SAMPLE bracket, from the
 * sampler's level record and the sector's tables given here (host pointers, copied; the rules above for `levels` levels).  While soft readout is
 * off -- and for recorded events, which carry no levels -- the path decodes with the plan's prior (stride 0): the same answers as
 * qldpc_circuit_plan_use_correlated with no links.  So the lut entry of every run of length 1 must equal the plan's prior of that column bit for
 * bit; the plan's prior of a column with measurements is the caller's (the marginal one, say), and OSD-CS keeps scoring its candidates with the
 * plan's sector prior, not the per-shot one.  The rules of the erasure-aware path apply: a circuit plan, damping = 1, OSD-0, OSD-CS or LSD may
 * follow in either call order, no other path, a second call replaces the arguments.  QLDPC_ERR_INVALID for these, for `levels` other than the
 * levels of the soft readout in force, for arguments qldpc_shotprior_decode_batch refuses and for tables that break a rule (the text names the
 * sector and the index); QLDPC_ERR_UNSUPPORTED when a sector's matrix is one qldpc_shotprior_decode_batch or qldpc_soft_priors refuses.  A refused
 * call leaves the plan as it was. */
int qldpc_circuit_plan_use_soft_aware(qldpc_circuit_plan *plan, double alpha, int32_t levels, const int32_t *meas_col_z, const int32_t *meas_w_z,
                                      const int32_t *lut_ptr_z, const double *lut_z, const int32_t *meas_col_x, const int32_t *meas_w_x,
                                      const int32_t *lut_ptr_x, const double *lut_x);
/* qldpc_circuit_plan_sample plus level uint8[count][n_meas] (all zero while soft readout is off) and, where prior_z / prior_x are not NULL (both or
 * neither; needs the soft-aware path), the per-shot priors f64[count][n_z] / f64[count][n_x] the plan would decode those levels with.  n_meas
 * is the number of MeasX / MeasZ locations of the plan's base circuit. */
int qldpc_circuit_plan_sample_soft(qldpc_circuit_plan *plan, uint64_t seed, int64_t trial_begin, int64_t count, int8_t *sparse_z, int8_t *true_z,
                                   int8_t *sparse_x, int8_t *true_x, uint8_t *level, double *prior_z, double *prior_x);

/* ---- recorded detection events in place of the sampler: events -> decode -> OSD -> predict.  New here: the reference has no counterpart. ---------
 * The second front door of a circuit plan, for plans of qldpc_circuit_plan_create and _create_dem alike: the syndromes come from the caller's records
 * (Stim samples, hardware shots) and the predicted observable flips go back, the `decode_batch` of other DEM decoders.  Everything between is the plan's:
 * the same buffers, the same decode of a sector, every qldpc_circuit_plan_use_* switch.  Nothing here touches the tally, the sampled truth or the outcomes,
 * and _run, _run_outcomes and _sample are unaffected by calls made before them.
 *
 * The record format: shot i starts at byte i * stride of `events`; bit d of a record is (rec[d >> 3] >> (d & 7)) & 1 (Stim's "b8").  n_bits is the number of
 * bits rows may name; a record holds at least ceil(n_bits / 8) bytes (stride may be larger: the bytes beyond, and the high bits of the last byte, are never
 * used; bytes beyond are never read).
 * The layout: row r of sector s (a row of that sector's graph; what _sample calls sparse_z / sparse_x) reads bit bit_of_row<s>[r]; -1 makes the row
 * constant 0; a bit no row names is ignored; two rows may name one bit.  Without a call the layout is the default: sector 0's rows, then sector 1's
 * (n_bits = rows of g0 + rows of g1).  _set_event_layout may be called again; NULL for a sector = a contiguous run at that sector's default base (0, and
 * the rows of g0); the tables are copied.  bit_of_row1 is ignored on a one-sector plan.  QLDPC_ERR_INVALID: n_bits outside 1..131070, a table entry outside
 * [-1, n_bits), n_bits too small for a default run. */
int qldpc_circuit_plan_set_event_layout(qldpc_circuit_plan *plan, int32_t n_bits, const int32_t *bit_of_row0, const int32_t *bit_of_row1);
/* Decodes `count` records (host memory) in pieces of the plan's batch: per batch, copy to the device and unpack (inside the QLDPC_PHASE_SAMPLE bracket),
 * decode + OSD of every sector inside their brackets exactly as _run does, predict (inside QLDPC_PHASE_JUDGE), copy the results back, synchronise `stream`.
 *   pred0[i] / pred1[i]: bit r = the correction of shot i flips observable r of sector 0 / 1 (the XOR of the logical masks of the correction's ones);
 *   flags[i]: bit 0 / 1 = BP (or whatever the plan's path is) converged in sector 0 / 1, bit 2 / 3 = the correction does NOT reproduce the sector's
 *   syndrome, bit 4 / 5 = the sector's syndrome was all zero.
 * A one-sector plan leaves the odd flag bits 0; pred1 may then be NULL and is zeroed otherwise.
 * seed and shot_begin + i go where _run passes its seed and trial index: Relay-BP draws from them, every other path ignores them.  So the result for a
 * shot is a pure function of (record, seed, shot_begin + i): it depends neither on the plan's batch nor on how a range is split over calls.
 * QLDPC_ERR_INVALID, with qldpc_last_error naming the argument: plan, events, pred0, flags (pred1 with two sectors) NULL; count or shot_begin negative;
 * stride below ceil(n_bits / 8) (or above 2^30).  count == 0 returns QLDPC_OK and touches nothing. */
int qldpc_circuit_plan_decode_events(qldpc_circuit_plan *plan, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *events,
                                     int64_t stride, void *stream, uint64_t *pred0, uint64_t *pred1, uint8_t *flags);
/* The same on device pointers: everything is enqueued on `stream`, nothing is copied and nothing synchronised. */
int qldpc_circuit_plan_decode_events_dev(qldpc_circuit_plan *plan, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *d_events,
                                         int64_t stride, void *stream, uint64_t *d_pred0, uint64_t *d_pred1, uint8_t *d_flags);
/* qldpc_circuit_plan_decode_events[_dev] on a plan with a confidence (qldpc_circuit_plan_use_confidence), and score[i] of shot i (uint64[count], host /
 * device like the other outputs).  Recorded events have no outcome, so the plan's histogram is left alone.  QLDPC_ERR_INVALID on a plan without a
 * confidence or with score NULL; predictions and flags are those of the unscored call. */
int qldpc_circuit_plan_decode_events_scored(qldpc_circuit_plan *plan, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *events,
                                            int64_t stride, void *stream, uint64_t *pred0, uint64_t *pred1, uint8_t *flags, uint64_t *score);
int qldpc_circuit_plan_decode_events_scored_dev(qldpc_circuit_plan *plan, uint64_t seed, int64_t shot_begin, int64_t count, const uint8_t *d_events,
                                                int64_t stride, void *stream, uint64_t *d_pred0, uint64_t *d_pred1, uint8_t *d_flags,
                                                uint64_t *d_score);
/* The unpacker alone, the counterpart of qldpc_circuit_plan_sample: sparse0 int8[count][rows of g0], sparse1 int8[count][rows of g1] (host; values
 * 0 / 1; sparse1 may be NULL on a one-sector plan). */
int qldpc_circuit_plan_unpack_events(qldpc_circuit_plan *plan, int64_t count, const uint8_t *events, int64_t stride, int8_t *sparse0, int8_t *sparse1);

/* ---- (e) multi-GPU: the one collective of the path, natively on RCCL --------------------------------------------------------
 * Sum of the int64[QLDPC_TALLY_SLOTS] tally over the GPUs of a node; replaces the Python loop that sums the workers' results in
 * src/simulation/engine.py:450-457.  librccl is loaded on the first qldpc_comm_* call.  Two ways to form the communicator:
 *   qldpc_comm_init_all(ndev, devices, &comm)            one process drives `ndev` GPUs (ncclCommInitAll); devices NULL = 0..ndev-1
 *   qldpc_comm_unique_id(id) on rank 0, id handed to the other ranks by the launcher, then
 *   qldpc_comm_init_rank(nranks, rank, id, device, &comm)  one process per GPU (ncclCommInitRank)
 * qldpc_tally_allreduce(comm, tallies): host int64[nlocal][QLDPC_TALLY_SLOTS] (nlocal = ndev after init_all, 1 after init_rank);
 * on return every row holds the sum over all ranks.  The _dev form reduces a device-resident tally in place on `stream` without
 * synchronising; with several local ranks, issue the calls of all local ranks between qldpc_comm_group_begin / _end. */
#define QLDPC_COMM_ID_BYTES 128
typedef struct qldpc_comm qldpc_comm;
int qldpc_comm_init_all(int ndev, const int *devices, qldpc_comm **out);
int qldpc_comm_unique_id(uint8_t *id /* [QLDPC_COMM_ID_BYTES] */);
int qldpc_comm_init_rank(int nranks, int rank, const uint8_t *id, int device, qldpc_comm **out);
int qldpc_comm_size(const qldpc_comm *comm, int *nranks, int *nlocal);
int qldpc_tally_allreduce(qldpc_comm *comm, int64_t *tallies);
int qldpc_tally_allreduce_dev(qldpc_comm *comm, int local_rank, int64_t *d_tally, void *stream);
int qldpc_comm_group_begin(void);
int qldpc_comm_group_end(void);
void qldpc_comm_destroy(qldpc_comm *comm);

/* Philox4x32-10 reference vector helper (host; lets tests pin the generator against the oracle) */
void qldpc_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* Diagnostic: the device allocations the library's own handles hold right now, process-wide and over all devices -- *buffers their number, *bytes
 * their sum (either may be NULL).  Every handle's device memory is counted, staging of a host-pointer call in flight included; memory the caller
 * allocated and the diagnostic build's process-lifetime timer buffer are not.  A handle's destroy function brings both numbers back to what they
 * were before its create, which is what tests of ownership compare (a shared card's free-memory figure moves with other processes). */
int qldpc_device_memory(int64_t *buffers, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* QLDPC_HIP_H */
