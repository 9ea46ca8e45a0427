// Every prototype and host-only struct that one .hip file implements for another, for the whole library.  Nothing here can reach a kernel's
// instruction stream: no device function, no kernel argument struct, no constant a kernel body names (those live in the device headers, which
// tools/isa_mix.py RECORDED lists per kernel).  Appending to this file therefore leaves every committed instruction count valid.
#pragma once
#include "common.h"

#include <functional>
#include <vector>

struct qldpc_window_decoder;
struct qldpc_layered_decoder;

namespace qldpc {

struct OsdLaunch;      // osd_plan.h
struct OsdGjArgs;      // osd_gj.h
struct SigTab;         // sampler_common.h
struct SampleOut;      // sampler_common.h
struct JudgeSector;    // judge.h
struct EventsSector;   // judge.h

// internal flag (upper half of `flags`): the caller verified on the host that every prior is finite
#define QLDPC_FLAG_PUBLIC_MASK 0x0FFFFFFF          // flag bits callers may set (include/qldpc_hip.h)
#define QLDPC_FLAG_INTERNAL_PRIOR_FINITE 0x40000000
#define QLDPC_FLAG_INTERNAL_PRIOR_LE_CLIP 0x20000000   // ... and every |prior| <= clip (iteration 0 then needs no unclipped special case)
#define QLDPC_FLAG_INTERNAL_OSD_QUEUE_CLEAN 0x10000000 // OSD-0 launches: the handle's small-kernel ticket counter is zero and the caller zeroes it again afterwards

// Host-side launchers implemented by the kernel files.
int minsum_stream_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                         const double *d_alpha, double damping, double clip, int flags, int8_t *d_err, double *d_llr,
                         uint8_t *d_conv, int32_t *d_iter, hipStream_t stream);

int minsum_resident_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                           const double *d_alpha, double damping, double clip, int flags, int8_t *d_err, double *d_llr,
                           uint8_t *d_conv, int32_t *d_iter, hipStream_t stream);
bool resident_supported(const qldpc_graph *g, double damping);
int resident_detail(const qldpc_graph *g, double damping);     // QLDPC_DETAIL_RES_* | QLDPC_DETAIL_DAMPING of a launch on this graph
int mc_resident_launch(const qldpc_graph *g, int64_t B, const double *d_prior, int max_iter, const double *d_alpha, double clip, int flags,
                       uint64_t seed, int64_t shot_begin, uint32_t thr, int use_osd, const uint64_t *d_Lmask, void *d_cold, hipStream_t stream);
// regular-degree fast path (minsum_regular.hip).  nanfree: the caller proved prior / clip / alphas finite.
bool regular_supported(const qldpc_graph *g, double clip, int max_iter);
int minsum_regular_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                          const double *d_alpha, double damping, double clip, int flags, bool nanfree, int8_t *d_err, double *d_llr,
                          uint8_t *d_conv, int32_t *d_iter, hipStream_t stream);
int mc_regular_launch(const qldpc_graph *g, int64_t B, const double *d_prior, int max_iter, const double *d_alpha, double clip, int flags,
                      bool nanfree, uint64_t seed, int64_t shot_begin, uint32_t thr, int use_osd, const uint64_t *d_Lmask,
                      void *d_cold, hipStream_t stream, const int32_t *d_shot_list = nullptr, const int32_t *d_shot_count = nullptr);
// bit-sliced first iteration of a uniform-prior Monte-Carlo plan under reference semantics (mc_first.hip)
bool mc_first_table(const qldpc_graph *g, double p0, double alpha0, double clip, int max_iter, unsigned &negbits);
int mc_first_launch(const qldpc_graph *g, int k, const int32_t *d_lptr, const int32_t *d_lidx, int64_t B, uint64_t seed, int64_t shot_begin, uint32_t thr,
                    unsigned negbits, unsigned long long *d_tally, int32_t *d_cont_list, int32_t *d_cont_count, unsigned long long *d_clk, hipStream_t stream);
void mc_first_set_bits(int bits);
void regular_set_list_shots(int s);
void regular_set_own_edges(int v);
void regular_set_place(int v);           // minsum_regular.hip: qldpc_set_option("regular_place")
void regular_set_wave_classes(int v);    // minsum_regular.hip: qldpc_set_option("regular_wave_classes")
int regular_own_search_choice();         // options.hip: qldpc_set_option("regular_own_search"), read by qldpc_graph_create
void mc_set_big_lanes(int n);
int mc_tail_overlap_choice();  // qldpc_set_option("mc_tail_overlap"): 1 = OSD-0 + judge of a batch on a side stream beside the next batch's decode (default)
int mc_first_choice();       // qldpc_set_option("mc_first_iteration"): 1 = use it where it applies (default), 0 = full decoder for every shot
int mc_regular_fill_cold(void *d_cold, unsigned long long *d_tally, int32_t *d_fail_count, int32_t *d_fail_list, int8_t *f_synd,
                         int8_t *f_err, int8_t *f_hard, double *f_llr, unsigned long long *d_clk);
size_t mc_regular_cold_bytes();
int judge_failed_launch(const qldpc_graph *g, int32_t *d_count, bool reset_counters, int *d_osd_queue, const uint64_t *d_Lmask, const int8_t *f_err, const int8_t *f_synd,
                        const int8_t *f_dec, unsigned long long *d_tally, hipStream_t stream);
// wave-private kernel for (6,3)-regular graphs and clean inputs (minsum_wave.hip); option "regular_kernel" selects between the two
bool wave_supported(const qldpc_graph *g, double damping, bool clean);
int wave_kernel_choice();     // 0 automatic, 1 team kernel, 2 wave kernel (qldpc_set_option)
int minsum_wave_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter, const double *d_alpha,
                       double clip, int flags, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t stream);
int mc_wave_launch(const qldpc_graph *g, int64_t B, const double *d_prior, int max_iter, const double *d_alpha, double clip, int flags,
                   uint64_t seed, int64_t shot_begin, uint32_t thr, int use_osd, const uint64_t *d_Lmask, void *d_cold, hipStream_t stream);
// workgroup-per-shot kernel for large graphs (minsum_wg.hip)
bool wg_supported(const qldpc_graph *g, double damping);
int minsum_wg_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter, const double *d_alpha,
                     double damping, double clip, int flags, bool clean, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t stream);
// which form of that kernel a call gets: decided once here, launched by minsum_wg_launch and reported by qldpc_minsum_decode_path
struct WgChoice {
    bool vg, damp, lean, ridx, has_deg1;   // posteriors in global memory; damping slab; lean kernel; row indices in registers; degree-1 template
    int nan_deg1_only, block, edge_lanes;
    int detail() const {
        return (lean ? QLDPC_DETAIL_LEAN : 0) | (ridx ? QLDPC_DETAIL_REG_INDICES : 0) | (vg ? QLDPC_DETAIL_VGLOBAL : 0) | (damp ? QLDPC_DETAIL_DAMPING : 0) |
               (block == 1024 ? QLDPC_DETAIL_BLOCK_1024 : 0) | (has_deg1 ? QLDPC_DETAIL_DEG1 : 0) | (nan_deg1_only ? QLDPC_DETAIL_NAN_DEG1_ONLY : 0);
    }
};
// the degree-1 checks of a graph (their messages are +-inf): whether it has any, and whether no column meets two of them -- then a NaN can only arise
// on the edge of a degree-1 check itself.  What WgChoice and the tables of minsum_wg2.hip both record.
struct Deg1 { bool any; int nan_deg1_only; };
Deg1 deg1_checks(const qldpc_graph *g);
WgChoice wg_choose(const qldpc_graph *g, double damping, int flags, bool clean);
int wg_check_variant(int flags);                 // QLDPC_ERR_UNSUPPORTED for an experiment selector in the product library
// LDS-resident form of that kernel for callers whose prior is known on the host (minsum_wg2.hip); *out = NULL when the input is not eligible
struct Wg2Prep;
int wg2_prepare(const qldpc_graph *g, const double *h_prior, const Wg2Prep **out);
int minsum_wg2_launch(const qldpc_graph *g, const Wg2Prep *P, int64_t B, const int8_t *d_synd, int max_iter, const double *d_alpha, double clip, int flags,
                      int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t stream);
void wg2_cache_free(void *cache);
int wg2_detail(const Wg2Prep *P);                // QLDPC_DETAIL_* bits of a launch with these tables
// the decoder form a call takes (QLDPC_PATH_*, QLDPC_DETAIL_*) and, for QLDPC_PATH_WG2, its tables; callers hold g->mu
struct DecodePath { int path, detail; const Wg2Prep *prep; };
int select_decode_path(const qldpc_graph *g, int max_iter, double damping, double clip, int flags, bool nanfree, const double *h_prior, DecodePath &out);
// "clean" decoder inputs, verified on the host: every prior finite and not -0.0, clip finite > 0, every alpha finite > 0.
// Then no message or posterior can be -0.0 and no |q| NaN, which the regular and lean kernels exploit (see their headers).
bool inputs_clean(const double *prior, int n, double clip, const double *alpha, int n_alpha);
// Relay-BP (relay_bp.hip): memory min-sum in legs.  Parameters as in qldpc_relay_decode_batch; callers validate them with relay_check_params.
struct RelayParams { double alpha, clip, gamma0, gamma_min, gamma_max; int t0, tr, max_legs, stop_after; };
int relay_check_params(const RelayParams &P);
int relay_mode(const qldpc_graph *g);            // 0: not supported, 1: V in LDS, 2: V in a per-workgroup HBM/L2 slab
int relay_unsupported(const qldpc_graph *g);     // sets the error text, returns QLDPC_ERR_UNSUPPORTED
// callers hold g->mu.  iter_bias is added to every iteration count written to d_iters; d_legs / d_sol may be NULL
int relay_decode_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, const RelayParams &P, uint64_t seed,
                        int64_t shot_begin, int tag, int iter_bias, int8_t *d_err, uint8_t *d_conv, int32_t *d_legs, int32_t *d_iters,
                        int32_t *d_sol, hipStream_t stream);
int relay_legs_tally_launch(int64_t B, const int32_t *d_legs_z, const int32_t *d_legs_x, unsigned long long *d_tally, hipStream_t stream);
// BP with guided decimation (decimation.hip): rounds of constant-alpha min-sum with the most reliable columns frozen in between.  Parameters as in
// qldpc_decim_decode_batch; callers validate them with decim_check_params.
struct DecimParams { double alpha, clip, fix; int t_round, max_rounds, per_round; };
int decim_check_params(const DecimParams &P);
bool decim_supported(const qldpc_graph *g);
int decim_unsupported(const qldpc_graph *g);     // sets the error text, returns QLDPC_ERR_UNSUPPORTED
// callers hold g->mu.  iter_bias is added to every iteration count written to d_iters; d_llr / d_rounds / d_fixed may be NULL
int decim_decode_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, const DecimParams &P, int iter_bias, int8_t *d_err,
                        double *d_llr, uint8_t *d_conv, int32_t *d_iters, int32_t *d_rounds, int32_t *d_fixed, hipStream_t stream);
// Min-sum with a per-shot prior (shot_prior.hip): P[b][j] = min(prior[b * stride + j], the link_llr of column j's links whose source fired in src_err[b]),
// then one leg of constant-alpha min-sum with that prior.  ShotLinks: device pointers, ptr == NULL means no tables (the other three are then NULL as well).
struct ShotLinks { int n_src; const int8_t *src_err; const int32_t *ptr, *src; const double *llr; };
int shotprior_check_params(double alpha, double clip_llr, int max_iter);
// host tables of n columns: ptr[0] = 0 and monotone, 0 <= src < n_src strictly ascending inside a column's run, every llr finite (the text names the index)
int shotprior_check_links(int n, int n_src, const int32_t *link_ptr, const int32_t *link_src, const double *link_llr);
int shotprior_mode(const qldpc_graph *g);        // 0: not supported; where V / P live with link tables: 1 LDS / LDS, 2 LDS / global, 3 global / global
int shotprior_unsupported(const qldpc_graph *g); // sets the error text, returns QLDPC_ERR_UNSUPPORTED
// callers hold g->mu.  stride: 0 or n.  iter_bias is added to every iteration count written to d_iters; d_llr / d_prior_out may be NULL
int shotprior_decode_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int64_t stride, const ShotLinks &K, double alpha,
                            double clip, int max_iter, int iter_bias, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iters, double *d_prior_out,
                            hipStream_t stream);
// h_prior: the same prior on the host when the caller has it (a circuit plan, the host-pointer entry point), else NULL
int minsum_decode_dispatch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                           const double *d_alpha, double damping, double clip, int flags, bool nanfree, int8_t *d_err, double *d_llr,
                           uint8_t *d_conv, int32_t *d_iter, hipStream_t stream, const double *h_prior = nullptr);

// ---- Monte-Carlo pipeline and circuit plan ----
int build_alpha_table(int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len, std::vector<double> &tab);
int gf2_spmv_launch(const qldpc_graph *g, int64_t B, const int8_t *d_vec, int8_t *d_out, hipStream_t stream);

// OSD-0 on the shots listed in d_list[0 .. *d_count) (device-resident count: no host sync).  d_ordering may be NULL
// (stable ascending |llr|); otherwise int32[B][n] indexed by shot.  solution may alias hard.  max_listed: an upper bound of *d_count.
// judge: a caller's per-record judge (logical failure / syndrome check of the solution against the true error, tallied) that the launch MAY take over --
// the one-wave kernels of small matrices do (fused = true on return); the caller launches its own judge kernel when fused stays false
struct OsdJudge { const int8_t *err; const uint64_t *Lmask; unsigned long long *tally; int32_t *count; int64_t max_listed; bool fused; };
int osd0_listed_launch(const qldpc_graph *g, const int32_t *d_list, const int32_t *d_count, int64_t max_listed, const int8_t *d_synd, const double *d_llr,
                       const int8_t *d_hard, const int32_t *d_ordering, int8_t *d_solution, int flags, hipStream_t stream, OsdJudge *judge = nullptr);
// OSD-CS (osd_cs.hip) on the listed shots, weights on the device; the shots whose right-hand side lies outside the column space go through
// osd0_listed_launch behind it.  Callers hold g->mu and have checked order (osdcs_check_order) and the graph (osdcs_supported).
int osdcs_listed_launch(const qldpc_graph *g, const int32_t *d_list, const int32_t *d_count, int64_t max_listed, const int8_t *d_synd,
                        const double *d_llr, const int8_t *d_hard, const double *d_weights, int order, int8_t *d_solution, int32_t *d_flips,
                        hipStream_t stream);
int osdcs_check_order(int order);
// BP+LSD (lsd.hip) on the listed shots; the shots that end capped or without candidates go through osd0_listed_launch behind it.  d_info int32[B][4];
// d_counts (may be NULL): uint64[3], the shots that ended with flag 0 / 1 / 2, accumulated by the kernel.  Callers hold g->mu and have checked the
// parameters (lsd_check_params) and the graph at that cap (lsd_graph_supported: QLDPC_OK, or QLDPC_ERR_UNSUPPORTED with the error text set).
// d_stats (may be NULL): uint64[B][8], the cluster statistics of the listed shots (qldpc_lsd_stats_batch), with d_weight uint16[n] (may be NULL).
int lsd_listed_launch(const qldpc_graph *g, const int32_t *d_list, const int32_t *d_count, int64_t max_listed, const int8_t *d_synd, const double *d_llr,
                      const int8_t *d_hard, int bits_per_step, int max_rows, int8_t *d_solution, int32_t *d_info, unsigned long long *d_counts,
                      const uint16_t *d_weight, unsigned long long *d_stats, hipStream_t stream);
int lsd_check_params(int bits_per_step, int max_rows);
int lsd_graph_supported(const qldpc_graph *g, int max_rows);
// The confidence of B trials (confidence.hip) from the cluster statistics uint64[B][8] of sector Z and of sector X (NULL: one sector): d_score[B], and
// with d_hist (may be NULL; then nbins = 1) hist[bin][d_outcome[b] & 3] += 1 at bin = #{d_edges <= score}.  kind and the edges have passed
// confidence_check (QLDPC_OK, or QLDPC_ERR_INVALID with the error text set).
constexpr int kConfLdsMax = 4096 * 8 + 4096 * 16;      // the edge table and the workgroup's counts at QLDPC_CONF_MAX_BINS
int confidence_launch(int device, int64_t B, int kind, const unsigned long long *d_stats_z, const unsigned long long *d_stats_x, const uint8_t *d_outcome,
                      unsigned long long *d_score, int nbins, const unsigned long long *d_edges, unsigned long long *d_hist, hipStream_t stream);
int confidence_check(int kind, int nbins, const uint64_t *edges);
// Sliding-window decoding (window.hip) inside a circuit plan.  create_tab: qldpc_window_decoder_create on a ready alpha table.  lock_and_launch enqueues
// the window loop for B shots; the last window's commit fills the plan's per-trial slots: conv = 1 iff every window converged, iter = iterations - 1 (the
// judge adds one per trial), *osd_count += 1 per trial with an OSD-0 window.  mark(0 / 1, open) brackets the BP and the OSD + commit part of every window.
struct WindowPlanSlots { uint8_t *conv; int32_t *iter; int32_t *osd_count; };
int window_decoder_create_tab(const qldpc_graph *g, int layer_rows, int window, int commit, const double *prior, int max_iter,
                              const std::vector<double> &tab, double clip_llr, int flags, qldpc_window_decoder **out);
int window_decoder_lock_and_launch(qldpc_window_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, const WindowPlanSlots *plan,
                                   const std::function<int(int, bool)> *mark, hipStream_t s);
// Layered-schedule min-sum (minsum_layered.hip) inside a circuit plan.  create_tab: qldpc_layered_decoder_create on a ready alpha table (row_layer NULL = the
// greedy colouring).  lock_and_launch enqueues the decode of B shots with the outputs of minsum_decode_dispatch.
int layered_decoder_create_tab(const qldpc_graph *g, const int32_t *row_layer, const double *prior, int max_iter, const std::vector<double> &tab,
                               double clip_llr, int flags, qldpc_layered_decoder **out);
int layered_lock_and_launch(qldpc_layered_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter,
                            hipStream_t s);
// Single-precision min-sum (minsum_f32.hip) inside a circuit plan.  create_tab: qldpc_minsum32_decoder_create on a ready f64 alpha table.
// lock_and_launch enqueues the decode of B shots with the outputs of minsum_decode_dispatch.
int minsum32_decoder_create_tab(const qldpc_graph *g, const double *prior, int max_iter, const std::vector<double> &tab, double clip_llr, int flags,
                                qldpc_minsum32_decoder **out);
int minsum32_lock_and_launch(qldpc_minsum32_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter,
                             hipStream_t s);
int osdcs_supported(const qldpc_graph *g);      // QLDPC_OK, or QLDPC_ERR_UNSUPPORTED with the error text set
// The samplers of a circuit plan.  Every *_sample_launch takes (B, trial_begin, seed, its own parameters, the two sectors' SigTab, SampleOut, stream);
// SigTab and SampleOut (sampler_common.h) hold device pointers and travel to the kernel by value.
// Detector-error-model sampler (dem.hip).  T0 / T1: the sectors' projections of the mechanisms: ptr int32[n_mech + 1], idx detector indices, log the logical
// masks.  d_thr: uint32 thresholds, zero-padded to a multiple of four.
int dem_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, int n_mech, const uint32_t *d_thr, const SigTab &T0, const SigTab &T1, const SampleOut &O,
                      hipStream_t s);
int dem_validate(const qldpc_dem_desc *D);      // QLDPC_OK, or QLDPC_ERR_INVALID with the error text naming the sector or the mechanism
// Fixed-weight sampler of a circuit plan (fixed_weight.hip): exactly `weight` members of 0 .. n_locs - 1 per trial.  dem = false: T0 / T1 are the fault signatures
// of sectors Z / X (entry 2 * location + slot) and d_loc_type the locations' op types; dem = true: the mechanisms' projections (entry = mechanism), d_loc_type
// unused.  fixed_weight_check: the limits of (n_locs, weight), QLDPC_ERR_INVALID / _UNSUPPORTED with the text set.
int fixed_weight_check(int64_t n_locs, int weight);
int fixed_weight_sample_launch(int device, int64_t B, int64_t trial_begin, uint64_t seed, int weight, int n_locs, bool dem, const uint8_t *d_loc_type,
                               const SigTab &T0, const SigTab &T1, const SampleOut &O, hipStream_t s);
// Heralded-erasure noise of a circuit plan (erasure.hip).  sample: circuit_sample_kernel's draws at threshold thr plus the erasures at ethr[op code]
// (erasure_rates_check turns rate[7] into them: QLDPC_ERR_INVALID naming the class), the herald record uint32[B][ceil(n_locs / 32)] written to d_erased.
// prior: heralds and the tables of one sector (device pointers) -> d_prior f64[B][n].  check_tables: the table rules of qldpc_erasure_priors on host
// arrays, QLDPC_ERR_INVALID with the text naming the offending index.  *_supported: QLDPC_OK, or QLDPC_ERR_UNSUPPORTED with the text set (LDS).
int erasure_rates_check(const double *rate, uint32_t thr[8]);
int erasure_sample_supported(int nsx, int nsz, int64_t n_locs);
int erasure_sample_launch(int device, int64_t B, int64_t trial_begin, uint64_t seed, uint32_t thr, const uint32_t ethr[8], int n_locs,
                          const uint8_t *d_loc_type, const SigTab &Z, const SigTab &X, const SampleOut &O, uint32_t *d_erased, hipStream_t s);
int erasure_check_tables(int n_locs, const int32_t *loc_ptr, const int32_t *loc_col, const uint8_t *loc_h, int n, const int32_t *lut_ptr, const double *lut);
int erasure_prior_supported(int n);
int erasure_prior_launch(int device, int64_t B, int n_locs, const uint32_t *d_erased, const int32_t *d_loc_ptr, const int32_t *d_loc_col,
                         const uint8_t *d_loc_h, int n, const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, hipStream_t s);
// Per-class, biased Pauli noise of a circuit plan (noise_model.hip).  NoiseModelHost: what a checked qldpc_noise_model becomes on the host -- the
// threshold per op code, whether a weight table was given and its cuts (uint64: a cut may be 2^32).  check: the rules of
// qldpc_circuit_plan_use_noise_model on the model alone, QLDPC_ERR_INVALID with the text naming the class or the index.  pack_classes: the op codes
// of the four locations of Philox block b as the four bytes of word b (zero padding: class 0 has threshold 0).  sample: circuit_sample_kernel with a
// threshold per class and the cut-based Pauli choice; d_loc_cls is pack_classes' array on the device.
struct NoiseModelHost { uint32_t thr[8]; bool idle_weighted, cnot_weighted; uint64_t idle_cut[2], cnot_cut[14]; };
int noise_model_check(const qldpc_noise_model *M, NoiseModelHost *out);
std::vector<uint32_t> noise_model_pack_classes(const std::vector<uint8_t> &loc_type);
int noise_model_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, const NoiseModelHost &M, int n_locs, const uint32_t *d_loc_cls, const SigTab &Z,
                              const SigTab &X, const SampleOut &O, hipStream_t s);
// Soft-readout noise of a circuit plan (soft.hip).  SoftReadoutHost: what checked masses become on the host -- K and the 2K cuts of the law (uint64:
// the last is 2^32).  readout_check: the rules of qldpc_circuit_plan_use_soft_readout on the masses alone, QLDPC_ERR_INVALID with the text naming the
// index.  sample: circuit_sample_kernel's draws at threshold thr plus the readout bins, the level record uint8[B][n_meas] written to d_levels;
// d_loc_cls is noise_model_pack_classes' array on the device, d_meas_rank int32[n_locs] the rank of a MeasX / MeasZ location among them.  prior: levels
// and the tables of one sector (device pointers) -> d_prior f64[B][n].  check_tables: the table rules of qldpc_soft_priors on host arrays,
// QLDPC_ERR_INVALID with the text naming the offending index.  prior_supported: QLDPC_OK, or QLDPC_ERR_UNSUPPORTED with the text set (LDS).
struct SoftReadoutHost { int levels; uint64_t cut[32]; };
int soft_readout_check(int levels, const double *flip_mass, const double *keep_mass, SoftReadoutHost *out);
int soft_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, uint32_t thr, const SoftReadoutHost &R, int n_locs, const uint8_t *d_loc_type,
                       const uint32_t *d_loc_cls, const int32_t *d_meas_rank, int n_meas, const SigTab &Z, const SigTab &X, const SampleOut &O, uint8_t *d_levels,
                       hipStream_t s);
int soft_check_tables(int levels, int n_meas, const int32_t *meas_col, const int32_t *meas_w, int n, const int32_t *lut_ptr, const double *lut);
int soft_prior_supported(int n);
int soft_prior_launch(int device, int64_t B, int levels, int n_meas, const uint8_t *d_levels, const int32_t *d_meas_col, const int32_t *d_meas_w, int n,
                      const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, hipStream_t s);
// Recorded detection events in place of a sampler (events.hip).  unpack: B bit-packed records (shot i at d_events + i * stride, bit d = (rec[d >> 3] >> (d & 7)) & 1;
// only the first ceil(n_bits / 8) bytes of a record are read) -> the sectors' syndromes int8[B][nsyn]; d_fail_counts as SampleOut's fail_counts (may be NULL).
// predict: the judge without a truth -- pred[b] = XOR of the logical masks of the correction's ones; flags[b] bit 0 / 1 = converged, 2 / 3 = the correction does
// not reproduce the syndrome, 4 / 5 = zero syndrome, of sector 0 / 1.  two = false: sector 1 is not touched and its bits stay 0.
int events_unpack_launch(int64_t B, const uint8_t *d_events, int64_t stride, int n_bits, const EventsSector &S0, const EventsSector &S1, bool two,
                         int32_t *d_fail_counts, hipStream_t s);
int events_predict_launch(int64_t B, const JudgeSector &Z, const JudgeSector &X, bool two, unsigned long long *d_pred0, unsigned long long *d_pred1,
                          uint8_t *d_flags, hipStream_t s);

unsigned long long *osd_timer_buffer();      // device buffer of the current device, NULL in the default build

// ---- OSD-0: the launchers osd0_listed_launch (gf2.hip) calls for the kernels its plan chose, and what they share.  Callers hold g->mu.
// the shots of a launch: list [0 .. *count) on the device, *count <= max_listed; the arrays are indexed by shot
struct OsdShots { const int32_t *list, *count; int64_t max_listed; const int8_t *synd; const double *llr; const int8_t *hard; const int32_t *ordering; int8_t *solution; };
int osd0_small_launch(const qldpc_graph *g, const OsdLaunch &L, const OsdShots &S, hipStream_t stream, int flags, struct OsdJudge *judge);      // osd_small.hip
int osd0_gj_launch(const qldpc_graph *g, const OsdLaunch &L, const OsdShots &S, hipStream_t stream, bool w16, bool queue_first);        // osd_gj.hip
int osd0_gjg_launch(const qldpc_graph *g, const OsdLaunch &L, const OsdShots &S, hipStream_t stream);                                   // osd_gjg.hip
int osd_ug_slabs(const qldpc_graph *g, int grid, bool ug, uint16_t *&ordws, unsigned long long *&U, unsigned long long *&keys);          // gf2.hip
int host_gf2_rank(const qldpc_graph *g);      // gf2.hip: rank of H over GF(2), what g->gf2_rank caches
int ensure_col_rows(const qldpc_graph *g);    // gf2.hip: g->d_col_rows on first use
int osd_small_queue(const qldpc_graph *g, int **queue);      // osd_small.hip: the ticket counter of the one-wave kernels
void iota_list_launch(int64_t B, int32_t *list, int32_t *count, hipStream_t s);      // gf2.hip: list = 0 .. B - 1, *count = B
int osd_presort_choice();          // option "osd_presort" (options.hip); osd_presort_columns (osd_plan.h) turns it into P.presort
int osd_gj_fill(const qldpc_graph *g, const OsdShots &S, hipStream_t stream, OsdGjArgs &P);      // osd_gj.hip: what GJ and GJG fill alike
#ifdef QLDPC_EXPERIMENTS
int osd0_gjq_launch(const qldpc_graph *g, const OsdGjArgs &base, int grid, hipStream_t stream, bool &launched);      // osd_gjq.hip
#endif

}  // namespace qldpc
