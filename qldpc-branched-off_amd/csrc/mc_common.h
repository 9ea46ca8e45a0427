// Philox4x32-10 counter-based generator and shared declarations of the Monte-Carlo pipeline.
// Stream definition (a pure function of (seed, shot, block, domain), reproducible on any device):
//   key = (seed_lo, seed_hi); counter = (shot_lo, shot_hi, block, domain).
//   domain 0: code-capacity error bits -- bit j of a shot uses word (j & 3) of block (j >> 2); error iff word < thr,
//   thr = floor(p * 2^32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <functional>
#include <vector>

#include "../../include/qldpc_hip.h"

struct qldpc_graph;
struct qldpc_window_decoder;
struct qldpc_layered_decoder;

namespace qldpc {

__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                       uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// NB independent Philox4x32-10 blocks with the ROUND loop outermost: the ten rounds of one block are a dependent chain of 64-bit multiplies
// (ILP 2); written one block after the other the compiler leaves them that way and a wave that holds several blocks waits for every multiply
// (mc_first.hip: 2.6x off its issue time).  Same outputs as philox4x32_10 per block: block i uses counter (c0[i], c1[i], c2, c3).
template <int NB>
__device__ __forceinline__ void philox4x32_10_batch(const uint32_t (&c0)[NB], const uint32_t (&c1)[NB], uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                    uint32_t (&out)[NB][4]) {
    uint32_t a[NB], b[NB], c[NB], d[NB];
#pragma unroll
    for (int i = 0; i < NB; i++) { a[i] = c0[i]; b[i] = c1[i]; c[i] = c2; d[i] = c3; }
#pragma unroll
    for (int r = 0; r < 10; r++) {
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * a[i], p1 = (uint64_t)0xCD9E8D57u * c[i];
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ b[i] ^ k0, n1 = (uint32_t)p1;
            const uint32_t n2 = (uint32_t)(p0 >> 32) ^ d[i] ^ k1, n3 = (uint32_t)p0;
            a[i] = n0; b[i] = n1; c[i] = n2; d[i] = n3;
        }
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
#pragma unroll
    for (int i = 0; i < NB; i++) { out[i][0] = a[i]; out[i][1] = b[i]; out[i][2] = c[i]; out[i][3] = d[i]; }
}

inline uint32_t bernoulli_threshold(double p) {
    if (p <= 0.0) return 0u;
    if (p >= 1.0) return 0xFFFFFFFFu;
    return (uint32_t)std::floor(p * 4294967296.0);
}

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
// Detector-error-model sampler of a circuit plan (dem.hip).  DemTab: one sector's projection of the mechanisms (device pointers): ptr int32[n_mech + 1],
// idx detector indices, log the logical masks.  d_thr: uint32 thresholds, zero-padded to a multiple of four.  two = false: sector 1 is not touched.
struct DemTab { const int32_t *ptr; const uint16_t *idx; const uint64_t *log; };
int dem_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, int n_mech, const uint32_t *d_thr, const DemTab &T0, const DemTab &T1, int n0, int n1,
                      bool two, int8_t *d_syn0, int8_t *d_syn1, unsigned long long *d_true0, unsigned long long *d_true1, int32_t *d_fail_counts,
                      hipStream_t s);
int dem_validate(const qldpc_dem_desc *D);      // QLDPC_OK, or QLDPC_ERR_INVALID with the error text naming the sector or the mechanism

}  // namespace qldpc
