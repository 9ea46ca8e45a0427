// Min-sum with a prior that differs per shot, and the reweighting step of two-pass correlated decoding.  The law is stated at
// qldpc_shotprior_decode_batch in include/qldpc_hip.h; tests/correlated_model.py is the numpy model the kernel equals bit for bit.
//
// Shot b decodes with P[b][j] = min(prior[b * stride + j], min of link_llr over the links of column j whose source fired in src_err[b]) as
// one round of guided decimation with nothing frozen: V = P[b], then one leg of bp_leg.h (the third user of that leg, after relay_bp.hip and
// decimation.hip) with bias(j, .) = P[b][j].  A minimum of finite doubles rounds nothing and has no order, so the lane order cannot matter.
//
// One workgroup per shot, persistent grid, shots handed out through an atomic queue (shot_queue_launch).  Where P[b] lives (PM):
//   0  no link tables: the bias reads prior + b * stride where it is, as decim_bp_kernel reads its prior; nothing is copied
//   1  links, and V | SP | SI | P fits in 160 KB: P in LDS
//   2  links otherwise: P in a per-workgroup slab in global memory (g->ws_prior), the way the VG form keeps V (g->ws_vals)
// and above the limit of V | SP | SI the leg's VG rule moves V out as well.  The fill is a gather: thread tid owns columns tid, tid + NT, ...
// and walks each one's own link run, so it needs no atomics.  Every loop is bounded by n, m, max_iter or a link run; workgroup barriers and
// the queue's atomicAdd are the only synchronisation.
#include "bp_leg.h"
#include "launchers.h"

#include <algorithm>
#include <cmath>

namespace qldpc {

struct ShotPriorArgs {
    SlotGraph G;
    int64_t B, stride;             // stride: 0 (one prior[n] for every shot) or n
    const int8_t *synd;
    const double *prior;           // finite (host-verified, or the documented precondition of the _dev entry)
    int n_src;
    const int8_t *src_err;         // [B][n_src]; the four link pointers are all NULL or all set
    const int32_t *link_ptr, *link_src;
    const double *link_llr;
    double alpha, clip;
    int max_iter;
    int iter_bias;                 // added to the iteration count written out (-1: the circuit plan's judge adds one per shot)
    int8_t *out_err; double *out_llr; uint8_t *out_conv; int32_t *out_iters; double *out_prior;      // out_llr / out_prior may be NULL
    int offP, offI, offQ, offF;
    double *vglobal;               // VG: V[n] per workgroup in HBM/L2
    double *pglobal;               // PM 2: P[n] per workgroup in HBM/L2
    int *queue;                    // next shot (zeroed before the launch)
};

template <bool VG, int PM>
__global__ __launch_bounds__(1024) void shot_prior_kernel(ShotPriorArgs A) {
    extern __shared__ unsigned char lds[];
    double *V;
    if (VG) V = A.vglobal + (size_t)blockIdx.x * A.G.n; else V = reinterpret_cast<double *>(lds);
    double2 *SP = reinterpret_cast<double2 *>(lds + A.offP);                       // (alpha*min1, alpha*min2) per check
    unsigned long long *SI = reinterpret_cast<unsigned long long *>(lds + A.offI); // bits 0-55 input signs, 56-62 argmin (127 = none), 63 total sign
    int *F = reinterpret_cast<int *>(lds + A.offF);                                // [0], [1] unsat flags, [2] shot
    double *PW = PM == 1 ? reinterpret_cast<double *>(lds + A.offQ) : PM == 2 ? A.pglobal + (size_t)blockIdx.x * A.G.n : nullptr;
    const int n = A.G.n, tid = threadIdx.x, NT = blockDim.x;

    for (;;) {
        if (tid == 0) F[2] = atomicAdd(A.queue, 1);
        __syncthreads();
        const int64_t b = F[2];
        if (b >= A.B) break;
        const double *pr = A.prior + b * A.stride;
        const double *P = PM == 0 ? pr : PW;
        if (PM == 0) {
            for (int j = tid; j < n; j += NT) V[j] = pr[j];
        } else {
            const int8_t *src = A.src_err + b * A.n_src;
            for (int j = tid; j < n; j += NT) {
                double p = pr[j];
                const int end = A.link_ptr[j + 1];
                for (int l = A.link_ptr[j]; l < end; l++) {
                    const int s = A.link_src[l];
                    if ((unsigned)s < (unsigned)A.n_src && src[s] == 1) { const double x = A.link_llr[l]; if (x < p) p = x; }
                }
                PW[j] = p;
                V[j] = p;
            }
        }
        if (tid < 2) F[tid] = 0;
        __syncthreads();
        const LegResult L = bp_leg(A.G, A.synd, b, A.max_iter, A.alpha, A.clip, V, SP, SI, F, [&](int j, double) { return P[j]; });   // V_j = s_j + P[b][j]
        for (int j = tid; j < n; j += NT) {
            const double v = V[j];
            A.out_err[b * n + j] = (v < 0.0) ? 1 : 0;
            if (A.out_llr) A.out_llr[b * n + j] = v;
            if (A.out_prior) A.out_prior[b * n + j] = P[j];
        }
        if (tid == 0) {
            A.out_conv[b] = L.conv ? 1 : 0;
            A.out_iters[b] = L.itc + A.iter_bias;
        }
        __syncthreads();
    }
}

// the leg's prefix V | SP | SI (V leaves it in the VG form) | P[n] f64 when it lives in LDS | 16 bytes of flags
static size_t shotprior_lds_bytes(const qldpc_graph *g, bool vg, bool p_lds, ShotPriorArgs &A) {
    A.offQ = leg_lds_prefix(g, vg, A.offP, A.offI);
    A.offF = A.offQ + (p_lds ? (int)round_up((int64_t)g->n * 8, 16) : 0);
    return (size_t)A.offF + 16;
}

// 0: not supported; with link tables 1: V and P in LDS, 2: V in LDS and P in global memory, 3: both in global memory.  Without link tables there is
// no P to keep: a launch then has V in LDS in modes 1 and 2 and in global memory in mode 3, so what is accepted does not depend on the tables.
int shotprior_mode(const qldpc_graph *g) {
    if (!g->d_ell_col_s || !g->d_ell_var_s || !g->d_row_of_slot || !g->d_col_of_slot) return 0;
    if (g->m <= 0 || g->n <= 0 || g->max_row_deg > 56) return 0;
    ShotPriorArgs A;
    if (shotprior_lds_bytes(g, false, true, A) <= 160 * 1024) return 1;
    if (shotprior_lds_bytes(g, false, false, A) <= 160 * 1024) return 2;
    return shotprior_lds_bytes(g, true, false, A) <= 160 * 1024 ? 3 : 0;
}

int shotprior_unsupported(const qldpc_graph *g) {
    set_error("per-shot-prior min-sum does not support this graph (m=%d n=%d, max row degree %d): it needs the slot tables, row degree <= 56 and the "
              "check state in 160 KB of LDS", g->m, g->n, g->max_row_deg);
    return QLDPC_ERR_UNSUPPORTED;
}

int shotprior_check_params(double alpha, double clip_llr, int max_iter) {
    QLDPC_REQUIRE(std::isfinite(alpha) && alpha > 0.0, "alpha must be finite and > 0");
    QLDPC_REQUIRE(std::isfinite(clip_llr) && clip_llr > 0.0, "clip_llr must be finite and > 0");
    QLDPC_REQUIRE(max_iter >= 1, "max_iter must be >= 1");
    return QLDPC_OK;
}

int shotprior_check_links(int n, int n_src, const int32_t *link_ptr, const int32_t *link_src, const double *link_llr) {
    QLDPC_REQUIRE(n_src >= 0, "n_src = %d is negative", n_src);
    QLDPC_REQUIRE(link_ptr[0] == 0, "link_ptr[0] = %d, not 0", link_ptr[0]);
    for (int j = 0; j < n; j++) QLDPC_REQUIRE(link_ptr[j + 1] >= link_ptr[j], "link_ptr[%d] = %d is below link_ptr[%d] = %d", j + 1, link_ptr[j + 1], j, link_ptr[j]);
    QLDPC_REQUIRE(link_ptr[n] == 0 || (link_src && link_llr), "link_src or link_llr is NULL but link_ptr holds %d links", link_ptr[n]);
    for (int j = 0; j < n; j++)
        for (int l = link_ptr[j]; l < link_ptr[j + 1]; l++) {
            QLDPC_REQUIRE(link_src[l] >= 0 && link_src[l] < n_src, "link_src[%d] = %d is outside 0..%d", l, link_src[l], n_src - 1);
            QLDPC_REQUIRE(l == link_ptr[j] || link_src[l] > link_src[l - 1], "link_src[%d] = %d does not ascend inside the run of column %d", l, link_src[l], j);
            QLDPC_REQUIRE(std::isfinite(link_llr[l]), "link_llr[%d] is not finite", l);
        }
    return QLDPC_OK;
}

// callers hold g->mu and have validated the parameters (shotprior_check_params); the workspaces are handed over in stream order (common.h)
int shotprior_decode_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int64_t stride, const ShotLinks &K, double alpha,
                            double clip, int max_iter, int iter_bias, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iters, double *d_prior_out,
                            hipStream_t stream) {
    const int mode = shotprior_mode(g);
    if (mode == 0) return shotprior_unsupported(g);
    if (B == 0) return QLDPC_OK;
    const bool links = K.ptr != nullptr;
    ShotPriorArgs A;
    A.G = slot_graph(g);
    A.B = B; A.stride = stride; A.synd = d_synd; A.prior = d_prior;
    A.n_src = K.n_src; A.src_err = K.src_err; A.link_ptr = K.ptr; A.link_src = K.src; A.link_llr = K.llr;
    A.alpha = alpha; A.clip = clip; A.max_iter = max_iter; A.iter_bias = iter_bias;
    A.out_err = d_err; A.out_llr = d_llr; A.out_conv = d_conv; A.out_iters = d_iters; A.out_prior = d_prior_out;
    A.pglobal = nullptr;
    const bool vg = mode == 3, p_lds = links && mode == 1, p_slab = links && mode != 1;
    const size_t lds = shotprior_lds_bytes(g, vg, p_lds, A);
    void (*kern)(ShotPriorArgs) = !links ? (vg ? shot_prior_kernel<true, 0> : shot_prior_kernel<false, 0>)
                                  : p_lds ? shot_prior_kernel<false, 1>
                                          : (vg ? shot_prior_kernel<true, 2> : shot_prior_kernel<false, 2>);
    if (!p_slab) return shot_queue_launch(g, B, kern, A, lds, vg, stream);
    // the P slab: one P[n] per workgroup, for the largest grid shot_queue_launch can choose (2048 / block workgroups per compute unit)
    const int block = (g->m > 512 || g->n > 4096) ? 1024 : 512;
    const int64_t grid_max = std::min<int64_t>(B, (int64_t)cu_count(g->device) * (2048 / block));
    int rc = g->ws_acquire(stream);
    if (rc != QLDPC_OK) return rc;
    if ((rc = g->ws_prior.ensure((size_t)grid_max * g->n * 8)) == QLDPC_OK) {
        A.pglobal = g->ws_prior.as<double>();
        rc = shot_queue_launch(g, B, kern, A, lds, vg, stream);
    }
    const int rel = g->ws_release(stream);          // always: the next stream has to wait for what was enqueued
    return rc != QLDPC_OK ? rc : rel;
}

}  // namespace qldpc

using namespace qldpc;

static int shotprior_entry_checks(const qldpc_graph *g, int64_t B, int64_t stride, int n_src, double alpha, double clip_llr, int max_iter) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    QLDPC_REQUIRE(stride == 0 || stride == g->n, "prior_stride = %lld is neither 0 nor n = %d", (long long)stride, g->n);
    QLDPC_REQUIRE(n_src >= 0, "n_src = %d is negative", n_src);
    return shotprior_check_params(alpha, clip_llr, max_iter);
}

QLDPC_EXPORT int qldpc_shotprior_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior, int64_t prior_stride,
                                                  int32_t n_src, const int8_t *d_src_err, const int32_t *d_link_ptr, const int32_t *d_link_src,
                                                  const double *d_link_llr, double alpha, double clip_llr, int max_iter, int8_t *d_err, double *d_llr,
                                                  uint8_t *d_conv, int32_t *d_iters, double *d_prior_out, void *stream) {
    int rc = shotprior_entry_checks(g, B, prior_stride, n_src, alpha, clip_llr, max_iter);
    if (rc != QLDPC_OK) return rc;
    const bool any = d_src_err || d_link_ptr || d_link_src || d_link_llr, all = d_src_err && d_link_ptr && d_link_src && d_link_llr;
    QLDPC_REQUIRE(any == all, "the link tables (src_err, link_ptr, link_src, link_llr) are all NULL or all given");
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_syndromes && d_prior && d_err && d_conv && d_iters, "a device pointer is NULL");
    QLDPC_USE_DEVICE(g->device);
    std::lock_guard<std::mutex> lk(g->mu);
    return shotprior_decode_launch(g, B, d_syndromes, d_prior, prior_stride, ShotLinks{n_src, d_src_err, d_link_ptr, d_link_src, d_link_llr}, alpha, clip_llr,
                                   max_iter, 0, d_err, d_llr, d_conv, d_iters, d_prior_out, reinterpret_cast<hipStream_t>(stream));
}

QLDPC_EXPORT int qldpc_shotprior_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, int64_t prior_stride,
                                              int32_t n_src, const int8_t *src_err, const int32_t *link_ptr, const int32_t *link_src,
                                              const double *link_llr, double alpha, double clip_llr, int max_iter, int8_t *err, double *llr,
                                              uint8_t *conv, int32_t *iters, double *prior_out) {
    int rc = shotprior_entry_checks(g, B, prior_stride, n_src, alpha, clip_llr, max_iter);
    if (rc != QLDPC_OK) return rc;
    const bool any = src_err || link_ptr || link_src || link_llr, all = src_err && link_ptr && link_src && link_llr;
    QLDPC_REQUIRE(any == all, "the link tables (src_err, link_ptr, link_src, link_llr) are all NULL or all given");
    const size_t m = g->m, n = g->n;
    if (all && (rc = shotprior_check_links((int)n, n_src, link_ptr, link_src, link_llr)) != QLDPC_OK) return rc;
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(syndromes && prior && err && conv && iters, "a pointer is NULL");
    const size_t np = prior_stride ? (size_t)B * n : n;
    for (size_t j = 0; j < np; j++) QLDPC_REQUIRE(std::isfinite(prior[j]), "prior[%zu] is not finite", j);
    QLDPC_USE_DEVICE(g->device);
    if (shotprior_mode(g) == 0) return shotprior_unsupported(g);
    const size_t nl = all ? (size_t)link_ptr[n] : 0;
    HostStage S(g->ws_io, g->mu_io);          // the graph handle's grow-only slab
    const auto dp = S.in(prior, np);
    const auto dl = llr ? S.out(llr, B, n) : Staged<double>{};        // not asked for: the launch gets NULL
    const auto dq = prior_out ? S.out(prior_out, B, n) : Staged<double>{};
    const auto ds = S.in(syndromes, B, m);
    const auto dse = all ? S.in(src_err, B, n_src) : Staged<int8_t>{};
    const auto dlp = all ? S.in(link_ptr, n + 1) : Staged<int32_t>{};
    const auto dls = all ? S.in(link_src, nl) : Staged<int32_t>{};
    const auto dll = all ? S.in(link_llr, nl) : Staged<double>{};
    const auto de = S.out(err, B, n);
    const auto dc = S.out(conv, B);
    const auto di = S.out(iters, B);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        rc = shotprior_decode_launch(g, B, S[ds], S[dp], prior_stride, ShotLinks{n_src, S[dse], S[dlp], S[dls], S[dll]}, alpha, clip_llr, max_iter, 0,
                                     S[de], S[dl], S[dc], S[di], S[dq], nullptr);
    }
    return rc != QLDPC_OK ? rc : S.finish("per-shot-prior decode", HostStage::kCopies);
}
