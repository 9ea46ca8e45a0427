// Sliding-window decoding over the layers of a space-time decoding matrix (semantics: include/qldpc_hip.h, qldpc_window_decoder_create).
//
// The rows of a circuit-level decoding matrix come in layers (one per syndrome cycle) and every column lives in one layer or in two
// consecutive ones, so W layers are a graph of their own whose size does not depend on the length of the experiment: a window of
// [[144,12,12]] is 72 W rows however many cycles were measured, and runs on the LDS-resident kernels (minsum_wg2.hip, the pipelined OSD-0)
// that the whole matrix outgrows beyond 12 cycles.  The host cuts the windows once (sub-CSR, prior slice, column map, commit CSR); windows
// whose CSR and prior slice coincide share one graph handle, so the interior of a long experiment costs one set of tables.
//
// Per window, on the caller's stream:  gather (running syndrome rows -> the window's syndrome array)  ->  the existing min-sum dispatch  ->
// collect + the existing OSD-0 on the unconverged shots, in place  ->  commit (decisions of the committed columns -> err, their FULL
// columns XORed into the running syndrome, per-shot counters).  The two kernels here are the gather and the commit; both are bounded by the
// host's tables, and the commit accumulates its parity flips in LDS (32-bit atomicXor) before it touches the running syndrome with plain stores.
#include "common.h"
#include "launchers.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace qldpc {

// one workgroup per shot (grid-stride): rows [row0, row0 + wm) of the running syndrome -> wsyn[b][0 .. wm); also clears the OSD list counter
__global__ __launch_bounds__(256) void window_gather_kernel(int64_t B, int m, int row0, int wm, const int8_t *__restrict__ run,
                                                            int8_t *__restrict__ wsyn, int32_t *__restrict__ count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const int8_t *src = run + b * m + row0;
        int8_t *dst = wsyn + b * wm;
        for (int i = threadIdx.x; i < wm; i += blockDim.x) dst[i] = src[i];
    }
}

__global__ void window_collect_kernel(int64_t B, const uint8_t *__restrict__ conv, int32_t *__restrict__ list, int32_t *__restrict__ count) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && !conv[b]) list[atomicAdd(count, 1)] = (int32_t)b;
}

struct WindowCommitArgs {
    int64_t B;
    int m, n, wn;                 // full rows / columns, window columns
    int ncommit;                  // committed columns of this window
    const int32_t *ccol;          // [ncommit] window column of committed column c
    const int32_t *colmap;        // [wn] window column -> original column
    const int32_t *cptr, *crow;   // commit CSR: FULL row list of committed column c (original row indices, all in [row0, row0 + nrows))
    int row0, nrows, nfinal;      // rows the commit can flip; the first nfinal of them are final afterwards (no later column meets them)
    int first, last;              // first / last window of the shot
    const int8_t *sol;            // [B][wn] the window's decision (BP, or OSD-0 written over it)
    const uint8_t *wconv;         // [B]
    const int32_t *witer;         // [B] final_iter of the window's decode
    int8_t *run;                  // [B][m] running syndrome
    int8_t *err;                  // [B][n]
    int32_t *acc;                 // [B][4] windows converged, iterations, windows through OSD-0, unsatisfied
    // written by the last window (each may be NULL)
    int32_t *o_conv, *o_iters, *o_osd;
    uint8_t *o_unsat;
    uint8_t *p_conv;              // circuit plan: 1 iff every window converged
    int32_t *p_iter;              // circuit plan: iterations - 1 (the judge adds one per trial)
    int32_t *p_osd_count;         // circuit plan: += 1 per trial with at least one OSD-0 window
};

// one workgroup per shot (grid-stride)
__global__ __launch_bounds__(256) void window_commit_kernel(WindowCommitArgs A) {
    extern __shared__ uint32_t flips[];                  // nrows bits: parity flips of this shot's committed ones
    const int nwords = (A.nrows + 31) >> 5;
    for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
        for (int w = threadIdx.x; w < nwords; w += blockDim.x) flips[w] = 0u;
        __syncthreads();
        const int8_t *sol = A.sol + b * A.wn;
        int8_t *err = A.err + b * A.n;
        for (int c = threadIdx.x; c < A.ncommit; c += blockDim.x) {
            const int wc = A.ccol[c];
            const int bit = sol[wc] & 1;
            err[A.colmap[wc]] = (int8_t)bit;
            if (bit)
                for (int e = A.cptr[c]; e < A.cptr[c + 1]; e++) {
                    const int r = A.crow[e] - A.row0;
                    atomicXor(&flips[r >> 5], 1u << (r & 31));
                }
        }
        __syncthreads();
        int8_t *run = A.run + b * A.m + A.row0;
        int bad = 0;
        for (int i = threadIdx.x; i < A.nrows; i += blockDim.x) {
            int v = run[i] & 1;
            if ((flips[i >> 5] >> (i & 31)) & 1u) { v ^= 1; run[i] = (int8_t)v; }
            if (i < A.nfinal) bad |= v;
        }
        bad = __syncthreads_or(bad);                      // (also the barrier before the next shot clears `flips`)
        if (threadIdx.x == 0) {
            int32_t *acc = A.acc + b * 4;
            const int cv = A.wconv[b] ? 1 : 0;
            const int nconv = (A.first ? 0 : acc[0]) + cv, iters = (A.first ? 0 : acc[1]) + A.witer[b] + 1;
            const int osd = (A.first ? 0 : acc[2]) + (1 - cv), unsat = (A.first ? 0 : acc[3]) | (bad ? 1 : 0);
            if (!A.last) { acc[0] = nconv; acc[1] = iters; acc[2] = osd; acc[3] = unsat; }
            else {
                if (A.o_conv) A.o_conv[b] = nconv;
                if (A.o_iters) A.o_iters[b] = iters;
                if (A.o_osd) A.o_osd[b] = osd;
                if (A.o_unsat) A.o_unsat[b] = (uint8_t)unsat;
                if (A.p_conv) A.p_conv[b] = (uint8_t)(osd == 0);
                if (A.p_iter) A.p_iter[b] = iters - 1;
                if (A.p_osd_count && osd) atomicAdd(A.p_osd_count, 1);
            }
        }
    }
}

}  // namespace qldpc

using namespace qldpc;

struct qldpc_window_decoder {
    const qldpc_graph *full = nullptr;
    int device = 0, m = 0, n = 0, layer_rows = 0, layers = 0, window = 0, commit = 0, max_iter = 0, flags = 0;
    double clip = 20;
    std::vector<double> alpha;                       // alpha_k, k < max_iter
    struct Shared {                                  // one per distinct (CSR, prior slice)
        Handle<qldpc_graph, qldpc_graph_destroy> g;
        std::vector<int32_t> indptr, indices;
        std::vector<double> prior;
        DevBuf d_prior;
        bool nanfree = false;
        int path = -1;
    };
    struct Stage {                                   // one per window
        int shared = 0, row0 = 0, wm = 0, wn = 0, ncommit = 0, c_row0 = 0, c_nrows = 0, c_nfinal = 0;
        DevBuf d_colmap, d_ccol, d_cptr, d_crow;
    };
    std::vector<std::unique_ptr<Shared>> shared;
    std::vector<std::unique_ptr<Stage>> stages;
    int max_wm = 0, max_wn = 0;
    // device workspaces for the shots of one call, handed from stream to stream like a graph handle's (common.h)
    std::mutex mu, mu_io;
    DevBuf run, wsyn, werr, wllr, wconv, witer, list, count, acc;
    StreamHandover hand;
    ~qldpc_window_decoder() { quiesce(device, hand); }
};

namespace qldpc {

// Creation on a ready alpha table (the circuit plan holds one per sector); the exported form builds the table from the alpha mode.
int window_decoder_create_tab(const qldpc_graph *g, int layer_rows, int window, int commit, const double *prior, int max_iter,
                              const std::vector<double> &tab, double clip_llr, int flags, qldpc_window_decoder **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(g != nullptr && prior != nullptr, "NULL argument");
    QLDPC_REQUIRE(layer_rows >= 1 && g->m >= 1 && g->m % layer_rows == 0, "layer_rows = %d does not divide the %d rows", layer_rows, g->m);
    QLDPC_REQUIRE(window >= 1 && commit >= 1 && commit <= window, "need window >= 1 and 1 <= commit <= window (got window = %d, commit = %d)", window, commit);
    QLDPC_REQUIRE(max_iter >= 0, "negative max_iter");
    QLDPC_REQUIRE(!(clip_llr != clip_llr), "clip_llr is NaN");
    for (int j = 0; j < g->n; j++) QLDPC_REQUIRE(std::isfinite(prior[j]), "the prior of column %d is not finite", j);
    const int m = g->m, n = g->n, lr = layer_rows, Lyr = m / lr;
    // column layers: tau = the first layer a column has a row in (rows of a column ascend in the CSC view); a column spans at most two layers
    std::vector<int32_t> tau(n, 0);
    for (int j = 0; j < n; j++) {
        if (g->colptr[j + 1] == g->colptr[j]) continue;
        const int lo = g->rowidx[g->colptr[j]] / lr, hi = g->rowidx[g->colptr[j + 1] - 1] / lr;
        QLDPC_REQUIRE(hi - lo <= 1, "column %d has rows in layers %d .. %d: a column may span two consecutive layers at most", j, lo, hi);
        tau[j] = lo;
    }
    QLDPC_USE_DEVICE(g->device);
    std::unique_ptr<qldpc_window_decoder> D(new qldpc_window_decoder());
    D->full = g; D->device = g->device; D->m = m; D->n = n; D->layer_rows = lr; D->layers = Lyr; D->window = window; D->commit = commit;
    D->max_iter = max_iter; D->flags = flags & QLDPC_FLAG_PUBLIC_MASK; D->clip = clip_llr; D->alpha = tab;
    int rc;
    std::vector<int32_t> wcol(n);
    for (int64_t a = 0;; a += commit) {
        const bool last = a + window >= Lyr;
        const int lend = (int)std::min<int64_t>(a + window, Lyr), la = (int)a;
        std::unique_ptr<qldpc_window_decoder::Stage> S(new qldpc_window_decoder::Stage());
        S->row0 = la * lr; S->wm = (lend - la) * lr;
        std::vector<int32_t> colmap, ccol, cptr(1, 0), crow;
        for (int j = 0; j < n; j++) {
            wcol[j] = -1;
            if (tau[j] < la || tau[j] >= lend) continue;
            wcol[j] = (int32_t)colmap.size();
            colmap.push_back(j);
            if (!last && tau[j] >= la + commit) continue;
            ccol.push_back(wcol[j]);
            for (int e = g->colptr[j]; e < g->colptr[j + 1]; e++) crow.push_back(g->rowidx[e]);
            cptr.push_back((int32_t)crow.size());
        }
        S->wn = (int)colmap.size(); S->ncommit = (int)ccol.size();
        if (S->wn == 0) { set_error("the window at layer %d has no columns", la); return QLDPC_ERR_UNSUPPORTED; }
        S->c_row0 = S->row0;
        S->c_nrows = last ? m - S->row0 : (std::min(la + commit + 1, Lyr) - la) * lr;
        S->c_nfinal = last ? S->c_nrows : commit * lr;
        for (int32_t r : crow)
            if (r < S->c_row0 || r >= S->c_row0 + S->c_nrows) { set_error("internal: a committed column leaves its rows"); return QLDPC_ERR_INVALID; }
        if (S->c_nrows > (1 << 19)) { set_error("a commit touches %d rows: more than the LDS bit set holds", S->c_nrows); return QLDPC_ERR_UNSUPPORTED; }
        // the window graph: the covered rows restricted to the window's columns (entries of columns committed earlier are already in the running syndrome)
        std::vector<int32_t> ip(1, 0), ix;
        for (int i = S->row0; i < S->row0 + S->wm; i++) {
            for (int e = g->indptr[i]; e < g->indptr[i + 1]; e++) if (wcol[g->indices[e]] >= 0) ix.push_back(wcol[g->indices[e]]);
            ip.push_back((int32_t)ix.size());
        }
        std::vector<double> pw(S->wn);
        for (int c = 0; c < S->wn; c++) pw[c] = prior[colmap[c]];
        int found = -1;
        for (size_t k = 0; k < D->shared.size() && found < 0; k++)
            if (D->shared[k]->indptr == ip && D->shared[k]->indices == ix && D->shared[k]->prior.size() == pw.size() &&
                std::memcmp(D->shared[k]->prior.data(), pw.data(), pw.size() * 8) == 0)
                found = (int)k;
        if (found < 0) {
            std::unique_ptr<qldpc_window_decoder::Shared> H(new qldpc_window_decoder::Shared());
            qldpc_graph *wg = nullptr;
            if ((rc = qldpc_graph_create(S->wm, S->wn, ip.data(), ix.data(), g->device, &wg)) != QLDPC_OK) return rc;
            H->g.reset(wg);
            found = (int)D->shared.size();
            D->shared.push_back(std::move(H));
            qldpc_window_decoder::Shared &R = *D->shared.back();
            R.indptr = std::move(ip); R.indices = std::move(ix); R.prior = std::move(pw);
            if ((rc = upload(R.d_prior, R.prior)) != QLDPC_OK) return rc;
            R.nanfree = inputs_clean(R.prior.data(), S->wn, clip_llr, tab.data(), max_iter);
            // which decoder form the window takes; this also builds the LDS-resident form's tables now, so that decode calls only enqueue
            DecodePath P;
            {
                std::lock_guard<std::mutex> lk(R.g->mu);
                rc = select_decode_path(R.g.get(), max_iter, 1.0, clip_llr, D->flags | QLDPC_FLAG_INTERNAL_PRIOR_FINITE, R.nanfree, R.prior.data(), P);
            }
            if (rc != QLDPC_OK) return rc;
            R.path = P.path;
        }
        S->shared = found;
        if ((rc = upload(S->d_colmap, colmap)) || (rc = upload(S->d_ccol, ccol)) || (rc = upload(S->d_cptr, cptr)) || (rc = upload(S->d_crow, crow))) return rc;
        D->max_wm = std::max(D->max_wm, S->wm); D->max_wn = std::max(D->max_wn, S->wn);
        D->stages.push_back(std::move(S));
        if (last) break;
    }
    if ((rc = D->count.ensure(64)) != QLDPC_OK) return rc;
    *out = D.release();
    return QLDPC_OK;
}

// The window loop of window_decode_launch, which owns the hand-over: an error return may leave earlier stages enqueued.
static int window_stages_launch(qldpc_window_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, int32_t *d_conv, int32_t *d_iters, int32_t *d_osd,
                                uint8_t *d_unsat, const WindowPlanSlots *plan, const std::function<int(int, bool)> *mark, hipStream_t s) {
    int rc;
    const size_t Bz = (size_t)B;
    if ((rc = D->run.ensure(Bz * D->m)) || (rc = D->wsyn.ensure(Bz * D->max_wm)) || (rc = D->werr.ensure(Bz * D->max_wn)) ||
        (rc = D->wllr.ensure(Bz * D->max_wn * 8)) || (rc = D->wconv.ensure(Bz)) || (rc = D->witer.ensure(Bz * 4)) || (rc = D->list.ensure(Bz * 4)) ||
        (rc = D->acc.ensure(Bz * 16)))
        return rc;
    QLDPC_HIP_TRY(hipMemcpyAsync(D->run.p, d_synd, Bz * D->m, hipMemcpyDeviceToDevice, s));
    const unsigned grid = (unsigned)std::min<int64_t>(B, 8192);
    int32_t *count = D->count.as<int32_t>();
    for (size_t k = 0; k < D->stages.size(); k++) {
        const qldpc_window_decoder::Stage &S = *D->stages[k];
        const qldpc_window_decoder::Shared &R = *D->shared[S.shared];
        if (mark && (rc = (*mark)(0, true)) != QLDPC_OK) return rc;
        hipLaunchKernelGGL(window_gather_kernel, dim3(grid), dim3(256), 0, s, B, D->m, S.row0, S.wm, D->run.as<int8_t>(), D->wsyn.as<int8_t>(), count);
        QLDPC_HIP_TRY(hipGetLastError());
        {
            std::lock_guard<std::mutex> lk(R.g->mu);
            const double *d_alpha = nullptr;
            if ((rc = R.g->alpha_table(D->alpha, s, &d_alpha)) != QLDPC_OK) return rc;
            rc = minsum_decode_dispatch(R.g.get(), B, D->wsyn.as<int8_t>(), R.d_prior.as<double>(), D->max_iter, d_alpha, 1.0, D->clip,
                                        D->flags | QLDPC_FLAG_INTERNAL_PRIOR_FINITE, R.nanfree, D->werr.as<int8_t>(), D->wllr.as<double>(),
                                        D->wconv.as<uint8_t>(), D->witer.as<int32_t>(), s, R.prior.data());
        }
        if (rc != QLDPC_OK) return rc;
        if (mark && ((rc = (*mark)(0, false)) != QLDPC_OK || (rc = (*mark)(1, true)) != QLDPC_OK)) return rc;
        hipLaunchKernelGGL(window_collect_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, D->wconv.as<uint8_t>(), D->list.as<int32_t>(), count);
        QLDPC_HIP_TRY(hipGetLastError());
        {
            std::lock_guard<std::mutex> lk(R.g->mu);
            rc = osd0_listed_launch(R.g.get(), D->list.as<int32_t>(), count, B, D->wsyn.as<int8_t>(), D->wllr.as<double>(), D->werr.as<int8_t>(), nullptr,
                                    D->werr.as<int8_t>(), D->flags, s);
        }
        if (rc != QLDPC_OK) return rc;
        WindowCommitArgs A{};
        A.B = B; A.m = D->m; A.n = D->n; A.wn = S.wn; A.ncommit = S.ncommit;
        A.ccol = S.d_ccol.as<int32_t>(); A.colmap = S.d_colmap.as<int32_t>(); A.cptr = S.d_cptr.as<int32_t>(); A.crow = S.d_crow.as<int32_t>();
        A.row0 = S.c_row0; A.nrows = S.c_nrows; A.nfinal = S.c_nfinal;
        A.first = k == 0; A.last = k + 1 == D->stages.size();
        A.sol = D->werr.as<int8_t>(); A.wconv = D->wconv.as<uint8_t>(); A.witer = D->witer.as<int32_t>();
        A.run = D->run.as<int8_t>(); A.err = d_err; A.acc = D->acc.as<int32_t>();
        A.o_conv = d_conv; A.o_iters = d_iters; A.o_osd = d_osd; A.o_unsat = d_unsat;
        if (plan) { A.p_conv = plan->conv; A.p_iter = plan->iter; A.p_osd_count = plan->osd_count; }
        const size_t lds = (size_t)((S.c_nrows + 31) / 32) * 4;
        if (lds > 48 * 1024 && (rc = ensure_max_lds(D->device, reinterpret_cast<const void *>(window_commit_kernel), (int)lds)) != QLDPC_OK) return rc;
        hipLaunchKernelGGL(window_commit_kernel, dim3(grid), dim3(256), lds, s, A);
        QLDPC_HIP_TRY(hipGetLastError());
        if (mark && (rc = (*mark)(1, false)) != QLDPC_OK) return rc;
    }
    return QLDPC_OK;
}

// Enqueues the window loop for B shots on `stream`.  Callers hold D->mu.  plan: the circuit plan's per-trial slots (see WindowCommitArgs); mark: brackets
// the BP part (phase 0) and the OSD + commit part (phase 1) of every window for the plan's phase times.
int window_decode_launch(qldpc_window_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, int32_t *d_conv, int32_t *d_iters, int32_t *d_osd,
                         uint8_t *d_unsat, const WindowPlanSlots *plan, const std::function<int(int, bool)> *mark, hipStream_t s) {
    int rc = D->hand.acquire(s);
    if (rc != QLDPC_OK) return rc;
    rc = window_stages_launch(D, B, d_synd, d_err, d_conv, d_iters, d_osd, d_unsat, plan, mark, s);
    const int rel = D->hand.release(s);             // always: a failing call may have enqueued stages the next stream has to wait for
    return rc != QLDPC_OK ? rc : rel;
}

int window_decoder_lock_and_launch(qldpc_window_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, const WindowPlanSlots *plan,
                                   const std::function<int(int, bool)> *mark, hipStream_t s) {
    std::lock_guard<std::mutex> lk(D->mu);
    return window_decode_launch(D, B, d_synd, d_err, nullptr, nullptr, nullptr, nullptr, plan, mark, s);
}

}  // namespace qldpc

QLDPC_EXPORT int qldpc_window_decoder_create(const qldpc_graph *g, int layer_rows, int window, int commit, const double *prior, int max_iter,
                                             int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len, double clip_llr, int flags,
                                             qldpc_window_decoder **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(max_iter >= 0, "negative max_iter");
    std::vector<double> tab;
    const int rc = build_alpha_table(max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, tab);
    if (rc != QLDPC_OK) return rc;
    return window_decoder_create_tab(g, layer_rows, window, commit, prior, max_iter, tab, clip_llr, flags, out);
}

QLDPC_EXPORT void qldpc_window_decoder_destroy(qldpc_window_decoder *D) { delete D; }

QLDPC_EXPORT int qldpc_window_decoder_info(const qldpc_window_decoder *D, int *windows, int *graphs, int *max_rows, int *max_cols, int *wg2_windows) {
    QLDPC_REQUIRE(D != nullptr, "decoder is NULL");
    if (windows) *windows = (int)D->stages.size();
    if (graphs) *graphs = (int)D->shared.size();
    if (max_rows) *max_rows = D->max_wm;
    if (max_cols) *max_cols = D->max_wn;
    if (wg2_windows) {
        *wg2_windows = 0;
        for (const auto &S : D->stages) *wg2_windows += D->shared[S->shared]->path == QLDPC_PATH_WG2 ? 1 : 0;
    }
    return QLDPC_OK;
}

static int window_check_call(const qldpc_window_decoder *D, int64_t B, const void *synd, const void *err, const void *conv, const void *iters,
                             const void *osd, const void *unsat) {
    QLDPC_REQUIRE(D != nullptr, "decoder is NULL");
    QLDPC_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "batch out of range");
    if (B > 0) QLDPC_REQUIRE(synd && err && conv && iters && osd && unsat, "NULL buffer");
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_window_decode_batch_dev(qldpc_window_decoder *D, int64_t B, const int8_t *d_syndromes, int8_t *d_err, int32_t *d_conv,
                                               int32_t *d_iters, int32_t *d_osd, uint8_t *d_unsat, void *stream) {
    int rc = window_check_call(D, B, d_syndromes, d_err, d_conv, d_iters, d_osd, d_unsat);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(D->device);
    if (B == 0) return QLDPC_OK;
    std::lock_guard<std::mutex> lk(D->mu);
    return window_decode_launch(D, B, d_syndromes, d_err, d_conv, d_iters, d_osd, d_unsat, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

QLDPC_EXPORT int qldpc_window_decode_batch(qldpc_window_decoder *D, int64_t B, const int8_t *syndromes, int8_t *err, int32_t *conv, int32_t *iters,
                                           int32_t *osd, uint8_t *unsat) {
    int rc = window_check_call(D, B, syndromes, err, conv, iters, osd, unsat);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(D->device);
    if (B == 0) return QLDPC_OK;
    HostStage S;
    const auto ds = S.in(syndromes, B, D->m);
    const auto de = S.out(err, B, D->n);
    const auto dc = S.out(conv, B);
    const auto di = S.out(iters, B);
    const auto dq = S.out(osd, B);
    const auto du = S.out(unsat, B);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(D->mu);
        rc = window_decode_launch(D, B, S[ds], S[de], S[dc], S[di], S[dq], S[du], nullptr, nullptr, nullptr);
    }
    return rc != QLDPC_OK ? rc : S.finish("window decode", HostStage::kStream);
}
