// C-ABI entry points of the batched min-sum decoder (a1/a2) and kernel selection.
#include "common.h"
#include "launchers.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace qldpc {

// alpha_k for k < max_iter, evaluated exactly as the reference does (src/decoding/kernels.py:272-275, 402-405).
int build_alpha_table(int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq, int alpha_len,
                      std::vector<double> &tab) {
    QLDPC_REQUIRE(alpha_mode == QLDPC_ALPHA_CONST || alpha_mode == QLDPC_ALPHA_DYNAMIC || alpha_mode == QLDPC_ALPHA_SEQ,
                  "unknown alpha_mode %d", alpha_mode);
    if (alpha_mode == QLDPC_ALPHA_SEQ) QLDPC_REQUIRE(alpha_seq != nullptr && alpha_len > 0, "alpha_seq must be a non-empty sequence for QLDPC_ALPHA_SEQ");
    tab.resize(max_iter > 0 ? max_iter : 1);
    for (int k = 0; k < max_iter; k++) {
        if (alpha_mode == QLDPC_ALPHA_DYNAMIC) tab[k] = 1.0 - std::ldexp(1.0, -(k + 1));   // 1.0 - 2.0**(-(k+1)), exact
        else if (alpha_mode == QLDPC_ALPHA_SEQ) tab[k] = (k < alpha_len) ? alpha_seq[k] : alpha_seq[alpha_len - 1];
        else tab[k] = alpha_val;
    }
    return QLDPC_OK;
}

bool resident_supported(const qldpc_graph *g, double damping);

bool inputs_clean(const double *prior, int n, double clip, const double *alpha, int n_alpha) {
    if (!(std::isfinite(clip) && clip > 0.0)) return false;
    for (int k = 0; k < n_alpha; k++) if (!(std::isfinite(alpha[k]) && alpha[k] > 0.0)) return false;
    for (int j = 0; j < n; j++) if (!std::isfinite(prior[j]) || (prior[j] == 0.0 && std::signbit(prior[j]))) return false;
    return true;
}

// The one predicate of kernel selection: which decoder form serves these arguments.  dispatch_kernel launches what it returns and
// qldpc_minsum_decode_path reports it, so the query cannot drift from what runs.  May build and cache the tables of the LDS-resident
// workgroup form (callers hold g->mu).
int select_decode_path(const qldpc_graph *g, int max_iter, double damping, double clip, int flags, bool nanfree, const double *h_prior, DecodePath &out) {
    out.path = QLDPC_PATH_STREAM; out.detail = 0; out.prep = nullptr;
    const bool want_stream = flags & QLDPC_FLAG_KERNEL_STREAM;
    const bool want_res = flags & (QLDPC_FLAG_KERNEL_RESIDENT | QLDPC_FLAG_KERNEL_GENERIC);
    const bool can_res = resident_supported(g, damping);
    if (!want_stream && !(flags & QLDPC_FLAG_KERNEL_GENERIC) && regular_supported(g, clip, max_iter)) {
        out.path = QLDPC_PATH_REGULAR;
#ifdef QLDPC_EXPERIMENTS
        const bool clean = nanfree && (flags & QLDPC_FLAG_INTERNAL_PRIOR_LE_CLIP);
        if (wave_kernel_choice() == 2 && wave_supported(g, damping, clean)) out.path = QLDPC_PATH_WAVE;
#endif
        return QLDPC_OK;
    }
    if (want_res && !can_res) {
        set_error("resident kernel does not support this graph (m=%d n=%d max row degree %d, max column degree %d)", g->m, g->n,
                  g->max_row_deg, g->max_col_deg);
        return QLDPC_ERR_UNSUPPORTED;
    }
    if (!want_stream && can_res) { out.path = QLDPC_PATH_RESIDENT; out.detail = resident_detail(g, damping); return QLDPC_OK; }
    if (!want_stream && wg_supported(g, damping)) {
        // the prior is known on the host and the inputs are clean: the form with every table in LDS (minsum_wg2.hip), unless a flag asks for a form of the
        // table kernel (QLDPC_FLAG_WG_TABLES and the layout / experiment selectors)
        if (h_prior && nanfree && damping == 1.0 && !(flags & (QLDPC_FLAG_WG_TABLES | QLDPC_FLAG_WG_VGLOBAL | QLDPC_FLAG_WG_GENERIC | QLDPC_FLAG_WG_ROWMAJOR |
                                                                  QLDPC_FLAG_WG_EDGE_LANES | QLDPC_FLAG_WG_IDXLOAD))) {
            const int rcp = wg2_prepare(g, h_prior, &out.prep);
            if (rcp != QLDPC_OK) return rcp;
            if (out.prep) { out.path = QLDPC_PATH_WG2; out.detail = wg2_detail(out.prep); return QLDPC_OK; }
        }
        const int rcx = wg_check_variant(flags);
        if (rcx != QLDPC_OK) return rcx;
        out.path = QLDPC_PATH_WG;
        out.detail = wg_choose(g, damping, flags, nanfree).detail();
        return QLDPC_OK;
    }
    return QLDPC_OK;
}

static int dispatch_kernel(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                           const double *d_alpha, double damping, double clip, int flags, bool nanfree, int8_t *d_err, double *d_llr,
                           uint8_t *d_conv, int32_t *d_iter, hipStream_t stream, const double *h_prior) {
    DecodePath P;
    const int rc = select_decode_path(g, max_iter, damping, clip, flags, nanfree, h_prior, P);
    if (rc != QLDPC_OK) return rc;
    switch (P.path) {
#ifdef QLDPC_EXPERIMENTS
    case QLDPC_PATH_WAVE: return minsum_wave_launch(g, B, d_synd, d_prior, max_iter, d_alpha, clip, flags, d_err, d_llr, d_conv, d_iter, stream);
#endif
    case QLDPC_PATH_REGULAR: return minsum_regular_launch(g, B, d_synd, d_prior, max_iter, d_alpha, damping, clip, flags, nanfree, d_err, d_llr, d_conv, d_iter, stream);
    case QLDPC_PATH_RESIDENT: return minsum_resident_launch(g, B, d_synd, d_prior, max_iter, d_alpha, damping, clip, flags, d_err, d_llr, d_conv, d_iter, stream);
    case QLDPC_PATH_WG2: return minsum_wg2_launch(g, P.prep, B, d_synd, max_iter, d_alpha, clip, flags, d_err, d_llr, d_conv, d_iter, stream);
    case QLDPC_PATH_WG: return minsum_wg_launch(g, B, d_synd, d_prior, max_iter, d_alpha, damping, clip, flags, nanfree, d_err, d_llr, d_conv, d_iter, stream);
    default: return minsum_stream_launch(g, B, d_synd, d_prior, max_iter, d_alpha, damping, clip, flags, d_err, d_llr, d_conv, d_iter, stream);
    }
}

// callers hold g->mu; the graph's device workspaces are handed over in stream order (common.h)
int minsum_decode_dispatch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                           const double *d_alpha, double damping, double clip, int flags, bool nanfree, int8_t *d_err, double *d_llr,
                           uint8_t *d_conv, int32_t *d_iter, hipStream_t stream, const double *h_prior) {
    int rc = g->ws_acquire(stream);
    if (rc != QLDPC_OK) return rc;
    rc = dispatch_kernel(g, B, d_synd, d_prior, max_iter, d_alpha, damping, clip, flags, nanfree, d_err, d_llr, d_conv, d_iter, stream, h_prior);
    const int rel = g->ws_release(stream);          // always: a failing call may have enqueued launches the next stream has to wait for
    return rc != QLDPC_OK ? rc : rel;
}

}  // namespace qldpc

using namespace qldpc;

static int check_decode_args(const qldpc_graph *g, int64_t B, const void *synd, const void *prior, int max_iter, double clip,
                             const void *e, const void *l, const void *c, const void *it) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    QLDPC_REQUIRE(max_iter >= 0, "negative max_iter");
    QLDPC_REQUIRE(!(clip != clip), "clip_llr is NaN");
    if (B > 0) {
        QLDPC_REQUIRE(prior != nullptr || g->n == 0, "prior is NULL");
        QLDPC_REQUIRE(synd != nullptr || g->m == 0, "syndromes is NULL");
        QLDPC_REQUIRE(e && l && c && it, "an output pointer is NULL");
    }
    return QLDPC_OK;
}

// What the host knows about a decode call's inputs: nanfree ("clean": host-verified clean prior -- finite, no -0.0 -- and clip, alphas, damping
// checked the same way) and the internal flag bits that carry the prior's facts to the launchers.
static bool decode_facts(bool prior_finite, bool prior_le_clip, double damping, double clip_llr, const std::vector<double> &tab, int max_iter, int &flags) {
    flags = (flags & QLDPC_FLAG_PUBLIC_MASK) | (prior_finite ? QLDPC_FLAG_INTERNAL_PRIOR_FINITE : 0) |
            ((prior_finite && prior_le_clip) ? QLDPC_FLAG_INTERNAL_PRIOR_LE_CLIP : 0);
    return prior_finite && std::isfinite(damping) && inputs_clean(nullptr, 0, clip_llr, tab.data(), max_iter);
}

// the facts of a host prior (the *_dev entry points know neither)
static void host_prior_facts(const double *prior, size_t n, double clip_llr, bool &finite, bool &le_clip) {
    const double one = 1.0;
    finite = inputs_clean(prior, (int)n, 1.0, &one, 1);
    le_clip = finite;
    for (size_t j = 0; j < n && le_clip; j++) le_clip = std::fabs(prior[j]) <= clip_llr;
}

static int decode_dev_impl(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior,
                                               int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq,
                                               int alpha_len, double damping, double clip_llr, int flags, bool prior_finite, bool prior_le_clip, int8_t *d_err,
                                               double *d_llr, uint8_t *d_conv, int32_t *d_iter, void *stream, const double *h_prior = nullptr) {
    int rc = check_decode_args(g, B, d_synd, d_prior, max_iter, clip_llr, d_err, d_llr, d_conv, d_iter);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(g->device);
    if (B == 0) return QLDPC_OK;
    std::vector<double> tab;
    if ((rc = build_alpha_table(max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, tab)) != QLDPC_OK) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const double *d_alpha = nullptr;          // per-graph cache of alpha tables: a new schedule is uploaded once, nothing synchronises
    if ((rc = g->alpha_table(tab, s, &d_alpha)) != QLDPC_OK) return rc;
    const bool nanfree = decode_facts(prior_finite, prior_le_clip, damping, clip_llr, tab, max_iter, flags);
    return minsum_decode_dispatch(g, B, d_synd, d_prior, max_iter, d_alpha, damping, clip_llr, flags, nanfree, d_err,
                                  d_llr, d_conv, d_iter, s, h_prior);
}

QLDPC_EXPORT int qldpc_minsum_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior,
                                               int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq,
                                               int alpha_len, double damping, double clip_llr, int flags, int8_t *d_err,
                                               double *d_llr, uint8_t *d_conv, int32_t *d_iter, void *stream) {
    // the prior lives on the device: its finiteness is unknown here, so the NaN test of kernels.py:328 stays in
    return decode_dev_impl(g, B, d_synd, d_prior, max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, damping, clip_llr, flags, false, false,
                           d_err, d_llr, d_conv, d_iter, stream);
}

QLDPC_EXPORT int qldpc_minsum_decode_path(const qldpc_graph *g, const double *prior, int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq,
                                          int alpha_len, double damping, double clip_llr, int flags, int *path, int *detail) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(path != nullptr && detail != nullptr, "an output pointer is NULL");
    QLDPC_REQUIRE(max_iter >= 0, "negative max_iter");
    QLDPC_REQUIRE(!(clip_llr != clip_llr), "clip_llr is NaN");
    QLDPC_USE_DEVICE(g->device);
    std::vector<double> tab;
    int rc = build_alpha_table(max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, tab);
    if (rc != QLDPC_OK) return rc;
    bool prior_finite = false, prior_le_clip = false;            // prior == NULL: the *_dev entry point, which knows neither
    if (prior) host_prior_facts(prior, (size_t)g->n, clip_llr, prior_finite, prior_le_clip);
    const bool nanfree = decode_facts(prior_finite, prior_le_clip, damping, clip_llr, tab, max_iter, flags);
    std::lock_guard<std::mutex> lk(g->mu);
    DecodePath P;
    if ((rc = select_decode_path(g, max_iter, damping, clip_llr, flags, nanfree, prior, P)) != QLDPC_OK) return rc;
    *path = P.path; *detail = P.detail;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_minsum_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior,
                                           int max_iter, int alpha_mode, double alpha_val, const double *alpha_seq,
                                           int alpha_len, double damping, double clip_llr, int flags, int8_t *out_err,
                                           double *out_llr, uint8_t *out_conv, int32_t *out_iter) {
    // out_llr may be NULL: the posteriors (8n of the 9n + 5 result bytes per shot) then stay on the device
    int rc = check_decode_args(g, B, syndromes, prior, max_iter, clip_llr, out_err, out_llr ? (const void *)out_llr : (const void *)out_err, out_conv, out_iter);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(g->device);
    if (B == 0) return QLDPC_OK;
    // The graph handle's grow-only slab (no hipMalloc / hipFree per call: the reference-style single-shot call is latency bound); small results
    // return in ONE copy through the handle's pinned staging buffer, large ones directly into the caller's arrays.
    HostStage S(g->ws_io, g->mu_io);
    const auto dp = S.in(prior, g->n);
    const auto ds = S.in(syndromes, B, g->m);
    const auto dl = S.out(out_llr, B, g->n);
    const auto di = S.out(out_iter, B);
    const auto de = S.out(out_err, B, g->n);
    const auto dc = S.out(out_conv, B);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    bool prior_finite, prior_le_clip;
    host_prior_facts(prior, (size_t)g->n, clip_llr, prior_finite, prior_le_clip);
    rc = decode_dev_impl(g, B, S[ds], S[dp], max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, damping, clip_llr, flags, prior_finite, prior_le_clip,
                         S[de], S[dl], S[dc], S[di], nullptr, prior);
    if (rc != QLDPC_OK) return rc;
    return out_llr ? S.finish_pinned("min-sum decode", g->pin) : S.finish("min-sum decode", HostStage::kCopies);
}
