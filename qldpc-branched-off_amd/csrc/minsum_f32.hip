// Single-precision flooding min-sum (semantics: include/qldpc_hip.h, qldpc_minsum32_decoder_create): the algorithm of qldpc_minsum_decode_batch with
// damping 1 and every floating-point operation one correctly rounded f32 operation.  tests/minsum32_model.py is the numpy model the kernel equals
// bit for bit; it cannot be compared with the f64 decoders on ordinary inputs (rounding, amplified by a chaotic iteration).
//
// One workgroup per shot, persistent grid over an atomic shot queue, per-shot early exit.  The round is the one of decimation.hip / relay_bp.hip: a
// check pass with one thread per row (rows in degree order: a wave's rows have one degree) that also tests the syndrome of the posteriors the
// pass before left, and a variable pass with one thread per column that rebuilds every incoming message from its check's record in ascending check
// order.  Messages never reach memory.
// LDS: V[n] f32, a 16-byte record per row (alpha*min1, alpha*min2, sign bits 0-55, argmin 56-62, total sign 63: one ds_read_b128), one byte per row
// (degree | syndrome bit << 7) and the unsat flags.  The index tables stay where the graph handle keeps them (HBM/L2, slot-major: coalesced, read-only,
// shared by every workgroup of the chip): at 4 + 2 bytes per edge they would cost circ144 more LDS than V and the records together, and LDS is what
// buys the second workgroup of a CU here.  circ72 Z 14 KB, circ144 Z 51 KB (LDS would hold three workgroups; 87 VGPRs = 5 waves per SIMD hold two of
// 512 threads, which is what the occupancy query at creation reports), circ288 Z 150 KB (one workgroup of 1024).
// CLEAN (host-verified: no degree-1 row, finite priors, bounded alpha -- no NaN or inf can arise): the NaN test goes and the clip is one v_med3_f32.
// Every loop is bounded by the host tables and max_iter; workgroup barriers are the only synchronisation.
#include "common.h"
#include "launchers.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace qldpc {

constexpr int kF32Lds = 160 * 1024;       // dynamic LDS of a workgroup: all of a CU's (the kernel has no static LDS)
constexpr int kF32RowDeg = 56;            // sign bits of a record

struct alignas(16) F32Rec { float a1, a2; uint32_t lo, hi; };

struct F32Args {
    int m, n, cdeg;
    const int32_t *row_of_slot, *col_of_slot;
    const uint8_t *degr;           // [m] degree of the row in slot s
    const uint16_t *ell_col;       // [round_up(rdeg, 8)][m] by row slot
    const uint32_t *ell_var;       // [cdeg][n] by column slot: (row slot << 8) | position in the row, ascending rows
    int64_t B;
    const int8_t *synd;
    const float *prior_s;          // [n] prior32 by column SLOT
    const float *alpha;            // [max_iter] alpha32
    float clip;
    int max_iter;
    int8_t *out_err; double *out_llr; uint8_t *out_conv; int32_t *out_iter;
    int offR, offD, offF;
    int *queue;                    // next shot (zeroed before the launch)
};

// NaN -> 0, then clip (the reference's rules, src/decoding/kernels.py:325-333); clean inputs have no NaN
template <bool CLEAN>
__device__ __forceinline__ float clip_f32(float q, float clip) {
    if (CLEAN) return __builtin_amdgcn_fmed3f(q, -clip, clip);
    if (q != q) return 0.0f;
    if (q > clip) return clip;
    if (q < -clip) return -clip;
    return q;
}

template <int BLOCK, bool CLEAN>
__global__ __launch_bounds__(BLOCK) void minsum_f32_kernel(F32Args A) {
    extern __shared__ unsigned char lds[];
    float *V = reinterpret_cast<float *>(lds);
    F32Rec *REC = reinterpret_cast<F32Rec *>(lds + A.offR);
    uint8_t *SD = lds + A.offD;                                                    // degree | syndrome bit << 7, by row slot
    int *F = reinterpret_cast<int *>(lds + A.offF);                                // [0], [1] unsat flags, [2] shot
    const int m = A.m, n = A.n, tid = threadIdx.x, T = A.max_iter;
    const float clip = A.clip;

    for (;;) {
        if (tid == 0) F[2] = atomicAdd(A.queue, 1);
        if (tid < 2) F[tid] = 0;
        __syncthreads();
        const int64_t b = F[2];
        if (b >= A.B) break;
        for (int c = tid; c < n; c += BLOCK) V[A.col_of_slot[c]] = A.prior_s[c];
        for (int i = tid; i < m; i += BLOCK) SD[i] = (uint8_t)(A.degr[i] | ((A.synd[b * m + A.row_of_slot[i]] & 1) << 7));
        __syncthreads();
        bool conv = false;
        int itc = T - 1;
        for (int it = 0; it <= T; it++) {                                            // (pass T only tests the syndrome of iteration T - 1)
            const float alpha = A.alpha[it < T ? it : T - 1];
            // ---------------- check pass: syndrome of V (iteration it - 1), then the records of iteration it ----------------
            for (int i = tid; i < m; i += BLOCK) {                                   // i = row slot
                const unsigned sd = SD[i];
                const int deg = (int)(sd & 127u);
                const bool csyn = sd >> 7;
                float p1p = 0.0f, p2p = 0.0f;
                unsigned long long ip = 0ull;
                if (it > 0 && deg > 0) { const F32Rec t = REC[i]; p1p = t.a1; p2p = t.a2; ip = (unsigned long long)t.lo | ((unsigned long long)t.hi << 32); }
                const int argp = (int)((ip >> 56) & 127);
                const bool spp = (ip >> 63) & 1;
                bool par = csyn, sp = csyn;
                float min1 = INFINITY, min2 = INFINITY;
                int arg = 127;
                unsigned long long negbits = 0ull;
                for (int k = 0; k < deg; k++) {
                    const int col = A.ell_col[(size_t)k * m + i];
                    const float v = V[col];
                    par ^= (v < 0.0f);
                    float x = v;                                                     // iteration 0: Q = prior32, unclipped
                    if (it > 0) {
                        const float mag = (k == argp) ? p2p : p1p;
                        const float rr = (spp != (bool)((ip >> k) & 1)) ? -mag : mag;
                        x = clip_f32<CLEAN>(v - rr, clip);
                    }
                    const bool neg = CLEAN ? (x < 0.0f) : !(x >= 0.0f);
                    sp ^= neg;
                    negbits |= (unsigned long long)neg << k;
                    const float a = fabsf(x);
                    if (a < min1) { min2 = min1; min1 = a; arg = k; }
                    else if (a < min2) { min2 = a; }
                }
                if (it >= 1 && par) F[it & 1] = 1;                                   // (a row without entries and syndrome 1: never satisfied)
                if (it < T && deg > 0) {
                    const unsigned long long w = negbits | ((unsigned long long)arg << 56) | ((unsigned long long)sp << 63);
                    F32Rec t;
                    t.a1 = alpha * min1; t.a2 = alpha * min2; t.lo = (uint32_t)w; t.hi = (uint32_t)(w >> 32);
                    REC[i] = t;
                }
            }
            __syncthreads();
            if (it >= 1 && F[it & 1] == 0) { conv = true; itc = it - 1; break; }     // V holds the posteriors of iteration it - 1: they reproduce the syndrome
            if (it == T) break;
            if (tid == 0) F[(it + 1) & 1] = 0;
            // ---------------- variable pass: V_j = (0 + R ... in ascending check order) + prior32_j ----------------
            for (int c = tid; c < n; c += BLOCK) {                                   // c = column slot
                float s = 0.0f;
                for (int d = 0; d < A.cdeg; d++) {
                    const uint32_t e = A.ell_var[(size_t)d * n + c];
                    if (e == 0xFFFFFFFFu) break;
                    const int i = (int)(e >> 8), k = (int)(e & 255u);
                    const F32Rec t = REC[i];
                    const unsigned long long inf = (unsigned long long)t.lo | ((unsigned long long)t.hi << 32);
                    const float mag = (k == (int)((inf >> 56) & 127)) ? t.a2 : t.a1;
                    s += ((bool)((inf >> 63) & 1) != (bool)((inf >> k) & 1)) ? -mag : mag;
                }
                V[A.col_of_slot[c]] = s + A.prior_s[c];
            }
            __syncthreads();
        }
        for (int j = tid; j < n; j += BLOCK) {
            const float v = V[j];
            A.out_llr[b * n + j] = (double)v;
            A.out_err[b * n + j] = (v < 0.0f) ? 1 : 0;
        }
        if (tid == 0) { A.out_conv[b] = conv ? 1 : 0; A.out_iter[b] = itc; }
        __syncthreads();                                                             // every thread has read the flags and V before the next shot resets them
    }
}

typedef void (*F32Kernel)(F32Args);
static F32Kernel f32_kernel(int block, bool clean) {
    if (block == 256) return clean ? minsum_f32_kernel<256, true> : minsum_f32_kernel<256, false>;
    if (block == 512) return clean ? minsum_f32_kernel<512, true> : minsum_f32_kernel<512, false>;
    return clean ? minsum_f32_kernel<1024, true> : minsum_f32_kernel<1024, false>;
}

}  // namespace qldpc

using namespace qldpc;

struct qldpc_minsum32_decoder : DecoderBase {
    float clip = 20.0f;
    int wg_per_cu = 0;
    bool clean = false;
    int offR = 0, offD = 0, offF = 0;
    ~qldpc_minsum32_decoder() { quiesce(device, hand); }
    int launch(int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t s);
};

// Enqueues the decode of B shots on `s`.  Callers hold mu.
int qldpc_minsum32_decoder::launch(int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t s) {
    F32Args A;
    A.m = m; A.n = n; A.cdeg = g->max_col_deg;
    A.row_of_slot = g->d_row_of_slot; A.col_of_slot = g->d_col_of_slot; A.degr = g->d_deg_of_rslot;
    A.ell_col = g->d_ell_col_s; A.ell_var = g->d_ell_var_s;
    A.B = B; A.synd = d_synd; A.prior_s = d_prior.as<float>(); A.alpha = d_alpha.as<float>(); A.clip = clip; A.max_iter = max_iter;
    A.out_err = d_err; A.out_llr = d_llr; A.out_conv = d_conv; A.out_iter = d_iter;
    A.offR = offR; A.offD = offD; A.offF = offF;
    A.queue = d_queue.as<int>();
    return decoder_launch(*this, f32_kernel(block, clean), kF32Lds, A, B, s);
}

namespace qldpc {

// Creation on a ready f64 alpha table (the circuit plan holds one per sector); the exported form builds the table from the alpha mode.
int minsum32_decoder_create_tab(const qldpc_graph *g, const double *prior, int max_iter, const std::vector<double> &tab, double clip_llr, int flags,
                                qldpc_minsum32_decoder **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(g != nullptr && prior != nullptr, "NULL argument");
    QLDPC_REQUIRE(max_iter >= 1, "max_iter must be >= 1 (got %d)", max_iter);
    const float clip32 = (float)clip_llr;
    QLDPC_REQUIRE(std::isfinite(clip32) && clip32 > 0.0f, "clip_llr must be finite and > 0 as an f32 (got %g)", clip_llr);
    const int fb = flags & (QLDPC_FLAG_F32_BLOCK_256 | QLDPC_FLAG_F32_BLOCK_512 | QLDPC_FLAG_F32_BLOCK_1024);
    QLDPC_REQUIRE((fb & (fb - 1)) == 0, "more than one QLDPC_FLAG_F32_BLOCK_* flag");
    const int m = g->m, n = g->n;
    // ---- what the kernel holds
    if (m < 1 || n < 1 || !g->d_ell_col_s || !g->d_ell_var_s || !g->d_row_of_slot || !g->d_col_of_slot || !g->d_deg_of_rslot) {
        set_error("the f32 decoder needs 1 <= m < 2^24 and 1 <= n < 65535 (m=%d n=%d)", m, n);
        return QLDPC_ERR_UNSUPPORTED;
    }
    if (g->max_row_deg > kF32RowDeg) {
        set_error("the f32 decoder supports row degree <= %d (this graph: %d)", kF32RowDeg, g->max_row_deg);
        return QLDPC_ERR_UNSUPPORTED;
    }
    QLDPC_USE_DEVICE(g->device);                                    // ahead of D: a return deletes D on its device, then the caller's device comes back
    std::unique_ptr<qldpc_minsum32_decoder> D(new qldpc_minsum32_decoder());
    D->g = g; D->device = g->device; D->m = m; D->n = n; D->max_iter = max_iter; D->flags = flags & QLDPC_FLAG_PUBLIC_MASK; D->clip = clip32;
    // LDS layout: V | records | degree and syndrome bytes | flags
    D->offR = (int)round_up((int64_t)n * 4, 16);
    D->offD = D->offR + m * 16;
    D->offF = (int)round_up((int64_t)D->offD + m, 16);
    const int64_t bytes = (int64_t)D->offF + 16;
    if (bytes > kF32Lds) {
        set_error("the f32 decoder keeps 4 bytes per column and 17 per row in LDS: %d columns and %d rows need %lld bytes, more than %d", n, m, (long long)bytes,
                  kF32Lds);
        return QLDPC_ERR_UNSUPPORTED;
    }
    D->lds = (int)bytes;
    // ---- inputs in f32: round to nearest even; +-inf and NaN pass through
    std::vector<float> alpha32(max_iter), prior_s(n);
    for (int k = 0; k < max_iter; k++) alpha32[k] = (float)tab[k];
    std::vector<int32_t> cos(n);                                    // the graph handle's column slots: stable, by descending degree (graph.hip)
    for (int j = 0; j < n; j++) cos[j] = j;
    std::stable_sort(cos.begin(), cos.end(), [&](int a, int b) { return g->colptr[a + 1] - g->colptr[a] > g->colptr[b + 1] - g->colptr[b]; });
    for (int c = 0; c < n; c++) prior_s[c] = (float)prior[cos[c]];
    // clean: nothing below can produce an inf or a NaN (|V| <= max_col_deg * alpha * max(|prior|, clip) + |prior| < 2^128)
    bool clean = !(flags & QLDPC_FLAG_F32_GENERIC) && clip32 <= 0x1p100f && g->max_col_deg < 65536;
    for (int i = 0; i < m && clean; i++) clean = g->indptr[i + 1] - g->indptr[i] != 1;
    for (int k = 0; k < max_iter && clean; k++) clean = alpha32[k] > 0.0f && alpha32[k] <= 1024.0f;
    for (int c = 0; c < n && clean; c++) clean = std::fabs(prior_s[c]) <= 0x1p100f;
    D->clean = clean;
    // ---- workgroup size.  One workgroup of a CU: all 1024 threads; else the size whose passes have work for every thread (a row and eight columns),
    // and the host asks the runtime whether as many workgroups as LDS allows (two are enough) are resident with it; if not, the next smaller size.
    const int by_lds = kF32Lds / D->lds, work = std::max(m, n / 8);
    int block = fb == QLDPC_FLAG_F32_BLOCK_256 ? 256 : fb == QLDPC_FLAG_F32_BLOCK_512 ? 512 : fb == QLDPC_FLAG_F32_BLOCK_1024 ? 1024
                : by_lds < 2 ? 1024 : work > 256 ? 512 : 256;
    int rc;
    for (;; block >>= 1) {
        const void *kern = reinterpret_cast<const void *>(f32_kernel(block, clean));
        if ((rc = ensure_max_lds(g->device, kern, kF32Lds)) != QLDPC_OK) return rc;
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, block, (size_t)D->lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
        D->block = block; D->wg_per_cu = nb;
        if (fb || block == 256 || nb >= std::min(by_lds, 2)) break;
    }
    if (D->wg_per_cu < 1) { set_error("the f32 decoder's kernel is not launchable with %d threads and %d bytes of LDS", D->block, D->lds); return QLDPC_ERR_HIP; }
    D->grid_cap = cu_count(g->device) * D->wg_per_cu;
    if ((rc = upload(D->d_prior, prior_s)) || (rc = upload(D->d_alpha, alpha32)) || (rc = D->d_queue.ensure(16))) return rc;
    *out = D.release();
    return QLDPC_OK;
}

int minsum32_lock_and_launch(qldpc_minsum32_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter,
                             hipStream_t s) {
    return decoder_lock_and_launch(D, B, d_synd, d_err, d_llr, d_conv, d_iter, s);
}

}  // namespace qldpc

QLDPC_EXPORT int qldpc_minsum32_decoder_create(const qldpc_graph *g, const double *prior, int max_iter, int alpha_mode, double alpha_val,
                                               const double *alpha_seq, int alpha_len, double clip_llr, int flags, qldpc_minsum32_decoder **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(max_iter >= 1, "max_iter must be >= 1 (got %d)", max_iter);
    std::vector<double> tab;
    const int rc = build_alpha_table(max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, tab);
    if (rc != QLDPC_OK) return rc;
    return minsum32_decoder_create_tab(g, prior, max_iter, tab, clip_llr, flags, out);
}

QLDPC_EXPORT void qldpc_minsum32_decoder_destroy(qldpc_minsum32_decoder *D) { delete D; }

QLDPC_EXPORT int qldpc_minsum32_decoder_info(const qldpc_minsum32_decoder *D, int *lds_bytes, int *threads, int *wg_per_cu, int *form) {
    QLDPC_REQUIRE(D != nullptr, "decoder is NULL");
    if (lds_bytes) *lds_bytes = D->lds;
    if (threads) *threads = D->block;
    if (wg_per_cu) *wg_per_cu = D->wg_per_cu;
    if (form) *form = D->clean ? QLDPC_F32_FORM_CLEAN : 0;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_minsum32_decode_batch_dev(qldpc_minsum32_decoder *D, int64_t B, const int8_t *d_syndromes, int8_t *d_err, double *d_llr,
                                                 uint8_t *d_conv, int32_t *d_iter, void *stream) {
    return decoder_decode_dev(D, B, d_syndromes, d_err, d_llr, d_conv, d_iter, stream);
}

QLDPC_EXPORT int qldpc_minsum32_decode_batch(qldpc_minsum32_decoder *D, int64_t B, const int8_t *syndromes, int8_t *err, double *llr, uint8_t *conv,
                                             int32_t *iter) {
    return decoder_decode_host(D, "f32 decode", B, syndromes, err, llr, conv, iter);
}
