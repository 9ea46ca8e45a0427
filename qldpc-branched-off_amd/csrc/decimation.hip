// BP with guided decimation (Yao, Laird, Gokduman, Pfister et al., "Belief propagation decoding of quantum LDPC codes with guided decimation",
// 2024): constant-alpha min-sum in short rounds.  A round that does not converge is followed by a decimation step: the `per_round` most
// reliable undecided columns (largest |V_j|, ties to the lowest column) are frozen to their hard decision by replacing their prior with
// +-fix_llr, and the next round starts from the marginals the last one left.  The semantics are stated at qldpc_decim_decode_batch in
// include/qldpc_hip.h; tests/decimation_model.py is the numpy model the kernel equals bit for bit.
//
// One workgroup per shot, persistent grid, shots handed out through an atomic queue.  A round is one leg of relay_bp_kernel (relay_bp.hip)
// with gamma_j = 0 and bias_j in place of prior_j: both kernels call the one leg of bp_leg.h (slot tables, 24-byte compressed check state,
// order of every floating-point operation) and differ in the bias they hand it.
// LDS: V[n] f64 (or a per-workgroup slab in HBM/L2 when it does not fit: VG), the check states, two bits per ORIGINAL column (fixed, sign of
// the fixed value) as two bit planes of 32-bit words, the unsat flags and the per-wave candidates of the selection.
// Selection: every thread keeps the best (|V| bits, column) of its own columns j = tid, tid + NT, ...; a pick is a lexicographic max over
// the wave through __shfl_xor, one candidate per wave in LDS (two buffers that alternate: one barrier per pick), and the same combine over
// the waves in every thread.  The thread that owns the winner freezes it and rescans its own columns.  The comparison is exact (integer
// compare of the magnitude bits, then the column), so lane and wave order cannot matter.  Every loop is bounded by per_round, n, t_round and
// max_rounds; workgroup barriers are the only synchronisation.
#include "bp_leg.h"
#include "launchers.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace qldpc {

struct DecimArgs {
    SlotGraph G;
    int64_t B;
    const int8_t *synd;
    const double *prior;           // [n] finite (host-verified, or the documented precondition of the _dev entry)
    double alpha, clip, fix;
    int t_round, max_rounds, per_round;
    int iter_bias;                 // added to the iteration count written out (-1: the circuit plan's judge adds one per shot)
    int8_t *out_err; double *out_llr; uint8_t *out_conv; int32_t *out_iters, *out_rounds, *out_fixed;   // out_llr / out_rounds / out_fixed may be NULL
    int offP, offI, offB, offS, offF, offK, offC;
    double *vglobal;               // VG: V[n] per workgroup in HBM/L2
    int *queue;                    // next shot (zeroed before the launch)
};

// selection key of a marginal: the bits of |v| (they order like the magnitudes, +inf the largest); a NaN counts as 0
__device__ __forceinline__ unsigned long long decim_key(double v) {
    return (v != v) ? 0ull : ((unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull);
}
// (k, c) before (ok, oc): larger key, then lower column.  "No candidate" is (0, INT_MAX), which every real column beats.
__device__ __forceinline__ bool decim_better(unsigned long long ok, int oc, unsigned long long k, int c) { return ok > k || (ok == k && oc < c); }

template <bool VG>
__global__ __launch_bounds__(1024) void decim_bp_kernel(DecimArgs A) {
    extern __shared__ unsigned char lds[];
    double *V;
    if (VG) V = A.vglobal + (size_t)blockIdx.x * A.G.n; else V = reinterpret_cast<double *>(lds);
    double2 *SP = reinterpret_cast<double2 *>(lds + A.offP);                       // (alpha*min1, alpha*min2) per check
    unsigned long long *SI = reinterpret_cast<unsigned long long *>(lds + A.offI); // bits 0-55 input signs, 56-62 argmin (127 = none), 63 total sign
    uint32_t *FX = reinterpret_cast<uint32_t *>(lds + A.offB);                     // bit j: ORIGINAL column j is fixed
    uint32_t *SG = reinterpret_cast<uint32_t *>(lds + A.offS);                     // bit j: it is fixed to -fix_llr
    int *F = reinterpret_cast<int *>(lds + A.offF);                                // [0], [1] unsat flags, [2] shot
    unsigned long long *WK = reinterpret_cast<unsigned long long *>(lds + A.offK); // [2][16] per-wave candidate keys
    int *WC = reinterpret_cast<int *>(lds + A.offC);                               // [2][16] and their columns
    const int n = A.G.n, tid = threadIdx.x, NT = blockDim.x, T = A.t_round;
    const int nw = NT >> 6, nwords = (n + 31) >> 5;
    const double clip = A.clip, alpha = A.alpha, fix = A.fix;

    for (;;) {
        if (tid == 0) F[2] = atomicAdd(A.queue, 1);
        __syncthreads();
        const int64_t b = F[2];
        if (b >= A.B) break;
        for (int j = tid; j < n; j += NT) V[j] = A.prior[j];
        for (int w = tid; w < nwords; w += NT) { FX[w] = 0u; SG[w] = 0u; }
        int iters = 0, rounds = 0, nfix = 0;
        bool conv = false;
        for (int r = 0; r <= A.max_rounds; r++) {                                    // (uniform: every thread holds the same r, nfix, conv)
            if (tid < 2) F[tid] = 0;
            __syncthreads();
            const LegResult L = bp_leg(A.G, A.synd, b, T, alpha, clip, V, SP, SI, F, [&](int j, double) {       // V_j = s_j + bias_j
                const uint32_t bit = 1u << (j & 31);
                return (FX[j >> 5] & bit) ? ((SG[j >> 5] & bit) ? -fix : fix) : A.prior[j];
            });
            if (L.conv) conv = true;                                                 // (a converged round ends the loop below)
            iters += L.itc;
            rounds = r + 1;
            if (conv || r == A.max_rounds || nfix == n) break;
            // ---------------- decimation: freeze the min(per_round, unfixed) most reliable unfixed columns ----------------
            unsigned long long lk = 0ull;
            int lc = INT_MAX;
            for (int j = tid; j < n; j += NT) {                                      // ascending j and a strict >: the lowest column among equals
                if ((FX[j >> 5] >> (j & 31)) & 1u) continue;
                const unsigned long long k = decim_key(V[j]);
                if (lc == INT_MAX || k > lk) { lk = k; lc = j; }
            }
            const int npick = min(A.per_round, n - nfix);
            for (int p = 0; p < npick; p++) {
                unsigned long long wk = lk;
                int wc = lc;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned long long ok = __shfl_xor(wk, off, 64);
                    const int oc = __shfl_xor(wc, off, 64);
                    if (decim_better(ok, oc, wk, wc)) { wk = ok; wc = oc; }
                }
                const int buf = (p & 1) * 16;
                if ((tid & 63) == 0) { WK[buf + (tid >> 6)] = wk; WC[buf + (tid >> 6)] = wc; }
                __syncthreads();
                unsigned long long gk = WK[buf];
                int gc = WC[buf];
                for (int w = 1; w < nw; w++) {
                    const unsigned long long ok = WK[buf + w];
                    const int oc = WC[buf + w];
                    if (decim_better(ok, oc, gk, gc)) { gk = ok; gc = oc; }
                }
                // npick <= the number of unfixed columns, so gc is a column; the test keeps every index in bounds whatever happens
                if (gc < n && gc % NT == tid) {                                      // the owner freezes it and looks for its next best
                    const uint32_t bit = 1u << (gc & 31);
                    const bool neg = V[gc] < 0.0;
                    V[gc] = neg ? -fix : fix;
                    FX[gc >> 5] |= bit;                                              // one writer between two barriers
                    if (neg) SG[gc >> 5] |= bit;
                    lk = 0ull; lc = INT_MAX;
                    for (int j = tid; j < n; j += NT) {
                        if ((FX[j >> 5] >> (j & 31)) & 1u) continue;
                        const unsigned long long k = decim_key(V[j]);
                        if (lc == INT_MAX || k > lk) { lk = k; lc = j; }
                    }
                }
                if (gc < n) nfix++;
            }
        }
        for (int j = tid; j < n; j += NT) {
            const double v = V[j];
            A.out_err[b * n + j] = (v < 0.0) ? 1 : 0;
            if (A.out_llr) A.out_llr[b * n + j] = v;
        }
        if (tid == 0) {
            A.out_conv[b] = conv ? 1 : 0;
            A.out_iters[b] = iters + A.iter_bias;
            if (A.out_rounds) A.out_rounds[b] = rounds;
            if (A.out_fixed) A.out_fixed[b] = nfix;
        }
        __syncthreads();
    }
}

// Relay-BP's layout with its round_up(n, 4) * 2 bytes of draws replaced by two bit planes of ceil(n / 32) words, plus 384 bytes of candidates
static size_t decim_lds_bytes(const qldpc_graph *g, bool vg, DecimArgs &A) {
    A.offB = leg_lds_prefix(g, vg, A.offP, A.offI);
    const int plane = (int)round_up((int64_t)((g->n + 31) / 32) * 4, 16);
    A.offS = A.offB + plane;
    A.offF = A.offS + plane;
    A.offK = A.offF + 16;
    A.offC = A.offK + 2 * 16 * 8;
    return (size_t)A.offC + 2 * 16 * 4;
}

// 0: not supported, 1: everything in LDS, 2: V in global memory.  A graph Relay-BP refuses (tables, row degree, LDS) is refused here too.
static int decim_mode(const qldpc_graph *g) {
    if (relay_mode(g) == 0) return 0;
    DecimArgs A;
    if (decim_lds_bytes(g, false, A) <= 160 * 1024) return 1;
    return decim_lds_bytes(g, true, A) <= 160 * 1024 ? 2 : 0;
}

int decim_unsupported(const qldpc_graph *g) {
    set_error("guided decimation does not support this graph (m=%d n=%d, max row degree %d): it needs row degree <= 56 and the check state in 160 KB of LDS",
              g->m, g->n, g->max_row_deg);
    return QLDPC_ERR_UNSUPPORTED;
}

bool decim_supported(const qldpc_graph *g) { return decim_mode(g) != 0; }

int decim_check_params(const DecimParams &P) {
    QLDPC_REQUIRE(std::isfinite(P.alpha) && P.alpha > 0.0, "alpha must be finite and > 0");
    QLDPC_REQUIRE(std::isfinite(P.clip) && P.clip > 0.0, "clip_llr must be finite and > 0");
    QLDPC_REQUIRE(std::isfinite(P.fix) && P.fix > 0.0, "fix_llr must be finite and > 0");
    QLDPC_REQUIRE(P.t_round >= 1, "t_round must be >= 1");
    QLDPC_REQUIRE(P.max_rounds >= 0 && P.max_rounds < (1 << 20), "max_rounds must be in [0, 2^20)");
    QLDPC_REQUIRE(P.per_round >= 1 && P.per_round <= 64, "per_round must be in 1..64");
    return QLDPC_OK;
}

// callers hold g->mu and have validated the parameters (decim_check_params); the workspaces are handed over in stream order (common.h)
int decim_decode_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, const DecimParams &P, int iter_bias, int8_t *d_err,
                        double *d_llr, uint8_t *d_conv, int32_t *d_iters, int32_t *d_rounds, int32_t *d_fixed, hipStream_t stream) {
    const int mode = decim_mode(g);
    if (mode == 0) return decim_unsupported(g);
    if (B == 0) return QLDPC_OK;
    DecimArgs A;
    A.G = slot_graph(g);
    A.B = B; A.synd = d_synd; A.prior = d_prior;
    A.alpha = P.alpha; A.clip = P.clip; A.fix = P.fix;
    A.t_round = P.t_round; A.max_rounds = P.max_rounds; A.per_round = P.per_round;
    A.iter_bias = iter_bias;
    A.out_err = d_err; A.out_llr = d_llr; A.out_conv = d_conv; A.out_iters = d_iters; A.out_rounds = d_rounds; A.out_fixed = d_fixed;
    const bool vg = mode == 2;
    const size_t lds = decim_lds_bytes(g, vg, A);
    return shot_queue_launch(g, B, vg ? decim_bp_kernel<true> : decim_bp_kernel<false>, A, lds, vg, stream);
}

}  // namespace qldpc

using namespace qldpc;

static int decim_entry_checks(const qldpc_graph *g, int64_t B, const DecimParams &P) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    return decim_check_params(P);
}

QLDPC_EXPORT int qldpc_decim_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior, double alpha,
                                              double clip_llr, int t_round, int max_rounds, int per_round, double fix_llr, int8_t *d_err,
                                              double *d_llr, uint8_t *d_conv, int32_t *d_iters, int32_t *d_rounds, int32_t *d_fixed, void *stream) {
    const DecimParams P{alpha, clip_llr, fix_llr, t_round, max_rounds, per_round};
    int rc = decim_entry_checks(g, B, P);
    if (rc != QLDPC_OK) return rc;
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_syndromes && d_prior && d_err && d_llr && d_conv && d_iters, "a device pointer is NULL");
    QLDPC_USE_DEVICE(g->device);
    std::lock_guard<std::mutex> lk(g->mu);
    return decim_decode_launch(g, B, d_syndromes, d_prior, P, 0, d_err, d_llr, d_conv, d_iters, d_rounds, d_fixed, reinterpret_cast<hipStream_t>(stream));
}

QLDPC_EXPORT int qldpc_decim_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, double alpha, double clip_llr,
                                          int t_round, int max_rounds, int per_round, double fix_llr, int8_t *err, double *llr, uint8_t *conv,
                                          int32_t *iters, int32_t *rounds, int32_t *fixed) {
    const DecimParams P{alpha, clip_llr, fix_llr, t_round, max_rounds, per_round};
    int rc = decim_entry_checks(g, B, P);
    if (rc != QLDPC_OK) return rc;
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(syndromes && prior && err && conv && iters, "a pointer is NULL");
    const size_t m = g->m, n = g->n;
    for (size_t j = 0; j < n; j++) QLDPC_REQUIRE(std::isfinite(prior[j]), "prior[%zu] is not finite", j);
    QLDPC_USE_DEVICE(g->device);
    if (!decim_supported(g)) return decim_unsupported(g);
    HostStage S(g->ws_io, g->mu_io);          // the graph handle's grow-only slab
    const auto dp = S.in(prior, n);
    const auto dl = llr ? S.out(llr, B, n) : Staged<double>{};        // not asked for: the launch gets NULL
    const auto ds = S.in(syndromes, B, m);
    const auto de = S.out(err, B, n);
    const auto dc = S.out(conv, B);
    const auto di = S.out(iters, B);
    const auto dr = S.out(rounds, B);           // rounds, fixed: NULL stays on the device
    const auto df = S.out(fixed, B);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        rc = decim_decode_launch(g, B, S[ds], S[dp], P, 0, S[de], S[dl], S[dc], S[di], S[dr], S[df], nullptr);
    }
    return rc != QLDPC_OK ? rc : S.finish("decimation decode", HostStage::kCopies);
}
