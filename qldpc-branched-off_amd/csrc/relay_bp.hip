// Relay-BP (Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memory", 2025): normalised
// min-sum with a per-variable memory term, run in legs.  Leg 0 uses one memory strength gamma0 for every column; every later leg draws
// new, disordered strengths gamma_j in [gamma_min, gamma_max] from Philox and starts from the previous leg's final marginals.  Every
// converged leg is a solution; the decoder keeps the one of least weight sum_{j: e_j = 1} q_j and stops after `stop_after` solutions
// or after leg `max_legs`.  No OSD stage.
//
// One workgroup per shot, persistent grid, shots handed out through an atomic queue -- the structure of minsum_wg_kernel (minsum_wg.hip)
// with its slot tables and its 24-byte compressed check state (alpha*min1, alpha*min2, argmin, sign bits).  One leg (bp_leg.h, shared
// with decimation.hip) is that kernel's loop with two changes: V (the marginals) is not reset to the prior at the start of a leg r >= 1, and the variable pass writes
//     V_j = s_j + ((1 - gamma_j) * prior_j + gamma_j * V_j)           s_j = 0.0 + sum of R in ascending check order
// (with gamma_j = 0 the existing update).  A marginal that is not finite -- the +-inf messages of degree-1 checks, which the circuit-level
// X-sector matrices have, make it +-inf -- enters the memory term as 0.0: gamma_j * inf would turn the marginal into NaN for gamma_j <= 0,
// and with this rule gamma_j = 0 is the existing update bit for bit on every input.  The check state is rebuilt at every leg start (its
// first check pass is the it == 0 pass).
// LDS: V[n] f64 (or a per-workgroup slab in HBM/L2 when it does not fit: VG), the check states, the memory draws as u16 per column and
// a few words of flags and the weight accumulator.  Every loop is bounded by the iteration and leg counts.
#include "bp_leg.h"
#include "launchers.h"
#include "mc_common.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace qldpc {

struct RelayArgs {
    SlotGraph G;
    int64_t B, shot_begin;
    const int8_t *synd;
    const double *prior;           // [n] finite (host-verified, or the documented precondition of the _dev entry)
    double alpha, clip, gamma0, gamma_min, gamma_range;
    int t0, tr, max_legs, stop_after;
    uint32_t seed_lo, seed_hi, domain;   // domain = 0x52000000 | tag << 20; the leg index is or-ed in
    int iter_bias;                 // added to the iteration count written out (-1: the circuit plan's judge adds one per shot)
    int8_t *out_err; uint8_t *out_conv; int32_t *out_legs, *out_iters, *out_sol;   // out_legs / out_sol may be NULL
    int offP, offI, offG, offF;
    double *vglobal;               // VG: V[n] per workgroup in HBM/L2
    int *queue;                    // next shot (zeroed before the launch)
};

template <bool VG>
__global__ __launch_bounds__(1024) void relay_bp_kernel(RelayArgs A) {
    extern __shared__ unsigned char lds[];
    double *V;
    if (VG) V = A.vglobal + (size_t)blockIdx.x * A.G.n; else V = reinterpret_cast<double *>(lds);
    double2 *SP = reinterpret_cast<double2 *>(lds + A.offP);                       // (alpha*min1, alpha*min2) per check
    unsigned long long *SI = reinterpret_cast<unsigned long long *>(lds + A.offI); // bits 0-55 input signs, 56-62 argmin (127 = none), 63 total sign
    uint16_t *G = reinterpret_cast<uint16_t *>(lds + A.offG);                      // memory draws of the leg by ORIGINAL column
    int *F = reinterpret_cast<int *>(lds + A.offF);                                // [0], [1] unsat flags, [2] shot
    unsigned long long *Wacc = reinterpret_cast<unsigned long long *>(lds + A.offF + 16);   // weight of the leg's hard decision (two's complement)
    const int n = A.G.n, tid = threadIdx.x, NT = blockDim.x;
    const double clip = A.clip, alpha = A.alpha;
    const int nblk = (n + 3) >> 2;

    for (;;) {
        if (tid == 0) F[2] = atomicAdd(A.queue, 1);
        __syncthreads();
        const int64_t b = F[2];
        if (b >= A.B) break;
        const uint64_t shot = (uint64_t)(A.shot_begin + b);
        for (int j = tid; j < n; j += NT) V[j] = A.prior[j];                         // leg 0 starts from the prior
        long long best = LLONG_MAX;
        int nsol = 0, iters = 0, legs = 0;
        for (int r = 0; r <= A.max_legs; r++) {                                      // (uniform: every thread holds the same r, nsol)
            const int T = (r == 0) ? A.t0 : A.tr;
            if (r > 0) {                                                             // gamma_j of leg r: word (j & 3) of block j >> 2, top 16 bits
                for (int q = tid; q < nblk; q += NT) {
                    uint32_t o[4];
                    philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), (uint32_t)q, A.domain | (uint32_t)r, A.seed_lo, A.seed_hi, o);
#pragma unroll
                    for (int w = 0; w < 4; w++)
                        if (4 * q + w < n) G[4 * q + w] = (uint16_t)(o[w] >> 16);
                }
            }
            if (tid < 2) F[tid] = 0;
            if (tid == 0) *Wacc = 0ull;
            __syncthreads();
            const LegResult L = bp_leg(A.G, A.synd, b, T, alpha, clip, V, SP, SI, F, [&](int j, double vj) {   // the variable pass with memory
                const double gam = (r == 0) ? A.gamma0 : A.gamma_min + A.gamma_range * ((double)G[j] * (1.0 / 65536.0));
                const double pj = A.prior[j];
                const double mem = (fabs(vj) < INFINITY) ? vj : 0.0;                 // a non-finite marginal carries no memory (see the header)
                return (1.0 - gam) * pj + gam * mem;
            });
            iters += L.itc;
            legs = r + 1;
            if (L.conv) {
                long long part = 0;
                for (int j = tid; j < n; j += NT)
                    if (V[j] < 0.0) part += relay_weight(A.prior[j]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
                if ((tid & 63) == 0) atomicAdd(Wacc, (unsigned long long)part);
                __syncthreads();
                const long long w = (long long)*Wacc;
                nsol++;
                if (w < best) {                                                      // strictly lighter: the earlier leg wins ties
                    best = w;
                    for (int j = tid; j < n; j += NT) A.out_err[b * n + j] = (V[j] < 0.0) ? 1 : 0;
                }
                __syncthreads();                                                     // the accumulator is read before the next leg zeroes it
            }
            if (nsol >= A.stop_after) break;
        }
        if (nsol == 0)
            for (int j = tid; j < n; j += NT) A.out_err[b * n + j] = (V[j] < 0.0) ? 1 : 0;   // the last leg's hard decision
        if (tid == 0) {
            A.out_conv[b] = nsol > 0 ? 1 : 0;
            A.out_iters[b] = iters + A.iter_bias;
            if (A.out_legs) A.out_legs[b] = legs;
            if (A.out_sol) A.out_sol[b] = nsol;
        }
        __syncthreads();
    }
}

static size_t relay_lds_bytes(const qldpc_graph *g, bool vg, int &offP, int &offI, int &offG, int &offF) {
    offG = leg_lds_prefix(g, vg, offP, offI);
    offF = (int)round_up(offG + round_up(g->n, 4) * 2, 16);
    return (size_t)offF + 32;
}

// 0: not supported, 1: everything in LDS, 2: check states and draws in LDS, V in global memory
int relay_mode(const qldpc_graph *g) {
    if (!g->d_ell_col_s || !g->d_ell_var_s || !g->d_row_of_slot || !g->d_col_of_slot) return 0;
    if (g->m <= 0 || g->n <= 0 || g->max_row_deg > 56) return 0;
    int a, b, c, d;
    if (relay_lds_bytes(g, false, a, b, c, d) <= 160 * 1024) return 1;
    return relay_lds_bytes(g, true, a, b, c, d) <= 160 * 1024 ? 2 : 0;
}

int relay_unsupported(const qldpc_graph *g) {
    set_error("Relay-BP does not support this graph (m=%d n=%d, max row degree %d): it needs row degree <= 56 and the check state in 160 KB of LDS",
              g->m, g->n, g->max_row_deg);
    return QLDPC_ERR_UNSUPPORTED;
}

// callers hold g->mu and have validated the parameters (relay_check_params); the workspaces are handed over in stream order (common.h)
int relay_decode_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, const RelayParams &P, uint64_t seed,
                        int64_t shot_begin, int tag, int iter_bias, int8_t *d_err, uint8_t *d_conv, int32_t *d_legs, int32_t *d_iters,
                        int32_t *d_sol, hipStream_t stream) {
    const int mode = relay_mode(g);
    if (mode == 0) return relay_unsupported(g);
    if (B == 0) return QLDPC_OK;
    RelayArgs A;
    A.G = slot_graph(g);
    A.B = B; A.shot_begin = shot_begin; A.synd = d_synd; A.prior = d_prior;
    A.alpha = P.alpha; A.clip = P.clip; A.gamma0 = P.gamma0; A.gamma_min = P.gamma_min; A.gamma_range = P.gamma_max - P.gamma_min;
    A.t0 = P.t0; A.tr = P.tr; A.max_legs = P.max_legs; A.stop_after = P.stop_after;
    A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32); A.domain = 0x52000000u | ((uint32_t)tag << 20);
    A.iter_bias = iter_bias;
    A.out_err = d_err; A.out_conv = d_conv; A.out_legs = d_legs; A.out_iters = d_iters; A.out_sol = d_sol;
    const bool vg = mode == 2;
    const size_t lds = relay_lds_bytes(g, vg, A.offP, A.offI, A.offG, A.offF);
    return shot_queue_launch(g, B, vg ? relay_bp_kernel<true> : relay_bp_kernel<false>, A, lds, vg, stream);
}

int relay_check_params(const RelayParams &P) {
    QLDPC_REQUIRE(std::isfinite(P.alpha) && P.alpha > 0.0, "alpha must be finite and > 0");
    QLDPC_REQUIRE(std::isfinite(P.clip) && P.clip > 0.0, "clip_llr must be finite and > 0");
    QLDPC_REQUIRE(std::isfinite(P.gamma0) && std::isfinite(P.gamma_min) && std::isfinite(P.gamma_max), "memory strengths must be finite");
    QLDPC_REQUIRE(P.gamma_min <= P.gamma_max, "gamma_min (%g) > gamma_max (%g)", P.gamma_min, P.gamma_max);
    QLDPC_REQUIRE(P.t0 >= 1 && P.tr >= 1, "t0 and tr must be >= 1");
    QLDPC_REQUIRE(P.max_legs >= 0 && P.max_legs < (1 << 20), "max_legs must be in [0, 2^20)");
    QLDPC_REQUIRE(P.stop_after >= 1, "stop_after must be >= 1");
    return QLDPC_OK;
}

// legs summed over the batch into the tally slots of the two sectors (circuit plans after qldpc_circuit_plan_use_relay)
__global__ void relay_legs_tally_kernel(int64_t B, const int32_t *__restrict__ legs_z, const int32_t *__restrict__ legs_x,
                                        unsigned long long *__restrict__ tally) {
    unsigned long long z = 0, x = 0;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) { z += legs_z[b]; if (legs_x) x += legs_x[b]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { z += __shfl_xor(z, off, 64); x += __shfl_xor(x, off, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (z) atomicAdd(&tally[QLDPC_TALLY_LEGS_Z], z);
        if (x) atomicAdd(&tally[QLDPC_TALLY_LEGS_X], x);
    }
}

// d_legs_x NULL: a one-sector plan (the X slot stays as it is)
int relay_legs_tally_launch(int64_t B, const int32_t *d_legs_z, const int32_t *d_legs_x, unsigned long long *d_tally, hipStream_t stream) {
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((B + 255) / 256, 64));
    hipLaunchKernelGGL(relay_legs_tally_kernel, dim3(grid), dim3(256), 0, stream, B, d_legs_z, d_legs_x, d_tally);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc

using namespace qldpc;

static int relay_entry_checks(const qldpc_graph *g, int64_t B, const RelayParams &P, int tag) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    QLDPC_REQUIRE(tag >= 0 && tag <= 15, "tag must be in 0..15");
    return relay_check_params(P);
}

QLDPC_EXPORT int qldpc_relay_decode_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_prior, double alpha,
                                              double clip_llr, double gamma0, double gamma_min, double gamma_max, int t0, int tr, int max_legs,
                                              int stop_after, uint64_t seed, int64_t shot_begin, int tag, int8_t *d_err, uint8_t *d_conv,
                                              int32_t *d_legs, int32_t *d_iters, int32_t *d_solutions, void *stream) {
    const RelayParams P{alpha, clip_llr, gamma0, gamma_min, gamma_max, t0, tr, max_legs, stop_after};
    int rc = relay_entry_checks(g, B, P, tag);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(shot_begin >= 0, "negative shot_begin");
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_syndromes && d_prior && d_err && d_conv && d_legs && d_iters && d_solutions, "a device pointer is NULL");
    QLDPC_USE_DEVICE(g->device);
    std::lock_guard<std::mutex> lk(g->mu);
    return relay_decode_launch(g, B, d_syndromes, d_prior, P, seed, shot_begin, tag, 0, d_err, d_conv, d_legs, d_iters, d_solutions,
                               reinterpret_cast<hipStream_t>(stream));
}

QLDPC_EXPORT int qldpc_relay_decode_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *prior, double alpha,
                                          double clip_llr, double gamma0, double gamma_min, double gamma_max, int t0, int tr, int max_legs,
                                          int stop_after, uint64_t seed, int64_t shot_begin, int tag, int8_t *err, uint8_t *conv, int32_t *legs,
                                          int32_t *iters, int32_t *solutions) {
    const RelayParams P{alpha, clip_llr, gamma0, gamma_min, gamma_max, t0, tr, max_legs, stop_after};
    int rc = relay_entry_checks(g, B, P, tag);
    if (rc != QLDPC_OK) return rc;
    QLDPC_REQUIRE(shot_begin >= 0, "negative shot_begin");
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(syndromes && prior && err && conv && legs && iters && solutions, "a pointer is NULL");
    const size_t m = g->m, n = g->n;
    for (size_t j = 0; j < n; j++) QLDPC_REQUIRE(std::isfinite(prior[j]), "prior[%zu] is not finite", j);
    QLDPC_USE_DEVICE(g->device);
    if (relay_mode(g) == 0) return relay_unsupported(g);
    HostStage S(g->ws_io, g->mu_io);          // the graph handle's grow-only slab
    const auto dp = S.in(prior, n);
    const auto ds = S.in(syndromes, B, m);
    const auto de = S.out(err, B, n);
    const auto dc = S.out(conv, B);
    const auto dg = S.out(legs, B);
    const auto di = S.out(iters, B);
    const auto dn = S.out(solutions, B);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        rc = relay_decode_launch(g, B, S[ds], S[dp], P, seed, shot_begin, tag, 0, S[de], S[dc], S[dg], S[di], S[dn], nullptr);
    }
    return rc != QLDPC_OK ? rc : S.finish("Relay-BP decode", HostStage::kCopies);
}
