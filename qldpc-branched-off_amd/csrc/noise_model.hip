// Per-class, biased Pauli noise of a circuit plan.  New here: the reference fires every location at one p and draws uniform Paulis.  The law is
// stated at qldpc_circuit_plan_use_noise_model in include/qldpc_hip.h; tests/noise_model_model.py is the numpy model the kernel equals bit for bit.
//
// The kernel is circuit_sample_kernel (circuit.hip) with two changes.  A location's threshold is that of its class: the classes of the four
// locations of a Philox block come as ONE uint32 (a byte each, coalesced: lane = block), and the threshold is picked out of the seven that travel in
// the argument struct by a chain of selects -- no table load per location.  A faulty IDLE or CNOT with a weight table picks its Pauli by counting the
// cuts its random word has reached instead of r % K.  The law's compare is a 64-bit one (a cut may be 2^32); the kernel does it in 32 bits:
// for 1 <= cut <= 2^32, r >= cut iff r > cut - 1 with cut - 1 a uint32, and the cuts that are 0 -- a prefix, the cuts ascend -- are reached by
// every r, so they travel as a count and their slots hold 0xFFFFFFFF, which no r exceeds.
#include "common.h"
#include "launchers.h"
#include "sampler_common.h"

#include <algorithm>
#include <cmath>

namespace qldpc {

// By value, so in SGPRs: every index below is a compile-time constant after unrolling (a run-time index would put the struct in scratch).
struct NoiseModelArgs {
    uint32_t thr[7];           // threshold per op code (C_OP_*); [0] stays 0
    uint32_t weighted;         // bit 0: the idle cuts are in force (else r % 3); bit 1: the CNOT cuts (else r % 15)
    uint32_t idle_zero, cnot_zero;                 // how many cuts are 0
    uint32_t idle_cm1[2], cnot_cm1[14];            // cut - 1 of the others (0xFFFFFFFF in the slot of a zero cut)
};

__device__ __forceinline__ uint32_t class_threshold(const NoiseModelArgs &A, uint32_t ty) {
    uint32_t t = 0u;           // an op code outside 1..6 (the zero padding of the last block) never fires
#pragma unroll
    for (uint32_t c = C_OP_CNOT; c <= C_OP_IDLE; c++) t = ty == c ? A.thr[c] : t;
    return t;
}

// The Pauli components (mask of sampler_common.h) of faulty location l of type ty in trial g: fault_components with the cut-based choice
__device__ __forceinline__ int model_components(const NoiseModelArgs &A, uint32_t ty, uint64_t g, int l, uint32_t seed_lo, uint32_t seed_hi) {
    if (ty == C_OP_MEAS_X || ty == C_OP_PREP_X) return 4;
    if (ty == C_OP_MEAS_Z || ty == C_OP_PREP_Z) return 1;
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)l, 2u, seed_lo, seed_hi, r);
    if (ty == C_OP_IDLE) {
        uint32_t i = r[0] % 3u;
        if (A.weighted & 1u) i = A.idle_zero + (uint32_t)(r[0] > A.idle_cm1[0]) + (uint32_t)(r[0] > A.idle_cm1[1]);
        return c_idle_comp[i];                       // i <= 2: a slot counts in idle_zero or in a compare, never both
    }
    uint32_t i = r[0] % 15u;
    if (A.weighted & 2u) {
        i = A.cnot_zero;
#pragma unroll
        for (int j = 0; j < 14; j++) i += (uint32_t)(r[0] > A.cnot_cm1[j]);
    }
    return c_cnot_comp[i];                           // i <= 14, likewise
}

// The frame of sampler_common.h with nothing behind its words.  loc_cls holds ceil(n_locs / 4) words; every signature index is bounded by l < n_locs.
__global__ __launch_bounds__(256) void noise_model_sample_kernel(int64_t B, int64_t trial_begin, uint32_t seed_lo, uint32_t seed_hi, NoiseModelArgs A, int n_locs,
                                                                 const uint32_t *__restrict__ loc_cls, SigTab Z, SigTab X, SampleOut O) {
    extern __shared__ uint32_t sm[];
    const int nblk = (n_locs + 3) >> 2;
    sample_trials<true>(sm, B, trial_begin, O, 0, nullptr, [&](int64_t, uint64_t g, const SampleLds &L) {
        for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
            uint32_t o[4];
            const uint32_t cls = loc_cls[blk];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 1u, seed_lo, seed_hi, o);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int l = 4 * blk + w;
                const uint32_t ty = (cls >> (8 * w)) & 0xFFu;
                if (l < n_locs && o[w] < class_threshold(A, ty))
                    fire_components(Z, X, model_components(A, ty, g, l, seed_lo, seed_hi), l, L.b0, L.b1, L.lacc);
            }
        }
    });
}

// cut[j] of the law for j = 0 .. K - 2; QLDPC_ERR_INVALID naming the table and the index
static int weight_cuts(const char *name, const double *w, int K, uint64_t *cut) {
    double S[15];
    double run = 0.0;
    for (int j = 0; j < K; j++) {
        QLDPC_REQUIRE(std::isfinite(w[j]) && w[j] >= 0.0, "%s[%d] = %g is negative or not finite", name, j, w[j]);
        run += w[j];
        S[j] = run;
    }
    QLDPC_REQUIRE(S[K - 1] > 0.0 && std::isfinite(S[K - 1]), "%s[0..%d] sums to %g: a weight table needs a positive finite sum", name, K - 1, S[K - 1]);
    for (int j = 0; j < K - 1; j++) cut[j] = (uint64_t)std::floor(std::ldexp(S[j] / S[K - 1], 32));
    return QLDPC_OK;
}

int noise_model_check(const qldpc_noise_model *M, NoiseModelHost *out) {
    static const char *const cls[7] = {"", "CNOT", "PrepX", "PrepZ", "MeasX", "MeasZ", "IDLE"};
    NoiseModelHost H{};
    for (int ty = C_OP_CNOT; ty <= C_OP_IDLE; ty++) {
        QLDPC_REQUIRE(M->rate[ty] >= 0.0 && M->rate[ty] < 1.0, "noise model rate[%d] (%s) = %g is outside [0, 1)", ty, cls[ty], M->rate[ty]);      // (NaN fails both)
        H.thr[ty] = bernoulli_threshold(M->rate[ty]);
    }
    int rc;
    H.idle_weighted = M->idle_w != nullptr;
    H.cnot_weighted = M->cnot_w != nullptr;
    if (M->idle_w && (rc = weight_cuts("idle_w", M->idle_w, 3, H.idle_cut)) != QLDPC_OK) return rc;
    if (M->cnot_w && (rc = weight_cuts("cnot_w", M->cnot_w, 15, H.cnot_cut)) != QLDPC_OK) return rc;
    *out = H;
    return QLDPC_OK;
}

std::vector<uint32_t> noise_model_pack_classes(const std::vector<uint8_t> &loc_type) {
    std::vector<uint32_t> out((loc_type.size() + 3) / 4, 0u);
    for (size_t l = 0; l < loc_type.size(); l++) out[l >> 2] |= (uint32_t)loc_type[l] << (8 * (l & 3));
    return out;
}

int noise_model_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, const NoiseModelHost &M, int n_locs, const uint32_t *d_loc_cls, const SigTab &Z,
                              const SigTab &X, const SampleOut &O, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    NoiseModelArgs A{};
    for (int ty = C_OP_CNOT; ty <= C_OP_IDLE; ty++) A.thr[ty] = M.thr[ty];
    A.weighted = (M.idle_weighted ? 1u : 0u) | (M.cnot_weighted ? 2u : 0u);
    for (int j = 0; j < 2; j++) { A.idle_zero += M.idle_cut[j] == 0; A.idle_cm1[j] = (uint32_t)(M.idle_cut[j] - 1); }        // (0 - 1 wraps to 0xFFFFFFFF)
    for (int j = 0; j < 14; j++) { A.cnot_zero += M.cnot_cut[j] == 0; A.cnot_cm1[j] = (uint32_t)(M.cnot_cut[j] - 1); }
    const SampleShape shape = sample_shape(O.n0, O.n1, O.two, B);
    hipLaunchKernelGGL(noise_model_sample_kernel, dim3(shape.grid), dim3(256), shape.words * 4, s, B, trial_begin, (uint32_t)seed, (uint32_t)(seed >> 32), A, n_locs,
                       d_loc_cls, Z, X, O);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc
