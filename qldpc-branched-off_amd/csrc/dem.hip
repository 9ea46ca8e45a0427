// Sampler of a detector error model (DEM) for the circuit plan (circuit.hip): a list of independent error mechanisms, each with a probability, the
// detectors it flips and the logical observables it flips, in at most two sectors.  New here: the reference has no counterpart.
//
// The law (include/qldpc_hip.h, qldpc_circuit_plan_create_dem): trial g = trial_begin + t; mechanism l lives in Philox block q = l >> 2, word w = l & 3 of
// o = philox4x32_10(counter (lo32(g), hi32(g), q, 3), key (lo32(seed), hi32(seed))) and fires iff o[w] < thr_l = floor(p_l * 2^32).  Domain word 3 is this
// sampler's (0: code capacity, 1 and 2: the circuit sampler, 0x52......: Relay-BP).  A firing mechanism XORs its detector lists into the sectors' bit
// sets and its logical masks into the sectors' accumulators, so the result does not depend on grid, block size or lane mapping.
#include "common.h"
#include "launchers.h"
#include "sampler_common.h"

namespace qldpc {

// The frame of sampler_common.h; one lane per Philox block = four mechanisms.  thr is padded with zeros to a multiple of four (a padded entry never
// fires: no word is < 0), so a lane reads its four thresholds as one 16-byte load; l < n_mech still bounds every table access.
__global__ __launch_bounds__(256) void dem_sample_kernel(int64_t B, int64_t trial_begin, uint32_t seed_lo, uint32_t seed_hi, int n_mech,
                                                         const uint4 *__restrict__ thr4, SigTab T0, SigTab T1, SampleOut O) {
    extern __shared__ uint32_t sm[];
    const int nblk = (n_mech + 3) >> 2;
    sample_trials<false>(sm, B, trial_begin, O, 0, nullptr, [&](int64_t, uint64_t g, const SampleLds &L) {
        for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
            const uint4 th = thr4[blk];
            if ((th.x | th.y | th.z | th.w) == 0u) continue;                                   // four mechanisms with p = 0 (or padding): nothing to draw
            uint32_t o[4];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 3u, seed_lo, seed_hi, o);
            const uint32_t tw[4] = {th.x, th.y, th.z, th.w};
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int l = 4 * blk + w;
                if (l < n_mech && o[w] < tw[w]) {
                    xor_signature(T0, l, L.b0, &L.lacc[0]);
                    if (O.two) xor_signature(T1, l, L.b1, &L.lacc[1]);
                }
            }
        }
    });
}

int dem_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, int n_mech, const uint32_t *d_thr, const SigTab &T0, const SigTab &T1, const SampleOut &O,
                      hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    const SampleShape shape = sample_shape(O.n0, O.n1, O.two, B);
    hipLaunchKernelGGL(dem_sample_kernel, dim3(shape.grid), dim3(256), shape.words * 4, s, B, trial_begin, (uint32_t)seed, (uint32_t)(seed >> 32), n_mech,
                       reinterpret_cast<const uint4 *>(d_thr), T0, T1, O);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

// Every rule of qldpc_circuit_plan_create_dem that the descriptor alone decides; the error text names the sector or the mechanism.
int dem_validate(const qldpc_dem_desc *D) {
    QLDPC_REQUIRE(D != nullptr, "detector error model descriptor is NULL");
    QLDPC_REQUIRE(D->n_sectors == 1 || D->n_sectors == 2, "n_sectors must be 1 or 2 (got %d)", D->n_sectors);
    QLDPC_REQUIRE(D->n_mech >= 0 && D->n_mech < ((int64_t)1 << 31) - 4, "n_mech out of range (%lld)", (long long)D->n_mech);
    QLDPC_REQUIRE(D->prob != nullptr, "detector error model: prob is NULL");
    for (int s = 0; s < D->n_sectors; s++) {
        QLDPC_REQUIRE(D->det_ptr[s] && D->det_idx[s] && D->logmask[s], "detector error model: sector %d has a NULL table (det_ptr, det_idx, logmask)", s);
        QLDPC_REQUIRE(D->k[s] >= 0 && D->k[s] <= 64, "detector error model: sector %d has k = %d (0..64)", s, D->k[s]);
        QLDPC_REQUIRE(D->n_det[s] >= 1 && D->n_det[s] < 65536, "detector error model: sector %d has %d detectors (1..65535)", s, D->n_det[s]);
        QLDPC_REQUIRE(D->layer_rows[s] >= 0, "detector error model: sector %d has layer_rows = %d", s, D->layer_rows[s]);
    }
    for (int64_t l = 0; l < D->n_mech; l++) {
        const double p = D->prob[l];
        QLDPC_REQUIRE(p >= 0.0 && p < 1.0, "detector error model: mechanism %lld has probability %g (0 <= p < 1)", (long long)l, p);   // NaN fails both
    }
    for (int s = 0; s < D->n_sectors; s++) {
        const int32_t *ptr = D->det_ptr[s];
        const uint64_t allowed = D->k[s] == 64 ? ~(uint64_t)0 : (((uint64_t)1 << D->k[s]) - 1);
        QLDPC_REQUIRE(ptr[0] == 0, "detector error model: sector %d: det_ptr[0] = %d, not 0", s, ptr[0]);
        for (int64_t l = 0; l < D->n_mech; l++) {
            QLDPC_REQUIRE(ptr[l + 1] >= ptr[l], "detector error model: sector %d, mechanism %lld: det_ptr is not monotone", s, (long long)l);
            for (int32_t e = ptr[l]; e < ptr[l + 1]; e++) {
                const int d = D->det_idx[s][e];
                QLDPC_REQUIRE(d < D->n_det[s], "detector error model: sector %d, mechanism %lld: detector %d out of range (%d detectors)", s, (long long)l, d,
                              D->n_det[s]);
                QLDPC_REQUIRE(e == ptr[l] || d > (int)D->det_idx[s][e - 1], "detector error model: sector %d, mechanism %lld: detectors not strictly ascending",
                              s, (long long)l);
            }
            QLDPC_REQUIRE((D->logmask[s][l] & ~allowed) == 0, "detector error model: sector %d, mechanism %lld: logmask has a bit at or above k = %d", s,
                          (long long)l, D->k[s]);
        }
    }
    return QLDPC_OK;
}

}  // namespace qldpc
