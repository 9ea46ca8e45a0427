// Fixed-weight sampler of a circuit plan: every trial has exactly w faulty locations (circuit) or firing mechanisms (detector error model), the set
// uniform among the w-subsets.  It is the stratum "exactly w faults" of the plan's independent sampler when that one draws every location with one
// probability; qldpc_circuit_plan_use_fixed_weight switches a plan to it and back.  New here: the reference has no counterpart.
//
// The law (include/qldpc_hip.h, qldpc_circuit_plan_use_fixed_weight): trial g = trial_begin + t, N = n_locs.  Floyd's algorithm, for i = 0 .. w-1:
// j = N - w + i; o_i = word (i & 3) of philox4x32_10(counter (lo32(g), hi32(g), i >> 2, 4), key (lo32(seed), hi32(seed))); t = (o_i * (j + 1)) >> 32;
// S gets j if t is already in S, else t.  Domain word 4 is this sampler's (0: code capacity, 1 and 2: the circuit sampler, 3: the DEM sampler,
// 0x52......: Relay-BP).  A member of S then does what a faulty location / firing mechanism does in circuit_sample_kernel / dem_sample_kernel:
// XORs into the sectors' bit sets and logical accumulators, so the result is a function of (seed, g, w) alone.
#include "common.h"
#include "launchers.h"
#include "sampler_common.h"

namespace qldpc {

// The frame of sampler_common.h.  LDS behind the frame's words: the membership bit set of S (ceil(N / 32) words) and the list of S (w words).  Per trial:
//   draw     lanes compute t_i for all i in parallel, one Philox block per four steps, into the list;
//   resolve  lane 0 walks the list once against the membership bit set ("taken -> j"): w dependent LDS test-and-set steps.  Step i needs the set
//            after steps 0 .. i-1, so this is the one sequential part; at w ~ 100 it is microseconds per trial beside a decode of milliseconds per batch;
//   fire     lanes take the list entries in parallel, clear the entry's membership word (the set is empty again for the next trial) and XOR the
//            location's signatures (DEM = false) or the mechanism's detector lists and logical masks (DEM = true).
// The membership set is zeroed once (the frame's first barrier comes before anything reads it); the list is written before it is read, never zeroed.
// Every index is bounded on the host: w <= min(N, 4096), t_i <= j < N, and the tables hold 2 N (circuit) or N (DEM) entries.
template <bool DEM>
__global__ __launch_bounds__(256) void fixed_weight_sample_kernel(int64_t B, int64_t trial_begin, uint32_t seed_lo, uint32_t seed_hi, int weight, int n_locs,
                                                                  const uint8_t *__restrict__ loc_type, SigTab T0, SigTab T1, SampleOut O) {
    extern __shared__ uint32_t sm[];
    const int nmem = (n_locs + 31) >> 5, nblk = (weight + 3) >> 2;
    uint32_t *member = sample_carve<false>(sm, O).more, *list = member + nmem;
    for (int i = threadIdx.x; i < nmem; i += blockDim.x) member[i] = 0;
    sample_trials<false>(sm, B, trial_begin, O, 0, nullptr, [&](int64_t, uint64_t g, const SampleLds &L) {
        for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
            uint32_t o[4];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 4u, seed_lo, seed_hi, o);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = 4 * blk + k;
                if (i < weight) list[i] = __umulhi(o[k], (uint32_t)(n_locs - weight + i) + 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < weight; i++) {
                uint32_t l = list[i];
                if ((member[l >> 5] >> (l & 31)) & 1u) { l = (uint32_t)(n_locs - weight + i); list[i] = l; }
                member[l >> 5] |= 1u << (l & 31);
            }
        __syncthreads();
        for (int i = threadIdx.x; i < weight; i += blockDim.x) {
            const int l = (int)list[i];
            member[l >> 5] = 0;                                                                // (several lanes may store the same zero)
            if (DEM) {
                xor_signature(T0, l, L.b0, &L.lacc[0]);
                if (O.two) xor_signature(T1, l, L.b1, &L.lacc[1]);
            } else {
                fire_location(T0, T1, loc_type, g, l, seed_lo, seed_hi, L.b0, L.b1, L.lacc);
            }
        }
    });
}

int fixed_weight_check(int64_t n_locs, int weight) {
    QLDPC_REQUIRE(weight >= 0, "fixed weight %d is negative (-1 switches back to the independent draws)", weight);
    QLDPC_REQUIRE(weight <= QLDPC_FIXED_WEIGHT_MAX, "fixed weight %d is above the limit of %d faults per trial", weight, QLDPC_FIXED_WEIGHT_MAX);
    QLDPC_REQUIRE(weight <= n_locs, "fixed weight %d is above the plan's %lld fault locations", weight, (long long)n_locs);
    if (n_locs > QLDPC_FIXED_WEIGHT_MAX_LOCS) {
        set_error("the fixed-weight sampler holds one bit per fault location in LDS: %lld locations are above its limit of %d", (long long)n_locs,
                  QLDPC_FIXED_WEIGHT_MAX_LOCS);
        return QLDPC_ERR_UNSUPPORTED;
    }
    return QLDPC_OK;
}

int fixed_weight_sample_launch(int device, int64_t B, int64_t trial_begin, uint64_t seed, int weight, int n_locs, bool dem, const uint8_t *d_loc_type,
                               const SigTab &T0, const SigTab &T1, const SampleOut &O, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    int rc = fixed_weight_check(n_locs, weight);
    if (rc != QLDPC_OK) return rc;
    const SampleShape shape = sample_shape(O.n0, O.n1, O.two, B);
    // the frame (at most 16 KiB + 16 B) + membership (at most 64 KiB) + list (at most 16 KiB)
    const size_t lds = (shape.words + (size_t)(n_locs + 31) / 32 + (size_t)weight) * 4;
    const auto kern = dem ? fixed_weight_sample_kernel<true> : fixed_weight_sample_kernel<false>;
    // (the attribute is set once per kernel: the largest request the limits allow, 96 KiB + 16 B)
    const int lds_max = (2 * 2048 + 4 + QLDPC_FIXED_WEIGHT_MAX_LOCS / 32 + QLDPC_FIXED_WEIGHT_MAX) * 4;
    if (lds > 48 * 1024 && (rc = ensure_max_lds(device, reinterpret_cast<const void *>(kern), lds_max)) != QLDPC_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(shape.grid), dim3(256), lds, s, B, trial_begin, (uint32_t)seed, (uint32_t)(seed >> 32), weight, n_locs, d_loc_type, T0, T1, O);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc
