// Soft-readout noise of a circuit plan and the per-shot prior its confidence levels buy the decoder.  New here: the reference has no counterpart.  The
// laws are stated at qldpc_circuit_plan_use_soft_readout and qldpc_soft_priors in include/qldpc_hip.h; tests/soft_model.py is the numpy model both
// kernels equal bit for bit.
//
// Sampler.  On top of the plan's ordinary faults (domains 1 and 2, drawn exactly as circuit_sample_kernel draws them) the readout of every MeasX / MeasZ
// location l of trial g lands in one of 2K bins -- K confidence levels on the wrong side, then K on the right side -- by counting the cuts that word
// l & 3 of Philox(g, l >> 2, domain 7) has reached.  A readout on the wrong side XORs the location's measurement-fault signature; the level, and only the
// level, goes into the record uint8[B][n_meas].  The law's compare is a 64-bit one (a cut may be 2^32); the kernel does it in 32 bits the way
// noise_model.hip does: the zero cuts travel as a count, the others as cut - 1.
//
// Prior.  Levels and the host-built tables in, prior[B][n] out: every measurement adds level * weight to its column's 16-bit counter in LDS (a mixed-radix
// index over the column's measurements), and the row is then stored coalesced as lut[lut_ptr[j] + I_j].  I_j is an integer sum, so the lane order cannot
// matter, and the device takes no logarithm: the lut holds every value a column can take.
#include "common.h"
#include "launchers.h"
#include "sampler_common.h"

#include <algorithm>
#include <cmath>

namespace qldpc {

// By value, so in SGPRs (every index is a compile-time constant after unrolling).  The 2K - 1 cuts of the law, in bin order; the slots past them
// hold 0xFFFFFFFF, which no word exceeds.
struct SoftArgs {
    uint32_t levels;           // K
    uint32_t zero;             // how many cuts are 0 (a prefix: the cuts ascend)
    uint32_t cm1[31];          // cut - 1 of the others (0xFFFFFFFF in the slot of a zero cut)
};

__device__ __forceinline__ uint32_t soft_bin(const SoftArgs &A, uint32_t u) {
    uint32_t b = A.zero;
#pragma unroll
    for (int i = 0; i < 31; i++) b += (uint32_t)(u > A.cm1[i]);
    return b;                  // <= 2K - 1: a slot counts in `zero` or in a compare, never both
}

// The frame of sampler_common.h with nothing behind its words.  loc_cls holds ceil(n_locs / 4) words (the op codes of a Philox block, zero padded);
// meas_rank[l] is read for MeasX / MeasZ locations only and is their rank 0 .. n_meas - 1, so a level lands inside its row; every signature index is
// bounded by l < n_locs.
__global__ __launch_bounds__(256) void soft_sample_kernel(int64_t B, int64_t trial_begin, uint32_t seed_lo, uint32_t seed_hi, uint32_t thr, SoftArgs A, int n_locs,
                                                          const uint8_t *__restrict__ loc_type, const uint32_t *__restrict__ loc_cls,
                                                          const int32_t *__restrict__ meas_rank, int n_meas, SigTab Z, SigTab X, SampleOut O,
                                                          uint8_t *__restrict__ levels) {
    extern __shared__ uint32_t sm[];
    const int nblk = (n_locs + 3) >> 2;
    sample_trials<true>(sm, B, trial_begin, O, 0, nullptr, [&](int64_t t, uint64_t g, const SampleLds &L) {
        uint8_t *rec = levels + t * (int64_t)n_meas;
        for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
            uint32_t o[4];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 1u, seed_lo, seed_hi, o);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int l = 4 * blk + w;
                if (l < n_locs && o[w] < thr) fire_location(Z, X, loc_type, g, l, seed_lo, seed_hi, L.b0, L.b1, L.lacc);
            }
            const uint32_t cls = loc_cls[blk];
            // a byte is MeasX (4) or MeasZ (5) iff byte >> 1 == 2; most blocks hold no measurement and draw no second Philox
            bool any = false;
#pragma unroll
            for (int w = 0; w < 4; w++) any = any || (((cls >> (8 * w)) & 0xFEu) == 4u);
            if (!any) continue;
            uint32_t u[4];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 7u, seed_lo, seed_hi, u);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int l = 4 * blk + w;
                const uint32_t ty = (cls >> (8 * w)) & 0xFFu;
                if (l >= n_locs || (ty != C_OP_MEAS_X && ty != C_OP_MEAS_Z)) continue;
                const uint32_t bin = soft_bin(A, u[w]);
                const bool flipped = bin < A.levels;
                const int k = meas_rank[l];
                if ((unsigned)k < (unsigned)n_meas) rec[k] = (uint8_t)(flipped ? bin : bin - A.levels);
                if (flipped) {
                    if (ty == C_OP_MEAS_X) xor_signature(Z, 2 * l, L.b0, &L.lacc[0]);      // component 4: Z on slot 0
                    else xor_signature(X, 2 * l, L.b1, &L.lacc[1]);                        // component 1: X on slot 0
                }
            }
        }
    });
}

// One workgroup per shot (grid-stride).  LDS: ceil(n / 2) uint32 words of 16-bit counters, column j in half j & 1 of word j >> 1 (the host checks
// that a column's run has at most 65536 entries, so with levels below K a half never carries into its neighbour).
//   scatter  thread tid takes measurements tid, tid + NT, ... and adds level * weight to the counter of the measurement's column;
//   store    thread tid stores columns tid, tid + NT, ...: consecutive lanes write consecutive doubles.
// A level is clamped to K - 1, a column outside 0 .. n - 1 is skipped (-1 is the rule's "no column") and I_j is held inside the column's lut run, so
// tables that break the rules (possible only through the _dev entry, which cannot read them) still address nothing outside lut, the counters and the row.
__global__ __launch_bounds__(256) void soft_prior_kernel(int64_t B, int K, int n_meas, const uint8_t *__restrict__ levels, const int32_t *__restrict__ meas_col,
                                                         const int32_t *__restrict__ meas_w, int n, const int32_t *__restrict__ lut_ptr,
                                                         const double *__restrict__ lut, double *__restrict__ prior) {
    extern __shared__ uint32_t sm[];
    const int nc = (n + 1) >> 1;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        for (int w = threadIdx.x; w < nc; w += blockDim.x) sm[w] = 0;
        __syncthreads();
        const uint8_t *rec = levels + b * (int64_t)n_meas;
        for (int k = threadIdx.x; k < n_meas; k += blockDim.x) {
            const int j = meas_col[k];
            if ((unsigned)j >= (unsigned)n) continue;
            const uint32_t lv = min((uint32_t)rec[k], (uint32_t)(K - 1));
            const uint32_t add = (lv * (uint32_t)meas_w[k]) & 0xFFFFu;
            if (add) atomicAdd(&sm[j >> 1], add << (16 * (j & 1)));
        }
        __syncthreads();
        double *row = prior + b * (int64_t)n;
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const int base = lut_ptr[j], last = lut_ptr[j + 1] - 1 - base;
            int I = (int)((sm[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
            if (I > last) I = last;
            if (I < 0) I = 0;
            row[j] = lut[base + I];
        }
        __syncthreads();
    }
}

static size_t prior_lds_bytes(int n) { return ((size_t)(n + 1) / 2) * 4; }
static const size_t kMaxLds = 160 * 1024;
static const int kMaxRun = 65536;

int soft_readout_check(int levels, const double *flip_mass, const double *keep_mass, SoftReadoutHost *out) {
    QLDPC_REQUIRE(levels >= 1 && levels <= QLDPC_SOFT_MAX_LEVELS, "levels = %d is outside 1..%d", levels, QLDPC_SOFT_MAX_LEVELS);
    QLDPC_REQUIRE(flip_mass != nullptr && keep_mass != nullptr, "flip_mass or keep_mass is NULL");
    const int K = levels;
    double S[2 * QLDPC_SOFT_MAX_LEVELS];
    double run = 0.0;
    for (int b = 0; b < 2 * K; b++) {
        const double w = b < K ? flip_mass[b] : keep_mass[b - K];
        QLDPC_REQUIRE(std::isfinite(w) && w >= 0.0, "%s[%d] = %g is negative or not finite", b < K ? "flip_mass" : "keep_mass", b < K ? b : b - K, w);
        run += w;
        S[b] = run;
    }
    QLDPC_REQUIRE(S[2 * K - 1] > 0.0 && std::isfinite(S[2 * K - 1]), "flip_mass[0..%d] and keep_mass[0..%d] sum to %g: a readout channel needs a positive finite sum",
                  K - 1, K - 1, S[2 * K - 1]);
    SoftReadoutHost H{};
    H.levels = K;
    for (int b = 0; b < 2 * K - 1; b++) H.cut[b] = (uint64_t)std::floor(std::ldexp(S[b] / S[2 * K - 1], 32));
    H.cut[2 * K - 1] = (uint64_t)1 << 32;
    for (int lv = 0; lv < K; lv++) {
        const uint64_t f = H.cut[lv] - (lv ? H.cut[lv - 1] : 0), k = H.cut[K + lv] - H.cut[K + lv - 1];
        QLDPC_REQUIRE(f + k > 0, "level %d has no mass: flip_mass[%d] and keep_mass[%d] both come to 0 of 2^32, so the level has no flip probability", lv, lv, lv);
    }
    *out = H;
    return QLDPC_OK;
}

int soft_sample_launch(int64_t B, int64_t trial_begin, uint64_t seed, uint32_t thr, const SoftReadoutHost &R, int n_locs, const uint8_t *d_loc_type,
                       const uint32_t *d_loc_cls, const int32_t *d_meas_rank, int n_meas, const SigTab &Z, const SigTab &X, const SampleOut &O, uint8_t *d_levels,
                       hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    SoftArgs A{};
    A.levels = (uint32_t)R.levels;
    for (int i = 0; i < 31; i++) {
        const uint64_t cut = i < 2 * R.levels - 1 ? R.cut[i] : (uint64_t)1 << 32;
        A.zero += cut == 0;
        A.cm1[i] = (uint32_t)(cut - 1);                          // (0 - 1 wraps to 0xFFFFFFFF; 2^32 - 1 is 0xFFFFFFFF too)
    }
    const SampleShape shape = sample_shape(O.n0, O.n1, O.two, B);
    hipLaunchKernelGGL(soft_sample_kernel, dim3(shape.grid), dim3(256), shape.words * 4, s, B, trial_begin, (uint32_t)seed, (uint32_t)(seed >> 32), thr, A, n_locs,
                       d_loc_type, d_loc_cls, d_meas_rank, n_meas, Z, X, O, d_levels);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

int soft_check_tables(int levels, int n_meas, const int32_t *meas_col, const int32_t *meas_w, int n, const int32_t *lut_ptr, const double *lut) {
    QLDPC_REQUIRE(levels >= 1 && levels <= QLDPC_SOFT_MAX_LEVELS, "levels = %d is outside 1..%d", levels, QLDPC_SOFT_MAX_LEVELS);
    QLDPC_REQUIRE(n_meas >= 0, "n_meas = %d is negative", n_meas);
    QLDPC_REQUIRE(n >= 1, "n = %d is below 1", n);
    QLDPC_REQUIRE(lut_ptr && lut, "lut_ptr or lut is NULL");
    QLDPC_REQUIRE(n_meas == 0 || (meas_col && meas_w), "meas_col or meas_w is NULL but n_meas = %d", n_meas);
    std::vector<int64_t> run((size_t)n, 1);                     // K^c of the measurements met so far: the weight the next one must carry
    for (int k = 0; k < n_meas; k++) {
        const int j = meas_col[k];
        QLDPC_REQUIRE(j >= -1 && j < n, "meas_col[%d] = %d is outside -1..%d", k, j, n - 1);
        if (j < 0) continue;
        QLDPC_REQUIRE((int64_t)meas_w[k] == run[j], "meas_w[%d] = %d, but the measurements of column %d before it span %lld entries (that weight, levels^rank, expected)",
                      k, meas_w[k], j, (long long)run[j]);
        run[j] *= levels;
        QLDPC_REQUIRE(run[j] <= kMaxRun, "column %d: measurement %d brings its run to %lld entries, above the %d a 16-bit counter addresses", j, k,
                      (long long)run[j], kMaxRun);
    }
    QLDPC_REQUIRE(lut_ptr[0] == 0, "lut_ptr[0] = %d, not 0", lut_ptr[0]);
    for (int j = 0; j < n; j++)
        QLDPC_REQUIRE((int64_t)lut_ptr[j + 1] - lut_ptr[j] == run[j], "lut_ptr[%d] - lut_ptr[%d] = %d, but column %d has a run of %lld entries (levels^measurements)",
                      j + 1, j, lut_ptr[j + 1] - lut_ptr[j], j, (long long)run[j]);
    for (int i = 0; i < lut_ptr[n]; i++) QLDPC_REQUIRE(std::isfinite(lut[i]), "lut[%d] is not finite", i);
    return QLDPC_OK;
}

int soft_prior_supported(int n) {
    if (prior_lds_bytes(n) > kMaxLds) {
        set_error("the soft prior kernel holds a 16-bit counter per column in LDS: n = %d does not fit in 160 KB (n <= 81920)", n);
        return QLDPC_ERR_UNSUPPORTED;
    }
    return QLDPC_OK;
}

int soft_prior_launch(int device, int64_t B, int levels, int n_meas, const uint8_t *d_levels, const int32_t *d_meas_col, const int32_t *d_meas_w, int n,
                      const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    int rc = soft_prior_supported(n);
    if (rc != QLDPC_OK) return rc;
    const size_t lds = prior_lds_bytes(n);
    if (lds > 48 * 1024 && (rc = ensure_max_lds(device, reinterpret_cast<const void *>(soft_prior_kernel), (int)kMaxLds)) != QLDPC_OK) return rc;
    const unsigned grid = (unsigned)std::min<int64_t>(B, 256 * 16);
    hipLaunchKernelGGL(soft_prior_kernel, dim3(grid), dim3(256), lds, s, B, levels, n_meas, d_levels, d_meas_col, d_meas_w, n, d_lut_ptr, d_lut, d_prior);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc

using namespace qldpc;

static int current_device(int *device) {
    QLDPC_HIP_TRY(hipGetDevice(device));
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_soft_priors_dev(int64_t B, int32_t levels, int32_t n_meas, const uint8_t *d_levels, const int32_t *d_meas_col, const int32_t *d_meas_w,
                                       int32_t n, const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, void *stream) {
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    QLDPC_REQUIRE(levels >= 1 && levels <= QLDPC_SOFT_MAX_LEVELS, "levels = %d is outside 1..%d", levels, QLDPC_SOFT_MAX_LEVELS);
    QLDPC_REQUIRE(n_meas >= 0 && n >= 1, "n_meas = %d or n = %d is out of range", n_meas, n);
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_levels && d_meas_col && d_meas_w && d_lut_ptr && d_lut && d_prior, "a device pointer is NULL");
    int device = 0, rc = current_device(&device);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(device);
    return soft_prior_launch(device, B, levels, n_meas, d_levels, d_meas_col, d_meas_w, n, d_lut_ptr, d_lut, d_prior, reinterpret_cast<hipStream_t>(stream));
}

QLDPC_EXPORT int qldpc_soft_priors(int64_t B, int32_t levels, int32_t n_meas, const uint8_t *level, const int32_t *meas_col, const int32_t *meas_w, int32_t n,
                                   const int32_t *lut_ptr, const double *lut, double *prior) {
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    int rc = soft_check_tables(levels, n_meas, meas_col, meas_w, n, lut_ptr, lut);
    if (rc != QLDPC_OK) return rc;
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(prior != nullptr && (level != nullptr || n_meas == 0), "level or prior is NULL");
    for (int64_t b = 0; b < B; b++)
        for (int k = 0; k < n_meas; k++)
            QLDPC_REQUIRE(level[b * n_meas + k] < levels, "level[%lld][%d] = %d is not below levels = %d (shot %lld, measurement %d)", (long long)b, k,
                          (int)level[b * n_meas + k], levels, (long long)b, k);
    int device = 0;
    if ((rc = current_device(&device)) != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(device);
    if ((rc = soft_prior_supported(n)) != QLDPC_OK) return rc;
    HostStage S;
    const auto dl = S.in(level, B, (size_t)n_meas);
    const auto dc = S.in(meas_col, (size_t)n_meas);
    const auto dw = S.in(meas_w, (size_t)n_meas);
    const auto dup = S.in(lut_ptr, (size_t)n + 1);
    const auto dlu = S.in(lut, (size_t)lut_ptr[n]);
    const auto dp = S.out(prior, B, n);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    rc = soft_prior_launch(device, B, levels, n_meas, S[dl], S[dc], S[dw], n, S[dup], S[dlu], S[dp], nullptr);
    return rc != QLDPC_OK ? rc : S.finish("soft priors", HostStage::kCopies);
}
