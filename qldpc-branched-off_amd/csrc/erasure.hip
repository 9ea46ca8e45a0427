// Heralded-erasure noise of a circuit plan and the per-shot prior it buys the decoder.  New here: the reference has no counterpart.  The laws are
// stated at qldpc_circuit_plan_use_erasure_noise and qldpc_erasure_priors in include/qldpc_hip.h; tests/erasure_model.py is the numpy model both
// kernels equal bit for bit.
//
// Sampler.  On top of the plan's ordinary faults (domains 1 and 2, drawn exactly as circuit_sample_kernel draws them) location l of trial g is ERASED
// iff word l & 3 of Philox(g, l >> 2, domain 5) is below the threshold of its class; an erased location is fully depolarised (a uniform Pauli of its
// class, identity included, from word 0 of Philox(g, l, domain 6)) and its bit goes into the herald record uint32[B][ceil(n_locs / 32)].
//
// Prior.  Heralds and the host-built tables in, prior[B][n] out: the erased locations of a shot push their (column, h) lists into per-column counters
// in LDS -- an integer add for h = 1, a bit for h = INF -- and the row is then stored coalesced: 0.0 where the bit is set, else lut[lut_ptr[j] + H].
// H is an integer sum, so the lane order cannot matter, and the device takes no logarithm: the lut holds every value a column can take.
#include "common.h"
#include "launchers.h"
#include "sampler_common.h"

#include <algorithm>
#include <cmath>

namespace qldpc {

struct ErasureThr { uint32_t t[8]; };      // threshold per op code (C_OP_*); [0] and [7] stay 0

// the component mask (sampler_common.h) of erased location l of type ty in trial g: uniform over the Paulis of the class, identity included
__device__ __forceinline__ int erased_components(int ty, uint64_t g, int l, uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)l, 6u, seed_lo, seed_hi, r);
    if (ty == C_OP_CNOT) return (int)(r[0] & 15u);
    if (ty == C_OP_IDLE) { const int c = (int)(r[0] & 3u); return c == 2 ? 5 : c == 3 ? 4 : c; }      // {0, 1, 5, 4}: I, X, Y, Z
    if (ty == C_OP_MEAS_X || ty == C_OP_PREP_X) return (r[0] & 1u) ? 4 : 0;
    return (r[0] & 1u) ? 1 : 0;                                                                         // MeasZ / PrepZ
}

// The frame of sampler_common.h.  LDS behind the frame's words: the erased bit set (ceil(n_locs / 32) words), which the frame zeroes per trial and
// stores as the trial's herald row.  Every index is bounded by n_locs or a signature run; the host bounds the LDS request.
__global__ __launch_bounds__(256) void erasure_sample_kernel(int64_t B, int64_t trial_begin, uint32_t seed_lo, uint32_t seed_hi, uint32_t thr, ErasureThr E,
                                                             int n_locs, const uint8_t *__restrict__ loc_type, SigTab Z, SigTab X, SampleOut O,
                                                             uint32_t *__restrict__ erased) {
    extern __shared__ uint32_t sm[];
    const int nblk = (n_locs + 3) >> 2;
    sample_trials<true>(sm, B, trial_begin, O, (n_locs + 31) >> 5, erased, [&](int64_t, uint64_t g, const SampleLds &L) {
        for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
            uint32_t o[4], e[4];
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 1u, seed_lo, seed_hi, o);
            philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)blk, 5u, seed_lo, seed_hi, e);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int l = 4 * blk + w;
                if (l >= n_locs) continue;
                if (o[w] < thr) fire_location(Z, X, loc_type, g, l, seed_lo, seed_hi, L.b0, L.b1, L.lacc);
                const int ty = loc_type[l];
                if (e[w] < E.t[ty & 7]) {
                    atomicOr(&L.more[l >> 5], 1u << (l & 31));
                    fire_components(Z, X, erased_components(ty, g, l, seed_lo, seed_hi), l, L.b0, L.b1, L.lacc);
                }
            }
        }
    });
}

// One workgroup per shot (grid-stride).  LDS (uint32 words): ceil(n / 2) words of 16-bit counters (column j in half j & 1 of word j >> 1; the host
// checks that no column has more than 65535 h = 1 contributions, so a half never carries into its neighbour) and ceil(n / 32) words of INF bits.
//   scatter  a thread takes herald words tid, tid + NT, ... and, for every set bit below n_locs, walks that location's run;
//   store    thread tid stores columns tid, tid + NT, ...: consecutive lanes write consecutive doubles.
// Reads of the tables are bounded by the run ends; a column outside 0 .. n - 1 is skipped and H is held below the column's lut run, so tables that
// break the rules (possible only through the _dev entry, which cannot read them) still address nothing outside lut, the counters and the row.
__global__ __launch_bounds__(256) void erasure_prior_kernel(int64_t B, int n_locs, const uint32_t *__restrict__ erased, const int32_t *__restrict__ loc_ptr,
                                                            const int32_t *__restrict__ loc_col, const uint8_t *__restrict__ loc_h, int n,
                                                            const int32_t *__restrict__ lut_ptr, const double *__restrict__ lut, double *__restrict__ prior) {
    extern __shared__ uint32_t sm[];
    const int nc = (n + 1) >> 1, ni = (n + 31) >> 5, nw = (n_locs + 31) >> 5;
    uint32_t *cnt = sm, *inf = sm + nc;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        for (int w = threadIdx.x; w < nc + ni; w += blockDim.x) sm[w] = 0;
        __syncthreads();
        const uint32_t *rec = erased + b * nw;
        for (int w = threadIdx.x; w < nw; w += blockDim.x) {
            uint32_t bits = rec[w];
            if (w == nw - 1 && (n_locs & 31)) bits &= (1u << (n_locs & 31)) - 1u;
            while (bits) {
                const int l = 32 * w + __builtin_ctz(bits);
                bits &= bits - 1u;
                const int end = loc_ptr[l + 1];
                for (int k = loc_ptr[l]; k < end; k++) {
                    const int j = loc_col[k];
                    if ((unsigned)j >= (unsigned)n) continue;
                    if (loc_h[k] == QLDPC_ERASURE_H_INF) atomicOr(&inf[j >> 5], 1u << (j & 31));
                    else atomicAdd(&cnt[j >> 1], 1u << (16 * (j & 1)));
                }
            }
        }
        __syncthreads();
        double *row = prior + b * n;
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const int base = lut_ptr[j], last = lut_ptr[j + 1] - 1 - base;
            int H = (int)((cnt[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
            if (H > last) H = last;
            if (H < 0) H = 0;
            row[j] = ((inf[j >> 5] >> (j & 31)) & 1u) ? 0.0 : lut[base + H];
        }
        __syncthreads();
    }
}

static size_t sample_lds_bytes(int nsx, int nsz, int n_locs) {
    return (sample_shape(nsx, nsz, true, 1).words + (size_t)(n_locs + 31) / 32) * 4;
}
static size_t prior_lds_bytes(int n) { return ((size_t)(n + 1) / 2 + (size_t)(n + 31) / 32) * 4; }
static const size_t kMaxLds = 160 * 1024;

int erasure_sample_supported(int nsx, int nsz, int64_t n_locs) {
    if (n_locs > (int64_t)8 * kMaxLds || sample_lds_bytes(nsx, nsz, (int)n_locs) > kMaxLds) {
        set_error("the erasure sampler holds one bit per fault location in LDS: %lld locations do not fit in 160 KB", (long long)n_locs);
        return QLDPC_ERR_UNSUPPORTED;
    }
    return QLDPC_OK;
}

int erasure_rates_check(const double *rate, uint32_t thr[8]) {
    for (int ty = 0; ty < 8; ty++) thr[ty] = 0;
    for (int ty = C_OP_CNOT; ty <= C_OP_IDLE; ty++) {
        QLDPC_REQUIRE(rate[ty] >= 0.0 && rate[ty] < 1.0, "erasure rate[%d] = %g is outside [0, 1)", ty, rate[ty]);      // (NaN fails both)
        thr[ty] = bernoulli_threshold(rate[ty]);
    }
    return QLDPC_OK;
}

int erasure_sample_launch(int device, int64_t B, int64_t trial_begin, uint64_t seed, uint32_t thr, const uint32_t ethr[8], int n_locs,
                          const uint8_t *d_loc_type, const SigTab &Z, const SigTab &X, const SampleOut &O, uint32_t *d_erased, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    int rc = erasure_sample_supported(O.n0, O.n1, n_locs);
    if (rc != QLDPC_OK) return rc;
    ErasureThr E;
    for (int i = 0; i < 8; i++) E.t[i] = ethr[i];
    const size_t lds = sample_lds_bytes(O.n0, O.n1, n_locs);
    if (lds > 48 * 1024 && (rc = ensure_max_lds(device, reinterpret_cast<const void *>(erasure_sample_kernel), (int)kMaxLds)) != QLDPC_OK) return rc;
    hipLaunchKernelGGL(erasure_sample_kernel, dim3(sample_shape(O.n0, O.n1, O.two, B).grid), dim3(256), lds, s, B, trial_begin, (uint32_t)seed, (uint32_t)(seed >> 32), thr, E, n_locs,
                       d_loc_type, Z, X, O, d_erased);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

int erasure_check_tables(int n_locs, const int32_t *loc_ptr, const int32_t *loc_col, const uint8_t *loc_h, int n, const int32_t *lut_ptr,
                         const double *lut) {
    QLDPC_REQUIRE(n_locs >= 0, "n_locs = %d is negative", n_locs);
    QLDPC_REQUIRE(n >= 1, "n = %d is below 1", n);
    QLDPC_REQUIRE(loc_ptr && lut_ptr && lut, "loc_ptr, lut_ptr or lut is NULL");
    QLDPC_REQUIRE(loc_ptr[0] == 0, "loc_ptr[0] = %d, not 0", loc_ptr[0]);
    for (int l = 0; l < n_locs; l++) QLDPC_REQUIRE(loc_ptr[l + 1] >= loc_ptr[l], "loc_ptr[%d] = %d is below loc_ptr[%d] = %d", l + 1, loc_ptr[l + 1], l, loc_ptr[l]);
    QLDPC_REQUIRE(loc_ptr[n_locs] == 0 || (loc_col && loc_h), "loc_col or loc_h is NULL but loc_ptr holds %d entries", loc_ptr[n_locs]);
    std::vector<int32_t> c((size_t)n, 0);
    for (int l = 0; l < n_locs; l++)
        for (int k = loc_ptr[l]; k < loc_ptr[l + 1]; k++) {
            QLDPC_REQUIRE(loc_col[k] >= 0 && loc_col[k] < n, "loc_col[%d] = %d is outside 0..%d", k, loc_col[k], n - 1);
            QLDPC_REQUIRE(k == loc_ptr[l] || loc_col[k] > loc_col[k - 1], "loc_col[%d] = %d does not ascend inside the run of location %d", k, loc_col[k], l);
            QLDPC_REQUIRE(loc_h[k] == 1 || loc_h[k] == QLDPC_ERASURE_H_INF, "loc_h[%d] = %d is neither 1 nor %d", k, (int)loc_h[k], QLDPC_ERASURE_H_INF);
            if (loc_h[k] == 1) c[loc_col[k]]++;
        }
    QLDPC_REQUIRE(lut_ptr[0] == 0, "lut_ptr[0] = %d, not 0", lut_ptr[0]);
    for (int j = 0; j < n; j++) {
        QLDPC_REQUIRE(c[j] <= 65535, "column %d has %d contributions with h = 1, above the 65535 a 16-bit counter holds", j, c[j]);
        QLDPC_REQUIRE(lut_ptr[j + 1] - lut_ptr[j] == c[j] + 1, "lut_ptr[%d] - lut_ptr[%d] = %d, but column %d has %d contributions with h = 1 (%d entries expected)",
                      j + 1, j, lut_ptr[j + 1] - lut_ptr[j], j, c[j], c[j] + 1);
    }
    for (int i = 0; i < lut_ptr[n]; i++) QLDPC_REQUIRE(std::isfinite(lut[i]), "lut[%d] is not finite", i);
    return QLDPC_OK;
}

int erasure_prior_supported(int n) {
    if (prior_lds_bytes(n) > kMaxLds) {
        set_error("the erasure prior kernel holds a 16-bit counter and a bit per column in LDS: n = %d does not fit in 160 KB", n);
        return QLDPC_ERR_UNSUPPORTED;
    }
    return QLDPC_OK;
}

int erasure_prior_launch(int device, int64_t B, int n_locs, const uint32_t *d_erased, const int32_t *d_loc_ptr, const int32_t *d_loc_col,
                         const uint8_t *d_loc_h, int n, const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    int rc = erasure_prior_supported(n);
    if (rc != QLDPC_OK) return rc;
    const size_t lds = prior_lds_bytes(n);
    if (lds > 48 * 1024 && (rc = ensure_max_lds(device, reinterpret_cast<const void *>(erasure_prior_kernel), (int)kMaxLds)) != QLDPC_OK) return rc;
    const unsigned grid = (unsigned)std::min<int64_t>(B, 256 * 16);
    hipLaunchKernelGGL(erasure_prior_kernel, dim3(grid), dim3(256), lds, s, B, n_locs, d_erased, d_loc_ptr, d_loc_col, d_loc_h, n, d_lut_ptr, d_lut, d_prior);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc

using namespace qldpc;

static int current_device(int *device) {
    QLDPC_HIP_TRY(hipGetDevice(device));
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_erasure_priors_dev(int64_t B, int32_t n_locs, const uint32_t *d_erased, const int32_t *d_loc_ptr, const int32_t *d_loc_col,
                                          const uint8_t *d_loc_h, int32_t n, const int32_t *d_lut_ptr, const double *d_lut, double *d_prior, void *stream) {
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    QLDPC_REQUIRE(n_locs >= 0 && n >= 1, "n_locs = %d or n = %d is out of range", n_locs, n);
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_erased && d_loc_ptr && d_loc_col && d_loc_h && d_lut_ptr && d_lut && d_prior, "a device pointer is NULL");
    int device = 0, rc = current_device(&device);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(device);
    return erasure_prior_launch(device, B, n_locs, d_erased, d_loc_ptr, d_loc_col, d_loc_h, n, d_lut_ptr, d_lut, d_prior, reinterpret_cast<hipStream_t>(stream));
}

QLDPC_EXPORT int qldpc_erasure_priors(int64_t B, int32_t n_locs, const uint32_t *erased, const int32_t *loc_ptr, const int32_t *loc_col, const uint8_t *loc_h,
                                      int32_t n, const int32_t *lut_ptr, const double *lut, double *prior) {
    QLDPC_REQUIRE(B >= 0, "negative batch size");
    int rc = erasure_check_tables(n_locs, loc_ptr, loc_col, loc_h, n, lut_ptr, lut);
    if (rc != QLDPC_OK) return rc;
    if (B == 0) return QLDPC_OK;
    QLDPC_REQUIRE(prior != nullptr && (erased != nullptr || n_locs == 0), "erased or prior is NULL");
    int device = 0;
    if ((rc = current_device(&device)) != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(device);
    if ((rc = erasure_prior_supported(n)) != QLDPC_OK) return rc;
    const size_t nw = (size_t)(n_locs + 31) / 32, ne = (size_t)loc_ptr[n_locs];
    HostStage S;
    const auto de = S.in(erased, B, nw);
    const auto dlp = S.in(loc_ptr, (size_t)n_locs + 1);
    const auto dlc = S.in(loc_col, ne);
    const auto dlh = S.in(loc_h, ne);
    const auto dup = S.in(lut_ptr, (size_t)n + 1);
    const auto dlu = S.in(lut, (size_t)lut_ptr[n]);
    const auto dp = S.out(prior, B, n);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    rc = erasure_prior_launch(device, B, n_locs, S[de], S[dlp], S[dlc], S[dlh], n, S[dup], S[dlu], S[dp], nullptr);
    return rc != QLDPC_OK ? rc : S.finish("erasure priors", HostStage::kCopies);
}
