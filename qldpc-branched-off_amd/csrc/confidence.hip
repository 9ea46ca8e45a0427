// The confidence of a decoded trial and its histogram.  New here: the reference has no counterpart.  The score is built from the cluster statistics
// that lsd_kernel leaves per shot and sector (qldpc_lsd_stats_batch in include/qldpc_hip.h: uint64[8] a shot, eight zeros where the sector had nothing
// to solve, eight all-ones words where LSD made no statement); the laws are stated at qldpc_circuit_plan_use_confidence, and
// tests/lsd_stats_model.py is the numpy model the kernel equals bit for bit.
//
// One thread per trial.  kind k reads slot k + 1 of each sector: the 1- and 2-norms add over the sectors (saturating at 2^64 - 2, so that the all-ones
// word stays "no statement"), the infinity norms take the maximum; no statement in either sector is no statement for the trial.  With a histogram
// the thread finds bin = #{edges <= score} by bisection of the edge table in LDS and counts hist[bin][outcome]; a workgroup counts in LDS (uint32: at
// most 256 trials a workgroup) and adds every cell it touched to the global histogram once.  Integer counts and sums only: no order enters.
#include "common.h"
#include "launchers.h"

#include <algorithm>

namespace qldpc {

constexpr int kConfBlock = 256;

__device__ __forceinline__ unsigned long long conf_score(int kind, const unsigned long long *z, const unsigned long long *x) {
    const unsigned long long none = ~0ull;
    const unsigned long long a = z[kind + 1], b = x ? x[kind + 1] : 0ull;
    if (z[0] == none || (x && x[0] == none)) return none;
    if (kind % 3 == 2) return a > b ? a : b;
    const unsigned long long s = a + b;
    return (s < a || s == none) ? none - 1ull : s;
}

// LDS: edges uint64[nbins - 1] (padded to 16 bytes), then counts uint32[nbins][4]; both only with a histogram
__global__ __launch_bounds__(kConfBlock) void confidence_kernel(int64_t B, int kind, const unsigned long long *__restrict__ stats_z,
                                                                const unsigned long long *__restrict__ stats_x, const uint8_t *__restrict__ outcome,
                                                                unsigned long long *__restrict__ score, int nbins,
                                                                const unsigned long long *__restrict__ edges, unsigned long long *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char conf_lds[];
    unsigned long long *E = reinterpret_cast<unsigned long long *>(conf_lds);
    unsigned int *cnt = reinterpret_cast<unsigned int *>(conf_lds + ((size_t)(nbins - 1) * 8 + 15) / 16 * 16);
    const int tid = threadIdx.x, T = blockDim.x;
    if (hist) {
        for (int i = tid; i < nbins - 1; i += T) E[i] = edges[i];
        for (int i = tid; i < nbins * 4; i += T) cnt[i] = 0u;
        __syncthreads();
    }
    const int64_t b = (int64_t)blockIdx.x * T + tid;
    if (b < B) {
        const unsigned long long sc = conf_score(kind, stats_z + b * 8, stats_x ? stats_x + b * 8 : nullptr);
        score[b] = sc;
        if (hist) {
            int lo = 0, hi = nbins - 1;                                      // the first edge above the score, nbins - 1 when there is none
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (E[mid] <= sc) lo = mid + 1; else hi = mid;
            }
            atomicAdd(&cnt[lo * 4 + (outcome[b] & 3)], 1u);
        }
    }
    if (hist) {
        __syncthreads();
        for (int i = tid; i < nbins * 4; i += T)
            if (cnt[i]) atomicAdd(&hist[i], (unsigned long long)cnt[i]);
    }
}

int confidence_launch(int device, int64_t B, int kind, const unsigned long long *d_stats_z, const unsigned long long *d_stats_x, const uint8_t *d_outcome,
                      unsigned long long *d_score, int nbins, const unsigned long long *d_edges, unsigned long long *d_hist, hipStream_t stream) {
    if (B == 0) return QLDPC_OK;
    const size_t lds = d_hist ? ((size_t)(nbins - 1) * 8 + 15) / 16 * 16 + (size_t)nbins * 16 : 0;
    const int rc = ensure_max_lds(device, reinterpret_cast<const void *>(confidence_kernel), kConfLdsMax);
    if (rc != QLDPC_OK) return rc;
    hipLaunchKernelGGL(confidence_kernel, dim3((unsigned)((B + kConfBlock - 1) / kConfBlock)), dim3(kConfBlock), lds, stream, B, kind, d_stats_z, d_stats_x,
                       d_outcome, d_score, nbins, d_edges, d_hist);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

int confidence_check(int kind, int nbins, const uint64_t *edges) {
    QLDPC_REQUIRE(kind >= QLDPC_CONF_COLS_1 && kind <= QLDPC_CONF_LLR_INF, "confidence kind %d outside 0..5 (QLDPC_CONF_*)", kind);
    QLDPC_REQUIRE(nbins >= 1 && nbins <= QLDPC_CONF_MAX_BINS, "confidence nbins %d outside 1..%d", nbins, QLDPC_CONF_MAX_BINS);
    QLDPC_REQUIRE(nbins == 1 || edges != nullptr, "edges is NULL but nbins = %d", nbins);
    for (int i = 1; i < nbins - 1; i++)
        QLDPC_REQUIRE(edges[i] > edges[i - 1], "edges[%d] = %llu does not lie above edges[%d] = %llu", i, (unsigned long long)edges[i], i - 1,
                      (unsigned long long)edges[i - 1]);
    return QLDPC_OK;
}

}  // namespace qldpc
