// Recorded detection events in place of a sampler: the second front door of the circuit plan (circuit.hip: events -> decode -> OSD -> predict).  New here: the
// reference has no counterpart.
//
// The record format (include/qldpc_hip.h, qldpc_circuit_plan_decode_events): shot i starts at byte i * stride; bit d of a record is (rec[d >> 3] >> (d & 7)) & 1
// (Stim's b8).  Row r of sector s reads bit bit_of_row[s][r]; -1 makes the row constant 0.  Only the first ceil(n_bits / 8) bytes of a record are read and only the
// bits some row names are used.  Both kernels are data movement: no atomics, and nothing depends on grid, block size or lane mapping.
#include "common.h"
#include "launchers.h"
#include "judge.h"

namespace qldpc {

// four 0 / 1 values in the low nibble -> one per byte (the partial products land on disjoint bits, so nothing carries)
__device__ __forceinline__ uint32_t nibble_to_bytes(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }

// rec: the record in LDS as dwords, shifted up by sh bits (the record's byte offset inside its first global dword), so record bit d is bit d + sh of the
// little-endian dword array.  Each lane assembles four consecutive rows and writes them as one aligned dword; the ragged head and tail of the shot's row
// range go as bytes (the way judge_sector_sparse scans det).
template <bool TAB>
__device__ __forceinline__ void unpack_sector(const uint32_t *rec, int sh, const EventsSector &S, int64_t t) {
    int8_t *out = S.syn + t * S.nsyn;
    const int tid = threadIdx.x;
    auto bit = [&](int r) -> uint32_t {
        int d = TAB ? S.tab[r] : S.base + r;
        if (TAB && d < 0) return 0u;
        d += sh;
        return (rec[d >> 5] >> (d & 31)) & 1u;
    };
    const int head = (int)((4 - (reinterpret_cast<uintptr_t>(out) & 3)) & 3), nhead = head < S.nsyn ? head : S.nsyn;
    if (tid < nhead) out[tid] = (int8_t)bit(tid);
    const int nw = (S.nsyn - nhead) >> 2;
    uint32_t *ow = reinterpret_cast<uint32_t *>(out + nhead);
    for (int w = tid; w < nw; w += blockDim.x) {
        const int r = nhead + 4 * w;
        if (TAB) ow[w] = bit(r) | (bit(r + 1) << 8) | (bit(r + 2) << 16) | (bit(r + 3) << 24);
        else {
            const int d = S.base + r + sh;                                 // four consecutive bits, possibly across two dwords (the staging has one dword of slack)
            ow[w] = nibble_to_bytes(__builtin_amdgcn_alignbit(rec[(d >> 5) + 1], rec[d >> 5], d & 31) & 15u);
        }
    }
    const int tail0 = nhead + 4 * nw;
    if (tail0 + tid < S.nsyn) out[tail0 + tid] = (int8_t)bit(tail0 + tid);
}

// one workgroup per shot (grid-stride, as dem_sample_kernel).  The record is staged into LDS once: its aligned dwords as dwords, at most three bytes before and
// after them as bytes, at the byte offset the record has inside its first global dword -- nothing outside [rec, rec + nbytes) is read.
__global__ __launch_bounds__(256) void events_unpack_kernel(int64_t B, const uint8_t *__restrict__ events, int64_t stride, int nbytes, EventsSector S0,
                                                            EventsSector S1, int two, int32_t *__restrict__ fail_counts) {
    extern __shared__ uint32_t sm[];
    if (fail_counts && blockIdx.x == 0 && threadIdx.x < 8) fail_counts[threadIdx.x] = 0;      // as both samplers: the batch's BP failure counters
    uint8_t *sb = reinterpret_cast<uint8_t *>(sm);
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < B; t += gridDim.x) {
        const uint8_t *rec = events + t * stride;
        const int a = (int)(reinterpret_cast<uintptr_t>(rec) & 3);
        const int head = (4 - a) & 3, nhead = head < nbytes ? head : nbytes;
        if (tid < nhead) sb[a + tid] = rec[tid];
        const int nw = (nbytes - nhead) >> 2;
        const uint32_t *gw = reinterpret_cast<const uint32_t *>(rec + nhead);
        uint32_t *lw = sm + ((a + nhead) >> 2);
        for (int w = tid; w < nw; w += blockDim.x) lw[w] = gw[w];
        const int tail0 = nhead + 4 * nw;
        if (tail0 + tid < nbytes) sb[a + tail0 + tid] = rec[tail0 + tid];
        __syncthreads();
        if (S0.tab) unpack_sector<true>(sm, 8 * a, S0, t); else unpack_sector<false>(sm, 8 * a, S0, t);
        if (two) { if (S1.tab) unpack_sector<true>(sm, 8 * a, S1, t); else unpack_sector<false>(sm, 8 * a, S1, t); }
        __syncthreads();
    }
}

int events_unpack_launch(int64_t B, const uint8_t *d_events, int64_t stride, int n_bits, const EventsSector &S0, const EventsSector &S1, bool two,
                         int32_t *d_fail_counts, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    const int nbytes = (n_bits + 7) / 8;
    const size_t lds = (size_t)(((nbytes + 3 + 3) >> 2) + 1) * 4;                             // n_bits <= 131070: at most 16 KiB + 8 B
    const unsigned grid = (unsigned)std::min<int64_t>(B, 256 * 16);
    hipLaunchKernelGGL(events_unpack_kernel, dim3(grid), dim3(256), lds, s, B, d_events, stride, nbytes, S0, S1, two ? 1 : 0, d_fail_counts);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

// The judge without a truth (circuit_judge_kernel's shape: 32 lanes per shot, eight shots per workgroup): the sectors' predictions and one flags byte per shot.
// It reads what the decode left (syndromes, corrections, converged flags) and writes nothing else: no tally, no truth, no outcome.
// TWO = false: X is not read, pred1 is not written and the odd flag bits stay 0.
template <bool SPARSE, bool TWO>
__global__ __launch_bounds__(256) void events_predict_kernel(int64_t B, JudgeSector Z, JudgeSector X, unsigned long long *__restrict__ pred0,
                                                             unsigned long long *__restrict__ pred1, uint8_t *__restrict__ flags) {
    __shared__ uint32_t parbits[SPARSE ? 8 * 2 * 128 : 1];                      // per shot of the workgroup: the two sectors' parity bits (m <= 4096)
    const int lane = threadIdx.x & 31;
    const int64_t b = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (b >= B) return;
    bool zn, zb, xn = true, xb = false;
    uint64_t lz, lx = 0;
    if (SPARSE) {
        uint32_t *par = parbits + (threadIdx.x >> 5) * 256;
        lz = judge_sector_sparse(Z, b, lane, par, zn, zb);
        if (TWO) lx = judge_sector_sparse(X, b, lane, par + 128, xn, xb);
    } else {
        lz = judge_sector(Z, b, lane, zn, zb);
        if (TWO) lx = judge_sector(X, b, lane, xn, xb);
    }
    if (lane == 0) {
        pred0[b] = lz;
        if (TWO) pred1[b] = lx;
        flags[b] = (uint8_t)((Z.conv[b] ? 1 : 0) | (TWO && X.conv[b] ? 2 : 0) | (zb ? 4 : 0) | (xb ? 8 : 0) | (zn ? 0 : 16) | (xn ? 0 : 32));
    }
}

int events_predict_launch(int64_t B, const JudgeSector &Z, const JudgeSector &X, bool two, unsigned long long *d_pred0, unsigned long long *d_pred1,
                          uint8_t *d_flags, hipStream_t s) {
    if (B <= 0) return QLDPC_OK;
    const bool sparse = Z.m <= 4096 && Z.colptr && (!two || (X.m <= 4096 && X.colptr));       // as the judge of a run
    const auto kernel = two ? (sparse ? events_predict_kernel<true, true> : events_predict_kernel<false, true>)
                            : (sparse ? events_predict_kernel<true, false> : events_predict_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + 7) / 8)), dim3(256), 0, s, B, Z, X, d_pred0, d_pred1, d_flags);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc
