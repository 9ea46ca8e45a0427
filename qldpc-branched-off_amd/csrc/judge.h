// What a circuit plan's per-trial kernels share across files: the judge of a sector's correction (circuit.hip judges it against the sampled truth,
// events.hip hands the prediction back) and the unpacker's view of a sector (events.hip).
// Device header: only what can reach a kernel's instruction stream (device functions and kernel argument structs); prototypes live in launchers.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

// per trial (32 lanes): decoded logical action H_logical @ det (engine.py:99,119), and whether the correction reproduces the syndrome
struct JudgeSector {
    int m, n;
    const int32_t *indptr, *indices, *colptr, *rowidx;
    const uint64_t *logmask;
    const int8_t *synd, *det;
    const uint8_t *conv;
    const int32_t *iters;
    const unsigned long long *true_log;
};

// returns the XOR of the logical masks of the correction's ones (bit r = logical row r), the same value in all 32 lanes
__device__ __forceinline__ uint64_t judge_sector(const JudgeSector &S, int64_t b, int lane, bool &nz, bool &bad) {
    const int8_t *d = S.det + b * S.n, *s = S.synd + b * S.m;
    uint64_t lm = 0;
    for (int j = lane; j < S.n; j += 32) if (d[j] & 1) lm ^= S.logmask[j];
    int bd = 0, z = 0;
    for (int i = lane; i < S.m; i += 32) {
        int p = 0;
        for (int k = S.indptr[i]; k < S.indptr[i + 1]; k++) p ^= d[S.indices[k]];
        bd |= ((p ^ s[i]) & 1);
        z |= (s[i] & 1);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) { lm ^= __shfl_xor(lm, off, 32); bd |= __shfl_xor(bd, off, 32); z |= __shfl_xor(z, off, 32); }
    nz = z != 0;
    bad = bd != 0;
    return lm;
}

// The same verdicts from the ONES of the correction: a decoded error has ~100 ones among ~8 800 columns, so H @ det is ~600 parity flips (the columns' rows, CSC) into a bit
// set of the trial in LDS instead of the ~31 000 byte gathers per sector of the row-wise form above (1.15 ms per 16 384-trial batch of config 5); the scan of det -- aligned
// dwords, the ragged head and tail as bytes -- is what is left.  `par`: m bits of LDS owned by the trial's 32 lanes.
__device__ __forceinline__ uint64_t judge_sector_sparse(const JudgeSector &S, int64_t b, int lane, uint32_t *par, bool &nz, bool &bad) {
    const uint8_t *d = reinterpret_cast<const uint8_t *>(S.det) + b * S.n;
    const int8_t *s = S.synd + b * S.m;
    const int mwords = (S.m + 31) >> 5;
    for (int w = lane; w < mwords; w += 32) par[w] = 0u;
    __builtin_amdgcn_wave_barrier();
    uint64_t lm = 0;
    auto one = [&](int j) {
        lm ^= S.logmask[j];
        for (int e = S.colptr[j]; e < S.colptr[j + 1]; e++) { const int r = S.rowidx[e]; atomicXor(&par[r >> 5], 1u << (r & 31)); }
    };
    const int head = (int)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3), nhead = head < S.n ? head : S.n;
    if (lane < nhead && (d[lane] & 1)) one(lane);
    const int nw = (S.n - nhead) >> 2;
    const uint32_t *dw = reinterpret_cast<const uint32_t *>(d + nhead);
    for (int w = lane; w < nw; w += 32) {
        uint32_t x = dw[w] & 0x01010101u;
        while (x) {                                                        // (rare: a correction is sparse)
            const int byte = (__builtin_ctz(x)) >> 3;
            x &= x - 1u;
            one(nhead + 4 * w + byte);
        }
    }
    const int tail0 = nhead + 4 * nw;
    if (tail0 + lane < S.n && (d[tail0 + lane] & 1)) one(tail0 + lane);
    __builtin_amdgcn_wave_barrier();
    int bd = 0, z = 0;
    for (int i = lane; i < S.m; i += 32) {
        const int si = s[i] & 1;
        bd |= (int)((par[i >> 5] >> (i & 31)) & 1u) ^ si;
        z |= si;
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) { lm ^= __shfl_xor(lm, off, 32); bd |= __shfl_xor(bd, off, 32); z |= __shfl_xor(z, off, 32); }
    nz = z != 0;
    bad = bd != 0;
    return lm;
}

// one sector as the event unpacker sees it (events.hip): row r of syn[shot][nsyn] reads record bit tab[r] (-1: the row is constant 0), or bit base + r
// when tab is NULL (the sector's rows are a contiguous run of bits)
struct EventsSector { int nsyn, base; const int32_t *tab; int8_t *syn; };

}  // namespace qldpc
