// What the samplers of a circuit plan share: the signature table of a sector, where a batch's samples go, the frame every sampler kernel runs its
// draws in, the XOR of one entry into a sector's bit set, and the Pauli component a faulty circuit location draws.  Included by circuit.hip
// (independent draws), dem.hip, fixed_weight.hip, erasure.hip, noise_model.hip and soft.hip.
// Device header (see mc_common.h): everything here can reach a kernel's instruction stream.
#pragma once
#include "mc_common.h"

#include <algorithm>

namespace qldpc {

enum { C_OP_CNOT = 1, C_OP_PREP_X = 2, C_OP_PREP_Z = 3, C_OP_MEAS_X = 4, C_OP_MEAS_Z = 5, C_OP_IDLE = 6 };   // noise/constants.py:8-14

struct SigTab {           // signatures of one sector (device pointers); circuit: entry e = 2 * location + slot; detector error model: entry e = mechanism
    const int32_t *ptr;   // [entries + 1]
    const uint16_t *idx;  // detector indices
    const uint64_t *log;  // logical flips, bit r = logical row r
};

// Where a sampler kernel writes a batch (device pointers), built once per launch and passed by value.  two = 0: a one-sector detector error model,
// nothing of sector 1 is read or written.  fail_counts (may be NULL): the batch's BP failure counters, [0] Z and [4] X, which the sampler zeroes so
// that a batch needs no memset launch.
struct SampleOut {
    int n0, n1, two;                       // detectors of sector 0 / 1
    int8_t *syn0, *syn1;                   // int8[B][n]
    unsigned long long *true0, *true1;     // the logical flips of a trial, bit r = logical row r
    int32_t *fail_counts;
};

// The launch shape every sampler shares: the LDS words of the frame below and one workgroup of 256 per trial, grid-stride above 4096 trials.  A
// sampler that keeps more in LDS adds its words behind these.
struct SampleShape { size_t words; unsigned grid; };
inline SampleShape sample_shape(int n0, int n1, bool two, int64_t B) {
    const int w0 = (n0 + 31) / 32, w1 = two ? (n1 + 31) / 32 : 0;
    return {(size_t)((w0 + w1 + 1) & ~1) + 4, (unsigned)std::min<int64_t>(B, 256 * 16)};      // at most 65535 detectors per sector: 16 KiB + 16 B
}

// component masks: bit0 = X on slot 0, bit1 = X on slot 1, bit2 = Z on slot 0, bit3 = Z on slot 1
static __constant__ uint8_t c_cnot_comp[15] = {1, 5, 4, 2, 10, 8, 3, 15, 12, 11, 7, 13, 14, 9, 6};   // order of noise/kernels.py:283-343
static __constant__ uint8_t c_idle_comp[3] = {1, 5, 4};                                               // X, Y, Z (kernels.py:263-268)

// A workgroup's LDS (uint32 words): both sectors' detector bit sets (b1 right behind b0), a pad to an even word count, the two 64-bit logical
// accumulators, then whatever else the sampler keeps (`more`).
struct SampleLds { uint32_t *b0, *b1; unsigned long long *lacc; uint32_t *more; int nbits; };

// TWO: the kernel always has two sectors (every circuit sampler); otherwise O.two decides, the same for every lane.
template <bool TWO>
__device__ __forceinline__ SampleLds sample_carve(uint32_t *sm, const SampleOut &O) {
    const int w0 = (O.n0 + 31) >> 5, w1 = (TWO || O.two) ? (O.n1 + 31) >> 5 : 0, pad = (w0 + w1 + 1) & ~1;
    return {sm, sm + w0, reinterpret_cast<unsigned long long *>(sm + pad), sm + pad + 4, w0 + w1};
}

// The frame of every sampler kernel: one workgroup per trial (grid-stride).  Per trial it zeroes the bit sets, the accumulators and the first
// nrec words of `more`, runs draw(t, g, L) between two barriers -- g = trial_begin + t; the draw XORs into L with atomics and may hold barriers
// of its own, which every lane must reach -- then unpacks the bit sets into the int8 syndromes, stores the logical flips and, where rec is given,
// the nrec words as trial t's row of rec.  The closing barrier keeps the next trial's zeroing behind these reads.
template <bool TWO, class Draw>
__device__ __forceinline__ void sample_trials(uint32_t *sm, int64_t B, int64_t trial_begin, const SampleOut &O, int nrec, uint32_t *rec, Draw draw) {
    if (O.fail_counts && blockIdx.x == 0 && threadIdx.x < 8) O.fail_counts[threadIdx.x] = 0;
    const SampleLds L = sample_carve<TWO>(sm, O);
    const bool two = TWO || O.two;
    for (int64_t t = blockIdx.x; t < B; t += gridDim.x) {
        for (int w = threadIdx.x; w < L.nbits; w += blockDim.x) sm[w] = 0;
        for (int w = threadIdx.x; w < nrec; w += blockDim.x) L.more[w] = 0;
        if (threadIdx.x < 2) L.lacc[threadIdx.x] = 0ull;
        __syncthreads();
        draw(t, (uint64_t)(trial_begin + t), L);
        __syncthreads();
        for (int i = threadIdx.x; i < O.n0; i += blockDim.x) O.syn0[t * O.n0 + i] = (L.b0[i >> 5] >> (i & 31)) & 1;
        if (two)
            for (int i = threadIdx.x; i < O.n1; i += blockDim.x) O.syn1[t * O.n1 + i] = (L.b1[i >> 5] >> (i & 31)) & 1;
        if (rec)
            for (int w = threadIdx.x; w < nrec; w += blockDim.x) rec[t * nrec + w] = L.more[w];
        if (threadIdx.x == 0) { O.true0[t] = L.lacc[0]; if (two) O.true1[t] = L.lacc[1]; }
        __syncthreads();
    }
}

__device__ __forceinline__ void xor_signature(const SigTab &T, int e, uint32_t *bits, unsigned long long *logacc) {
    for (int k = T.ptr[e]; k < T.ptr[e + 1]; k++) { const int d = T.idx[k]; atomicXor(&bits[d >> 5], 1u << (d & 31)); }
    const unsigned long long lm = T.log[e];
    if (lm) atomicXor(logacc, lm);
}

// The Pauli components (mask above) of faulty location l of type ty in trial g: fixed for measurements and preparations, else word 0 of
// Philox(g, l, domain 2) mod 3 (IDLE) or mod 15 (CNOT).
__device__ __forceinline__ int fault_components(int ty, uint64_t g, int l, uint32_t seed_lo, uint32_t seed_hi) {
    if (ty == C_OP_MEAS_X || ty == C_OP_PREP_X) return 4;            // Z flip (kernels.py:211-216, 241-246)
    if (ty == C_OP_MEAS_Z || ty == C_OP_PREP_Z) return 1;            // X flip (kernels.py:224-229, 253-258)
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)l, 2u, seed_lo, seed_hi, r);
    return (ty == C_OP_IDLE) ? c_idle_comp[r[0] % 3u] : c_cnot_comp[r[0] % 15u];
}

// The components `comp` (mask above) of circuit location l: their signatures into both sectors' bit sets (bz / bx) and logical accumulators
// (lacc[0] Z, lacc[1] X).
__device__ __forceinline__ void fire_components(const SigTab &Z, const SigTab &X, int comp, int l, uint32_t *bz, uint32_t *bx, unsigned long long *lacc) {
    if (comp & 1) xor_signature(X, 2 * l, bx, &lacc[1]);
    if (comp & 2) xor_signature(X, 2 * l + 1, bx, &lacc[1]);
    if (comp & 4) xor_signature(Z, 2 * l, bz, &lacc[0]);
    if (comp & 8) xor_signature(Z, 2 * l + 1, bz, &lacc[0]);
}

// A faulty circuit location: the components it draws, fired.
__device__ __forceinline__ void fire_location(const SigTab &Z, const SigTab &X, const uint8_t *__restrict__ loc_type, uint64_t g, int l, uint32_t seed_lo,
                                              uint32_t seed_hi, uint32_t *bz, uint32_t *bx, unsigned long long *lacc) {
    fire_components(Z, X, fault_components(loc_type[l], g, l, seed_lo, seed_hi), l, bz, bx, lacc);
}

}  // namespace qldpc
