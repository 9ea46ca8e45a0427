// What the samplers of a circuit plan share on the device: the signature table of a sector, the XOR of one entry into the sector's bit set, and the
// Pauli component a faulty circuit location draws.  Included by circuit.hip (independent draws) and fixed_weight.hip (exactly w faults).
// Device header (see mc_common.h): everything here can reach a kernel's instruction stream.
#pragma once
#include "mc_common.h"

namespace qldpc {

enum { C_OP_CNOT = 1, C_OP_PREP_X = 2, C_OP_PREP_Z = 3, C_OP_MEAS_X = 4, C_OP_MEAS_Z = 5, C_OP_IDLE = 6 };   // noise/constants.py:8-14

struct SigTab {           // signatures of one sector; circuit: entry e = 2 * location + slot; detector error model: entry e = mechanism (DemTab's layout)
    const int32_t *ptr;   // [entries + 1]
    const uint16_t *idx;  // detector indices
    const uint64_t *log;  // logical flips, bit r = logical row r
};

// component masks: bit0 = X on slot 0, bit1 = X on slot 1, bit2 = Z on slot 0, bit3 = Z on slot 1
static __constant__ uint8_t c_cnot_comp[15] = {1, 5, 4, 2, 10, 8, 3, 15, 12, 11, 7, 13, 14, 9, 6};   // order of noise/kernels.py:283-343
static __constant__ uint8_t c_idle_comp[3] = {1, 5, 4};                                               // X, Y, Z (kernels.py:263-268)

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

// A faulty circuit location: its components' signatures into both sectors' bit sets (bz / bx) and logical accumulators (lacc[0] Z, lacc[1] X).
__device__ __forceinline__ void fire_location(const SigTab &Z, const SigTab &X, const uint8_t *__restrict__ loc_type, uint64_t g, int l, uint32_t seed_lo,
                                              uint32_t seed_hi, uint32_t *bz, uint32_t *bx, unsigned long long *lacc) {
    const int comp = fault_components(loc_type[l], g, l, seed_lo, seed_hi);
    if (comp & 1) xor_signature(X, 2 * l, bx, &lacc[1]);
    if (comp & 2) xor_signature(X, 2 * l + 1, bx, &lacc[1]);
    if (comp & 4) xor_signature(Z, 2 * l, bz, &lacc[0]);
    if (comp & 8) xor_signature(Z, 2 * l + 1, bz, &lacc[0]);
}

}  // namespace qldpc
