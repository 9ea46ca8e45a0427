// Device helpers shared by the min-sum kernels.  All arithmetic is IEEE f64 in the reference's operand order.
// Device header: only what can reach a kernel's instruction stream (device functions, kernel argument structs shared between files, constants
// and macros kernel bodies name).  Prototypes and host-only structs live in launchers.h; tools/isa_mix.py RECORDED lists this file per kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace qldpc {

// Integer column weights of Relay-BP (relay_bp.hip) and OSD-CS (osd_cs.hip).
// q_j = floor(prior_j * 2^20 + 0.5) as int64, the product clamped to +-2^40 so that a sum over any column count fits
__host__ __device__ __forceinline__ long long relay_weight(double p) {
    double x = p * 1048576.0;
    if (x > 1099511627776.0) x = 1099511627776.0;
    if (x < -1099511627776.0) x = -1099511627776.0;
    return (long long)floor(x + 0.5);
}

// reference src/decoding/kernels.py:328-333: NaN -> 0, else clip to [-clip, clip]
__device__ __forceinline__ double clip_nan(double q, double clip) {
    if (q != q) return 0.0;
    if (q > clip) return clip;
    if (q < -clip) return -clip;
    return q;
}

// The reference evaluates  q_damped = damping * q_new + (1.0 - damping) * Q_old  even for damping == 1 (kernels.py:336).  Q_old of
// iteration 0 is the UNCLIPPED prior, so for a column whose prior is +-inf or NaN the product 0.0 * Q_old is NaN: every message into
// such a column's checks is NaN from iteration 1 on (NaN survives the second clip and 0.0 * NaN keeps it alive).  The kernels skip the
// damping arithmetic when damping == 1 (exact for finite Q_old) and reproduce this case explicitly: q = NaN where the prior is not finite.
__device__ __forceinline__ bool prior_not_finite(double p) { return !(fabs(p) < INFINITY); }

// reference src/decoding/kernels.py:339-342
__device__ __forceinline__ double clip_only(double q, double clip) {
    if (q > clip) return clip;
    if (q < -clip) return -clip;
    return q;
}

// The 24-byte compressed record of a check (minsum_wg.hip, minsum_layered.hip, bp_leg.h) is (alpha*min1, alpha*min2) and one word: bits 0-55 input signs, 56-62 argmin (127 = none), 63 total sign.
__device__ __forceinline__ int rec_argmin(unsigned long long w) { return (int)((w >> 56) & 127); }
__device__ __forceinline__ bool rec_total_sign(unsigned long long w) { return (w >> 63) & 1; }
__device__ __forceinline__ bool rec_sign_bit(unsigned long long w, int k) { return (w >> k) & 1; }
__device__ __forceinline__ unsigned long long rec_pack(unsigned long long negbits, int arg, bool sp) {
    return negbits | ((unsigned long long)arg << 56) | ((unsigned long long)sp << 63);
}
// the message the check sent to its position k
__device__ __forceinline__ double rec_message(double a1, double a2, unsigned long long w, int k) {
    const double mag = (k == (int)((w >> 56) & 127)) ? a2 : a1;
    return ((bool)((w >> 63) & 1) != (bool)((w >> k) & 1)) ? -mag : mag;
}

}  // namespace qldpc
