// OSD-CS: OSD with a combination sweep (Roffe et al. 2020, "Decoding across the quantum LDPC code landscape") after OSD-0, for matrices with
// m <= 1024 rows.  Semantics in include/qldpc_hip.h (qldpc_osdcs_batch); tests/osd_cs_model.py is the numpy model the kernel is held to.
//
// One workgroup per shot, as the free-pivot OSD-0 kernel (osd_gj.hip): U = T^T of the accumulated row transform T in LDS, row m all zero, row
// m + 1 the right-hand side b = s + H hard.  What differs:
//   * the sweep runs to rank(H): the single-flip candidates need the reduced column of EVERY non-pivot column against the final transform, so
//     the OSD-0 cut "residual gone" does not apply.  The whole column order is sorted up front.
//   * chunks of 64 columns: (A) their reduced columns r = XOR_{i in supp h} U[i] from the chunk's starting U, 16 lanes per column (lane = word);
//     (B) wave 0 walks the chunk's columns that have a one in an unused row (the others are dependent for good) in order, applies the pivots
//     already taken in this chunk (r ^= r[p_k] ? M_k : 0), and pivots on the first unused row with a one: M = r with bit p cleared;
//     (C) every row q of U (b included) takes the chunk's operations in order, U[q] ^= U[q][p_k] ? M_k : 0, 16 lanes per row.
//     Plain workgroup barriers between the phases: no spin waits.
//   * scoring.  With x0 the OSD-0 solution, sigma_k = 1 - 2 x0_k, q the quantised weights and pc(r) the pivot column of row r, the reduced
//     column r_j of a non-pivot column j is supported on pivot rows only, and
//         W(t = {j})    = W(x0) + sigma_j q_j + sum_{r in r_j} sigma_pc(r) q_pc(r)           ( = W(x0) + d_j )
//         W(t = {a, b}) = W(x0) + d_a + d_b - 2 sum_{r in r_a & r_b} sigma_pc(r) q_pc(r)
//     so no candidate needs an elimination of its own: U, the pivot map and x0 are enough.  The signed pivot weights sq[r] take the place of
//     the chunk's reduced columns in LDS; 16 lanes score one non-pivot column; the lambda columns the pairs need are kept in LDS.  The minimum
//     of (W, candidate index) is exact: int64 sums, and candidates are numbered 0 (OSD-0), 1 + sorted position (singles: the non-pivot columns
//     in the column order), n + 1 + lexicographic pair index (pairs) -- the same order as the candidate list of the header.
// A right-hand side outside the column space puts the shot on a list; the caller runs qldpc_osd0_batch's kernels on it behind this one.
#include "common.h"
#include "launchers.h"
#include "minsum_common.h"
#include "osd_common.h"
#include "osd_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace qldpc {

struct OsdCsArgs {
    int m, n, mw, rankH, cdeg, order;
    const uint16_t *col_rows;      // [n][cdeg] rows of every column, padded with m (the all-zero row of U)
    const int32_t *indptr, *indices;
    const int32_t *list, *count;
    const int8_t *synd; const double *llr; const int8_t *hard; const double *weights;
    int8_t *solution; int32_t *flips;
    uint16_t *ordws;               // [grid][n] the column order of the shot in flight
    unsigned long long *gsort;     // [grid][gsort_words] global sort scratch when the sort does not fit in LDS (else NULL)
    size_t gsort_words;
    int *queue;                    // next list entry (zeroed before the launch)
    int32_t *redo_list, *redo_count;
    int offUsed, offPc, offPr, offR, offTR, offPf, offMisc;
};

__device__ __forceinline__ unsigned long long cs_readlane64(unsigned long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long cs_shfl64(unsigned long long v, int src, int width) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, width);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, width);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ long long cs_shfl_xor64(long long v, int mask, int width) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(unsigned long long)v, mask, width);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), mask, width);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ bool cs_better(long long d1, int k1, long long d2, int k2) { return d1 < d2 || (d1 == d2 && k1 < k2); }

// (a, b) of pair index pi among the lam * (lam - 1) / 2 pairs a < b < lam in lexicographic order
__device__ __forceinline__ void cs_pair(int pi, int lam, int &a, int &b) {
    a = 0;
    while (pi >= lam - 1 - a) { pi -= lam - 1 - a; a++; }
    b = a + 1 + pi;
}

// sum of sq over the ones of x (word w of a reduced column)
__device__ __forceinline__ long long cs_bits_sum(unsigned long long x, const long long *sq, int w) {
    long long s = 0;
    while (x != 0ull) {
        const int b = __builtin_ctzll(x);
        x &= x - 1ull;
        s += sq[64 * w + b];
    }
    return s;
}

__global__ __launch_bounds__(1024) void osd_cs_kernel(OsdCsArgs P) {
    extern __shared__ unsigned char lds[];
    const int m = P.m, n = P.n, mw = P.mw, cd = P.cdeg, tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, g16 = tid >> 4, w16 = tid & 15, NG = T >> 4;
    const bool wmine = w16 < mw;                                             // this lane of its 16 holds a word of the row / column
    unsigned long long *U = reinterpret_cast<unsigned long long *>(lds);   // [m + 2][mw]
    unsigned long long *usedw = reinterpret_cast<unsigned long long *>(lds + P.offUsed);   // [16] rows that have pivoted
    uint16_t *pvcol = reinterpret_cast<uint16_t *>(lds + P.offPc);         // [m] column of pivot t
    uint16_t *pvrow = reinterpret_cast<uint16_t *>(lds + P.offPr);         // [m] row of pivot t
    unsigned long long *R = reinterpret_cast<unsigned long long *>(lds + P.offR);         // [64][mw] reduced columns of the chunk (sweep)
    long long *sq = reinterpret_cast<long long *>(lds + P.offR);                          // [m] sigma q of the pivot column of row r (scoring)
    unsigned long long *TR = reinterpret_cast<unsigned long long *>(lds + P.offTR);       // [order][mw] reduced columns of T[0 .. order)
    uint32_t *pflag = reinterpret_cast<uint32_t *>(lds + P.offPf);         // [(n + 31) / 32] pivot columns
    long long *tdel = reinterpret_cast<long long *>(lds + P.offMisc);      // [64] d of T[a]
    long long *wbest = tdel + kCsChunk;                                    // [16] per-wave minimum
    unsigned long long *WR = reinterpret_cast<unsigned long long *>(wbest + 16);          // [16] the winner's combination on the pivot rows
    int *ib = reinterpret_cast<int *>(WR + 16);                            // [0] item, [1] pivots of the chunk, [2] pivots so far, [5] lambda, [6] b outside, [7] winner
    int *pk = ib + 16;                                                     // [64] chunk pivots: row | chunk position << 16
    int *tcol = pk + kCsChunk;                                             // [64] T[a]
    int *wkey = tcol + kCsChunk;                                           // [16]
    uint16_t *sidx = reinterpret_cast<uint16_t *>(wkey + 16);              // [64] columns of the chunk
    uint16_t *ordw = P.ordws + (size_t)blockIdx.x * n;
    const int brow = m + 1;

    const int total = *P.count;
    for (;;) {
        if (tid == 0) ib[0] = atomicAdd(P.queue, 1);
        __syncthreads();
        const int item = ib[0];
        if (item >= total) break;
        const int64_t shot = P.list[item];
        const double *llr = P.llr + shot * n;
        const int8_t *hard = P.hard + shot * n, *synd = P.synd + shot * m;
        int8_t *sol = P.solution + shot * n;
        // ---- column order: ascending |llr|, NaN as +inf, ties by index (the order of qldpc_osd0_batch) ----
        if (!P.gsort) {
            unsigned long long *keys = reinterpret_cast<unsigned long long *>(lds);
            uint16_t *pa = reinterpret_cast<uint16_t *>(lds + (size_t)n * 8), *pb = pa + n;
            unsigned *cnt = reinterpret_cast<unsigned *>(lds + (((size_t)n * 12 + 15) & ~(size_t)15));
            for (int j = tid; j < n; j += T) { keys[j] = osd_key(llr[j]); pa[j] = (uint16_t)j; }
            osd_radix_passes<0>(keys, n, pa, pb, cnt, ordw);                 // (the register-cached passes of osd_radix_sort would spill here)
        } else {
            for (int j = tid; j < n; j += T) ordw[j] = (uint16_t)j;
            __threadfence_block();
            __syncthreads();
            unsigned long long *gk = P.gsort + (size_t)blockIdx.x * P.gsort_words;
            uint16_t *gpa = reinterpret_cast<uint16_t *>(gk + n), *gpb = gpa + n;
            osd_sort_rest(llr, n, 0, gk, gpa, gpb, reinterpret_cast<unsigned *>(gk + n + (n + 3) / 2), ordw);
        }
        __threadfence_block();
        __syncthreads();
        // ---- init: T = I, b = s + H hard ----
        for (int t = tid; t < (m + 2) * mw; t += T) U[t] = 0ull;
        if (tid < 16) usedw[tid] = (tid >= mw) ? ~0ull : ((tid == mw - 1 && (m & 63)) ? (~0ull << (m & 63)) : 0ull);
        for (int t = tid; t < (n + 31) / 32; t += T) pflag[t] = 0u;
        if (tid == 0) ib[2] = 0;
        __syncthreads();
        for (int r = tid; r < m; r += T) {
            U[r * mw + (r >> 6)] = 1ull << (r & 63);
            int sy = synd[r] & 1;
            for (int e = P.indptr[r]; e < P.indptr[r + 1]; e++) sy ^= hard[P.indices[e]] & 1;
            if (sy) atomicOr(&U[brow * mw + (r >> 6)], 1ull << (r & 63));
        }
        __syncthreads();
        // ---- the sweep, to rank(H) ----
        int row = 0;
        for (int base = 0; base < n && row < P.rankH; base += kCsChunk) {
            const int L = min(kCsChunk, n - base);
            // (A) reduced columns of the chunk from its starting U
            for (int c = g16; c < L; c += NG) {
                const int j = ordw[base + c];
                if (w16 == 0) sidx[c] = (uint16_t)j;
                if (wmine) {
                    const uint16_t *cr = P.col_rows + (size_t)j * cd;
                    unsigned long long acc = 0ull;
                    for (int d = 0; d < cd; d++) acc ^= U[(int)cr[d] * mw + w16];
                    R[c * mw + w16] = acc;
                }
            }
            __syncthreads();
            // (B) wave 0: the chunk's pivots in column order (lane w < mw holds word w)
            if (tid < 64) {
                const bool wl = lane < mw;
                const unsigned long long used0 = wl ? usedw[lane] : ~0ull;   // rows that had pivoted when the chunk began
                unsigned long long used = used0;
                int np = 0, rw = row, pkr = 0;                               // lane k holds chunk pivot k (row | position << 16)
                for (int c = 0; c < L && rw < P.rankH; c++) {
                    unsigned long long v = wl ? R[c * mw + lane] : 0ull;
                    if (__ballot((v & ~used0) != 0ull) == 0ull) continue;   // in the span of the pivots before the chunk: dependent for good
                    for (int k = 0; k < np; k++) {
                        const int e = __builtin_amdgcn_readlane(pkr, k);
                        const int p = e & 0xFFFF;
                        const unsigned long long mk = wl ? R[(e >> 16) * mw + lane] : 0ull;     // (loaded whatever the test says: off the chain)
                        const unsigned long long vw = cs_readlane64(v, p >> 6);
                        if ((vw >> (p & 63)) & 1ull) v ^= mk;
                    }
                    const unsigned long long z = v & ~used;
                    const unsigned long long bal = __ballot(z != 0ull);
                    if (bal == 0ull) continue;                               // dependent on the pivots so far
                    const int f = __builtin_ctzll(bal);
                    const unsigned long long zf = cs_readlane64(z, f);
                    const int p = 64 * f + __builtin_ctzll(zf);
                    if (lane == f) { v &= ~(1ull << (p & 63)); used |= 1ull << (p & 63); }
                    if (wl) R[c * mw + lane] = v;                            // the operation's mask M = r with the pivot bit cleared
                    if (lane == np) pkr = p | (c << 16);
                    if (lane == 0) { pvcol[rw] = sidx[c]; pvrow[rw] = (uint16_t)p; }
                    np++; rw++;
                }
                if (wl) usedw[lane] = used;
                if (lane < np) pk[lane] = pkr;
                if (lane == 0) { ib[1] = np; ib[2] = rw; }
            }
            __syncthreads();
            const int np = ib[1];
            row = ib[2];
            // (C) every row of U (b included) takes the chunk's operations in order
            if (np > 0) {
                const int pkl = (lane < np) ? pk[lane] : 0;                  // lane k holds chunk pivot k: a scalar per operation below
                for (int q = g16; q < m + 2; q += NG) {
                    unsigned long long v = wmine ? U[q * mw + w16] : 0ull;
                    for (int k = 0; k < np; k++) {
                        const int e = __builtin_amdgcn_readlane(pkl, k);
                        const int p = e & 0xFFFF;
                        const unsigned long long mk = wmine ? R[(e >> 16) * mw + w16] : 0ull;
                        const unsigned long long vw = cs_shfl64(v, p >> 6, 16);
                        if ((vw >> (p & 63)) & 1ull) v ^= mk;
                    }
                    if (wmine) U[q * mw + w16] = v;
                }
            }
            __syncthreads();
        }
        // ---- b outside the column space: the caller's OSD-0 answers the shot ----
        if (tid < 64) {
            const unsigned long long z = (lane < mw) ? (U[brow * mw + lane] & ~usedw[lane]) : 0ull;
            const bool bad = __ballot(z != 0ull) != 0ull;
            if (lane == 0) ib[6] = bad ? 1 : 0;
        }
        __syncthreads();
        if (ib[6]) {
            if (tid == 0) {
                P.redo_list[atomicAdd(P.redo_count, 1)] = (int32_t)shot;
                P.flips[2 * shot] = -1; P.flips[2 * shot + 1] = -1;
            }
            __syncthreads();
            continue;
        }
        // ---- scoring: sq[r] = sigma q of the pivot column of row r (0 for rows without a pivot), pivot flags ----
        for (int r = tid; r < m; r += T) sq[r] = 0;
        __syncthreads();
        for (int t = tid; t < row; t += T) {
            const int j = pvcol[t], r = pvrow[t];
            const int x0 = ((int)hard[j] ^ (int)((U[brow * mw + (r >> 6)] >> (r & 63)) & 1ull)) & 1;
            const long long q = relay_weight(P.weights[j]);
            sq[r] = x0 ? -q : q;
            atomicOr(&pflag[j >> 5], 1u << (j & 31));
        }
        __syncthreads();
        // T [0 .. lambda): the first non-pivot columns of the order
        if (tid < 64) {
            const int lam = P.order;
            int got = 0;
            for (int p0 = 0; p0 < n && got < lam; p0 += 64) {
                const int pos = p0 + lane;
                const int j = pos < n ? (int)ordw[pos] : 0;
                const bool nonpiv = pos < n && !((pflag[j >> 5] >> (j & 31)) & 1u);
                const unsigned long long bal = __ballot(nonpiv);
                const int rk = got + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                if (nonpiv && rk < lam) tcol[rk] = j;
                got += __builtin_popcountll(bal);
            }
            if (lane == 0) ib[5] = min(got, lam);
        }
        __syncthreads();
        const int lamE = ib[5];
        // d of T[a], and r_{T[a]} for the pairs
        for (int a = g16; a < lamE; a += NG) {
            const int j = tcol[a];
            unsigned long long acc = 0ull;
            if (wmine) {
                const uint16_t *cr = P.col_rows + (size_t)j * cd;
                for (int d = 0; d < cd; d++) acc ^= U[(int)cr[d] * mw + w16];
                TR[a * mw + w16] = acc;
            }
            long long s = cs_bits_sum(acc, sq, w16);
            for (int o = 8; o > 0; o >>= 1) s += cs_shfl_xor64(s, o, 16);
            const long long q = relay_weight(P.weights[j]);
            if (w16 == 0) tdel[a] = s + ((hard[j] & 1) ? -q : q);
        }
        // singles: every non-pivot column, 16 lanes each
        long long bd = 0;
        int bk = 0;                                                          // candidate 0: OSD-0
        for (int pos = g16; pos < n; pos += NG) {
            const int j = ordw[pos];
            if ((pflag[j >> 5] >> (j & 31)) & 1u) continue;                  // (the same for the 16 lanes)
            unsigned long long acc = 0ull;
            if (wmine) {
                const uint16_t *cr = P.col_rows + (size_t)j * cd;
                for (int d = 0; d < cd; d++) acc ^= U[(int)cr[d] * mw + w16];
            }
            long long s = cs_bits_sum(acc, sq, w16);
            for (int o = 8; o > 0; o >>= 1) s += cs_shfl_xor64(s, o, 16);
            const long long q = relay_weight(P.weights[j]);
            const long long dj = s + ((hard[j] & 1) ? -q : q);
            if (cs_better(dj, pos + 1, bd, bk)) { bd = dj; bk = pos + 1; }
        }
        __syncthreads();                                                     // TR / tdel complete
        // pairs {T[a], T[b]}, a < b < lambda
        const int npairs = lamE * (lamE - 1) / 2;
        for (int pi = tid; pi < npairs; pi += T) {
            int a, b;
            cs_pair(pi, lamE, a, b);
            long long s2 = 0;
            for (int w = 0; w < mw; w++) s2 += cs_bits_sum(TR[a * mw + w] & TR[b * mw + w], sq, w);
            const long long dp = tdel[a] + tdel[b] - 2 * s2;
            if (cs_better(dp, n + 1 + pi, bd, bk)) { bd = dp; bk = n + 1 + pi; }
        }
        // exact (d, candidate) minimum over the workgroup
        for (int o = 32; o > 0; o >>= 1) {
            const long long od = cs_shfl_xor64(bd, o, 64);
            const int ok = __shfl_xor(bk, o, 64);
            if (cs_better(od, ok, bd, bk)) { bd = od; bk = ok; }
        }
        if (lane == 0) { wbest[tid >> 6] = bd; wkey[tid >> 6] = bk; }
        __syncthreads();
        if (tid == 0) {
            long long d = wbest[0];
            int k = wkey[0];
            for (int v = 1; v < (T >> 6); v++) if (cs_better(wbest[v], wkey[v], d, k)) { d = wbest[v]; k = wkey[v]; }
            ib[7] = k;
        }
        __syncthreads();
        // ---- the winner: its columns of T and its combination on the pivot rows ----
        const int key = ib[7];
        int f0 = -1, f1 = -1;
        if (key == 0) {
            if (tid < 16) WR[tid] = 0ull;
        } else if (key <= n) {
            f0 = ordw[key - 1];
            if (tid < 16) {
                unsigned long long acc = 0ull;
                if (tid < mw) {
                    const uint16_t *cr = P.col_rows + (size_t)f0 * cd;
                    for (int d = 0; d < cd; d++) acc ^= U[(int)cr[d] * mw + tid];
                }
                WR[tid] = acc;
            }
        } else {
            int a, b;
            cs_pair(key - n - 1, lamE, a, b);
            f0 = tcol[a]; f1 = tcol[b];
            if (tid < 16) WR[tid] = (tid < mw) ? (TR[a * mw + tid] ^ TR[b * mw + tid]) : 0ull;
        }
        __syncthreads();
        // ---- x = hard + c: non-pivot columns keep hard unless flipped; pivot column of row r: hard ^ b[r] ^ WR[r] ----
        for (int j = tid; j < n; j += T) {
            if ((pflag[j >> 5] >> (j & 31)) & 1u) continue;
            if (j == f0 || j == f1) sol[j] = (int8_t)((hard[j] ^ 1) & 1);
            else if (sol != hard) sol[j] = hard[j];
        }
        for (int t = tid; t < row; t += T) {
            const int j = pvcol[t], r = pvrow[t];
            const int bit = (int)(((U[brow * mw + (r >> 6)] ^ WR[r >> 6]) >> (r & 63)) & 1ull);
            sol[j] = (int8_t)((hard[j] ^ bit) & 1);
        }
        if (tid == 0) { P.flips[2 * shot] = f0; P.flips[2 * shot + 1] = f1; }
        __syncthreads();
    }
}

// LDS layout (osd_cs_layout, osd_plan.h); gsort = true when the column sort has to run in global memory (it does not fit beside the rest in LDS)
static int osdcs_layout(const qldpc_graph *g, int order, OsdCsArgs &P, size_t &lds, bool &gsort) {
    const int m = g->m, n = g->n;
    P.m = m; P.n = n; P.mw = (m + 63) / 64; P.cdeg = std::max(g->max_col_deg, 1); P.order = order;
    lds = osd_cs_layout(m, n, order, P, gsort);
    if (lds != 0) return QLDPC_OK;
    // (no shape reaches this: with the sort in global memory the layout is at most 162 192 bytes at m = 1024, n = 65535, order 64, and a seeded sweep of
    //  m <= 1024, n <= 65535, every order -- tests/test_osd_cs_domain_cpu.py -- never came here.  Kept as the rule has it.)
    set_error("OSD-CS: %d x %d matrix needs more LDS than the 160 KiB of a workgroup", m, n);
    return QLDPC_ERR_UNSUPPORTED;
}

int osdcs_supported(const qldpc_graph *g) {
    if (g->m > 1024 || g->n > 65535) {
        set_error("OSD-CS supports m <= 1024 and n <= 65535 (this matrix is %d x %d)", g->m, g->n);
        return QLDPC_ERR_UNSUPPORTED;
    }
    OsdCsArgs P;
    size_t lds = 0;
    bool gsort = false;
    return osdcs_layout(g, kCsMaxOrder, P, lds, gsort);
}

// callers hold g->mu.  OSD-CS on the shots listed in d_list [0 .. *d_count); the shots whose right-hand side lies outside the column space get
// qldpc_osd0_batch's answer from the OSD-0 kernels, behind this launch on the same stream.
int osdcs_listed_launch(const qldpc_graph *g, const int32_t *d_list, const int32_t *d_count, int64_t max_listed, const int8_t *d_synd,
                        const double *d_llr, const int8_t *d_hard, const double *d_weights, int order, int8_t *d_solution, int32_t *d_flips,
                        hipStream_t stream) {
    if (g->m == 0 || g->n == 0 || max_listed == 0) return QLDPC_OK;
    int rc = osdcs_supported(g);
    if (rc != QLDPC_OK) return rc;
    OsdCsArgs P;
    size_t lds = 0;
    bool gsort = false;
    if ((rc = osdcs_layout(g, order, P, lds, gsort)) != QLDPC_OK) return rc;
    if ((rc = ensure_col_rows(g)) != QLDPC_OK) return rc;
    if (g->gf2_rank < 0) g->gf2_rank = host_gf2_rank(g);
    P.rankH = g->gf2_rank;
    const int grid = (int)std::min<int64_t>(512, max_listed);
    if ((rc = g->ws_acquire(stream)) != QLDPC_OK) return rc;
    auto launch = [&]() -> int {
        const size_t ord_bytes = (size_t)round_up((int64_t)grid * g->n * 2 + 64, 16);
        P.gsort_words = gsort ? (size_t)g->n + (size_t)(g->n + 3) / 2 + (256 * 16 + 64) / 2 + 8 : 0;
        int rcl = g->ws_misc.ensure(ord_bytes + (size_t)grid * P.gsort_words * 8);
        if (rcl != QLDPC_OK) return rcl;
        P.ordws = g->ws_misc.as<uint16_t>();
        P.gsort = gsort ? reinterpret_cast<unsigned long long *>(g->ws_misc.as<unsigned char>() + ord_bytes) : nullptr;
        if ((rcl = g->ws_cs.ensure((size_t)(max_listed + 4) * 4 + 16)) != QLDPC_OK) return rcl;
        if ((rcl = g->ws_queue.ensure(16)) != QLDPC_OK) return rcl;
        P.queue = g->ws_queue.as<int>();
        P.redo_count = g->ws_cs.as<int32_t>(); P.redo_list = P.redo_count + 4;
        QLDPC_HIP_TRY(hipMemsetAsync(P.queue, 0, 4, stream));
        QLDPC_HIP_TRY(hipMemsetAsync(P.redo_count, 0, 4, stream));
        P.col_rows = g->d_col_rows; P.indptr = g->d_indptr; P.indices = g->d_indices;
        P.list = d_list; P.count = d_count; P.synd = d_synd; P.llr = d_llr; P.hard = d_hard; P.weights = d_weights;
        P.solution = d_solution; P.flips = d_flips;
        if ((rcl = ensure_max_lds(g->device, reinterpret_cast<const void *>(osd_cs_kernel), kOsdLdsMax)) != QLDPC_OK) return rcl;
        hipLaunchKernelGGL(osd_cs_kernel, dim3(grid), dim3(osd_wide_block(g->m)), lds, stream, P);
        QLDPC_HIP_TRY(hipGetLastError());
        return QLDPC_OK;
    };
    rc = launch();
    const int rel = g->ws_release(stream);
    if (rc != QLDPC_OK) return rc;
    if (rel != QLDPC_OK) return rel;
    // the shots the kernel listed: OSD-0 (g->mu is held throughout, so nobody else enqueues on the workspaces in between)
    return osd0_listed_launch(g, P.redo_list, P.redo_count, max_listed, d_synd, d_llr, d_hard, nullptr, d_solution, 0, stream);
}

int osdcs_check_order(int order) {
    QLDPC_REQUIRE(order >= 0 && order <= kCsMaxOrder, "OSD-CS order %d outside 0..%d", order, kCsMaxOrder);
    return QLDPC_OK;
}

}  // namespace qldpc

using namespace qldpc;

QLDPC_EXPORT int qldpc_osdcs_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard,
                                       const double *d_weights, int order, const int32_t *d_select, const int32_t *d_select_count,
                                       int8_t *d_solution, int32_t *d_flips, void *stream) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "batch out of range");
    QLDPC_REQUIRE((d_select == nullptr) == (d_select_count == nullptr), "d_select and d_select_count go together");
    int rc = osdcs_check_order(order);
    if (rc != QLDPC_OK) return rc;
    if ((rc = osdcs_supported(g)) != QLDPC_OK) return rc;
    if (B == 0 || g->n == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_llr && d_hard && d_weights && d_solution && d_flips && (d_syndromes || g->m == 0), "NULL buffer");
    QLDPC_USE_DEVICE(g->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->m == 0) { set_error("OSD-CS on device pointers needs a matrix with rows"); return QLDPC_ERR_UNSUPPORTED; }
    if (!d_select) {
        if ((rc = g->ws_acquire(s)) != QLDPC_OK) return rc;
        if ((rc = g->ws_list.ensure((size_t)B * 4 + 16)) != QLDPC_OK) { (void)g->ws_release(s); return rc; }
        int32_t *cnt = g->ws_list.as<int32_t>(), *list = cnt + 4;
        iota_list_launch(B, list, cnt, s);
        d_select = list; d_select_count = cnt;
    }
    return osdcs_listed_launch(g, d_select, d_select_count, B, d_syndromes, d_llr, d_hard, d_weights, order, d_solution, d_flips, s);
}

QLDPC_EXPORT int qldpc_osdcs_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard,
                                   const double *weights, int order, int8_t *solution, int32_t *flips) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "batch out of range");
    int rc = osdcs_check_order(order);
    if (rc != QLDPC_OK) return rc;
    if ((rc = osdcs_supported(g)) != QLDPC_OK) return rc;
    if (B == 0 || g->n == 0) return QLDPC_OK;
    QLDPC_REQUIRE(llr && hard && weights && solution && flips && (syndromes || g->m == 0), "NULL buffer");
    const size_t m = g->m, n = g->n;
    for (size_t j = 0; j < n; j++) QLDPC_REQUIRE(std::isfinite(weights[j]), "weights[%zu] is not finite", j);
    QLDPC_USE_DEVICE(g->device);
    if (m == 0) {                                                            // no checks: x = hard is the only candidate of least weight ... and OSD-0
        std::memcpy(solution, hard, (size_t)B * n);
        for (int64_t b = 0; b < 2 * B; b++) flips[b] = -1;
        return QLDPC_OK;
    }
    HostStage S;
    const auto ds = S.in(syndromes, B, m);
    const auto dl = S.in(llr, B, n);
    const auto dh = S.in(hard, B, n);
    const auto dw = S.in(weights, n);
    const auto dsol = S.out(solution, B, n);
    const auto dfl = S.out(flips, B, 2);
    const auto dlist = S.scratch<int32_t>(B), dcnt = S.scratch<int32_t>(4);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    iota_list_launch(B, S[dlist], S[dcnt], nullptr);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        rc = osdcs_listed_launch(g, S[dlist], S[dcnt], B, S[ds], S[dl], S[dh], S[dw], order, S[dsol], S[dfl], nullptr);
    }
    return rc != QLDPC_OK ? rc : S.finish("OSD-CS kernel", HostStage::kDevice);
}
