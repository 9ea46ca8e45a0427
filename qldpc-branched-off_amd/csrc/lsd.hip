// BP+LSD: localized statistics decoding (Hillmann, Berent, Quintavalle, Eisert, Wille, Roffe 2024) as a post-processor of the OSD hand-over.  Clusters
// grow around the unsatisfied checks of s + H hard, one (or bits_per_step) least reliable column per invalid cluster and round, until the residual of
// every cluster lies in the span of the columns added inside it; the correction is the one on the pivots among those columns.  Semantics in
// include/qldpc_hip.h (qldpc_lsd_batch); tests/lsd_model.py is the numpy model the kernel is held to, bit for bit in solution and info.
//
// One workgroup of 256 threads per shot, the listed shots handed out by a ticket counter.  What it keeps (LDS layout: lsd_plan.h):
//   * one shot-wide incremental elimination.  A row of H gets a local index when it joins R; U = T^T of the accumulated row transform T over the local rows,
//     a new row starting as a unit vector, row max_rows the reduced right-hand side T b.  The system is block diagonal by cluster, so one U serves all of
//     them, and its size is set by the row cap max_rows, not by m.
//   * clusters as labels: the label of a local row is the least local index of its cluster; adding a column relabels the clusters of its rows to the least
//     of their labels.  A cluster is invalid iff T b has a one in a row that has not pivoted and carries its label.
//   * adding a column (whole workgroup, the columns of a round in ascending key order): wave 0 XORs the U rows of the column's rows (lane = word), takes the
//     first unpivoted row with a one as the pivot p and keeps M = the reduced column with bit p cleared; then every row of U, T b included, takes
//     U[q] ^= U[q][p] ? M : 0 (a thread per word), and the labels merge.  A column without such a row is dependent on the ones before it: labels only.
//   * candidate search: per cluster row the least key among its columns outside A is cached and rescanned only once that column has been added; a round's
//     first pick is then a min-reduction of the cached columns over the labels (LDS atomics: the 64-bit key first, then the index among the rows that hold
//     it, so the minimum of (key, index) is exact and no lane order enters).  Picks 2 .. bits_per_step rescan the rows of the clusters still picking for
//     the least key above the cluster's previous pick.
//   * the columns of a round are sorted by rank counting, in LDS up to 128 of them and in the workgroup's global scratch beyond.
//   * a round is a chain of barriers and dependent loads, so the loads are kept apart from branches: wave 0 loads a column's rows in one step (lane = row)
//     and hands them round by shuffle, and the scan of a row has no branch between one key load and the next (profiles/r23_lsd.txt: 81 -> 55 ms).
// The order in which seed rows get their local indices (an LDS atomic) is the one thing that varies between runs; it moves pivot ROWS only.  Which
// columns pivot (independence of the columns before them in A), the validity of a cluster and the solution on the pivots do not depend on it.
// A shot that ends capped (flag 1) or without candidates (flag 2) is listed; the caller runs qldpc_osd0_batch's kernels on the list behind this kernel.
// On request (qldpc_lsd_stats_batch) an epilogue behind the solution turns the final labels into the statistics of the clusters: sums and maxima over
// sets, by LDS integer atomics, so the order of the local indices does not enter them either; tests/lsd_stats_model.py is their model.
#include "common.h"
#include "launchers.h"
#include "osd_common.h"
#include "lsd_plan.h"
#include "osd_plan.h"

#include <algorithm>
#include <cstring>

namespace qldpc {

struct LsdArgs {
    int m, n, cdeg, mr, w, bps;
    const uint16_t *col_rows;      // [n][cdeg] rows of every column, padded with m
    const int32_t *indptr, *indices;
    const int32_t *list, *count;
    const int8_t *synd; const double *llr; const int8_t *hard;
    int8_t *solution; int32_t *info;
    unsigned char *scratch;        // [grid][scratch_bytes]: keys u64[n], unsorted u16[n], sorted u16[n] of the round in flight
    size_t scratch_bytes;
    int *queue;                    // next list entry (zeroed before the launch)
    int32_t *redo_list, *redo_count;
    unsigned long long *counts;    // [3] shots that ended with flag 0 / 1 / 2, accumulated (may be NULL)
    const uint16_t *weight;        // [n] weight of a column in the cluster statistics (may be NULL: slots 4 .. 6 stay 0)
    unsigned long long *stats;     // [B][8] cluster statistics of a shot (may be NULL: no epilogue)
    LsdOffsets o;
};

constexpr int kLsdNone = 0xFFFF, kLsdUnset = 0xFFFE;      // "no column" / "not scanned yet" in the uint16 column tables (n < 65535); kLsdNone also "no local index"
// slots of the workgroup's int scratch
enum { kIbItem = 0, kIbRows, kIbAdded, kIbNoCand, kIbAny, kIbListed, kIbPicked, kIbRowsNew, kIbPivot, kIbTarget, kIbDegree };

__device__ __forceinline__ bool lsd_bit(const uint32_t *bits, int j) { return (bits[j >> 5] >> (j & 31)) & 1u; }

// least (key, index) among the columns of row r outside A, above (tk, tj) when thr; kLsdNone when there is none
__device__ __forceinline__ int lsd_scan(const LsdArgs &P, const double *llr, const uint32_t *inA, int r, bool thr, unsigned long long tk, int tj) {
    int best = kLsdNone;
    unsigned long long bk = ~0ull;
    const int e1 = P.indptr[r + 1];
#pragma unroll 4
    for (int e = P.indptr[r]; e < e1; e++) {                                 // no branch between the loads: the keys of several columns are in flight at once
        const int j = P.indices[e];
        const unsigned long long k = osd_key(llr[j]);
        const bool open = !lsd_bit(inA, j) && (!thr || k > tk || (k == tk && j > tj));
        const bool take = open && (k < bk || (k == bk && j < best));
        bk = take ? k : bk;
        best = take ? j : best;
    }
    return best;
}

__global__ __launch_bounds__(kLsdBlock) void lsd_kernel(LsdArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int m = P.m, n = P.n, cd = P.cdeg, MR = P.mr, W = P.w, tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
    unsigned long long *U = reinterpret_cast<unsigned long long *>(lds);                          // [MR + 1][W]
    unsigned long long *usedw = reinterpret_cast<unsigned long long *>(lds + P.o.offUsed);       // [W]
    unsigned long long *Mrow = reinterpret_cast<unsigned long long *>(lds + P.o.offMask);        // [W]
    unsigned long long *bestKey = reinterpret_cast<unsigned long long *>(lds + P.o.offBestKey);  // [MR]
    unsigned int *bestJ = reinterpret_cast<unsigned int *>(lds + P.o.offBestJ);                  // [MR]
    uint16_t *lidx = reinterpret_cast<uint16_t *>(lds + P.o.offLidx);                            // [m]
    uint32_t *inA = reinterpret_cast<uint32_t *>(lds + P.o.offInA), *picked = reinterpret_cast<uint32_t *>(lds + P.o.offPicked);
    uint16_t *label = reinterpret_cast<uint16_t *>(lds + P.o.offLabel), *cache = reinterpret_cast<uint16_t *>(lds + P.o.offCache);
    uint16_t *cand = reinterpret_cast<uint16_t *>(lds + P.o.offCand), *rowg = reinterpret_cast<uint16_t *>(lds + P.o.offRowg);
    uint16_t *pivcol = reinterpret_cast<uint16_t *>(lds + P.o.offPivcol), *lastJ = reinterpret_cast<uint16_t *>(lds + P.o.offLastJ);
    unsigned char *invalid = lds + P.o.offInvalid;                                                // [MR]
    uint16_t *clab = reinterpret_cast<uint16_t *>(lds + P.o.offColLab);                           // [cdeg]
    unsigned long long *lK = reinterpret_cast<unsigned long long *>(lds + P.o.offListK);
    uint16_t *lJ = reinterpret_cast<uint16_t *>(lds + P.o.offListJ), *lS = reinterpret_cast<uint16_t *>(lds + P.o.offListS);
    int *ib = reinterpret_cast<int *>(lds + P.o.offMisc);
    unsigned long long *gK = reinterpret_cast<unsigned long long *>(P.scratch + (size_t)blockIdx.x * P.scratch_bytes);
    uint16_t *gJ = reinterpret_cast<uint16_t *>(gK + n), *gS = gJ + n;
    unsigned long long *Ub = U + (size_t)MR * W;                                                  // T b
    const int nbw = (n + 31) / 32;

    const int total = *P.count;
    for (;;) {
        if (tid == 0) ib[kIbItem] = atomicAdd(P.queue, 1);
        __syncthreads();
        const int item = ib[kIbItem];
        if (item >= total) break;
        const int64_t shot = P.list[item];
        const double *llr = P.llr + shot * n;
        const int8_t *hard = P.hard + shot * n, *synd = P.synd + shot * m;
        int8_t *sol = P.solution + shot * n;
        int32_t *info = P.info + shot * 4;
        // ---- b = s + H hard; its ones are the seeds ----
        for (int r = tid; r < m; r += T) lidx[r] = (uint16_t)kLsdNone;
        for (int t = tid; t < nbw; t += T) { inA[t] = 0u; picked[t] = 0u; }
        if (tid < W) { usedw[tid] = 0ull; Ub[tid] = 0ull; }
        if (tid == 0) { ib[kIbRows] = 0; ib[kIbAdded] = 0; ib[kIbNoCand] = 0; }
        __syncthreads();
        for (int r = tid; r < m; r += T) {
            int sy = synd[r] & 1;
            const int e0 = P.indptr[r], e1 = P.indptr[r + 1];
            for (int e = e0; e < e1; e++) sy ^= hard[P.indices[e]] & 1;
            if (sy) {
                if (e0 == e1) ib[kIbNoCand] = 1;                               // a seed without columns: its cluster has no candidate in round 1
                const int l = atomicAdd(&ib[kIbRows], 1);
                if (l < MR) { lidx[r] = (uint16_t)l; rowg[l] = (uint16_t)r; }
            }
        }
        __syncthreads();
        int nR = ib[kIbRows], rounds = 0, flag = 0;
        if (nR > MR) flag = ib[kIbNoCand] ? 2 : 1;                              // (round 1 looks for candidates before it looks at the cap)
        else if (nR > 0) {
            for (int q = tid; q < nR; q += T) {
                for (int w = 0; w < W; w++) U[(size_t)q * W + w] = 0ull;
                U[(size_t)q * W + (q >> 6)] = 1ull << (q & 63);
                label[q] = (uint16_t)q;
                cache[q] = (uint16_t)kLsdUnset;
            }
            if (tid < W) Ub[tid] = (nR >= 64 * (tid + 1)) ? ~0ull : (nR > 64 * tid ? ((1ull << (nR - 64 * tid)) - 1ull) : 0ull);
            __syncthreads();
            for (;;) {
                // ---- validity of every cluster ----
                for (int q = tid; q < nR; q += T) invalid[q] = 0;
                if (tid == 0) { ib[kIbAny] = 0; ib[kIbListed] = 0; }
                __syncthreads();
                for (int q = tid; q < nR; q += T)
                    if (((Ub[q >> 6] & ~usedw[q >> 6]) >> (q & 63)) & 1ull) { invalid[label[q]] = 1; ib[kIbAny] = 1; }
                __syncthreads();
                if (!ib[kIbAny]) break;
                rounds++;
                // ---- every invalid cluster picks its least keys; the list of the round is their union ----
                for (int it = 0; it < P.bps; it++) {
                    for (int q = tid; q < nR; q += T) { bestKey[q] = ~0ull; bestJ[q] = 0xFFFFFFFFu; }
                    __syncthreads();
                    for (int q = tid; q < nR; q += T) {
                        const int L = label[q];
                        int c = kLsdNone;
                        if (invalid[L] == 1) {
                            if (it == 0) {
                                c = cache[q];
                                if (c == kLsdUnset || (c != kLsdNone && lsd_bit(inA, c))) { c = lsd_scan(P, llr, inA, rowg[q], false, 0ull, 0); cache[q] = (uint16_t)c; }
                            } else {
                                const int tj = lastJ[L];
                                c = lsd_scan(P, llr, inA, rowg[q], true, osd_key(llr[tj]), tj);
                            }
                            if (c != kLsdNone) atomicMin(&bestKey[L], osd_key(llr[c]));
                        }
                        cand[q] = (uint16_t)c;
                    }
                    if (tid == 0) ib[kIbPicked] = 0;
                    __syncthreads();
                    for (int q = tid; q < nR; q += T) {
                        const int c = cand[q];
                        if (c != kLsdNone && osd_key(llr[c]) == bestKey[label[q]]) atomicMin(&bestJ[label[q]], (unsigned int)c);
                    }
                    __syncthreads();
                    for (int L = tid; L < nR; L += T) {
                        if (label[L] != L || invalid[L] != 1) continue;
                        const unsigned int j = bestJ[L];
                        if (j == 0xFFFFFFFFu) {                                 // out of candidates (in the first pass: none at all, flag 2)
                            invalid[L] = 2;
                            if (it == 0) ib[kIbNoCand] = 1;
                            continue;
                        }
                        lastJ[L] = (uint16_t)j;
                        ib[kIbPicked] = 1;
                        const uint32_t bit = 1u << (j & 31);
                        if (!(atomicOr(&picked[j >> 5], bit) & bit)) {          // (two clusters may pick the same column)
                            const int i = atomicAdd(&ib[kIbListed], 1);
                            gK[i] = bestKey[L]; gJ[i] = (uint16_t)j;
                            if (i < kLsdListCap) { lK[i] = bestKey[L]; lJ[i] = (uint16_t)j; }
                        }
                    }
                    __threadfence_block();
                    __syncthreads();
                    if (ib[kIbNoCand] || !ib[kIbPicked]) break;
                }
                if (ib[kIbNoCand]) { flag = 2; break; }
                // ---- the list in ascending key order (rank counting) ----
                const int nN = ib[kIbListed];
                const bool small = nN <= kLsdListCap;
                const unsigned long long *NK = small ? lK : gK;
                const uint16_t *NJ = small ? lJ : gJ;
                uint16_t *NS = small ? lS : gS;
                for (int i = tid; i < nN; i += T) {
                    const unsigned long long k = NK[i];
                    const int j = NJ[i];
                    int rank = 0;
                    for (int e = 0; e < nN; e++) { const unsigned long long ke = NK[e]; rank += (ke < k || (ke == k && (int)NJ[e] < j)) ? 1 : 0; }
                    NS[rank] = (uint16_t)j;
                    atomicOr(&inA[j >> 5], 1u << (j & 31));
                }
                __threadfence_block();
                __syncthreads();
                // ---- the rows the list brings in, in list order (wave 0); the cap ----
                if (tid < 64) {
                    int nr = nR;
                    for (int i = 0; i < nN; i++) {
                        const uint16_t *cr = P.col_rows + (size_t)NS[i] * cd;
                        for (int d0 = 0; d0 < cd; d0 += 64) {
                            const int r = (d0 + lane < cd) ? (int)cr[d0 + lane] : m;
                            const bool fresh = r < m && lidx[r] == kLsdNone;
                            const unsigned long long bal = __ballot(fresh);
                            if (fresh) {
                                const int l = nr + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                                lidx[r] = (uint16_t)(l < MR ? l : kLsdUnset);      // (beyond the cap: counted once, never used)
                                if (l < MR) rowg[l] = (uint16_t)r;
                            }
                            nr += __builtin_popcountll(bal);
                        }
                    }
                    if (lane == 0) ib[kIbRowsNew] = nr;
                }
                __syncthreads();
                const int nRn = ib[kIbRowsNew];
                if (nRn > MR) { flag = 1; break; }
                for (int q = nR + tid; q < nRn; q += T) {
                    for (int w = 0; w < W; w++) U[(size_t)q * W + w] = 0ull;
                    U[(size_t)q * W + (q >> 6)] = 1ull << (q & 63);
                    label[q] = (uint16_t)q;
                    cache[q] = (uint16_t)kLsdUnset;
                }
                nR = nRn;
                const int Wc = (nR + 63) >> 6;
                __syncthreads();
                // ---- the columns join A one by one ----
                for (int i = 0; i < nN; i++) {
                    const int j = NS[i];
                    if (tid < 64) {
                        const uint16_t *cr = P.col_rows + (size_t)j * cd;
                        unsigned long long acc = 0ull;
                        int tgt = kLsdNone, deg = 0;
                        for (int d0 = 0; d0 < cd; d0 += 64) {                    // one load per 64 rows of the column (they ascend, the padding comes last)
                            const int r = (d0 + lane < cd) ? (int)cr[d0 + lane] : m;
                            const int l = r < m ? (int)lidx[r] : 0;
                            int lab = r < m ? (int)label[l] : kLsdNone;
                            const int cnt = __builtin_popcountll(__ballot(r < m));   // (the lanes with a row are lanes 0 .. cnt - 1)
                            if (r < m) clab[d0 + lane] = (uint16_t)lab;
                            for (int dd = 0; dd < cnt; dd++) {
                                const int ld = __shfl(l, dd);
                                if (lane < W) acc ^= U[(size_t)ld * W + lane];
                            }
                            for (int o = 32; o > 0; o >>= 1) lab = min(lab, __shfl_xor(lab, o));
                            tgt = min(tgt, lab);
                            deg += cnt;
                        }
                        const unsigned long long z = (lane < W) ? (acc & ~usedw[lane]) : 0ull;
                        const unsigned long long bal = __ballot(z != 0ull);
                        int p = -1;
                        if (bal != 0ull) {
                            const int f = __builtin_ctzll(bal);
                            const uint32_t zlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)z, f), zhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(z >> 32), f);
                            p = 64 * f + __builtin_ctzll(((unsigned long long)zhi << 32) | zlo);
                            if (lane == f) { acc &= ~(1ull << (p & 63)); usedw[lane] |= 1ull << (p & 63); }
                        }
                        if (lane < W) Mrow[lane] = acc;
                        if (lane == 0) { ib[kIbPivot] = p; ib[kIbTarget] = tgt; ib[kIbDegree] = deg; if (p >= 0) pivcol[p] = (uint16_t)j; }
                    }
                    __syncthreads();
                    const int p = ib[kIbPivot], tgt = ib[kIbTarget], deg = ib[kIbDegree];
                    if (p >= 0) {
                        const int pw = p >> 6, pb = p & 63;
                        for (int t = tid; t < (nR + 1) * Wc; t += T) {
                            const int q = t / Wc, w = t - q * Wc;
                            unsigned long long *row = (q < nR) ? U + (size_t)q * W : Ub;
                            if ((row[pw] >> pb) & 1ull) row[w] ^= Mrow[w];       // (M has bit p cleared: the word tested does not lose that bit)
                        }
                    }
                    for (int q = tid; q < nR; q += T) {
                        const int lab = label[q];
                        if (lab == tgt) continue;
                        for (int d = 0; d < deg; d++)
                            if (clab[d] == lab) { label[q] = (uint16_t)tgt; break; }
                    }
                    __syncthreads();
                }
                if (tid == 0) ib[kIbAdded] += nN;
            }
        }
        __syncthreads();
        // ---- the answer: hard ^ c with c on the pivots, or the shot goes on the list for OSD-0 ----
        if (flag == 0) {
            if (sol != hard) {
                for (int j = tid; j < n; j += T) sol[j] = hard[j];
                __threadfence();
                __syncthreads();
            }
            for (int q = tid; q < nR; q += T)
                if (((usedw[q >> 6] & Ub[q >> 6]) >> (q & 63)) & 1ull) { const int j = pivcol[q]; sol[j] = (int8_t)((hard[j] ^ 1) & 1); }
        }
        if (tid == 0) {
            if (flag != 0) P.redo_list[atomicAdd(P.redo_count, 1)] = (int32_t)shot;
            info[0] = flag; info[1] = flag ? 0 : rounds; info[2] = flag ? 0 : nR; info[3] = flag ? 0 : ib[kIbAdded];
            if (P.counts) atomicAdd(&P.counts[flag], 1ull);
        }
        // ---- the cluster statistics (qldpc_lsd_stats_batch): per label the columns of A, their weight and the rows, then sums and maxima over the labels.
        // The accumulators are pieces that are dead once the solution is out: bestJ (columns), bestKey (weight), the first words of U (rows; T b in row MR
        // stays), the round's key list (the eight slots).  LDS integer atomics only, so neither lane order nor the order of the seed indices enters. ----
        if (P.stats) {
            unsigned int *rcnt = reinterpret_cast<unsigned int *>(U);                             // [nR] (nR <= MR < the words of U's rows)
            unsigned long long *acc = lK;                                                         // [8]
            const int nC = flag == 0 ? nR : 0;
            for (int q = tid; q < nC; q += T) { bestKey[q] = 0ull; bestJ[q] = 0u; rcnt[q] = 0u; }
            if (tid < 8) acc[tid] = 0ull;
            __syncthreads();
            if (nC > 0) {
                for (int q = tid; q < nC; q += T) atomicAdd(&rcnt[label[q]], 1u);
                for (int t = tid; t < nbw; t += T)
                    for (uint32_t bits = inA[t]; bits; bits &= bits - 1u) {
                        const int j = 32 * t + __builtin_ctz(bits);
                        const int L = label[lidx[P.col_rows[(size_t)j * cd]]];                    // (a column of A has a row, and its rows are in R)
                        atomicAdd(&bestJ[L], 1u);
                        if (P.weight) atomicAdd(&bestKey[L], (unsigned long long)P.weight[j]);
                    }
                __syncthreads();
                for (int L = tid; L < nC; L += T) {
                    if (label[L] != L) continue;
                    const unsigned long long a = bestJ[L], wt = bestKey[L];
                    atomicAdd(&acc[0], 1ull);
                    atomicAdd(&acc[1], a); atomicAdd(&acc[2], a * a); atomicMax(&acc[3], a);
                    atomicAdd(&acc[4], wt); atomicAdd(&acc[5], wt * wt); atomicMax(&acc[6], wt);
                    atomicMax(&acc[7], (unsigned long long)rcnt[L]);
                }
                __syncthreads();
            }
            if (tid < 8) P.stats[shot * 8 + tid] = flag ? ~0ull : acc[tid];                       // (capped or without candidates: no statement)
        }
        __syncthreads();
    }
}

// the layout (lsd_supported), and the hand-over: flag-1 and flag-2 shots go to osd0_listed_launch, so a matrix OSD-0 refuses is refused here, once, before
// anything is launched (whether a shot would be listed is not known until the cluster kernel has run)
int lsd_graph_supported(const qldpc_graph *g, int max_rows) {
    switch (lsd_supported(g->m, g->n, std::max(g->max_col_deg, 1), max_rows)) {
    case kLsdAccepted:
        if (osd0_plan(g->m, g->n, g->max_col_deg, 0).refused == kOsdAccepted) return QLDPC_OK;
        set_error("LSD hands the shots it cannot finish over to OSD-0, which refuses a %d x %d matrix (too large for its LDS scratch: m=%d nwords=%d)", g->m,
                  g->n, g->m, osd_global_nwords(g->n));
        break;
    case kLsdRefusedColumns: set_error("LSD supports n < 65535 (this matrix has %d columns)", g->n); break;
    case kLsdRefusedRows: set_error("LSD supports m <= 65535 (this matrix has %d rows)", g->m); break;
    case kLsdRefusedLds: set_error("LSD: a %d x %d matrix with max_rows = %d needs more LDS than the 160 KiB of a workgroup", g->m, g->n, max_rows); break;
    }
    return QLDPC_ERR_UNSUPPORTED;
}

int lsd_check_params(int bits_per_step, int max_rows) {
    QLDPC_REQUIRE(bits_per_step >= 1 && bits_per_step <= kLsdMaxBits, "LSD bits_per_step %d outside 1..%d", bits_per_step, kLsdMaxBits);
    QLDPC_REQUIRE(max_rows >= 1 && max_rows <= kLsdMaxRows, "LSD max_rows %d outside 1..%d", max_rows, kLsdMaxRows);
    return QLDPC_OK;
}

// callers hold g->mu.  LSD on the shots listed in d_list [0 .. *d_count); the shots that end capped or without candidates get qldpc_osd0_batch's answer
// from the OSD-0 kernels, behind this launch on the same stream.
int lsd_listed_launch(const qldpc_graph *g, const int32_t *d_list, const int32_t *d_count, int64_t max_listed, const int8_t *d_synd, const double *d_llr,
                      const int8_t *d_hard, int bits_per_step, int max_rows, int8_t *d_solution, int32_t *d_info, unsigned long long *d_counts,
                      const uint16_t *d_weight, unsigned long long *d_stats, hipStream_t stream) {
    if (g->m == 0 || g->n == 0 || max_listed == 0) return QLDPC_OK;
    int rc = lsd_graph_supported(g, max_rows);
    if (rc != QLDPC_OK) return rc;
    LsdArgs P;
    P.m = g->m; P.n = g->n; P.cdeg = std::max(g->max_col_deg, 1); P.mr = max_rows; P.w = (max_rows + 63) / 64; P.bps = bits_per_step;
    const size_t lds = lsd_layout(P.m, P.n, P.cdeg, max_rows, P.o);
    if ((rc = ensure_col_rows(g)) != QLDPC_OK) return rc;
    const int grid = (int)std::min<int64_t>(kLsdGrid, max_listed);
    if ((rc = g->ws_acquire(stream)) != QLDPC_OK) return rc;
    auto launch = [&]() -> int {
        P.scratch_bytes = lsd_scratch_bytes(g->n);
        int rcl = g->ws_misc.ensure((size_t)grid * P.scratch_bytes + 64);
        if (rcl != QLDPC_OK) return rcl;
        P.scratch = g->ws_misc.as<unsigned char>();
        if ((rcl = g->ws_cs.ensure((size_t)(max_listed + 4) * 4 + 16)) != QLDPC_OK) return rcl;
        if ((rcl = g->ws_queue.ensure(16)) != QLDPC_OK) return rcl;
        P.queue = g->ws_queue.as<int>();
        P.redo_count = g->ws_cs.as<int32_t>(); P.redo_list = P.redo_count + 4;
        QLDPC_HIP_TRY(hipMemsetAsync(P.queue, 0, 4, stream));
        QLDPC_HIP_TRY(hipMemsetAsync(P.redo_count, 0, 4, stream));
        P.col_rows = g->d_col_rows; P.indptr = g->d_indptr; P.indices = g->d_indices;
        P.list = d_list; P.count = d_count; P.synd = d_synd; P.llr = d_llr; P.hard = d_hard;
        P.solution = d_solution; P.info = d_info; P.counts = d_counts; P.weight = d_weight; P.stats = d_stats;
        if ((rcl = ensure_max_lds(g->device, reinterpret_cast<const void *>(lsd_kernel), kLsdLdsMax)) != QLDPC_OK) return rcl;
        hipLaunchKernelGGL(lsd_kernel, dim3(grid), dim3(kLsdBlock), lds, stream, P);
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

}  // namespace qldpc

using namespace qldpc;

// qldpc_lsd_batch_dev and qldpc_lsd_stats_batch_dev (want_stats: d_stats is an output the caller must give)
static int lsd_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard, int bits_per_step,
                         int max_rows, const int32_t *d_select, const int32_t *d_select_count, const uint16_t *d_weight, int8_t *d_solution,
                         int32_t *d_info, unsigned long long *d_stats, bool want_stats, void *stream) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "batch out of range");
    QLDPC_REQUIRE((d_select == nullptr) == (d_select_count == nullptr), "d_select and d_select_count go together");
    QLDPC_REQUIRE(!want_stats || d_stats != nullptr, "stats is NULL");
    int rc = lsd_check_params(bits_per_step, max_rows);
    if (rc != QLDPC_OK) return rc;
    if ((rc = lsd_graph_supported(g, max_rows)) != QLDPC_OK) return rc;
    if (B == 0 || g->n == 0) return QLDPC_OK;
    QLDPC_REQUIRE(d_llr && d_hard && d_solution && d_info && (d_syndromes || g->m == 0), "NULL buffer");
    QLDPC_USE_DEVICE(g->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->m == 0) { set_error("LSD on device pointers needs a matrix with rows"); return QLDPC_ERR_UNSUPPORTED; }
    if (!d_select) {
        if ((rc = g->ws_acquire(s)) != QLDPC_OK) return rc;
        if ((rc = g->ws_list.ensure((size_t)B * 4 + 16)) != QLDPC_OK) { (void)g->ws_release(s); return rc; }
        int32_t *cnt = g->ws_list.as<int32_t>(), *list = cnt + 4;
        iota_list_launch(B, list, cnt, s);
        d_select = list; d_select_count = cnt;
    }
    return lsd_listed_launch(g, d_select, d_select_count, B, d_syndromes, d_llr, d_hard, bits_per_step, max_rows, d_solution, d_info, nullptr, d_weight,
                             d_stats, s);
}

// qldpc_lsd_batch and qldpc_lsd_stats_batch
static int lsd_batch_host(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard, int bits_per_step, int max_rows,
                          const uint16_t *weight, int8_t *solution, int32_t *info, uint64_t *stats, bool want_stats) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    QLDPC_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "batch out of range");
    QLDPC_REQUIRE(!want_stats || stats != nullptr, "stats is NULL");
    int rc = lsd_check_params(bits_per_step, max_rows);
    if (rc != QLDPC_OK) return rc;
    if ((rc = lsd_graph_supported(g, max_rows)) != QLDPC_OK) return rc;
    if (B == 0 || g->n == 0) return QLDPC_OK;
    QLDPC_REQUIRE(llr && hard && solution && info && (syndromes || g->m == 0), "NULL buffer");
    const size_t m = g->m, n = g->n;
    QLDPC_USE_DEVICE(g->device);
    if (m == 0) {                                                            // no checks: the residual is zero
        std::memcpy(solution, hard, (size_t)B * n);
        std::memset(info, 0, (size_t)B * 16);
        if (stats) std::memset(stats, 0, (size_t)B * 64);
        return QLDPC_OK;
    }
    HostStage S;
    const auto ds = S.in(syndromes, B, m);
    const auto dl = S.in(llr, B, n);
    const auto dh = S.in(hard, B, n);
    const auto dsol = S.out(solution, B, n);
    const auto dinf = S.out(info, B, 4);
    const auto dlist = S.scratch<int32_t>(B), dcnt = S.scratch<int32_t>(4);
    Staged<uint16_t> dw;
    Staged<uint64_t> dst;
    if (weight) dw = S.in(weight, n);
    if (stats) dst = S.out(stats, B, 8);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    iota_list_launch(B, S[dlist], S[dcnt], nullptr);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        rc = lsd_listed_launch(g, S[dlist], S[dcnt], B, S[ds], S[dl], S[dh], bits_per_step, max_rows, S[dsol], S[dinf], nullptr, S[dw],
                               reinterpret_cast<unsigned long long *>(S[dst]), nullptr);
    }
    return rc != QLDPC_OK ? rc : S.finish("LSD kernel", HostStage::kDevice);
}

QLDPC_EXPORT int qldpc_lsd_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard,
                                     int bits_per_step, int max_rows, const int32_t *d_select, const int32_t *d_select_count, int8_t *d_solution,
                                     int32_t *d_info, void *stream) {
    return lsd_batch_dev(g, B, d_syndromes, d_llr, d_hard, bits_per_step, max_rows, d_select, d_select_count, nullptr, d_solution, d_info, nullptr, false,
                         stream);
}

QLDPC_EXPORT int qldpc_lsd_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard, int bits_per_step,
                                 int max_rows, int8_t *solution, int32_t *info) {
    return lsd_batch_host(g, B, syndromes, llr, hard, bits_per_step, max_rows, nullptr, solution, info, nullptr, false);
}

QLDPC_EXPORT int qldpc_lsd_stats_batch_dev(const qldpc_graph *g, int64_t B, const int8_t *d_syndromes, const double *d_llr, const int8_t *d_hard,
                                           int bits_per_step, int max_rows, const int32_t *d_select, const int32_t *d_select_count,
                                           const uint16_t *d_weight, int8_t *d_solution, int32_t *d_info, uint64_t *d_stats, void *stream) {
    return lsd_batch_dev(g, B, d_syndromes, d_llr, d_hard, bits_per_step, max_rows, d_select, d_select_count, d_weight, d_solution, d_info,
                         reinterpret_cast<unsigned long long *>(d_stats), true, stream);
}

QLDPC_EXPORT int qldpc_lsd_stats_batch(const qldpc_graph *g, int64_t B, const int8_t *syndromes, const double *llr, const int8_t *hard, int bits_per_step,
                                       int max_rows, const uint16_t *weight, int8_t *solution, int32_t *info, uint64_t *stats) {
    return lsd_batch_host(g, B, syndromes, llr, hard, bits_per_step, max_rows, weight, solution, info, stats, true);
}
