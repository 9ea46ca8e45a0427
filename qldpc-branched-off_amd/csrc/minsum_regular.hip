// Branch-free LDS/register-resident min-sum kernel for REGULAR Tanner graphs (every check of degree CDEG, every
// variable of degree VDEG -- all bivariate-bicycle codes: CDEG = 6, VDEG = 3), optionally fused with the whole
// code-capacity Monte-Carlo step.
//
// Thread mapping as in minsum_resident.hip (a team of TS threads owns one shot; a thread is the CHECK thread of one
// row -- its check->variable messages R stay in registers for the whole decode -- and the VARIABLE thread of two
// columns), but with compile-time degrees the check update is straight-line code:
//   * Q = clip(V[col] - R) as v_min_f64/v_max_f64 (the NaN test of kernels.py:328 is kept unless the launcher proved
//     that no NaN can arise: finite prior/clip/alpha and every check degree >= 2);
//   * the damped and the NaN-tolerant forms: min1 / min2 = the two smallest magnitudes WITH multiplicity (kernels.py:301-306);
//     the position that receives min2 is selected by |q| == min1: if the minimum is attained twice, min2 == min1, so
//     this equals the reference's "first strict minimum" rule at every position; signs are boolean masks (x < 0; note -0.0
//     counts as >= 0 exactly like `val >= 0`, kernels.py:296), the message is (+-alpha) * mag, one rounding, equal to the
//     reference's (alpha * sign) * mag;
//   * clean undamped inputs (CLIPMIN = NANFREE && !DAMP; "clean", inputs_clean() in decode_api.hip: every prior finite and not
//     -0.0, clip finite > 0, every alpha finite > 0) build the CDEG message words of a check with neither a compare nor a select,
//     from the UNCLIPPED t_k = V[col_k] - Rprev_k.  Why each word equals the reference's, bit for bit:
//       signs      A posterior is never -0.0: it is (a sum of messages) + prior (kernels.py:279,316,320), x + y is -0.0 only for
//                  x = y = -0.0 under round-to-nearest, and the prior is not -0.0 (with or without the leading 0.0 of "zero" below).
//                  a - b is -0.0 only for a = -0.0, b = +0.0, so no t_k is -0.0 either, and none is NaN (all operands finite:
//                  |R| <= max(|prior|, clip)).  Hence x < 0 <=> the sign bit of x's high word, for posteriors and for t_k:
//                  the parity of the hard decisions is the sign bit of the XOR of the posteriors' high words, and the sign of
//                  the whole row is that of spw = syndrome bit ^ hi(t_0) ^ ... ^ hi(t_{CDEG-1}).  Edge k's message takes the
//                  sign bit of spw ^ hi(t_k): the row without the edge itself (kernels.py:311-314).  The reference reads
//                  signs AFTER the clip; clip(t) < 0 <=> t < 0 for clip > 0.  (A MESSAGE may be -0.0, namely when its
//                  magnitude is 0; the reference's (alpha * sign) * 0.0 is the same word, and a - (-0.0) = a.)
//       ties       The reference gives min2 to the first strict minimum and min1 to every other edge (kernels.py:301-313).
//                  Here mag_k = min over j != k of |t_j|, from prefix minima p_k = min(|t_0|..|t_k|) and suffix minima
//                  s_k = min(|t_k|..|t_{CDEG-1}|): mag_0 = s_1, mag_{CDEG-1} = p_{CDEG-2}, mag_k = min(p_{k-1}, s_{k+1}).
//                  If the minimum is attained once, at k: mag_k = min2 and every other mag_j = min1 -- the reference's rule.
//                  If it is attained twice or more, min2 == min1 and every mag_j = min1 -- again what the reference stores at
//                  every position.  No selector exists, so a tie cannot pick a different position.
//       clip       |clip(t)| = min(|t|, clip) and min is associative, commutative, monotone and rounds nothing.  The two
//                  chain seeds are p_0 = min(|t_0|, cmin) and s_{CDEG-1} = min(|t_{CDEG-1}|, cmin); every mag_k contains at
//                  least one seed (CDEG >= 2), so mag_k = min(min over j != k of |t_j|, cmin) = the minimum over j != k of the
//                  CLIPPED magnitudes.  cmin = clip for it > 0 and +inf at it == 0, whose inputs are priors and take no clip
//                  (kernels.py:263-265).  clip == 0 is NOT covered (clip(t) = +-0.0 loses the sign the reference then reads as
//                  >= 0): such a call is not clean and takes the NaN-tolerant per-edge form, like the damped form, whose
//                  Q_old needs the clipped value of every edge.
//       rounding   The word is sign | (alpha * mag_k): one v_mul_f64 of the same two operands the reference multiplies
//                  (mag_k is its min1 or min2 after the clip), and (alpha * sign) * mag == sign * (alpha * mag) exactly for
//                  sign = +-1.  The sign bit goes in with v_bfi_b32; alpha * mag_k >= 0 has a clear sign bit to replace.
//       zero       The reference's variable sum is (((0.0 + a) + b) + c) + prior (kernels.py:279,316,320); the clean forms compute ((a + b) + c) + prior.
//                  0.0 + a differs from a only for a = -0.0, so the two running sums differ only while every addend so far is -0.0, and
//                  then as +0.0 against -0.0: once a nonzero message arrives both are that message's sum, exactly.  If all VDEG messages
//                  are -0.0 the sums are +0.0 and -0.0, and the prior closes the gap: (+-0.0) + x = x for x != 0, (+-0.0) + (+0.0) = +0.0.
//                  A prior of -0.0 would not: (+0.0) + (-0.0) = +0.0 but (-0.0) + (-0.0) = -0.0, a posterior the sign argument above
//                  excludes.  Clean inputs have no such prior; the damped and the NaN-tolerant forms accept one and keep the add.
//                  The same covers OWN with the own message first in check order: it adds o1 + own where the reference adds own + o1.
//     Per check and iteration: CDEG v_sub, 3 * CDEG - 4 v_min_f64 (two of them the seeds), CDEG v_mul_f64, 2 * CDEG + 1 v_xor,
//     CDEG v_bfi.  The suffix chain is built first, the prefix chain runs forward and each message leaves as soon as its two
//     inputs exist, so t_k dies edge by edge.
//   * clean (6,3) graphs with an ownership assignment (OWN; regular_own.h, built once per graph handle): the two columns of a thread are two columns of
//     its OWN check, edges 0 and 1 of the reordered row (the check update does not depend on edge order: min and XOR are exact and commutative and no
//     selector exists).  Their two messages never leave Rprev, their posteriors are gathered from registers, the row holds the other four words, and
//     the variable sum takes its two other messages from LDS in ascending check order with the own one selected into its place: the reference's
//     ((0 + a) + b) + c, whose posterior word (a + b) + c gives as well ("zero" above).  Per thread and pass 8 words gathered and 6 stored instead of
//     12 and 8, for eight v_cndmask_b32 -- the LDS pipe, not VALU issue, bounds the loop (profiles/r20_own_edges.txt).
//     qldpc_set_option("regular_own_edges", 0) takes the body without ownership.
//   * the fixed-work ownership form (PLACE) takes WHERE in LDS its posteriors and messages live from a per-thread record (regular_place.h), built per
//     (S, block) on the host by edge colouring and loaded once into 14 address registers: the four posterior gathers, the four message gathers and the
//     four message stores of every wave are free of bank conflicts, the two posterior stores nearly so.  The row leaves as four independent
//     ds_write_b64.  The kernel's edges 2 .. 5 are "whatever posterior gather k reads": the table may order a check's four stored edges as it likes,
//     because Rprev[k] and the message store of edge k follow the gather and the check update is order-free (above).  The readers of a thread's own
//     posterior (prologue store, final syndrome test, logical comparison, export, out_llr) use the record's store places.  No address is packed: the
//     bare loop keeps one basic block, 64 VGPRs and no scratch access with 14 address registers.  qldpc_set_option("regular_place", 0) launches the
//     same kernel with the linear addresses as a table.  The early-exit form keeps the slot-relative addresses (see PLACE below).
//   * class-uniform waves (PLACE; qldpc_set_option("regular_wave_classes", 0) turns them off).  The eight v_cndmask_b32 of the ownership form exist only because
//     `last` differs from lane to lane.  A placed table is therefore built from the assignment that owns the FEWEST last edges (regular_own.h: min-cost
//     flow) and deals the (slot, check) items of a workgroup to its threads so that whole waves hold checks that own no last edge (regular_place.h); the
//     record names the thread's (slot, member) and its wave's class, and in the bare passes such a wave runs straight through the sums (o1 + own) + o2,
//     without a select: one forward branch, not taken, and the back-edge; the other waves' sums sit out of line behind that branch.  Why no output word moves:
//       assignment   every perfect assignment gives the reference's words (regular_own.h, header: the sum is the ascending-order sum whichever of
//                    the column's three checks owns it);
//       thread order threads exchange data only through LDS addresses taken from the table, which is built for the order; the leaders of a team are
//                    `member == 0` by value, `threadIdx.x == 0` and `threadIdx.x < S` only pick one thread or S threads of the block for block-wide
//                    words, a lane of no team has slot S (in_team false) as before, and the tally's and the logical mask's atomics commute;
//       the arm      a wave takes it only if the table labels it "none", and the label is computed from the same `last` bits the selects read.
//     Four copies of the loop (or of the pass inside one loop) were built first and dropped: the register allocator reloads 8 to 15 loop invariants from
//     scratch inside three of four sequential loops, and four passes inside one loop cost five scalar branches per pass (profiles/r27_wave_classes.txt).
// MC = true fuses the sampler (Philox4x32-10 stream of mc_common.h), the GF(2) syndrome (a6), the decode, the logical
// comparison L (e xor e_hat) (engine.py:99-100) and the tally (engine.py:450-457) into the same launch: errors and
// syndromes live in LDS, the posterior in registers; only shots BP fails on are written out (for the OSD-0 stage).
#include "common.h"
#include "launchers.h"
#include "clocks.h"
#include "mc_common.h"
#include "minsum_common.h"
#include "minsum_f64.h"
#include "regular_plan.h"
#include "regular_own.h"
#include "regular_place.h"

#include <atomic>
#include <cstdlib>
#include <type_traits>

namespace qldpc {

struct RegArgs {
    int m, n, max_iter, fixed, S, TS;
    const int32_t *indptr, *indices, *colptr, *rowidx, *csc2csr;
    const int32_t *own;             // ownership records of the (6,3) clean form (regular_own.h), NULL = the body without ownership
    const int32_t *place;           // with `own`, fixed work: the LDS places of every thread of the workgroup, [block] records (regular_place.h)
    int64_t B;
    const double *prior, *alpha;
    double damping, clip;
    // decode mode
    const int8_t *synd; int8_t *out_err; double *out_llr; uint8_t *out_conv; int32_t *out_iter;
    // Monte-Carlo mode
    uint32_t seed_lo, seed_hi, thr; int use_osd;
    int64_t shot_begin;
    const uint64_t *Lmask;
    const int32_t *shot_list, *shot_count;   // Monte-Carlo mode: decode only the listed shots (offsets from shot_begin; device-resident count), else NULL
    const struct RegCold *cold;     // rarely used pointers live in device memory to keep scalar registers free
    // LDS carve (byte offsets)
    int offV, offE, offL, offI, offA, offT, offD;
};

// The compare-free message words of one check (header comment): x holds the gathered posteriors and becomes the unclipped t_k = x_k - Rprev_k
// (`later`: iteration 0 reads priors, nothing to subtract), the clip sits in the two chain seeds (cmin), the words go to Rprev and to the check's row.
// SKIP: the first SKIP edges are the thread's own columns (regular_own.h); their words stay in Rprev only, edge k >= SKIP goes to row[k - SKIP], or, with a
// place table `at` (regular_place.h), to row[at[k - SKIP]]: CDEG - SKIP independent stores.
template <int CDEG, int SKIP = 0>
__device__ __forceinline__ void clean_messages(double (&x)[CDEG], double (&Rprev)[CDEG], bool later, double alpha, double cmin, unsigned synw, double *row,
                                               const int *at = nullptr) {
    unsigned spw = synw;                                                       // sign of the whole row in bit 31
#pragma unroll
    for (int k = 0; k < CDEG; k++) {
        if (later) x[k] = x[k] - Rprev[k];                                     // kernels.py:325
        spw ^= (unsigned)__double2hiint(x[k]);
    }
    double suf[CDEG];                                                          // suf[k] = min(|t_k|, .., |t_{CDEG-1}|, cmin), k = CDEG-1 .. 1
    suf[CDEG - 1] = vmin_abs_u(x[CDEG - 1], cmin);
#pragma unroll
    for (int k = CDEG - 2; k >= 1; k--) suf[k] = vmin_abs(x[k], suf[k + 1]);
    double pre = 0.0;                                                          // pre = min(|t_0|, .., |t_{k-1}|, cmin) from k = 1 on
#pragma unroll
    for (int k = 0; k < CDEG; k++) {
        const double mag = (k == 0) ? suf[1] : (k == CDEG - 1) ? pre : vmin(pre, suf[k + 1]);   // the minimum over the other edges (kernels.py:301-313)
        const unsigned sgn = spw ^ (unsigned)__double2hiint(x[k]);             // the row's sign without the edge itself (kernels.py:311-314)
        if (k < CDEG - 1) pre = (k == 0) ? vmin_abs_u(x[0], cmin) : vmin_abs(x[k], pre);
        const double prod = alpha * mag;                                       // >= 0: (alpha * sign) * mag == sign * (alpha * mag)
        const unsigned hi = ((unsigned)__double2hiint(prod) & 0x7fffffffu) | (sgn & 0x80000000u);
        const double msg = __hiloint2double((int)hi, __double2loint(prod));
        Rprev[k] = msg;
        if (k >= SKIP) row[at ? at[k - SKIP] : k - SKIP] = msg;
    }
}

#ifndef QLDPC_LB_T
#define QLDPC_LB_T 512
#define QLDPC_LB_W 8
#endif
// FIXED (all max_iter iterations executed for every shot, outputs frozen at convergence) is a template parameter: the fixed-work and the
// early-exit forms are distinct kernel symbols, so a rocprofv3 --stats summary lists them separately.
// OWN: the thread of a check is the variable thread of two of the check's OWN columns (regular_own.h): edges 0 and 1 of the reordered row.  Their messages
// stay in Rprev, their posteriors are gathered from registers, and the row holds the other four words in slots 0 .. 3.  Clean (6,3) form only.
template <int CDEG, int VDEG, bool DAMP, bool NANFREE, bool MC, bool FIXED, bool OWN = false>
__global__ __launch_bounds__(QLDPC_LB_T, QLDPC_LB_W) void minsum_regular_kernel(RegArgs A) {
    extern __shared__ unsigned char lds[];
    constexpr int RST = (CDEG % 2 == 0) ? CDEG + 1 : CDEG;
    const int m = A.m, n = A.n, S = A.S, TS = A.TS, max_iter = A.max_iter;
    const int nq = (n + 3) >> 2;
    constexpr bool CLIPMIN = NANFREE && !DAMP;      // compare-free message words with the clip in the two chain seeds (header comment); needs clip > 0, which NANFREE includes
    static_assert(!OWN || (CLIPMIN && CDEG == kRegOwnCdeg && VDEG == kRegOwnVdeg), "edge ownership: the clean (6,3) form");
    // PLACE: the fixed-work ownership form takes every LDS address of its posteriors and messages from a per-thread place record (regular_place.h).  The
    // early-exit form keeps the slot-relative addresses: its iteration loop is the one with the freeze bookkeeping, three more address registers took its
    // spills from 16 to 25 VGPRs, and the launch on listed shots under reference semantics, a few iterations per workgroup, ran 27 % longer (profiles/r24_place.txt)
    constexpr bool PLACE = OWN && FIXED;
    // Which (slot, member) a thread is: thread / TS and the remainder, except where a PLACE record names them (word [15], regular_place.h: the threads of a
    // workgroup dealt so that whole waves hold checks of one class of the ownership table).  The order is unobservable: threads exchange data through the
    // table's LDS addresses only, the leaders of a team are `member == 0` by value, a lane of no team has slot S, and the tally's atomics commute.
    int slot = threadIdx.x / TS, member = threadIdx.x - slot * TS;
    int wave_class = kRegWaveMixed;                                                  // PLACE: wave-uniform, in a scalar register
    if (PLACE) {
        const int w = A.place[(size_t)threadIdx.x * kRegPlaceWords + kRegPlaceOrder];
        if (w & kRegPlaceOrdered) { slot = (w >> 12) & 0xfff; member = w & 0xfff; }
        wave_class = __builtin_amdgcn_readfirstlane((w >> 24) & 3);
    }
    const bool in_team = slot < S;
    const int sl = in_team ? slot : 0;
    // ALL: the iteration body of the clean form runs with every lane enabled.  plan_regular takes n == 2 m only, so TS == m and every lane of a team owns
    // a check and two columns; a team without a shot (b >= nshots) works on its own slot, which nobody else touches, and the lanes of the block that
    // belong to no team work on the dummy region Dl: a row of RST doubles, two posteriors, one parity word.  Nothing they compute is ever read.
    constexpr bool ALL = CLIPMIN;
    // ZEROFREE: the variable sum starts at its first message instead of at 0.0 + that message (header comment, "zero"): clean inputs only
    constexpr bool ZEROFREE = CLIPMIN;
    constexpr int NOWN = OWN ? kRegOwnOwned : 0;                                   // edges of a row that are not stored
    double *Dl = reinterpret_cast<double *>(lds + A.offD);
    double *Rl = (ALL && !in_team) ? Dl : reinterpret_cast<double *>(lds) + (size_t)sl * m * RST;
    double *Vl = (ALL && !in_team) ? Dl + RST : reinterpret_cast<double *>(lds + A.offV) + (size_t)sl * n;
    uint32_t *El = reinterpret_cast<uint32_t *>(lds + A.offE) + (size_t)sl * nq;
    unsigned long long *lacc = reinterpret_cast<unsigned long long *>(lds + A.offL) + sl;
    int *I = reinterpret_cast<int *>(lds + A.offI);
    int *unsat = I + 2 * sl;            // [2] by iteration parity
    int *active = I + 2 * S;            // [0] active shots, [1] any failure to export
    int *sres = I + 2 * S + 2 + 4 * sl; // conv, final_iter, nonzero syndrome, failure index
    const double *Al = reinterpret_cast<const double *>(lds + A.offA);                  // alpha_k staged in LDS
    unsigned long long *Tl = reinterpret_cast<unsigned long long *>(lds + A.offT);      // block tally (MC)
    static_assert(CDEG >= 3, "the prefix / suffix chains need a middle edge");
    const double clip = A.clip, nclip = -A.clip, damping = A.damping, one_minus_d = 1.0 - A.damping;
    for (int k = threadIdx.x; k < max_iter; k += blockDim.x) reinterpret_cast<double *>(lds + A.offA)[k] = A.alpha[k];
    if (MC && threadIdx.x < 6) Tl[threadIdx.x] = 0ull;
    const double prior0 = (MC && A.n > 0) ? A.prior[0] : 0.0;                                // Monte-Carlo plans: the uniform prior
    unsigned long long *clkbuf = MC ? A.cold->clk : nullptr;
    const ClkStamp clk0 = clk_begin(clkbuf);

    // ---- per-thread graph slices (registers, loaded once) ----
    const bool has_check = in_team && member < m;
    int coff[CDEG];
#pragma unroll
    for (int k = 0; k < CDEG; k++) {
        // coff[k]: where the posterior of the row's k-th column lives in V.  It is the column itself, except under OWN: a thread keeps its two posteriors at
        // member and member + TS, as without ownership (lane-contiguous, conflict-free stores), and the record names those places to the four gathers
        coff[k] = ALL ? (k & 1) : 0;
        if (has_check) coff[k] = !OWN ? A.indices[A.indptr[member] + k] : (k < NOWN) ? member + k * TS : A.own[member * kRegOwnWords + kRegOwnGather + k - NOWN];
    }
    // the column behind the row's k-th edge / behind the thread's v-th posterior (OWN: read from the record where needed, once or twice per shot, not kept in registers)
    auto ecol = [&](int k) { return OWN ? A.own[member * kRegOwnWords + kRegOwnCols + k] : coff[k]; };
    unsigned cnf = 0u;                                     // bit k: the prior of the row's k-th column is not finite (see minsum_common.h)
    if (!NANFREE && !DAMP) {
#pragma unroll
        for (int k = 0; k < CDEG; k++) if (has_check && prior_not_finite(A.prior[coff[k]])) cnf |= 1u << k;
    }
    const int roff = has_check ? member * RST : 0;
    bool has_var[2], vlast[2];
    int vj[2], voff[2][VDEG];
    double vprior[2];
#pragma unroll
    for (int v = 0; v < 2; v++) {
        const int j = member + v * TS;                                     // the posterior's place in V; the column itself unless OWN (vcol below)
        has_var[v] = in_team && j < n;
        vlast[v] = false;
        vj[v] = has_var[v] ? j : (ALL ? v : 0);
        vprior[v] = has_var[v] ? A.prior[OWN ? ecol(v) : j] : 0.0;
#pragma unroll
        for (int d = 0; d < VDEG; d++) {
            voff[v][d] = ALL ? d : 0;
            if (OWN) {
                // the two other messages of the column in ascending check order (voff[v][2] is not read); `last`: the own message is the third addend
                if (has_var[v] && d < 2) voff[v][d] = A.own[member * kRegOwnWords + kRegOwnOffs + 2 * v + d];
                if (has_var[v] && d == 0) vlast[v] = (A.own[member * kRegOwnWords + kRegOwnLast] >> v) & 1;
            } else if (has_var[v]) {
                const int k = A.colptr[j] + d, row = A.rowidx[k];
                voff[v][d] = row * RST + (A.csc2csr[k] - A.indptr[row]);
            }
        }
    }

    auto vcol = [&](int v) { return OWN ? ecol(v) : vj[v]; };             // OWN: the owned columns are edges 0 and 1 of the reordered row

    // PLACE: every LDS address of the posteriors and the messages comes from the thread's place record (regular_place.h), in doubles from the start of the
    // workgroup's LDS and loaded once; the slot-relative Rl / Vl / roff / coff / voff / vj and the redirection of the lanes of no team to Dl are not used by
    // this form (a lane of no team has places of its own in the record, or the dummy region's where the table holds the linear layout).  The kernel's
    // edges 2 .. 5 are whatever the four posterior gathers read: the same order in Rprev and in the message stores, any order for the check update.
    double *Lb = reinterpret_cast<double *>(lds);
    int pgat[CDEG], mgat[4], msto[4];       // pgat[k]: the posterior of edge k (k < NOWN: where the thread stores its own), mgat[2 v + d]: the two other messages of owned column v, msto[k - NOWN]: the row word of edge k
#pragma unroll
    for (int k = 0; k < CDEG; k++) pgat[k] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { mgat[k] = 0; msto[k] = 0; }
    if (PLACE) {
        static_assert(kRegPlaceWords == 16, "a record is four 16-byte loads");
        const int4 *rec4 = reinterpret_cast<const int4 *>(A.place) + (size_t)threadIdx.x * 4;
        const int4 r0 = rec4[0], r1 = rec4[1], r2 = rec4[2], r3 = rec4[3];
        const int pr[kRegPlaceWords] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
#pragma unroll
        for (int k = 0; k < CDEG; k++) pgat[k] = (k < NOWN) ? pr[kRegPlacePostStore + k] : pr[kRegPlacePostGather + k - NOWN];
#pragma unroll
        for (int k = 0; k < 4; k++) { mgat[k] = pr[kRegPlaceMsgGather + k]; msto[k] = pr[kRegPlaceMsgStore + k]; }
    }
    auto Vof = [&](int k) -> double & { return PLACE ? Lb[pgat[k]] : Vl[coff[k]]; };                   // the posterior of the row's k-th column
    auto Vmine = [&](int v) -> double & { return PLACE ? Lb[pgat[v]] : Vl[vj[v]]; };                   // the v-th posterior the thread writes
    auto Rin = [&](int v, int d) -> double & { return PLACE ? Lb[mgat[2 * v + d]] : Rl[voff[v][d]]; }; // the d-th message into it (OWN: d < 2, the other two)
    double *const rowp = PLACE ? Lb : Rl + roff;                                                     // the row words: rowp[k - NOWN], PLACE: rowp[msto[k - NOWN]]
    const int *const rowat = PLACE ? msto : nullptr;

    // a shot list (the shots the bit-sliced first iteration, mc_first.hip, did not finish) replaces the contiguous range
    const int64_t nshots = (MC && A.shot_list) ? (int64_t)*A.shot_count : A.B;
    for (int64_t base = (int64_t)blockIdx.x * S; base < nshots; base += (int64_t)gridDim.x * S) {
        const int64_t b = base + slot;
        const bool valid = in_team && b < nshots;
        bool csyn = false;
        // PLACE, Monte-Carlo: the columns of the thread's check, for the syndrome and, the first two, for the logical comparison at the freeze.  The record
        // is the same for every shot, but 64 VGPRs leave no room to keep it across the bare loop, so a shot reads it again -- here, in front of the sampler,
        // whose arithmetic hides the latency.  Read where they are used, the loads stood behind a barrier each (the sampler's, and at the freeze the check
        // phase's) with the whole workgroup waiting for a spilled pointer, the record and then the byte or the mask it names: profiles/r31_opening.txt.
        // The other forms read the record where they use it: their code objects do not move.
        constexpr bool EARLY_COLS = MC && PLACE;
        struct Cols { int c[CDEG]; };
        struct NoCols { int c[2]; };            // never touched
        std::conditional_t<EARLY_COLS, Cols, NoCols> ecs;
        if constexpr (EARLY_COLS) {
#pragma unroll
            for (int k = 0; k < CDEG; k++) ecs.c[k] = 0;
            if (valid && has_check) {
#pragma unroll
                for (int k = 0; k < CDEG; k++) ecs.c[k] = ecol(k);
            }
        }
        if (MC) {
            // ---- sample e ~ Bernoulli(p)^n (4 bits per Philox block), s = H e ----
            if (valid && member < nq) {
                const uint64_t g = (uint64_t)(A.shot_begin + (A.shot_list ? (int64_t)A.shot_list[b] : b));
                uint32_t o[4];
                philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)member, 0u, A.seed_lo, A.seed_hi, o);
                uint32_t w = 0;
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (4 * member + t < n && o[t] < A.thr) w |= 1u << (8 * t);
                El[member] = w;
            }
            if (in_team && member == 0) { sres[0] = 0; sres[1] = 0; sres[2] = 0; sres[3] = -1; *lacc = 0ull; }
            if (threadIdx.x == 0) active[1] = 0;
            __syncthreads();
            const uint8_t *Eb = reinterpret_cast<const uint8_t *>(El);
            if (valid && has_check) {
                int s = 0;
#pragma unroll
                for (int k = 0; k < CDEG; k++) {
                    if constexpr (EARLY_COLS) s ^= Eb[ecs.c[k]];
                    else s ^= Eb[ecol(k)];
                }
                csyn = s & 1;
                if (csyn) sres[2] = 1;
            }
        } else {
            csyn = (valid && has_check) ? (A.synd[b * m + member] & 1) : false;
        }
        // the two owned columns for the freeze, in one register across the passes before it (n <= 2 * QLDPC_LB_T: 16 bits each)
        int cols01 = 0;
        if constexpr (EARLY_COLS) cols01 = ecs.c[0] | (ecs.c[1] << 16);
        const unsigned synw = csyn ? 0x80000000u : 0u;       // the syndrome bit as the sign bit of a word: sign of 1 - 2 s (kernels.py:252,289)
        double Rprev[CDEG], Qold[CDEG];
#pragma unroll
        for (int k = 0; k < CDEG; k++) { Rprev[k] = 0.0; Qold[k] = 0.0; }
#pragma unroll
        for (int v = 0; v < 2; v++) if (ALL || has_var[v]) Vmine(v) = vprior[v];      // Q_{-1} = prior[col] (kernels.py:263-265)
        double Vown[2] = {vprior[0], vprior[1]};                                        // OWN: what this thread last wrote to Vl[vj[v]]; the check phase gathers it from here (re-reading it from LDS measured 9 % slower)
        if (in_team && member == 0) { unsat[0] = 0; unsat[1] = 0; }
        if (threadIdx.x == 0) { const int64_t left = nshots - base; active[0] = (int)(left < S ? left : S); }
        bool done = !valid;
        __syncthreads();

        int it = 0;
        for (; it <= max_iter; it++) {
            // ======== check phase: syndrome test of values_{it-1}, then R_it from Q_{it-1} ========
            const bool in_check = ALL ? (FIXED || !done) : (FIXED ? valid : !done) && has_check;
            double x[CDEG];
            if (in_check) {
                bool par = csyn;
                if (CLIPMIN) {                                        // clean inputs: a posterior is never -0.0 (header comment), so x < 0 <=> its sign bit: one XOR per edge
                    unsigned ph = synw;
#pragma unroll
                    for (int k = 0; k < CDEG; k++) { x[k] = (OWN && k < NOWN) ? Vown[k] : Vof(k); ph ^= (unsigned)__double2hiint(x[k]); }
                    par = (int)ph < 0;                                                            // kernels.py:349,356
                } else {
#pragma unroll
                    for (int k = 0; k < CDEG; k++) { x[k] = Vl[coff[k]]; par ^= (x[k] < 0.0); }   // kernels.py:349,356
                }
                if (it >= 1 && !done && par) unsat[it & 1] = 1;                               // kernels.py:357-359
            }
            // Reference semantics, iteration 1: at BASELINE's error rates ~97 % of the shots pass the syndrome test of values_0 here, and the
            // messages of iteration 1 computed alongside the test (the fused form below) are thrown away for them -- a quarter of all the
            // instructions a shot costs (PMC: 372 VALU wave-instructions per shot, profiles/r02a_pmc.txt).  One extra barrier at it == 1 lets
            // a team see its verdict first and skip them; later iterations keep the fused form (a team still running there is rarely done).
            bool skip_msg = false;
            if (!FIXED && it == 1) {
                __syncthreads();
                skip_msg = (unsat[1] == 0);
            }
            if (MC && NANFREE && !DAMP && it == 0) {
                // Monte-Carlo plans decode against a UNIFORM prior p0 (code capacity, alpha.py:119-120), so iteration 0 is a closed form: every
                // variable-to-check message is p0 (kernels.py:263-265, unclipped), hence min1 = min2 = |p0| and the sign of an edge's
                // message is the syndrome sign times the signs of the other CDEG - 1 inputs: msg = +-(alpha_0 * |p0|), the same single
                // rounding as the general form below.  Saves the gather, the min network and the selects: ~60 of the ~290 instructions a
                // converging shot costs under reference semantics.
                if (in_check && max_iter > 0) {
                    const double p0 = prior0;
                    const bool sneg = csyn != ((((CDEG - 1) & 1) != 0) && (p0 < 0.0));
                    const double mag = Al[0] * fabs(p0);
                    const double msg = sneg ? -mag : mag;
#pragma unroll
                    for (int k = 0; k < CDEG; k++) { Rprev[k] = msg; if (k >= NOWN) rowp[PLACE ? msto[k - NOWN] : k - NOWN] = msg; }
                }
            } else if (in_check && !skip_msg) {
                if (CLIPMIN && it < max_iter) {
                    // compare-free form (header comment); iteration 0 reads priors: no clip (kernels.py:263-265)
                    clean_messages<CDEG, NOWN>(x, Rprev, it > 0, Al[it], (it > 0) ? clip : INFINITY, synw, rowp, rowat);
                } else if (it < max_iter) {
                    const double alpha = Al[it];
                    if (it > 0) {
#pragma unroll
                        for (int k = 0; k < CDEG; k++) {
                            double t = x[k] - Rprev[k];                                        // kernels.py:325
                            if (!NANFREE) t = (t != t) ? 0.0 : t;                              // kernels.py:328-329
                            t = vmax(vmin(t, clip), nclip);                                    // kernels.py:330-333
                            if (DAMP) {                                                        // kernels.py:336-342
                                const double qd = damping * t + one_minus_d * Qold[k];
                                t = NANFREE ? vmax(vmin(qd, clip), nclip) : clip_only(qd, clip);       // a NaN (from a NaN Q_old) must survive the clip
                            }
                            if (!NANFREE && !DAMP && ((cnf >> k) & 1u)) t = NAN;               // kernels.py:336 with Q_old = +-inf
                            x[k] = t;
                        }
                    }
                    bool neg[CDEG];
                    bool sp = csyn;                                                            // sign of 1 - 2 s (kernels.py:252,289)
#pragma unroll
                    for (int k = 0; k < CDEG; k++) {
                        if (DAMP) Qold[k] = x[k];
                        neg[k] = NANFREE ? (x[k] < 0.0) : !(x[k] >= 0.0);                      // kernels.py:296-299 (-0.0 counts as >= 0)
                        sp ^= neg[k];
                    }
                    double min1, min2;
                    if (NANFREE) {
                        two_smallest_abs<CDEG>(x, min1, min2);                                 // kernels.py:301-306
                    } else {                                   // NaN-tolerant form: NaN magnitudes are ignored like `abs_val < min1`
                        min1 = INFINITY; min2 = INFINITY;
#pragma unroll
                        for (int k = 0; k < CDEG; k++) {
                            const double a = fabs(x[k]);
                            if (a < min1) { min2 = min1; min1 = a; } else if (a < min2) { min2 = a; }
                        }
                    }
                    // the first minimum gets min2, everybody else min1 (kernels.py:313).  If the minimum is attained twice,
                    // min2 == min1, so selecting on |q| == min1 gives the same value at every position.
                    const double p1 = alpha * min1, p2 = alpha * min2;                         // (+-alpha)*mag == +-(alpha*mag)
                    const int p1lo = __double2loint(p1), p1hi = __double2hiint(p1), p2lo = __double2loint(p2), p2hi = __double2hiint(p2);
#pragma unroll
                    for (int k = 0; k < CDEG; k++) {
                        const bool eq = (fabs(x[k]) == min1);
                        const int lo = eq ? p2lo : p1lo;
                        const int hi = (eq ? p2hi : p1hi) ^ ((sp != neg[k]) ? (int)0x80000000 : 0);   // kernels.py:311-314
                        const double msg = __hiloint2double(hi, lo);
                        Rprev[k] = msg;
                        Rl[roff + k] = msg;
                    }
                }
            }
            __syncthreads();
            // ======== variable phase: freeze test, then values_it ========
            if (valid && !done) {
                const bool conv = (it >= 1) && (unsat[it & 1] == 0);                           // kernels.py:361-364
                if (conv || it == max_iter) {
                    done = true;
                    if (MC) {
                        const bool exportit = !conv && A.use_osd;
                        if (!exportit) {
                            const uint8_t *Eb = reinterpret_cast<const uint8_t *>(El);
                            unsigned long long lm = 0ull;
#pragma unroll
                            for (int v = 0; v < 2; v++) {
                                int col;                                                           // the owned columns are edges 0 and 1 of the check
                                if constexpr (EARLY_COLS) {
                                    int packed = cols01;
                                    asm volatile("" : "+v"(packed));                               // unpacked here: two addresses hoisted out of the loop would cost it a spill
                                    col = (packed >> (16 * v)) & 0xffff;
                                }
                                else col = vcol(v);
                                if (has_var[v] && ((Eb[col] ^ ((it >= 1 && Vmine(v) < 0.0) ? 1 : 0)) & 1)) lm ^= A.Lmask[col];   // V still holds values_{it-1}
                            }
                            if (lm) atomicXor(lacc, lm);
                        } else if (member == 0) {
                            active[1] = 1;
                        }
                        if (member == 0) { sres[0] = conv ? 1 : 0; sres[1] = conv ? it - 1 : max_iter - 1; atomicSub(&active[0], 1); }
                    } else {
#pragma unroll
                        for (int v = 0; v < 2; v++)
                            if (has_var[v]) {
                                const double xo = (it >= 1) ? Vmine(v) : 0.0;        // V still holds values_{it-1}
                                A.out_llr[b * n + vcol(v)] = xo;
                                A.out_err[b * n + vcol(v)] = (xo < 0.0) ? 1 : 0;               // kernels.py:349
                            }
                        if (member == 0) {
                            A.out_conv[b] = conv ? 1 : 0;
                            A.out_iter[b] = conv ? it - 1 : max_iter - 1;                      // kernels.py:267,362
                            atomicSub(&active[0], 1);
                        }
                    }
                }
            }
            if (in_team && member == 0) unsat[(it + 1) & 1] = 0;
            if (it < max_iter && (ALL ? (FIXED || !done) : (FIXED ? valid : !done))) {
#pragma unroll
                for (int v = 0; v < 2; v++)
                    if (ALL || has_var[v]) {
                        double s = 0.0;                                                        // kernels.py:279
                        if (OWN) {
                            const double o1 = Rin(v, 0), o2 = Rin(v, 1), own = Rprev[v];
                            s = ZEROFREE ? o1 : s + o1;                                        // clean forms start at the first message (header comment, "zero")
                            s += vlast[v] ? o2 : own; s += vlast[v] ? own : o2;                // ascending check order (regular_own.h)
                        } else {
#pragma unroll
                            for (int d = 0; d < VDEG; d++) s = (ZEROFREE && d == 0) ? Rl[voff[v][0]] : s + Rl[voff[v][d]];   // kernels.py:316, ascending check order
                        }
                        const double xv = s + vprior[v];                                       // kernels.py:320
                        Vmine(v) = xv;
                        Vown[v] = xv;
                    }
            }
            __syncthreads();
            if ((!FIXED || ALL) && active[0] == 0) { it++; break; }       // block-uniform: early exit is finished; fixed work goes on below
        }
        if (ALL && FIXED) {
            // Every shot of the workgroup is frozen (a workgroup that holds a BP failure never gets here before it == max_iter): nothing computed from
            // here on is observable, and the remaining passes keep the arithmetic of a pass -- gather, hard-decision parity, message update, variable
            // update -- without its control: no unsat word, no freeze test, no `done`, no first-iteration case (it >= 2 here).  The parities are kept
            // alive by one OR per pass and one store per shot into the dummy region.
            unsigned parity = 0u;
            // alpha_it travels in scalar registers: the pass's own alpha was loaded during the pass before it (the first one comes from the staged table),
            // so no pass reads Al from LDS; the table A.alpha is never written by a kernel, hence the constant address space
            const __attribute__((address_space(4))) double *alpha_tab = (const __attribute__((address_space(4))) double *)A.alpha;
            double alpha_it = (it < max_iter) ? Al[it] : 0.0;
            // PLACE: the variable sums of a pass come in two forms, picked per WAVE (wave_class is wave-uniform, regular_place.h).  A wave whose team lanes
            // all own no `last` edge adds (o1 + own) + o2 for both columns without a select -- the common wave, seven of eight on bb144; every other wave
            // keeps the two selects per column.  How it is written decides what the common wave pays.  An if / else on the class comes out of the
            // compiler's control-flow structurizer as two guarded blocks and a flag, four scalar branches per pass for every wave
            // (profiles/r27_wave_classes.txt).  An `if` WITHOUT an else survives it as one forward branch: so the select-free sums are written
            // unconditionally and the form with selects overwrites them under the test.  The sums have no other use, so the code generator sinks them
            // onto the fall-through edge: the "none" wave runs test, not-taken branch, four adds, and no wave computes a sum twice
            // (profiles/r30_one_path.txt has the disassembly's counts).  The other arm sits out of line behind the taken branch and jumps back; both arms
            // lie between the same two barriers.  The test reads a copy of the class that an empty asm makes opaque in every pass: a scalar compare in
            // the pass itself, where a hoisted comparison is kept as a 64-bit lane mask in two scalar registers.  The empty asm inside the arm keeps it
            // from being folded into selects on the class.
            if constexpr (PLACE) {
                // the first alpha from the constant table too (the staged copy is the same words): the loop-carried alpha is then a scalar pair, no pass
                // moves it into a vector register, and the back-edge is the loop's one branch besides the class test
                it = __builtin_amdgcn_readfirstlane(it);
                // a 32-bit byte offset from the table's base: the scalar load takes it as its offset register, no 64-bit address arithmetic per pass
                auto alpha_at = [&](int i) {
                    return *reinterpret_cast<const __attribute__((address_space(4))) double *>(reinterpret_cast<const __attribute__((address_space(4))) char *>(alpha_tab) + (unsigned)i * 8u);
                };
                if (it < max_iter) alpha_it = alpha_at(it);
                for (; it < max_iter; it++) {
                    double x[CDEG];
                    unsigned ph = synw;
#pragma unroll
                    for (int k = 0; k < CDEG; k++) x[k] = (k < NOWN) ? Vown[k] : Vof(k);
#pragma unroll
                    for (int k = 0; k < CDEG; k++) ph ^= (unsigned)__double2hiint(x[k]);           // kernels.py:349,356
                    parity |= ph;
                    clean_messages<CDEG, NOWN>(x, Rprev, true, alpha_it, clip, synw, rowp, rowat);
                    __syncthreads();
                    __builtin_amdgcn_s_setprio(1);                                                 // the short LDS-only phase that releases the barrier goes first (measured: profiles/r18_bare_loop.txt)
                    double o[2][2], s[2];                                                          // o[v] = the two other messages of owned column v in ascending check order (regular_own.h)
#pragma unroll
                    for (int v = 0; v < 2; v++)
#pragma unroll
                        for (int d = 0; d < 2; d++) o[v][d] = Rin(v, d);
#pragma unroll
                    for (int v = 0; v < 2; v++) s[v] = (o[v][0] + Rprev[v]) + o[v][1];             // kernels.py:316 with the own message second or first ("zero")
                    int cls = wave_class;
                    asm volatile("" : "+s"(cls));
                    if (__builtin_expect(cls != kRegWaveNone, 0)) {
                        asm volatile("");
#pragma unroll
                        for (int v = 0; v < 2; v++) s[v] = (o[v][0] + (vlast[v] ? o[v][1] : Rprev[v])) + (vlast[v] ? Rprev[v] : o[v][1]);
                    }
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        // kernels.py:320.  A Monte-Carlo plan's prior is uniform (the closed form of iteration 0 above rests on it), so there the addend is the
                        // scalar prior0: four VGPRs less across the loop.  A lane of no team adds prior0 where vprior holds 0.0; nothing reads its sum.
                        Vown[v] = s[v] + (MC ? prior0 : vprior[v]);
                        Vmine(v) = Vown[v];
                    }
                    __builtin_amdgcn_s_setprio(0);
                    // the next pass's alpha, clamped (the table has max_iter entries): a uniform address, and the barrier below waits for LDS anyway
                    alpha_it = alpha_at(it + 1 < max_iter ? it + 1 : max_iter - 1);
                    __syncthreads();
                }
            } else {
            // the forms without a place table: the pass as it stands in the source since profiles/r18_bare_loop.txt, so that their code objects do not move
            for (; it < max_iter; it++) {
                double x[CDEG];
                unsigned ph = synw;
#pragma unroll
                for (int k = 0; k < CDEG; k++) x[k] = (OWN && k < NOWN) ? Vown[k] : Vof(k);
#pragma unroll
                for (int k = 0; k < CDEG; k++) ph ^= (unsigned)__double2hiint(x[k]);               // kernels.py:349,356
                parity |= ph;
                clean_messages<CDEG, NOWN>(x, Rprev, true, alpha_it, clip, synw, rowp, rowat);
                __syncthreads();
                __builtin_amdgcn_s_setprio(1);
                double r[2][VDEG];
#pragma unroll
                for (int v = 0; v < 2; v++)
#pragma unroll
                    for (int d = 0; d < VDEG - (OWN ? 1 : 0); d++) r[v][d] = Rin(v, d);
#pragma unroll
                for (int v = 0; v < 2; v++) {
                    if (OWN) {
                        const double o2 = r[v][1], own = Rprev[v];
                        r[v][1] = vlast[v] ? o2 : own;
                        r[v][2] = vlast[v] ? own : o2;
                    }
                    double s = 0.0;                                                                // kernels.py:279
#pragma unroll
                    for (int d = 0; d < VDEG; d++) s = (ZEROFREE && d == 0) ? r[v][0] : s + r[v][d];   // kernels.py:316
                    Vown[v] = s + vprior[v];                                                       // kernels.py:320
                    Vmine(v) = Vown[v];
                }
                __builtin_amdgcn_s_setprio(0);
                alpha_it = alpha_tab[it + 1 < max_iter ? it + 1 : max_iter - 1];
                __syncthreads();
            }
            }
            if (it == max_iter) {                                                                  // the syndrome test of values_{max_iter-1}
                unsigned ph = synw;
#pragma unroll
                for (int k = 0; k < CDEG; k++) ph ^= (unsigned)__double2hiint(Vof(k));
                parity |= ph;
            }
            reinterpret_cast<unsigned *>(Dl + RST + 2)[0] = parity;
        }
        __syncthreads();
        if (MC) {
            if (active[1]) {                        // block-uniform: some shot needs OSD-0 -> export its record
                const RegCold C = *A.cold;
                if (valid && member == 0 && sres[0] == 0 && A.use_osd) {
                    const int f = atomicAdd(C.fail_count, 1);
                    sres[3] = f;
                    C.fail_list[f] = f;
                }
                __syncthreads();
                const int f = valid ? sres[3] : -1;
                if (f >= 0) {
                    const uint8_t *Eb = reinterpret_cast<const uint8_t *>(El);
                    if (has_check) C.f_synd[(int64_t)f * m + member] = csyn ? 1 : 0;
#pragma unroll
                    for (int v = 0; v < 2; v++)
                        if (has_var[v]) {
                            const double xo = (max_iter >= 1) ? Vmine(v) : 0.0;
                            C.f_llr[(int64_t)f * n + vcol(v)] = xo;
                            C.f_hard[(int64_t)f * n + vcol(v)] = (xo < 0.0) ? 1 : 0;
                            C.f_err[(int64_t)f * n + vcol(v)] = (int8_t)Eb[vcol(v)];
                        }
                }
                __syncthreads();
            }
            if ((int)threadIdx.x < S && base + threadIdx.x < nshots) {
                const int *r = I + 2 * S + 2 + 4 * threadIdx.x;
                const unsigned long long lm = *(reinterpret_cast<unsigned long long *>(lds + A.offL) + threadIdx.x);
                const bool exported = (r[0] == 0) && A.use_osd;
                atomicAdd(&Tl[0], 1ull);
                if (r[0]) atomicAdd(&Tl[2], 1ull);
                atomicAdd(&Tl[3], (unsigned long long)(r[1] + 1));
                if (!r[2]) atomicAdd(&Tl[4], 1ull);
                if (!exported) { if (lm) atomicAdd(&Tl[1], 1ull); if (!r[0]) atomicAdd(&Tl[5], 1ull); }
            }
            __syncthreads();
        }
    }
    if (MC) clk_end(clkbuf, clk0);
    if (MC && threadIdx.x < 6 && Tl[threadIdx.x]) {
        unsigned long long *tally = A.cold->tally;
        const unsigned long long v = Tl[threadIdx.x];
        const int slotmap[6] = {QLDPC_TALLY_TRIALS, QLDPC_TALLY_Z_ERR, QLDPC_TALLY_BP_CONV_Z, QLDPC_TALLY_ITERS_Z, QLDPC_TALLY_ZERO_SYND_Z, QLDPC_TALLY_UNSAT_Z};
        atomicAdd(&tally[slotmap[threadIdx.x]], v);
        if (threadIdx.x == 1) atomicAdd(&tally[QLDPC_TALLY_TOTAL_ERR], v);
    }
}

// judge of the exported failures after OSD-0: logical error / unsat / OSD count (32 lanes per record, device-side count)
// reset != 0: the LAST workgroup to finish zeroes the piece's counters (count[0] failures, count[2] shots the first iteration handed on; count[3] counts
// finished workgroups) -- every workgroup reads `total` before it can be counted as finished, so the next piece on this lane needs no memset from the host
__global__ __launch_bounds__(256) void cc_judge_failed_kernel(int32_t *__restrict__ count, int reset, int *__restrict__ osd_queue, int m, int n,
                                                              const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                              const uint64_t *__restrict__ Lmask, const int8_t *__restrict__ err,
                                                              const int8_t *__restrict__ synd, const int8_t *__restrict__ dec,
                                                              unsigned long long *__restrict__ tally) {
    const int total = *count;
    const int lane = threadIdx.x & 31;
    unsigned long long nerr = 0, nbad = 0;
    for (int64_t b = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); b < total; b += (int64_t)gridDim.x * 8) {
        const int8_t *e = err + b * n, *d = dec + b * n, *s = synd + b * m;
        uint64_t lm = 0;
        for (int j = lane; j < n; j += 32)
            if ((e[j] ^ d[j]) & 1) lm ^= Lmask[j];
        int bad = 0;
        for (int i = lane; i < m; i += 32) {
            int p = 0;
            for (int k = indptr[i]; k < indptr[i + 1]; k++) p ^= d[indices[k]];
            bad |= ((p ^ s[i]) & 1);
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) { lm ^= __shfl_xor(lm, off, 32); bad |= __shfl_xor(bad, off, 32); }
        if (lane == 0) { nerr += lm ? 1 : 0; nbad += bad ? 1 : 0; }
    }
    if (lane == 0) {
        if (nerr) { atomicAdd(&tally[QLDPC_TALLY_Z_ERR], nerr); atomicAdd(&tally[QLDPC_TALLY_TOTAL_ERR], nerr); }
        if (nbad) atomicAdd(&tally[QLDPC_TALLY_UNSAT_Z], nbad);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && total) atomicAdd(&tally[QLDPC_TALLY_OSD_Z], (unsigned long long)total);
    if (reset) {
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            if (atomicAdd(&count[3], 1) == (int)gridDim.x - 1) { count[0] = 0; count[2] = 0; count[3] = 0; if (osd_queue) *osd_queue = 0; __threadfence(); }
        }
    }
}

// ------------------------------------------------------------------------------------------ host side
// RegPlan and the carve itself: regular_plan.h (host arithmetic only)
static int g_list_shots = 0;          // qldpc_set_option("mc_list_shots"): shots per workgroup of the shot-list launch (0 = as the full launch)
void regular_set_list_shots(int s) { g_list_shots = s; }
static std::atomic<int> g_own_edges{1};   // qldpc_set_option("regular_own_edges"): 1 = the clean (6,3) form keeps two edges of each check inside its thread (regular_own.h)
void regular_set_own_edges(int v) { g_own_edges = v; }

static bool plan_regular(const qldpc_graph *g, int max_iter, RegPlan &P, int force_S = 0) {
    if (g->m <= 0 || g->n <= 0) return false;
    const int cdeg = g->max_row_deg, vdeg = g->max_col_deg;
    for (int i = 0; i < g->m; i++) if (g->indptr[i + 1] - g->indptr[i] != cdeg) return false;
    for (int j = 0; j < g->n; j++) if (g->colptr[j + 1] - g->colptr[j] != vdeg) return false;
    return plan_regular_shape(cdeg, vdeg, g->m, g->n, max_iter, QLDPC_LB_T, force_S, P);
}

bool regular_supported(const qldpc_graph *g, double clip, int max_iter) {
    RegPlan P;
    return clip >= 0.0 && plan_regular(g, max_iter, P);
}

template <int CDEG, int VDEG, bool MC, bool FIXED>
static int launch_reg2(const RegArgs &A, bool damp, bool nanfree, unsigned grid, unsigned block, size_t lds, hipStream_t stream) {
    if (damp) {
        if (MC) return QLDPC_ERR_UNSUPPORTED;
        hipLaunchKernelGGL((minsum_regular_kernel<CDEG, VDEG, true, false, false, FIXED>), dim3(grid), dim3(block), lds, stream, A);
    } else if (nanfree && A.clip > 0.0) {             // the clean form folds the clip into its two chain seeds: exact for clip > 0 only (inputs_clean() has checked it; kept next to the launch)
        if constexpr (CDEG == kRegOwnCdeg && VDEG == kRegOwnVdeg) {
            if (A.own && (A.place || !FIXED)) {          // the fixed-work form reads its place table (regular_place_table), the early-exit form has none
                hipLaunchKernelGGL((minsum_regular_kernel<CDEG, VDEG, false, true, MC, FIXED, true>), dim3(grid), dim3(block), lds, stream, A);
                QLDPC_HIP_TRY(hipGetLastError());
                return QLDPC_OK;
            }
        }
        hipLaunchKernelGGL((minsum_regular_kernel<CDEG, VDEG, false, true, MC, FIXED>), dim3(grid), dim3(block), lds, stream, A);
    } else {
        hipLaunchKernelGGL((minsum_regular_kernel<CDEG, VDEG, false, false, MC, FIXED>), dim3(grid), dim3(block), lds, stream, A);
    }
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

template <int CDEG, int VDEG, bool MC>
static int launch_reg(const RegArgs &A, bool damp, bool nanfree, unsigned grid, unsigned block, size_t lds, hipStream_t stream) {
    return A.fixed ? launch_reg2<CDEG, VDEG, MC, true>(A, damp, nanfree, grid, block, lds, stream)
                   : launch_reg2<CDEG, VDEG, MC, false>(A, damp, nanfree, grid, block, lds, stream);
}

template <bool MC>
static int dispatch_reg(const RegPlan &P, const RegArgs &A, bool damp, bool nanfree, unsigned grid, hipStream_t stream) {
    if (P.cdeg == 6) return launch_reg<6, 3, MC>(A, damp, nanfree, grid, P.block, P.lds, stream);
    if (P.cdeg == 4) return launch_reg<4, 2, MC>(A, damp, nanfree, grid, P.block, P.lds, stream);
    return launch_reg<8, 4, MC>(A, damp, nanfree, grid, P.block, P.lds, stream);
}

static void fill_common(const qldpc_graph *g, const RegPlan &P, RegArgs &A, int64_t B, const double *d_prior, int max_iter,
                        const double *d_alpha, double damping, double clip, int flags) {
    A = RegArgs{};
    A.m = g->m; A.n = g->n; A.max_iter = max_iter; A.fixed = (flags & QLDPC_FLAG_FIXED_ITERS) ? 1 : 0;
    A.S = P.S; A.TS = P.TS;
    A.indptr = g->d_indptr; A.indices = g->d_indices; A.colptr = g->d_colptr; A.rowidx = g->d_rowidx; A.csc2csr = g->d_csc2csr;
    A.own = (g_own_edges.load() && P.cdeg == kRegOwnCdeg) ? g->d_regown : nullptr;      // NULL too where the graph has no assignment (graph.hip)
    A.B = B; A.prior = d_prior; A.alpha = d_alpha; A.damping = damping; A.clip = clip;
    A.offV = P.offV; A.offE = P.offE; A.offL = P.offL; A.offI = P.offI; A.offA = P.offA; A.offT = P.offT; A.offD = P.offD;
}

static std::atomic<int> g_place{1};       // qldpc_set_option("regular_place"): 1 = the ownership form takes its LDS addresses from the placement of regular_place.h, 0 = today's linear ones
void regular_set_place(int v) { g_place = v; }
static std::atomic<int> g_wave_classes{1};   // qldpc_set_option("regular_wave_classes"): 1 = a placed table is built from the min-last assignment under the thread order of regular_place_order
void regular_set_wave_classes(int v) { g_wave_classes = v; }

// The place table of the ownership form for this launch's workgroup shape, from the handle's cache (common.h); built and uploaded (a blocking copy) the
// first time the handle meets the shape.  The placement where the option asks for it and the header has one, else the linear layout as a table: the
// same kernel either way.  *own: the ownership table the place table was built from, which the launch must read with it -- the min-last assignment for a
// table with class-uniform waves ("regular_wave_classes" 1 and a placement), the bank-model assignment for every other.
static int regular_place_table(const qldpc_graph *g, const RegPlan &P, const int32_t **out, const int32_t **own) {
    *out = nullptr;
    *own = g->d_regown;
    if (g->regown.size() != (size_t)g->m * kRegOwnWords) { set_error("regular min-sum: the graph handle has no ownership table"); return QLDPC_ERR_INVALID; }
    const int rst = regular_row_stride(kRegOwnCdeg);
    std::lock_guard<std::mutex> lk(g->mu_place);
    // placed: 0 the linear layout, 1 the placement in the identity order, 2 the placement of the min-last table under a thread order
    auto find = [&](int placed, int offD) -> const qldpc_graph::PlaceEntry * {
        for (const auto &e : g->place_cache) if (e.S == P.S && e.block == (int)P.block && e.placed == placed && e.offD == offD) return &e;
        return nullptr;
    };
    auto add = [&](int placed, int offD, const std::vector<int32_t> &rec) -> int {
        qldpc_graph::PlaceEntry e;
        e.S = P.S; e.block = (int)P.block; e.placed = placed; e.offD = offD;
        if (!rec.empty()) { const int rc = upload(e.dev, rec); if (rc != QLDPC_OK) return rc; }
        g->place_cache.push_back(std::move(e));
        return QLDPC_OK;
    };
    std::vector<int32_t> rec;
    if (g_place.load()) {
        if (g_wave_classes.load() && g->d_regown_minlast && g->regown_minlast.size() == g->regown.size()) {
            if (!find(2, 0)) {
                RegPlaceOrder order;                                              // "none" leaves rec empty: the entry records that, so the build is not repeated
                if (regular_place_order(g->m, g->regown_minlast.data(), P, order)) regular_place_build(g->m, g->regown_minlast.data(), P, rst, rec, kRegPlaceOrderedMoves, &order);
                const int rc = add(2, 0, rec);
                if (rc != QLDPC_OK) return rc;
            }
            if (const auto *e = find(2, 0); e && e->dev.p) { *out = e->dev.as<int32_t>(); *own = g->d_regown_minlast; return QLDPC_OK; }
        }
        if (!find(1, 0)) {
            rec.clear();
            regular_place_build(g->m, g->regown.data(), P, rst, rec);
            const int rc = add(1, 0, rec);
            if (rc != QLDPC_OK) return rc;
        }
        if (const auto *e = find(1, 0); e && e->dev.p) { *out = e->dev.as<int32_t>(); return QLDPC_OK; }
    }
    if (!find(0, P.offD)) {
        regular_place_linear(g->m, g->regown.data(), P, rst, rec);
        const int rc = add(0, P.offD, rec);
        if (rc != QLDPC_OK) return rc;
    }
    *out = find(0, P.offD)->dev.as<int32_t>();
    return QLDPC_OK;
}

static unsigned persistent_grid(int64_t B, int S) {
    const int64_t groups = (B + S - 1) / S;
    const int64_t cap = 256 * 12;
    return (unsigned)(groups < cap ? (groups > 0 ? groups : 1) : cap);
}

int minsum_regular_launch(const qldpc_graph *g, int64_t B, const int8_t *d_synd, const double *d_prior, int max_iter,
                          const double *d_alpha, double damping, double clip, int flags, bool nanfree, int8_t *d_err, double *d_llr,
                          uint8_t *d_conv, int32_t *d_iter, hipStream_t stream) {
    RegPlan P;
    if (!plan_regular(g, max_iter, P)) { set_error("graph is not regular (6,3)/(4,2)/(8,4)"); return QLDPC_ERR_UNSUPPORTED; }
    RegArgs A;
    fill_common(g, P, A, B, d_prior, max_iter, d_alpha, damping, clip, flags);
    if (A.own && A.fixed && damping == 1.0 && nanfree && clip > 0.0) { const int rc = regular_place_table(g, P, &A.place, &A.own); if (rc != QLDPC_OK) return rc; }      // the launches that take the ownership form (launch_reg2)
    A.synd = d_synd; A.out_err = d_err; A.out_llr = d_llr; A.out_conv = d_conv; A.out_iter = d_iter;
    return dispatch_reg<false>(P, A, damping != 1.0, nanfree, persistent_grid(B, P.S), stream);
}

int mc_regular_launch(const qldpc_graph *g, int64_t B, const double *d_prior, int max_iter, const double *d_alpha, double clip, int flags,
                      bool nanfree, uint64_t seed, int64_t shot_begin, uint32_t thr, int use_osd, const uint64_t *d_Lmask,
                      void *d_cold, hipStream_t stream, const int32_t *d_shot_list, const int32_t *d_shot_count) {
    RegPlan P;
    // a shot list holds the few shots the first iteration did not finish; their iteration counts vary from 2 to max_iter, and a workgroup waits
    // for its slowest shot: fewer shots per workgroup there (mc_list_shots)
    if (!plan_regular(g, max_iter, P, d_shot_list ? g_list_shots : 0)) { set_error("graph is not regular (6,3)/(4,2)/(8,4)"); return QLDPC_ERR_UNSUPPORTED; }
    RegArgs A;
    fill_common(g, P, A, B, d_prior, max_iter, d_alpha, 1.0, clip, flags);
    if (A.own && A.fixed && nanfree && clip > 0.0) { const int rc = regular_place_table(g, P, &A.place, &A.own); if (rc != QLDPC_OK) return rc; }
    A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32); A.thr = thr; A.use_osd = use_osd; A.shot_begin = shot_begin;
    A.Lmask = d_Lmask; A.cold = reinterpret_cast<const RegCold *>(d_cold);
    A.shot_list = d_shot_list; A.shot_count = d_shot_count;
    // listed shots: a few percent of the batch at BASELINE's error rates -- a grid for B / 16 shots covers them in one or two rounds
    const unsigned grid = d_shot_list ? persistent_grid(std::max<int64_t>(B / 16, 1), P.S) * (unsigned)(g_list_shots > 0 ? 4 : 1) : persistent_grid(B, P.S);
    return dispatch_reg<true>(P, A, false, nanfree, grid, stream);
}

// Fills the device-resident cold-argument block of a Monte-Carlo plan (done once per plan).
int mc_regular_fill_cold(void *d_cold, unsigned long long *d_tally, int32_t *d_fail_count, int32_t *d_fail_list, int8_t *f_synd,
                         int8_t *f_err, int8_t *f_hard, double *f_llr, unsigned long long *d_clk) {
    RegCold C{d_tally, d_fail_count, d_fail_list, f_synd, f_err, f_hard, f_llr, d_clk};
    QLDPC_HIP_TRY(hipMemcpy(d_cold, &C, sizeof(C), hipMemcpyHostToDevice));
    return QLDPC_OK;
}
size_t mc_regular_cold_bytes() { return sizeof(RegCold); }

int judge_failed_launch(const qldpc_graph *g, int32_t *d_count, bool reset_counters, int *d_osd_queue, const uint64_t *d_Lmask, const int8_t *f_err, const int8_t *f_synd,
                        const int8_t *f_dec, unsigned long long *d_tally, hipStream_t stream) {
    hipLaunchKernelGGL(cc_judge_failed_kernel, dim3(64), dim3(256), 0, stream, d_count, reset_counters ? 1 : 0, d_osd_queue, g->m, g->n, g->d_indptr, g->d_indices, d_Lmask, f_err,
                       f_synd, f_dec, d_tally);
    QLDPC_HIP_TRY(hipGetLastError());
    return QLDPC_OK;
}

}  // namespace qldpc
