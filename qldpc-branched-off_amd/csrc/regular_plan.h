// Workgroup shape and LDS carve of the regular min-sum kernel (minsum_regular.hip): pure arithmetic, no HIP header, so a host program can print it
// (tests/regular_plan_main.cpp).  Byte offsets into the dynamic LDS of one workgroup of S teams of TS threads:
//   0     R     S * m * RST doubles   check-to-variable messages, one padded row of RST doubles per check
//   offV  V     S * n doubles         posteriors
//   offE  E     S * nq words          sampled errors, 4 columns per word (Monte-Carlo)
//   offL  L     S * 8 bytes           logical masks
//   offI  I     (6 S + 2) ints        unsat[2] per team, active[2], results[4] per team
//   offA  A     max_iter doubles      alpha_k
//   offT  T     6 * 8 bytes           block tally (Monte-Carlo)
//   offD  D     (RST + 3) doubles     dummy row, two dummy posteriors and a parity word: what the lanes of a block that belong to no team read and
//                                     write, so that the clean iteration body runs with every lane enabled (80 bytes for the (6,3) graphs)
#pragma once
#include <cstddef>

namespace qldpc {

struct RegPlan { int cdeg, vdeg, TS, S, offV, offE, offL, offI, offA, offT, offD; size_t lds; unsigned block; };

static const int kMaxIterLds = 1024;
static const int kRegularLdsTarget = 39 * 1024;     // 4 blocks per CU within 160 KiB, the dummy region not counted: it is under 100 bytes of the 1 KiB this leaves

inline int regular_row_stride(int cdeg) { return (cdeg % 2 == 0) ? cdeg + 1 : cdeg; }

// m checks of degree cdeg, n columns of degree vdeg (the caller has verified the degrees), team_threads = the block's thread budget.
inline bool plan_regular_shape(int cdeg, int vdeg, int m, int n, int max_iter, int team_threads, int force_S, RegPlan &P) {
    if (m <= 0 || n <= 0 || max_iter > kMaxIterLds) return false;
    if (!((cdeg == 6 && vdeg == 3) || (cdeg == 4 && vdeg == 2) || (cdeg == 8 && vdeg == 4))) return false;
    if (n != 2 * m) return false;                       // m * cdeg == n * vdeg with cdeg == 2 * vdeg: a thread owns one check and two columns, no lane of a team is idle
    const int ts = m;
    if (ts > team_threads) return false;
    const int rst = regular_row_stride(cdeg);
    const int nq = (n + 3) / 4;
    int S = team_threads / ts;                          // 4 blocks per CU fill its 32 wave slots
    if (force_S > 0 && force_S < S) S = force_S;
    auto layout = [&](int s) {
        P.offV = s * m * rst * 8;
        P.offE = P.offV + s * n * 8;
        P.offL = (P.offE + s * nq * 4 + 7) / 8 * 8;
        P.offI = P.offL + s * 8;
        P.offA = (P.offI + (6 * s + 2) * 4 + 7) / 8 * 8;
        P.offT = P.offA + (max_iter > 0 ? max_iter : 1) * 8;
        P.offD = P.offT + 6 * 8 + 16;
    };
    layout(S);
    while (S > 1 && P.offD > kRegularLdsTarget) { S--; layout(S); }
    P.lds = (size_t)P.offD + (size_t)((rst + 3) * 8 + 15) / 16 * 16;
    if (P.lds > 150 * 1024) return false;
    P.cdeg = cdeg; P.vdeg = vdeg; P.TS = ts; P.S = S;
    P.block = (unsigned)(((long long)S * ts + 63) / 64 * 64);
    return true;
}

}  // namespace qldpc
