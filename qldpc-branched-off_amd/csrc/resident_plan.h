// Team shape and LDS size of the resident min-sum kernel (minsum_resident.hip): pure arithmetic, no HIP header, so a host program can print it
// (tests/resident_plan_main.cpp).  One workgroup decodes S shots at a time, each by a team of TS threads; a thread owns cpt rows and vpt columns.
// The kernel carves the dynamic LDS itself, from (m, n, S) alone:
//   R      S * m * RST doubles    check-to-variable messages, one padded row of RST doubles per check
//   V      S * n doubles          posteriors
//   flags  (2 S + 2) ints         unsat[2] per team, active[2]
//   sres   4 S ints               (Monte-Carlo) conv, final iteration, non-zero syndrome, failure index per team; then padded to 8 bytes
//   lacc   S * 8 bytes            logical-row accumulators
//   T      6 * 8 bytes            block tally
//   E      S * nq * 4 bytes       sampled error bytes, nq = (n + 3) / 4
// per_slot below is what one shot adds to it; lds = S * per_slot + 96 covers the rest.
#pragma once
#include <algorithm>
#include <cstddef>

namespace qldpc {

struct ResidentPlan { int cdeg, vdeg, cpt, vpt, TS, S; size_t lds; unsigned block; };

static const int kResidentTeam = 1024;                   // threads of the largest team, and the budget S = kResidentTeam / TS is cut from
static const size_t kResidentShotBytes = 60 * 1024;      // one shot's share of the LDS
static const size_t kResidentLdsBudget = 64 * 1024;      // two workgroups per CU

inline int resident_row_stride(int cdeg) { return (cdeg % 2 == 0) ? cdeg + 1 : cdeg; }

// m checks of degree <= max_row_deg, n columns of degree <= max_col_deg, nnz edges
inline bool plan_resident_shape(int m, int n, long long nnz, int max_row_deg, int max_col_deg, ResidentPlan &P) {
    if (m <= 0 || n <= 0 || nnz <= 0) return false;
    if (max_row_deg > 8 || max_col_deg > 4) return false;
    P.cdeg = max_row_deg <= 6 ? 6 : 8;
    P.vdeg = max_col_deg <= 3 ? 3 : 4;
    if (P.cdeg == 8 || P.vdeg == 4) { P.cdeg = 8; P.vdeg = 4; }
    const int rst = resident_row_stride(P.cdeg);
    const size_t per_slot = ((size_t)m * rst + n) * 8 + 8 + 16 + 8 + (size_t)((n + 3) / 4) * 4;      // R, V, flags + Monte-Carlo state (results, logical accumulator, error bytes)
    if (per_slot > kResidentShotBytes) return false;
    // one check / two variables per thread when the team then fits 256 threads, else two / four
    P.cpt = 1; P.vpt = 2;
    int ts = std::max(m, (n + 1) / 2);
    if (ts > 256) { P.cpt = 2; P.vpt = 4; ts = std::max((m + 1) / 2, (n + 3) / 4); }
    if (ts > kResidentTeam) return false;
    P.TS = ts;
    int S = kResidentTeam / ts;
    while (S > 1 && (size_t)S * per_slot + 96 > kResidentLdsBudget) S--;
    if (S < 1) return false;
    P.S = S;
    P.lds = (size_t)S * per_slot + 16 + 16 + 48 + 16;      // + active[2], the block tally, alignment
    P.block = (unsigned)(((long long)S * ts + 63) / 64 * 64);
    return true;
}

}  // namespace qldpc
