// Edge ownership for the (6,3) form of the regular min-sum kernel (minsum_regular.hip): pure C++, no HIP header, so a host program can print it
// (tests/regular_own_main.cpp, tests/regular_own_cost_main.cpp).
//
// The thread of check i is the variable thread of two columns.  When both are columns OF check i, the two messages on those edges never leave the
// thread's registers and their posteriors are read from registers: per thread and pass 4 row words and 2 posteriors are stored instead of 6 and 2,
// and 8 words are gathered instead of 12.  That needs an assignment in which every check owns exactly two of its six columns and every column has
// exactly one owner -- a perfect matching of the columns into checks of capacity two.  x = 1/3 on every edge is a fractional solution, so an integral
// one exists for every (6,3)-regular graph without repeated edges; augmenting paths find it (n <= 1024 columns here).
//
// Per check, kRegOwnWords int32 words (the record the kernel loads once per thread):
//   [0..5]   the six columns, the two owned ones first (ascending), then the other four in CSR order
//   [6..9]   where edge k = 2..5 gathers its posterior: owner + m * v for the column that check `owner` holds as its v-th.  A thread keeps its two
//            posteriors at V[i] and V[i + m], lane-contiguous like the layout without ownership, so its two posterior stores stay free of bank
//            conflicts (stored at V[column] they were random, and SQ_LDS_BANK_CONFLICT rose by half: profiles/r20_own_edges.txt)
//   The row slot of stored edge k = 2..5 is k - 2: the word is R[i * RST + k - 2] (regular_own_slot), a constant in the kernel.
//   [10,11]  owned column 0: offsets (row * RST + slot, in doubles) of its two OTHER messages in ascending check order, o1 and o2
//   [12,13]  the same for owned column 1
//   [14]     bit v: `last` of owned column v -- the owning check has the highest index of the column's three checks
//   [15]     0
// The variable sum of an owned column is ((0.0 + o1) + X) + Y with (X, Y) = last ? (o2, own) : (own, o2): the reference's ascending-order sum
// ((0 + a) + b) + c word for word when the own message is second or third, and when it is first because (0 + r) + o1 and (0 + o1) + r are the same
// word (+-0.0 included: 0.0 + x is never -0.0).
//
// WHICH perfect assignment is used changes no output word (the argument above holds for every one of them) but it decides every address of the eight
// gathers of a pass -- V[owner + m * v] for the four posteriors, two row words per owned column -- and with them the LDS bank conflicts, the busiest
// resource of the fixed-work loop (profiles/r21_own_conflicts.txt).  regular_own_cost is the bank model of those gathers; regular_own_assign builds
// candidates in a fixed order and keeps the cheapest, ties to the earliest:
//   (a) Kuhn's augmenting paths, the first perfect assignment they find (addresses effectively random across lanes);
//   (b) quasi-cyclic: where the matrix is translation invariant on an L x M torus (check i = a * M + b, column j = h * m + a' * M + b', every check
//       with the same set of (h, a' - a, b' - b): all bivariate-bicycle matrices), "own the column at left shift s_A and the one at right shift
//       s_B" is a perfect assignment for each of the 3 x 3 pairs, and under it every gather address is a torus shift of the lane index;
//   (c) on graphs without (b): (a) polished by rotations of ownership along random alternating cycles, a fixed number of evaluations.
// The result is a function of the CSR alone: integer arithmetic, a PRNG of this header with a constant seed, no clock.
//
// A SECOND assignment, regular_own_assign_minlast, serves the fixed-work form on a placed table (regular_place.h).  There every gather address comes from an
// edge colouring that is conflict-free for any assignment, so the choice is free again and goes to the other cost an assignment has: the two selects per
// owned column that put the own message into its place, needed only where `last` differs between the lanes of a wave.  It owns the fewest last edges a
// perfect assignment can (min-cost flow, cost 1 per owned last edge: 7 / 11 / 22 / 9 / 9 on the Hx matrices of bb72 / bb144 / bb288 / bb90 / bb108), and a
// check that owns exactly one holds it as column v = 1, so a check is of one of three classes: none, one, both (word [14] = 0, 2, 3).  The graph handle
// keeps both tables; the assignment above stays, byte for byte, for every launch that reads no placed table (early exit, the linear layout as a table,
// qldpc_set_option "regular_wave_classes" 0).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#include "regular_plan.h"

namespace qldpc {

static const int kRegOwnWords = 16;
static const int kRegOwnCols = 0, kRegOwnGather = 6, kRegOwnOffs = 10, kRegOwnLast = 14;
static const int kRegOwnCdeg = 6, kRegOwnVdeg = 3, kRegOwnOwned = 2;
inline int regular_own_slot(int k) { return k - kRegOwnOwned; }          // row slot of stored edge k = 2 .. 5

static const int kRegOwnStreams = 8;                 // gathers of a pass: posteriors of edges 2..5, then row words (v, d) = (0,0) (0,1) (1,0) (1,1)
static const int kRegOwnTeamThreads = 512;           // the thread budget of a workgroup of minsum_regular.hip (QLDPC_LB_T)
static const int kRegOwnSearchEvals = 600;           // (c): assignments priced per graph.  Creating a handle takes 6 ms instead of 0.6 at m = 512 (profiles/r21_own_conflicts.txt)
static const int kRegOwnCycleSteps = 16;             // (c): longest alternating cycle of a move
enum { kRegOwnKindKuhn = 0, kRegOwnKindCyclic = 1, kRegOwnKindSearched = 2 };

// What regular_own_assign chose (tests/regular_own_cost_main.cpp prints it).  Costs are those of regular_own_cost over one workgroup.
struct RegOwnChoice {
    int kind = kRegOwnKindKuhn, L = 0, M = 0, candidates = 0;       // L x M: the torus of the chosen (b) candidate; candidates: (b) assignments priced
    long long kuhn_cost = 0, cost = 0, kuhn_stream[kRegOwnStreams] = {}, stream[kRegOwnStreams] = {};
};

// The workgroup shape the cost is taken at: the kernel's own carve without an iteration table.  A graph with more checks than a workgroup has threads
// never reaches the kernel; it is priced as one team in one workgroup of its own size, so that every (6,3) graph has a cost.
inline bool regular_own_plan(int m, RegPlan &P) {
    return plan_regular_shape(kRegOwnCdeg, kRegOwnVdeg, m, 2 * m, 0, m > kRegOwnTeamThreads ? m : kRegOwnTeamThreads, 0, P);
}

// LDS-array cycles of the eight gathers of one pass of the fixed-work loop over one workgroup (callers divide by P.S for a per-shot figure).  The model:
// ds_read_b64 serves lanes 0..31 and 32..63 of a wave as two groups; a double lives on pair-bank (byte address / 8) mod 32; a group costs the largest
// number of DISTINCT addresses on one pair-bank (equal addresses broadcast).  Addresses are the kernel's: a team lane reads Vl[coff[k]], k = 2..5, with
// Vl = V + slot * n and Rl[voff[v][d]], d = 0, 1, with Rl = R + slot * m * RST; a lane of no team reads the dummy region, Dl[RST + (k & 1)] and Dl[d].
// The posterior and the row gathers are separate instructions, so offV only rotates the banks of the former against the lanes: it moves no conflict
// between the two kinds.  It held SQ_LDS_BANK_CONFLICT to within 4 % on the bb144 graph (profiles/r21_own_conflicts.txt).
// load_sq: sum over groups and banks of (distinct addresses)^2, the smooth figure the search of (c) is guided by.
// `seen` is scratch the search hands in to price many tables without an allocation each.
inline long long regular_own_cost(int m, const int32_t *tab, const RegPlan &P, int rst, long long *per_stream = nullptr, long long *load_sq = nullptr,
                                  std::vector<int> *seen = nullptr) {
    const int n = 2 * m, vbase = P.offV / 8, dbase = P.offD / 8;
    std::vector<int> own_seen;
    std::vector<int> &at = seen ? *seen : own_seen;                             // at[address] = the last group that read it
    at.assign((size_t)dbase + rst + 2, -1);
    long long total = 0, sq = 0, cyc[kRegOwnStreams] = {};
    int group = 0, slot = 0, member = 0;                                             // of lane t0: t0 = slot * TS + member
    for (int t0 = 0; t0 < (int)P.block; t0 += 32) {
        for (int s = 0; s < kRegOwnStreams; s++, group++) {
            int load[32] = {}, worst = 0, sl = slot, mem = member;
            for (int l = 0; l < 32; l++) {
                int a;
                if (sl < P.S && mem < m) {
                    const int32_t *r = tab + (size_t)mem * kRegOwnWords;
                    a = s < 4 ? vbase + sl * n + r[kRegOwnGather + s] : sl * m * rst + r[kRegOwnOffs + s - 4];
                } else {
                    a = s < 4 ? dbase + rst + (s & 1) : dbase + (s & 1);              // edges 2..5: k & 1 = s & 1; (v, d): d = s & 1
                }
                if (++mem == P.TS) { mem = 0; sl++; }
                if (at[a] == group) continue;                                        // the same word again: a broadcast
                at[a] = group;
                const int c = load[a & 31]++;
                sq += 2 * c + 1;                                                     // (c + 1)^2 - c^2
                if (c + 1 > worst) worst = c + 1;
            }
            cyc[s] += worst;
        }
        for (int l = 0; l < 32; l++) if (++member == P.TS) { member = 0; slot++; }
    }
    for (int s = 0; s < kRegOwnStreams; s++) { total += cyc[s]; if (per_stream) per_stream[s] = cyc[s]; }
    if (load_sq) *load_sq = sq;
    return total;
}

// A (6,3)-regular CSR with n == 2 m and no repeated column in a row, and the three rows of every column in ascending order.
struct RegOwnGraph {
    int m = 0, n = 0, rst = 0;
    const int32_t *indptr = nullptr, *indices = nullptr;
    std::vector<int> rows;
    const int *rows_of(int j) const { return &rows[(size_t)j * kRegOwnVdeg]; }
};

inline bool regular_own_graph(int m, int n, const int32_t *indptr, const int32_t *indices, int rst, RegOwnGraph &G) {
    if (m <= 0 || n != 2 * m || rst < kRegOwnCdeg - kRegOwnOwned) return false;
    std::vector<int> cdeg(n, 0);
    for (int i = 0; i < m; i++) {
        if (indptr[i + 1] - indptr[i] != kRegOwnCdeg) return false;
        for (int e = indptr[i]; e < indptr[i + 1]; e++) {
            if (indices[e] < 0 || indices[e] >= n) return false;
            for (int f = indptr[i]; f < e; f++) if (indices[f] == indices[e]) return false;      // a repeated column in a row
            cdeg[indices[e]]++;
        }
    }
    for (int j = 0; j < n; j++) if (cdeg[j] != kRegOwnVdeg) return false;
    G.m = m; G.n = n; G.rst = rst; G.indptr = indptr; G.indices = indices;
    // rows of every column, ascending (rows are visited in ascending order)
    G.rows.assign((size_t)n * kRegOwnVdeg, 0);
    std::vector<int> fill(n, 0);
    for (int i = 0; i < m; i++)
        for (int e = indptr[i]; e < indptr[i + 1]; e++) G.rows[(size_t)indices[e] * kRegOwnVdeg + fill[indices[e]]++] = i;
    return true;
}

// (a) owner[j] = the check that owns column j.  Kuhn's augmenting paths: a column takes a free place of one of its checks, or evicts a column held by
// one of them, which then looks for a place among the checks this search has not visited.  The depth is at most m frames.
inline bool regular_own_kuhn(const RegOwnGraph &G, std::vector<int> &owner) {
    const int m = G.m, n = G.n;
    owner.assign(n, -1);
    std::vector<int> held((size_t)m * kRegOwnOwned, -1), seen(m, -1);
    int stamp = -1;
    std::function<bool(int)> place = [&](int j) {
        for (int d = 0; d < kRegOwnVdeg; d++) {
            const int i = G.rows_of(j)[d];
            if (seen[i] == stamp) continue;
            seen[i] = stamp;
            int *h = &held[(size_t)i * kRegOwnOwned];
            for (int t = 0; t < kRegOwnOwned; t++) if (h[t] < 0) { h[t] = j; owner[j] = i; return true; }
            for (int t = 0; t < kRegOwnOwned; t++) if (place(h[t])) { h[t] = j; owner[j] = i; return true; }
        }
        return false;
    };
    for (int j0 = 0; j0 < n; j0++) { stamp = j0; if (!place(j0)) return false; }
    return true;
}

// The records of an assignment.  False (tab empty) unless it is perfect: every column owned by one of its own checks, every check owning two.
// last_second: a check that owns exactly one `last` column holds it as its column v = 1 instead of the two in ascending order (the min-last table below).
inline bool regular_own_records(const RegOwnGraph &G, const std::vector<int> &owner, std::vector<int32_t> &tab, bool last_second = false) {
    const int m = G.m, n = G.n, rst = G.rst;
    const int32_t *indptr = G.indptr, *indices = G.indices;
    tab.clear();
    if ((int)owner.size() != n) return false;
    std::vector<int> held((size_t)m * kRegOwnOwned, -1);
    for (int j = 0; j < n; j++) {                                              // ascending j: the two owned columns of a check come out ascending
        const int i = owner[j];
        if (i < 0 || i >= m) return false;
        const int *rj = G.rows_of(j);
        if (rj[0] != i && rj[1] != i && rj[2] != i) return false;
        int *h = &held[(size_t)i * kRegOwnOwned];
        if (h[0] < 0) h[0] = j; else if (h[1] < 0) h[1] = j; else return false;
    }
    for (int i = 0; i < m; i++) if (held[(size_t)i * kRegOwnOwned] < 0 || held[(size_t)i * kRegOwnOwned + 1] < 0) return false;
    if (last_second)
        for (int i = 0; i < m; i++) {
            int *h = &held[(size_t)i * kRegOwnOwned];
            if (G.rows_of(h[0])[kRegOwnVdeg - 1] == i && G.rows_of(h[1])[kRegOwnVdeg - 1] != i) std::swap(h[0], h[1]);
        }
    // columns and slots first, the offsets need every row's slots
    tab.assign((size_t)m * kRegOwnWords, 0);
    for (int i = 0; i < m; i++) {
        int32_t *r = &tab[(size_t)i * kRegOwnWords];
        r[kRegOwnCols + 0] = held[(size_t)i * kRegOwnOwned]; r[kRegOwnCols + 1] = held[(size_t)i * kRegOwnOwned + 1];
        int k = kRegOwnOwned;
        for (int e = indptr[i]; e < indptr[i + 1]; e++)
            if (owner[indices[e]] != i) {
                if (k >= kRegOwnCdeg) { tab.clear(); return false; }
                const int c = indices[e], o = owner[c];
                r[kRegOwnCols + k] = c;
                r[kRegOwnGather + k - kRegOwnOwned] = o + m * (held[(size_t)o * kRegOwnOwned] == c ? 0 : 1);
                k++;
            }
        if (k != kRegOwnCdeg) { tab.clear(); return false; }
    }
    auto word_of = [&](int row, int col) {          // where check `row` stores its message to the column it does not own
        const int32_t *r = &tab[(size_t)row * kRegOwnWords];
        for (int k = kRegOwnOwned; k < kRegOwnCdeg; k++) if (r[kRegOwnCols + k] == col) return row * rst + regular_own_slot(k);
        return -1;
    };
    for (int i = 0; i < m; i++) {
        int32_t *r = &tab[(size_t)i * kRegOwnWords];
        for (int v = 0; v < kRegOwnOwned; v++) {
            const int j = r[kRegOwnCols + v];
            const int *rj = G.rows_of(j);
            int t = 0;
            for (int d = 0; d < kRegOwnVdeg; d++)
                if (rj[d] != i) { const int w = word_of(rj[d], j); if (w < 0 || t >= 2) { tab.clear(); return false; } r[kRegOwnOffs + 2 * v + t++] = w; }
            if (t != 2) { tab.clear(); return false; }
            if (rj[kRegOwnVdeg - 1] == i) r[kRegOwnLast] |= 1 << v;
        }
    }
    return true;
}

// (b) The translation-invariant assignments, for every factorisation m = L * M under which every check shows the same six (half, shift) pairs: one
// owner table per (left shift, right shift), in ascending order of L, then of the shifts.  lm[c] = (L, M) of owners[c].  Nothing where no
// factorisation fits.  A candidate is perfect by construction (column -> column minus shift is a bijection of each half onto the checks);
// regular_own_records verifies it all the same.
inline void regular_own_cyclic(const RegOwnGraph &G, std::vector<std::vector<int>> &owners, std::vector<std::pair<int, int>> &lm) {
    const int m = G.m;
    owners.clear(); lm.clear();
    for (int L = 1; L <= m; L++) {
        if (m % L) continue;
        const int M = m / L;
        // a shift as one word: half * m + da * M + db
        auto shifts_of = [&](int i, int (&sh)[kRegOwnCdeg]) {
            const int a = i / M, b = i - a * M;
            for (int k = 0; k < kRegOwnCdeg; k++) {
                const int j = G.indices[G.indptr[i] + k], h = j / m, c = j - h * m, ca = c / M, cb = c - ca * M;
                sh[k] = h * m + ((ca - a + L) % L) * M + (cb - b + M) % M;
            }
            std::sort(sh, sh + kRegOwnCdeg);
        };
        int s0[kRegOwnCdeg], si[kRegOwnCdeg];
        shifts_of(0, s0);
        bool same = true;
        for (int i = 1; i < m && same; i++) { shifts_of(i, si); same = std::equal(s0, s0 + kRegOwnCdeg, si); }
        if (!same) continue;
        for (int x = 0; x < kRegOwnCdeg; x++)
            for (int y = 0; y < kRegOwnCdeg; y++) {
                if (s0[x] >= m || s0[y] < m) continue;                           // x: a shift into the left half, y: into the right half
                std::vector<int> owner(G.n, -1);
                for (int i = 0; i < m; i++) {
                    const int a = i / M, b = i - a * M;
                    for (int s : {s0[x], s0[y]}) {
                        const int h = s / m, d = s - h * m, da = d / M, db = d - da * M;
                        owner[h * m + ((a + da) % L) * M + (b + db) % M] = i;
                    }
                }
                owners.push_back(owner); lm.emplace_back(L, M);
            }
    }
}

// (c) Polishes a perfect assignment by rotations along alternating cycles: a random column moves to another of its checks, which hands one of the two it
// held to another of ITS checks, and so on until a column reaches the check the first one left (within kRegOwnCycleSteps, else the move is dropped).
// Every state is a perfect assignment.  The hard cost is plateaus, so moves are judged on F = load_sq + 8 * cost and accepted while F rises by no more
// than a threshold that falls linearly to zero over the kRegOwnSearchEvals priced states (threshold accepting: annealing without a floating-point
// exponential, so that every host takes the same walk).  Leaves in `owner` the cheapest state seen (by cost, then F); false if it never beat the start.
inline bool regular_own_polish(const RegOwnGraph &G, const RegPlan &P, std::vector<int> &owner) {
    const int m = G.m, n = G.n;
    std::vector<int32_t> tab;
    std::vector<int> seen;
    if (!regular_own_records(G, owner, tab)) return false;
    long long sq = 0;
    const long long cost0 = regular_own_cost(m, tab.data(), P, G.rst, nullptr, &sq, &seen);
    long long cur = sq + 8 * cost0, best_cost = cost0, best_f = cur;
    std::vector<int> best = owner, held((size_t)m * kRegOwnOwned);
    auto reheld = [&](int i) {
        int t = 0;
        for (int e = G.indptr[i]; e < G.indptr[i + 1]; e++) if (owner[G.indices[e]] == i && t < kRegOwnOwned) held[(size_t)i * kRegOwnOwned + t++] = G.indices[e];
    };
    for (int i = 0; i < m; i++) reheld(i);
    uint64_t state = 0x9e3779b97f4a7c15ull;                                    // splitmix64, constant seed
    auto rnd = [&](uint32_t below) {
        uint64_t z = (state += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; z ^= z >> 31;
        return (uint32_t)(((z >> 32) * below) >> 32);
    };
    const long long t_start = 24;
    int col[kRegOwnCycleSteps], from[kRegOwnCycleSteps], to[kRegOwnCycleSteps];
    for (int ev = 0, tries = 0; ev < kRegOwnSearchEvals && tries < 8 * kRegOwnSearchEvals; tries++) {
        // walk an alternating cycle
        int len = 0, j = (int)rnd((uint32_t)n);
        const int i0 = owner[j];
        bool closed = false;
        for (int cur_check = i0; len < kRegOwnCycleSteps;) {
            const int *rj = G.rows_of(j);
            int opt[kRegOwnVdeg], nopt = 0, next = -1;
            for (int d = 0; d < kRegOwnVdeg; d++) {
                const int i = rj[d];
                if (i == cur_check) continue;
                if (i == i0 && len > 0) { next = i0; break; }                  // the cycle closes as soon as it can
                bool visited = (i == i0);
                for (int s = 0; s < len && !visited; s++) visited = (to[s] == i);
                if (!visited) opt[nopt++] = i;
            }
            if (next < 0) { if (!nopt) break; next = opt[rnd((uint32_t)nopt)]; }
            col[len] = j; from[len] = cur_check; to[len] = next; len++;
            if (next == i0) { closed = true; break; }
            j = held[(size_t)next * kRegOwnOwned + rnd(kRegOwnOwned)];
            cur_check = next;
        }
        if (!closed) continue;
        for (int s = 0; s < len; s++) owner[col[s]] = to[s];
        for (int s = 0; s < len; s++) reheld(to[s]);
        ev++;
        long long f = -1, c = 0;
        if (regular_own_records(G, owner, tab)) { c = regular_own_cost(m, tab.data(), P, G.rst, nullptr, &sq, &seen); f = sq + 8 * c; }
        const long long threshold = t_start * (kRegOwnSearchEvals - ev) / kRegOwnSearchEvals;
        if (f >= 0 && f <= cur + threshold) {
            cur = f;
            if (c < best_cost || (c == best_cost && f < best_f)) { best_cost = c; best_f = f; best = owner; }
        } else {
            for (int s = 0; s < len; s++) owner[col[s]] = from[s];
            for (int s = 0; s < len; s++) reheld(to[s]);
        }
    }
    owner = best;
    return best_cost < cost0;
}

// The min-last assignment, for the fixed-work form on a place table (regular_place.h), where bank conflicts no longer depend on who owns what: the
// perfect assignment that owns the FEWEST `last` edges (the owning check is the highest of the column's three).  A thread whose two `last` bits are
// clear adds (o1 + own) + o2 for both columns without a select, and regular_place.h deals such threads into waves of their own.  Min-cost flow by
// successive shortest augmenting paths: columns in ascending order, each along the cheapest alternating path to a check with a free place, cost 1 per
// owned last edge, Dijkstra on reduced costs over the n + m nodes (a binary heap of (distance, node), so ties go to the lowest node index), potentials kept across augmentations.
// Integer arithmetic only: a function of the CSR alone.
inline bool regular_own_minlast(const RegOwnGraph &G, std::vector<int> &owner) {
    const int m = G.m, n = G.n, N = n + m, INF = 1 << 29;
    owner.assign(n, -1);
    std::vector<int> held((size_t)m * kRegOwnOwned, -1), pot(N, 0), dist(N), from(N);
    std::vector<char> fin(N);
    std::vector<std::pair<int, int>> heap;
    auto push = [&](int d, int x) { heap.emplace_back(d, x); std::push_heap(heap.begin(), heap.end(), std::greater<std::pair<int, int>>()); };
    auto cost = [&](int j, int i) { return G.rows_of(j)[kRegOwnVdeg - 1] == i ? 1 : 0; };
    for (int j0 = 0; j0 < n; j0++) {
        std::fill(dist.begin(), dist.end(), INF); std::fill(fin.begin(), fin.end(), 0); std::fill(from.begin(), from.end(), -1);
        dist[j0] = 0;
        int target = -1;
        heap.clear();
        heap.emplace_back(0, j0);
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), std::greater<std::pair<int, int>>());       // the smallest (distance, node)
            const int du = heap.back().first, u = heap.back().second;
            heap.pop_back();
            if (fin[u] || du != dist[u]) continue;
            fin[u] = 1;
            if (u < n) {                                                             // a column: to each of its checks that does not hold it
                for (int d = 0; d < kRegOwnVdeg; d++) {
                    const int i = G.rows_of(u)[d];
                    if (owner[u] == i || fin[n + i]) continue;
                    const int w = dist[u] + cost(u, i) + pot[u] - pot[n + i];
                    if (w < dist[n + i]) { dist[n + i] = w; from[n + i] = u; push(w, n + i); }
                }
            } else {                                                                 // a check: done if it has a free place, else back along a column it holds
                const int i = u - n, *h = &held[(size_t)i * kRegOwnOwned];
                if (h[0] < 0 || h[1] < 0) { target = u; break; }
                for (int t = 0; t < kRegOwnOwned; t++) {
                    const int j = h[t];
                    if (fin[j]) continue;
                    const int w = dist[u] - cost(j, i) + pot[u] - pot[j];
                    if (w < dist[j]) { dist[j] = w; from[j] = u; push(w, j); }
                }
            }
        }
        if (target < 0) return false;
        for (int x = 0; x < N; x++) pot[x] += std::min(dist[x], dist[target]);
        for (int i = target - n;;) {                                                 // along the path backwards: column j moves to check i
            const int j = from[n + i], prev = owner[j];
            int *h = &held[(size_t)i * kRegOwnOwned];
            h[h[0] < 0 ? 0 : 1] = j;
            owner[j] = i;
            if (prev < 0) break;                                                     // j0
            int *hp = &held[(size_t)prev * kRegOwnOwned];
            hp[hp[0] == j ? 0 : 1] = -1;
            i = prev;
        }
    }
    return true;
}

// Owned last edges of a table, and the class of check i under it: 0 none, 1 one (its column v = 1), 2 both.
inline int regular_own_class(const int32_t *tab, int i) {
    const int l = tab[(size_t)i * kRegOwnWords + kRegOwnLast] & 3;
    return l == 0 ? 0 : l == 3 ? 2 : 1;
}

// The table of the min-last assignment in canonical order (a check owning exactly one last edge has it as column v = 1, so word [14] is 0, 2 or 3).
// Returns false and leaves tab empty exactly where regular_own_assign does.
inline bool regular_own_assign_minlast(int m, int n, const int32_t *indptr, const int32_t *indices, int rst, std::vector<int32_t> &tab) {
    tab.clear();
    RegOwnGraph G;
    std::vector<int> owner;
    if (!regular_own_graph(m, n, indptr, indices, rst, G) || !regular_own_minlast(G, owner) || !regular_own_records(G, owner, tab, true)) { tab.clear(); return false; }
    return true;
}

// CSR of m checks over n columns.  Returns false ("none": the launch takes the body without ownership) unless the graph is (6,3)-regular with
// n == 2 m, no row repeats a column, and the search places every column; on success tab holds m records of kRegOwnWords words.
// search = 0: the assignment of (a) as it comes.  search = 1: the cheapest of (a), (b), (c) by regular_own_cost (header comment); a candidate of (b) or
// (c) that does not validate is dropped, so a table is returned exactly where (a) returns one.
inline bool regular_own_assign(int m, int n, const int32_t *indptr, const int32_t *indices, int rst, std::vector<int32_t> &tab, int search = 1,
                               RegOwnChoice *choice = nullptr) {
    tab.clear();
    RegOwnGraph G;
    if (!regular_own_graph(m, n, indptr, indices, rst, G)) return false;
    std::vector<int> kuhn;
    if (!regular_own_kuhn(G, kuhn) || !regular_own_records(G, kuhn, tab)) { tab.clear(); return false; }
    RegOwnChoice C;
    RegPlan P;
    if (!regular_own_plan(m, P)) { if (choice) *choice = C; return true; }      // no shape to price at: (a)
    C.kuhn_cost = C.cost = regular_own_cost(m, tab.data(), P, rst, C.kuhn_stream);
    std::copy(C.kuhn_stream, C.kuhn_stream + kRegOwnStreams, C.stream);
    if (search) {
        std::vector<int32_t> cand;
        auto offer = [&](const std::vector<int> &owner, int kind, int L, int M) {
            long long st[kRegOwnStreams];
            if (!regular_own_records(G, owner, cand)) return;
            const long long c = regular_own_cost(m, cand.data(), P, rst, st);
            if (c < C.cost) { C.cost = c; C.kind = kind; C.L = L; C.M = M; std::copy(st, st + kRegOwnStreams, C.stream); tab.swap(cand); }
        };
        std::vector<std::vector<int>> cyc;
        std::vector<std::pair<int, int>> lm;
        regular_own_cyclic(G, cyc, lm);
        C.candidates = (int)cyc.size();
        for (size_t c = 0; c < cyc.size(); c++) offer(cyc[c], kRegOwnKindCyclic, lm[c].first, lm[c].second);
        if (cyc.empty()) {
            std::vector<int> owner = kuhn;
            if (regular_own_polish(G, P, owner)) offer(owner, kRegOwnKindSearched, 0, 0);
        }
    }
    if (choice) *choice = C;
    return true;
}

}  // namespace qldpc
