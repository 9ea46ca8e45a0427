// Edge ownership for the (6,3) form of the regular min-sum kernel (minsum_regular.hip): pure C++, no HIP header, so a host program can print it
// (tests/regular_own_main.cpp).
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
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

namespace qldpc {

static const int kRegOwnWords = 16;
static const int kRegOwnCols = 0, kRegOwnGather = 6, kRegOwnOffs = 10, kRegOwnLast = 14;
static const int kRegOwnCdeg = 6, kRegOwnVdeg = 3, kRegOwnOwned = 2;
inline int regular_own_slot(int k) { return k - kRegOwnOwned; }          // row slot of stored edge k = 2 .. 5

// CSR of m checks over n columns.  Returns false ("none": the launch takes the body without ownership) unless the graph is (6,3)-regular with
// n == 2 m, no row repeats a column, and the search places every column; on success tab holds m records of kRegOwnWords words.
inline bool regular_own_assign(int m, int n, const int32_t *indptr, const int32_t *indices, int rst, std::vector<int32_t> &tab) {
    tab.clear();
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
    // rows of every column, ascending (rows are visited in ascending order)
    std::vector<int> rows((size_t)n * kRegOwnVdeg), fill(n, 0);
    for (int i = 0; i < m; i++)
        for (int e = indptr[i]; e < indptr[i + 1]; e++) rows[(size_t)indices[e] * kRegOwnVdeg + fill[indices[e]]++] = i;
    // matching: owner[j] = check, held[i] = the (at most two) columns of check i
    std::vector<int> owner(n, -1), held((size_t)m * kRegOwnOwned, -1), seen(m, -1);
    // Kuhn's augmenting paths: a column takes a free place of one of its checks, or evicts a column held by one of them, which then looks for a place
    // among the checks this search has not visited.  The depth is at most m <= 512 frames.
    int stamp = -1;
    std::function<bool(int)> place = [&](int j) {
        for (int d = 0; d < kRegOwnVdeg; d++) {
            const int i = rows[(size_t)j * kRegOwnVdeg + d];
            if (seen[i] == stamp) continue;
            seen[i] = stamp;
            int *h = &held[(size_t)i * kRegOwnOwned];
            for (int t = 0; t < kRegOwnOwned; t++) if (h[t] < 0) { h[t] = j; owner[j] = i; return true; }
            for (int t = 0; t < kRegOwnOwned; t++) if (place(h[t])) { h[t] = j; owner[j] = i; return true; }
        }
        return false;
    };
    for (int j0 = 0; j0 < n; j0++) { stamp = j0; if (!place(j0)) return false; }
    for (int i = 0; i < m; i++) {
        int *h = &held[(size_t)i * kRegOwnOwned];
        if (h[0] < 0 || h[1] < 0 || owner[h[0]] != i || owner[h[1]] != i) return false;
        if (h[0] > h[1]) { const int t = h[0]; h[0] = h[1]; h[1] = t; }
    }
    // records: columns and slots first, the offsets need every row's slots
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
            const int *rj = &rows[(size_t)j * kRegOwnVdeg];
            int t = 0;
            for (int d = 0; d < kRegOwnVdeg; d++)
                if (rj[d] != i) { const int w = word_of(rj[d], j); if (w < 0 || t >= 2) { tab.clear(); return false; } r[kRegOwnOffs + 2 * v + t++] = w; }
            if (t != 2) { tab.clear(); return false; }
            if (rj[kRegOwnVdeg - 1] == i) r[kRegOwnLast] |= 1 << v;
        }
    }
    return true;
}

}  // namespace qldpc
