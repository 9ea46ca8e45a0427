// LDS placement for the fixed-work (6,3) ownership form of the regular min-sum kernel (minsum_regular.hip, PLACE): pure C++, no HIP header, so a host program can print
// it (tests/regular_place_main.cpp).
//
// A thread of the kernel keeps its (slot, member) for a whole launch, so WHERE in LDS it gathers and stores may be any per-thread table loaded once into
// registers.  regular_own_cost shows what the linear layout (row i at R + i * RST, posteriors at V[i], V[i + m], the same in every slot) costs: the eight
// gathers behind each barrier pay about twice their conflict-free LDS-array cycles, and no layout that is the same for every slot is conflict-free
// (profiles/r22_alpha_zero.txt).  A placement per (slot, check) is, by edge colouring.
//
// Messages.  An item is (slot, check r, stored edge t = 0 .. 3).  One lane writes it, in store stream t (ds_write_b64 serves 16-lane groups, bank =
// (address / 8) mod 16); one lane reads it, the owner of its column, in gather stream (v, d) (ds_read_b64 serves 32-lane groups, pair-bank = (address / 8)
// mod 32).  Bipartite multigraph: (gather stream, 16-lane half of a read group) on one side, (store stream, 16-lane group) on the other, one edge per
// item, every degree 16.  Koenig: 16 colours colour it properly.  bank = colour + 16 * (which half): a read group sees 32 distinct pair-banks, a store
// group 16 distinct banks.  Exact for every graph.
//
// Posteriors.  An item is (slot, owner o, v): one writer, TWO readers (the column's other two checks).  The columns are the edges of a 4-regular multigraph
// on the checks (an edge joins the two readers); an Euler orientation gives every check two "tail" and two "head" columns.  Tails go to posterior gathers
// 0 and 1, heads to 2 and 3 -- the check update does not depend on the order of a row's edges (minsum_regular.hip, header comment), only the posterior
// gather, Rprev and the message store of one edge have to agree, and they do: the kernel's edge k IS "whatever gather k reads".  Now every item is read once
// on the tail side and once on the head side: a bipartite multigraph between (tail gather, read group) and (head gather, read group), every degree 32, 32
// colours = pair-banks, the four gathers conflict-free.  The two posterior stores are a third constraint Koenig does not cover (distinct banks mod 16 in
// every 16-lane group of a store); they are reduced by Kempe moves -- a two-colour alternating component flipped as a whole keeps the colouring proper --
// judged by threshold accepting on the store cost, the best state kept.  A ds_write_b64 takes 6 cycles per wave-instruction whatever it hits, against 4 array cycles conflict-free,
// so the score counts cycles above 6 per instruction first and array cycles second.
//
// The lanes of a block that belong to no team take part as items of their own (each reads what it writes), so every degree is exactly 16 or 32, every
// colour class has the same size and an address is 32 * (rank inside its bank) + bank: 4 * block doubles of messages from offset 0, then 2 * block doubles of
// posteriors.  Both lie in the R and V regions of the carve (regular_plan.h), which are contiguous from offset 0; where they do not fit the answer is "none".
//
// Per thread t < block, kRegPlaceWords int32 words, every address in doubles from the start of the workgroup's LDS:
//   [0..3]    the four posterior gathers: the kernel's edges 2 .. 5
//   [4..7]    the four message gathers (v, d) = (0,0) (0,1) (1,0) (1,1): the two other messages of owned column v in ascending check order (regular_own.h)
//   [8,9]     where the thread stores the posteriors of its owned columns 0 and 1
//   [10..13]  where it stores the messages of the kernel's edges 2 .. 5
//   [14]      nibble k: the edge of the ownership record (2 .. 5, CSR order) that the kernel's edge 2 + k is; 0 for a lane of no team
//   [15]      0 in the identity order (thread t = slot * TS + member, the lanes of no team last).  Under a thread order (regular_place_order, below): bit 30,
//             the class of the thread's wave in bits 24 .. 25 (kRegWave*), its slot in bits 12 .. 23, its member in bits 0 .. 11
// Thread order.  Nothing requires thread t to be (t / TS, t % TS): every address is in the record, and slot and member are only values.  So the S * m
// (slot, check) items are dealt to the threads by the class of the check under the min-last ownership table (regular_own.h): whole waves of checks that own
// no last edge run the bare passes without selects (minsum_regular.hip).  The colourings below take an item's lane groups from the thread it is dealt to,
// so they are as exact under an order as without one; regular_place_cost prices records in thread order and needs no change.
// The table is a function of (ownership table, S, block) alone: integer arithmetic, a PRNG of this header with a constant seed, a fixed number of moves.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "regular_own.h"

namespace qldpc {

static const int kRegPlaceWords = 16;
static const int kRegPlacePostGather = 0, kRegPlaceMsgGather = 4, kRegPlacePostStore = 8, kRegPlaceMsgStore = 10, kRegPlaceEdges = 14;
static const int kRegPlaceStreams = 14;              // 8 gathers, 2 posterior stores, 4 message stores: words 0 .. 13 of a record
static const int kRegPlaceStored = kRegOwnCdeg - kRegOwnOwned;      // 4
// Kempe moves tried per table.  On the Hx matrices of bb72 / bb144 / bb288 the cycles above 6 per store instruction are 0 to 1 per workgroup from 4000
// moves on and neither figure moves between 8000 and 20000 (profiles/r24_place.txt); a move prices 2 * block items, 8000 of them take about 15 ms.
static const int kRegPlaceKempeMoves = 8000;
// Under a thread order (regular_place_order) the items a 16-lane group stores no longer sit next to each other in the graph and the walk needs more: 24000
// moves, thread swaps inside a 32-lane group among them, and up to four walks (regular_place_build; profiles/r27_wave_classes.txt has what each bought).
static const int kRegPlaceOrderedMoves = 24000, kRegPlaceSwapEvery = 4, kRegPlaceOrderedStarts = 4, kRegPlaceRestartBelow = 4;
#ifndef QLDPC_PLACE_THRESHOLD
#define QLDPC_PLACE_THRESHOLD 4
#endif
static const int kRegPlaceThreshold = QLDPC_PLACE_THRESHOLD;      // array cycles a move may cost at the start of the search (it never buys a cycle above 6: those weigh 100000)

// What the bank model charges one workgroup pass (LDS-array cycles).  over6: per store wave-instruction, cycles above the 6 it takes anyway.
struct RegPlaceCost {
    long long gather = 0, post_store = 0, msg_store = 0, post_store_over6 = 0, msg_store_over6 = 0, stream[kRegPlaceStreams] = {};
};

// The bank model of all 14 streams of a table of `block` records.  Gathers: regular_own_cost's rule (32-lane groups, pair-bank = address mod 32, a group
// costs the largest number of distinct addresses on one pair-bank).  Stores: 16-lane groups, bank = address mod 16, the same count; a wave-instruction is
// the sum of its four groups.
inline RegPlaceCost regular_place_cost(const int32_t *rec, int block) {
    RegPlaceCost C;
    auto group_cost = [&](int word, int t0, int lanes) {
        int addr[32], worst = 0;
        for (int l = 0; l < lanes; l++) addr[l] = rec[(size_t)(t0 + l) * kRegPlaceWords + word];
        std::sort(addr, addr + lanes);
        int load[32] = {};
        for (int l = 0; l < lanes; l++) {
            if (l && addr[l] == addr[l - 1]) continue;                                  // the same word again
            const int c = ++load[addr[l] & (lanes - 1)];
            if (c > worst) worst = c;
        }
        return worst;
    };
    for (int w = 0; w < kRegPlaceStreams; w++) {
        const bool store = w >= kRegPlacePostStore;
        for (int t0 = 0; t0 < block; t0 += 64) {
            int cyc = 0;
            if (!store) cyc = group_cost(w, t0, 32) + group_cost(w, t0 + 32, 32);
            else for (int g = 0; g < 4; g++) cyc += group_cost(w, t0 + 16 * g, 16);
            C.stream[w] += cyc;
            if (!store) C.gather += cyc;
            else if (w < kRegPlaceMsgStore) { C.post_store += cyc; C.post_store_over6 += std::max(0, cyc - 6); }
            else { C.msg_store += cyc; C.msg_store_over6 += std::max(0, cyc - 6); }
        }
    }
    return C;
}

// Today's addresses as a table: row i of slot s at R + (s * m + i) * RST, its posteriors at V[s * n + i] and V[s * n + i + m], the gathers where the ownership
// record says; a lane of no team works on the dummy region D.  What qldpc_set_option("regular_place", 0) launches with, and every shape placement declines.
inline void regular_place_linear(int m, const int32_t *own, const RegPlan &P, int rst, std::vector<int32_t> &rec) {
    const int n = 2 * m, vbase = P.offV / 8, dbase = P.offD / 8;
    rec.assign((size_t)P.block * kRegPlaceWords, 0);
    for (int t = 0; t < (int)P.block; t++) {
        int32_t *r = &rec[(size_t)t * kRegPlaceWords];
        const int s = t / P.TS, i = t - s * P.TS;
        if (s < P.S && i < m) {
            const int32_t *o = own + (size_t)i * kRegOwnWords;
            for (int k = 0; k < kRegPlaceStored; k++) {
                r[kRegPlacePostGather + k] = vbase + s * n + o[kRegOwnGather + k];
                r[kRegPlaceMsgGather + k] = s * m * rst + o[kRegOwnOffs + k];
                r[kRegPlaceMsgStore + k] = (s * m + i) * rst + k;
                r[kRegPlaceEdges] |= (kRegOwnOwned + k) << (4 * k);
            }
            for (int v = 0; v < kRegOwnOwned; v++) r[kRegPlacePostStore + v] = vbase + s * n + i + v * m;
        } else {
            for (int k = 0; k < kRegPlaceStored; k++) {
                r[kRegPlacePostGather + k] = dbase + rst + (k & 1);
                r[kRegPlaceMsgGather + k] = dbase + (k & 1);
                r[kRegPlaceMsgStore + k] = dbase + k;
            }
            for (int v = 0; v < kRegOwnOwned; v++) r[kRegPlacePostStore + v] = dbase + rst + v;
        }
    }
}

// A proper colouring of a bipartite multigraph with D colours (Koenig): every node of degree <= D, else false.  Edge by edge: a colour a free at the left
// end and b free at the right end; where a is taken at the right end, the a/b alternating path from there is flipped (it cannot reach the left end, which
// has no a-edge), after which a is free at both.  at_l[u * D + c], at_r[v * D + c] = the edge of colour c at the node, or -1.
struct RegPlaceColouring {
    int D = 0;
    std::vector<std::pair<int, int>> edges;
    std::vector<int> col, at_l, at_r;
    bool colour(int nl, int nr, int colours) {
        D = colours;
        col.assign(edges.size(), -1); at_l.assign((size_t)nl * D, -1); at_r.assign((size_t)nr * D, -1);
        std::vector<int> path;
        for (int e = 0; e < (int)edges.size(); e++) {
            const int u = edges[e].first, v = edges[e].second;
            int a = -1, b = -1;
            for (int c = 0; c < D && a < 0; c++) if (at_l[(size_t)u * D + c] < 0) a = c;
            for (int c = 0; c < D && b < 0; c++) if (at_r[(size_t)v * D + c] < 0) b = c;
            if (a < 0 || b < 0) return false;
            if (at_r[(size_t)v * D + a] >= 0) {
                path.clear();
                for (int x = at_r[(size_t)v * D + a], want = b; x >= 0; want = (want == a) ? b : a) {
                    path.push_back(x);
                    // an a-edge was entered from its right end and leaves through its left end, a b-edge the other way round
                    x = (want == b) ? at_l[(size_t)edges[x].first * D + b] : at_r[(size_t)edges[x].second * D + a];
                }
                flip(path, a, b);
            }
            set(e, a);
        }
        return true;
    }
    void set(int e, int c) { col[e] = c; at_l[(size_t)edges[e].first * D + c] = e; at_r[(size_t)edges[e].second * D + c] = e; }
    void flip(const std::vector<int> &comp, int a, int b) {
        for (int x : comp) { at_l[(size_t)edges[x].first * D + col[x]] = -1; at_r[(size_t)edges[x].second * D + col[x]] = -1; }
        for (int x : comp) set(x, col[x] == a ? b : a);
    }
    // the edges of the (a, b) two-colour component that holds e (col[e] is a or b)
    void component(int e, int a, int b, std::vector<int> &comp, std::vector<int> &mark, int stamp) const {
        comp.clear(); comp.push_back(e); mark[e] = stamp;
        for (size_t at = 0; at < comp.size(); at++) {
            const int x = comp[at], o = (col[x] == a) ? b : a;
            for (int y : {at_l[(size_t)edges[x].first * D + o], at_r[(size_t)edges[x].second * D + o]})
                if (y >= 0 && mark[y] != stamp) { mark[y] = stamp; comp.push_back(y); }
        }
    }
    bool proper() const {
        for (size_t e = 0; e < edges.size(); e++)
            if (col[e] < 0 || col[e] >= D || at_l[(size_t)edges[e].first * D + col[e]] != (int)e || at_r[(size_t)edges[e].second * D + col[e]] != (int)e) return false;
        return true;
    }
};

// ---- the thread order: which thread of the block is (slot, check), and the class of every wave
// Word [15] of a record built with an order: bit 30 set, the wave's class in bits 24 .. 25, the thread's slot in bits 12 .. 23 and its member (= check) in
// bits 0 .. 11; a lane of no team has slot = S.  Word [15] == 0 is the identity order, thread t = slot * TS + member, every wave mixed.
enum { kRegWaveMixed = 0, kRegWaveNone = 1, kRegWaveOne = 2, kRegWaveBoth = 3 };
static const int kRegPlaceOrder = 15, kRegPlaceOrdered = 1 << 30;
inline int32_t regular_place_pack(int wave_class, int slot, int member) { return kRegPlaceOrdered | (wave_class << 24) | (slot << 12) | member; }
inline int regular_place_wave_class(int32_t w) { return (w >> 24) & 3; }
inline int regular_place_slot(int32_t w) { return (w >> 12) & 0xfff; }
inline int regular_place_member(int32_t w) { return w & 0xfff; }

struct RegPlaceOrder {
    std::vector<int> thread_of;      // [S * m]: the thread of item slot * m + check
    std::vector<int> spare;          // the block - S * m threads of no team, ascending
    std::vector<int> wave_class;     // [block / 64]: kRegWave*
};

// Deals the S * m (slot, check) items of a workgroup to its threads so that as many waves as possible hold checks of ONE class of the ownership table
// (regular_own_class: none, one or both of the thread's owned columns `last`): such a wave runs a copy of the fixed-work loop without selects
// (minsum_regular.hip).  A lane of no team computes nothing that is read, so it completes any wave.  Per class, in the order none, one, both: its full
// waves of 64 items (slot-major, checks ascending).  Then the classes' remainders, the one that needs the fewest spare lanes first, each as a wave of its
// own while the spare lanes last.  What is left shares the mixed waves at the end of the block.  Integer arithmetic, a function of (table, S, block).
inline bool regular_place_order(int m, const int32_t *own, const RegPlan &P, RegPlaceOrder &O) {
    const int S = P.S, block = (int)P.block, team = S * m;
    O.thread_of.clear(); O.spare.clear(); O.wave_class.clear();
    if (m <= 0 || S <= 0 || P.TS != m || block % 64 || block < team || m > 0xfff || S >= 0xfff) return false;
    std::vector<int> items[3];
    for (int s = 0; s < S; s++) for (int i = 0; i < m; i++) items[regular_own_class(own, i)].push_back(s * m + i);
    O.thread_of.assign(team, -1);
    int t = 0, spare = block - team;
    size_t at[3] = {0, 0, 0};
    const int cls_of[3] = {kRegWaveNone, kRegWaveOne, kRegWaveBoth};
    auto put = [&](int c, int count) { for (int x = 0; x < count; x++) O.thread_of[items[c][at[c]++]] = t++; };
    auto idle = [&](int count) { for (int x = 0; x < count; x++) O.spare.push_back(t++); };
    for (int c = 0; c < 3; c++)
        for (; items[c].size() - at[c] >= 64;) { put(c, 64); O.wave_class.push_back(cls_of[c]); }
    for (bool more = true; more;) {
        int pick = -1;
        for (int c = 0; c < 3; c++) {
            const int left = (int)(items[c].size() - at[c]);
            if (left > 0 && 64 - left <= spare && (pick < 0 || left > (int)(items[pick].size() - at[pick]))) pick = c;
        }
        more = pick >= 0;
        if (more) { const int left = (int)(items[pick].size() - at[pick]); put(pick, left); idle(64 - left); spare -= 64 - left; O.wave_class.push_back(cls_of[pick]); }
    }
    for (int c = 0; c < 3; c++) put(c, (int)(items[c].size() - at[c]));
    idle(spare);
    if (t != block) return false;
    while ((int)O.wave_class.size() < block / 64) O.wave_class.push_back(kRegWaveMixed);
    // a "mixed" wave that happens to hold one class only (with or without spare lanes) is labelled by it
    std::vector<int> seen(block / 64, 0);
    for (int s = 0; s < S; s++) for (int i = 0; i < m; i++) seen[O.thread_of[s * m + i] / 64] |= 1 << regular_own_class(own, i);
    for (int w = 0; w < block / 64; w++)
        if (O.wave_class[w] == kRegWaveMixed && (seen[w] == 1 || seen[w] == 2 || seen[w] == 4)) O.wave_class[w] = cls_of[seen[w] == 1 ? 0 : seen[w] == 2 ? 1 : 2];
    return true;
}

// The placement of one workgroup: P.block records (header comment) from an ownership table (regular_own_assign, or regular_own_assign_minlast with an
// order).  False ("none", rec empty) where the arrays do not fit in [0, offV + S * n * 8), or the table is not one of m checks that own two columns each.
// order: the thread of every (slot, check) (regular_place_order); NULL = thread slot * m + check, the lanes of no team last, word [15] = 0.  The lane
// groups of the bank model are consecutive THREADS either way (32 for a gather, 16 for a store): an item's groups are those of the thread it is dealt to.
inline bool regular_place_build(int m, const int32_t *own, const RegPlan &P, int rst, std::vector<int32_t> &rec, int moves = kRegPlaceKempeMoves,
                                RegPlaceOrder *order = nullptr) {
    rec.clear();
    const int n = 2 * m, S = P.S, block = (int)P.block;
    if (m <= 0 || S <= 0 || P.TS != m || block % 64 || block < S * m || rst < kRegPlaceStored) return false;
    if (order && ((int)order->thread_of.size() != S * m || (int)order->spare.size() != block - S * m || (int)order->wave_class.size() != block / 64)) return false;
    const int nwin = block / 32, n16 = block / 16, msg_words = 4 * block, post_base = msg_words, post_words = 2 * block;
    if ((long long)(msg_words + post_words) * 8 > (long long)P.offV + (long long)S * n * 8) return false;        // the fit: both arrays inside R and V
    RegPlaceOrder ord;                                                                                             // the order as the swaps below leave it
    if (order) ord = *order;
    auto lane = [&](int s, int i) { return order ? ord.thread_of[(size_t)s * m + i] : s * m + i; };
    auto spare_lane = [&](int d) { return order ? ord.spare[d] : S * m + d; };                                     // the d-th lane of no team
    const int nspare = block - S * m;

    // ---- the two readers of every posterior item g = owner + m * v, and an Euler orientation of the reader multigraph
    std::vector<int> rd_check((size_t)n * 2, -1), rd_edge((size_t)n * 2, -1);
    for (int i = 0; i < m; i++)
        for (int q = 0; q < kRegPlaceStored; q++) {
            const int g = own[(size_t)i * kRegOwnWords + kRegOwnGather + q];
            if (g < 0 || g >= n || g % m == i) return false;
            const int at = rd_check[(size_t)g * 2] < 0 ? 0 : 1;
            if (rd_check[(size_t)g * 2 + at] >= 0) return false;                       // a third reader
            rd_check[(size_t)g * 2 + at] = i; rd_edge[(size_t)g * 2 + at] = q;
        }
    for (int g = 0; g < n; g++) if (rd_check[(size_t)g * 2 + 1] < 0 || rd_check[(size_t)g * 2] == rd_check[(size_t)g * 2 + 1]) return false;
    std::vector<int> tail(n, -1), next_q(m, 0);                                         // tail[g] = 0 / 1: which of the two readers gathers g on the tail side
    {
        // closed trails: every check has degree 4, so a trail that leaves a check along unused edges can only get stuck where it started
        auto unused_at = [&](int i) {
            for (int &q = next_q[i]; q < kRegPlaceStored; q++) {
                const int g = own[(size_t)i * kRegOwnWords + kRegOwnGather + q];
                if (tail[g] < 0) return g;
            }
            return -1;
        };
        for (int start = 0; start < m; start++)
            for (int u = start, g; (g = unused_at(u)) >= 0;) {
                const int at = rd_check[(size_t)g * 2] == u ? 0 : 1;
                tail[g] = at;
                u = rd_check[(size_t)g * 2 + 1 - at];
            }
    }
    // pos[i * 4 + q] = the kernel's stored edge (0 .. 3) that edge 2 + q of check i's ownership record becomes: tails 0 and 1, heads 2 and 3
    std::vector<int> pos((size_t)m * kRegPlaceStored, -1), ntail(m, 0), nhead(m, 0);
    for (int g = 0; g < n; g++) {
        const int at = tail[g], u = rd_check[(size_t)g * 2 + at], w = rd_check[(size_t)g * 2 + 1 - at];
        if (ntail[u] >= 2 || nhead[w] >= 2) return false;
        pos[(size_t)u * kRegPlaceStored + rd_edge[(size_t)g * 2 + at]] = ntail[u]++;
        pos[(size_t)w * kRegPlaceStored + rd_edge[(size_t)g * 2 + 1 - at]] = 2 + nhead[w]++;
    }
    for (int x : pos) if (x < 0) return false;

    rec.assign((size_t)block * kRegPlaceWords, 0);
    auto word = [&](int t, int w) -> int32_t & { return rec[(size_t)t * kRegPlaceWords + w]; };
    auto edges_word = [&]() {
        for (int s = 0; s < S; s++)
            for (int i = 0; i < m; i++)
                for (int q = 0; q < kRegPlaceStored; q++) word(lane(s, i), kRegPlaceEdges) |= (kRegOwnOwned + q) << (4 * pos[(size_t)i * kRegPlaceStored + q]);
    };
    if (!order) edges_word();                                                            // under an order: once the swaps below have settled who sits where

    // ---- posteriors: 32 colours, then Kempe moves for the two stores
    {
        RegPlaceColouring K;
        struct Item { int tail_lane, tail_k, head_lane, head_k, store_lane, v; };
        std::vector<Item> items;
        for (int s = 0; s < S; s++)
            for (int g = 0; g < n; g++) {
                const int at = tail[g], u = rd_check[(size_t)g * 2 + at], w = rd_check[(size_t)g * 2 + 1 - at];
                items.push_back({lane(s, u), pos[(size_t)u * kRegPlaceStored + rd_edge[(size_t)g * 2 + at]], lane(s, w),
                                 pos[(size_t)w * kRegPlaceStored + rd_edge[(size_t)g * 2 + 1 - at]] - 2, lane(s, g % m), g / m});
            }
        for (int d = 0; d < nspare; d++)
            for (int v = 0, t = spare_lane(d); v < kRegOwnOwned; v++) items.push_back({t, v, t, v, t, v});      // a lane of no team: gathers 0 and 2 read its item 0, 1 and 3 its item 1
        for (const Item &it : items) K.edges.emplace_back(it.tail_k * nwin + it.tail_lane / 32, it.head_k * nwin + it.head_lane / 32);
        if (!K.colour(2 * nwin, 2 * nwin, 32)) { rec.clear(); return false; }
        const int ni = (int)items.size();
        std::vector<int> grp(ni), cnt((size_t)2 * n16 * 16, 0), comp, mark(ni, -1), bad;
        for (int e = 0; e < ni; e++) { grp[e] = items[e].v * n16 + items[e].store_lane / 16; cnt[(size_t)grp[e] * 16 + (K.col[e] & 15)]++; }
        auto score = [&]() {                                                            // cycles above 6 per store wave-instruction first, array cycles second
            long long tot = 0, over = 0;
            for (int w = 0; w < 2 * n16; w += 4) {
                int cyc = 0;
                for (int g = w; g < w + 4; g++) cyc += *std::max_element(&cnt[(size_t)g * 16], &cnt[(size_t)g * 16] + 16);
                tot += cyc; over += std::max(0, cyc - 6);
            }
            return over * 100000 + tot;
        };
        auto recount = [&](const std::vector<int> &c, int d) { for (int x : c) cnt[(size_t)grp[x] * 16 + (K.col[x] & 15)] += d; };
        uint64_t state = 0x9e3779b97f4a7c15ull;                                          // splitmix64, constant seed
        auto rnd = [&](uint32_t below) {
            uint64_t z = (state += 0x9e3779b97f4a7c15ull);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; z ^= z >> 31;
            return (uint32_t)(((z >> 32) * below) >> 32);
        };
        // threshold accepting, as regular_own_polish: a move may raise the score by a bound that falls linearly to zero (greedy acceptance stalls within
        // 2000 moves); the best state seen is kept
        // Under an order every kRegPlaceSwapEvery-th move is a SWAP instead.  A ds_read_b64 serves 32-lane groups and a ds_write_b64 16-lane groups, and who
        // sits on which thread of a wave is free: two threads in different halves of one 32-lane group change places.  Every gather keeps its group, so the
        // colouring stays proper as it is; only the four posterior items the two threads store move to the other store group.  A swap is kept if the score
        // does not rise.  And the walk is run again from the Koenig colouring with another seed, up to kRegPlaceOrderedStarts times, while the best state
        // has 1 .. kRegPlaceRestartBelow cycles above 6 left: the walks end within a few cycles of each other, and on the BB matrices one of the first
        // four ends at none (profiles/r27_wave_classes.txt).  The identity order takes its one walk without swaps, as it always did.
        std::vector<int> at_pos(order ? block : 0), who(order ? block : 0), stores(order ? (size_t)block * 2 : 0, -1);      // at_pos[thread as dealt] = where it sits now; who = the inverse
        for (int t = 0; t < (int)at_pos.size(); t++) at_pos[t] = who[t] = t;
        if (order) for (int e = 0; e < ni; e++) stores[(size_t)items[e].store_lane * 2 + items[e].v] = e;
        auto move_thread = [&](int t, int to) {
            for (int v = 0; v < 2; v++) {
                const int e = stores[(size_t)t * 2 + v];
                if (e < 0) continue;
                cnt[(size_t)grp[e] * 16 + (K.col[e] & 15)]--;
                grp[e] = items[e].v * n16 + to / 16;
                cnt[(size_t)grp[e] * 16 + (K.col[e] & 15)]++;
            }
            at_pos[t] = to; who[to] = t;
        };
        long long cur = score(), best = cur;
        RegPlaceColouring best_K = K;
        std::vector<int> best_at = at_pos;
        const RegPlaceColouring K0 = K;
        const std::vector<int> cnt0 = cnt, grp0 = grp;
        const int starts = order ? kRegPlaceOrderedStarts : 1;
        for (int st = 0; st < starts; st++) {
        if (st) {
            if (best < 100000 || best > 100000LL * kRegPlaceRestartBelow + 99999) break;
            K = K0; cnt = cnt0; grp = grp0; cur = score();
            for (int t = 0; t < block; t++) at_pos[t] = who[t] = t;
            std::fill(mark.begin(), mark.end(), -1);
            state = 0x9e3779b97f4a7c15ull * (uint64_t)(2 * st + 1);
        }
        for (int mv = 0; mv < moves; mv++) {
            bad.clear();
            for (int e = 0; e < ni; e++) if (cnt[(size_t)grp[e] * 16 + (K.col[e] & 15)] > 1) bad.push_back(e);
            if (bad.empty()) break;
            if (order && mv % kRegPlaceSwapEvery == kRegPlaceSwapEvery - 1) {
                const int e = bad[rnd((uint32_t)bad.size())], ta = items[e].store_lane, pa = at_pos[ta];
                const int pb = (pa & ~31) | ((pa & 16) ^ 16) | (int)rnd(16), tb = who[pb];
                move_thread(ta, pb); move_thread(tb, pa);
                const long long now = score();
                if (now <= cur) {
                    cur = now;
                    if (cur < best) { best = cur; best_K = K; best_at = at_pos; }
                } else { move_thread(ta, pa); move_thread(tb, pb); }
                continue;
            }
            const int e = bad[rnd((uint32_t)bad.size())], a = K.col[e];
            int free_c[32], nfree = 0;
            for (int c = 0; c < 32; c++) if (c != a && cnt[(size_t)grp[e] * 16 + (c & 15)] == 0) free_c[nfree++] = c;
            const int b = nfree ? free_c[rnd((uint32_t)nfree)] : (a + 1 + (int)rnd(31)) & 31;
            K.component(e, a, b, comp, mark, mv);
            recount(comp, -1); K.flip(comp, a, b); recount(comp, +1);
            const long long now = score();
            if (now <= cur + (long long)kRegPlaceThreshold * (moves - mv) / moves) {
                cur = now;
                if (cur < best) { best = cur; best_K = K; best_at = at_pos; }
            } else { recount(comp, -1); K.flip(comp, a, b); recount(comp, +1); }
        }
        }
        if (best < cur || starts > 1) { K = best_K; at_pos = best_at; }
        if (!K.proper()) { rec.clear(); return false; }
        if (order) {
            // the threads as the swaps of the walk left them; the message colouring below is built on the result
            for (Item &it : items) { it.tail_lane = at_pos[it.tail_lane]; it.head_lane = at_pos[it.head_lane]; it.store_lane = at_pos[it.store_lane]; }
            for (int &t : ord.thread_of) t = at_pos[t];
            for (int &t : ord.spare) t = at_pos[t];
            std::sort(ord.spare.begin(), ord.spare.end());
            edges_word();
        }
        std::vector<int> rank(32, 0);
        for (int e = 0; e < ni; e++) {
            const int c = K.col[e], a = post_base + 32 * rank[c]++ + c;
            if (a >= post_base + post_words) { rec.clear(); return false; }
            const Item &it = items[e];
            word(it.tail_lane, kRegPlacePostGather + it.tail_k) = a;
            word(it.head_lane, kRegPlacePostGather + 2 + it.head_k) = a;
            word(it.store_lane, kRegPlacePostStore + it.v) = a;
        }
    }

    // ---- messages: 16 colours between (gather stream, 16-lane half-group) and (store stream, 16-lane group)
    {
        RegPlaceColouring K;
        struct Item { int read_lane, stream, store_lane, t; };
        std::vector<Item> items;
        for (int s = 0; s < S; s++)
            for (int i = 0; i < m; i++)
                for (int vd = 0; vd < 4; vd++) {
                    const int off = own[(size_t)i * kRegOwnWords + kRegOwnOffs + vd], r = off / rst, q = off - r * rst;
                    if (off < 0 || r >= m || q >= kRegPlaceStored) { rec.clear(); return false; }
                    items.push_back({lane(s, i), vd, lane(s, r), pos[(size_t)r * kRegPlaceStored + q]});
                }
        for (int d = 0; d < nspare; d++)
            for (int k = 0, t = spare_lane(d); k < 4; k++) items.push_back({t, k, t, k});
        for (const Item &it : items) K.edges.emplace_back(it.stream * n16 + it.read_lane / 16, it.t * n16 + it.store_lane / 16);
        if (!K.colour(4 * n16, 4 * n16, 16) || !K.proper()) { rec.clear(); return false; }
        std::vector<int> rank(32, 0);
        for (int e = 0; e < (int)items.size(); e++) {
            const Item &it = items[e];
            const int bank = K.col[e] + 16 * ((it.read_lane / 16) & 1), a = 32 * rank[bank]++ + bank;
            if (a >= msg_words) { rec.clear(); return false; }
            word(it.read_lane, kRegPlaceMsgGather + it.stream) = a;
            word(it.store_lane, kRegPlaceMsgStore + it.t) = a;
        }
    }
    if (order) {
        for (int s = 0; s < S; s++)
            for (int i = 0; i < m; i++) { const int t = lane(s, i); word(t, kRegPlaceOrder) = regular_place_pack(ord.wave_class[t / 64], s, i); }
        for (int d = 0; d < nspare; d++) { const int t = spare_lane(d); word(t, kRegPlaceOrder) = regular_place_pack(ord.wave_class[t / 64], S, 0); }
        *order = ord;                                                                   // the caller's order names the threads as the records do
    }
    return true;
}

}  // namespace qldpc
