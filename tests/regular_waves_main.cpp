// Prints what the class-uniform waves of the regular (6,3) min-sum kernel are built from (csrc/regular_own.h: the min-last assignment; csrc/regular_place.h:
// the thread order and the placement under it), for every graph of standard input: "m n rst", then the m + 1 words of indptr, then indptr[m] column
// indices.  Arguments: force_S (0 = the plan's own S), max_iter of the plan (default 0).  Per graph: "none" where the graph has no ownership table or no
// plan, else
//   "ok <S> <TS> <block> <placed: 1, or 0 where the placement answered none>"
//   "minlast <owned last edges> <checks owning none> <one> <both>"
//   "waves <the class of each of the block / 64 waves: 0 mixed, 1 none, 2 one, 3 both>"
//   "thread_of <the S * m threads of the items slot * m + check>"
//   "identity <gather> <post_store> <post_store_over6> <msg_store> <msg_store_over6> <the 14 per-stream cycles>"   if placed: the bank-model table in the identity order
//   "ordered <the same 19 figures>"                                                                                if placed: the min-last table under the order
//   m lines of the 16 words of the bank-model ownership record, m lines of the min-last record, then (if placed) block lines of the ordered place record.
// Host C++ only; tests/test_regular_waves_cpu.py compiles it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "regular_place.h"

static void print_cost(const char *tag, const qldpc::RegPlaceCost &C) {
    std::printf("%s %lld %lld %lld %lld %lld", tag, C.gather, C.post_store, C.post_store_over6, C.msg_store, C.msg_store_over6);
    for (int s = 0; s < qldpc::kRegPlaceStreams; s++) std::printf(" %lld", C.stream[s]);
    std::printf("\n");
}

static void print_table(const std::vector<int32_t> &t, int words) {
    for (size_t i = 0; i < t.size(); i++) std::printf("%d%c", t[i], (i + 1) % words ? ' ' : '\n');
}

int main(int argc, char **argv) {
    const int force_S = argc > 1 ? std::atoi(argv[1]) : 0, max_iter = argc > 2 ? std::atoi(argv[2]) : 0;
    for (int m, n, rst; std::scanf("%d %d %d", &m, &n, &rst) == 3;) {
        if (m < 0 || m > (1 << 20)) return 1;
        std::vector<int32_t> indptr(m + 1), indices, own, minlast, ident, rec;
        for (int i = 0; i <= m; i++) if (std::scanf("%d", &indptr[i]) != 1) return 1;
        if (indptr[m] < 0 || indptr[m] > (1 << 24)) return 1;
        for (int i = 0; i < m; i++) if (indptr[i] < 0 || indptr[i] > indptr[i + 1]) return 1;
        indices.resize(indptr[m]);
        for (int e = 0; e < indptr[m]; e++) if (std::scanf("%d", &indices[e]) != 1) return 1;
        qldpc::RegPlan P{};
        qldpc::RegPlaceOrder O;
        if (!qldpc::regular_own_assign(m, n, indptr.data(), indices.data(), rst, own) ||
            !qldpc::regular_own_assign_minlast(m, n, indptr.data(), indices.data(), rst, minlast) ||
            !qldpc::plan_regular_shape(qldpc::kRegOwnCdeg, qldpc::kRegOwnVdeg, m, n, max_iter, qldpc::kRegOwnTeamThreads, force_S, P) ||
            !qldpc::regular_place_order(m, minlast.data(), P, O)) { std::printf("none\n"); continue; }
        const bool placed = qldpc::regular_place_build(m, minlast.data(), P, rst, rec, qldpc::kRegPlaceOrderedMoves, &O);
        const bool base = qldpc::regular_place_build(m, own.data(), P, rst, ident);
        std::printf("ok %d %d %u %d\n", P.S, P.TS, P.block, placed && base ? 1 : 0);
        int count[3] = {0, 0, 0};
        for (int i = 0; i < m; i++) count[qldpc::regular_own_class(minlast.data(), i)]++;
        std::printf("minlast %d %d %d %d\n", count[1] + 2 * count[2], count[0], count[1], count[2]);
        std::printf("waves");
        for (int c : O.wave_class) std::printf(" %d", c);
        std::printf("\nthread_of");
        for (int t : O.thread_of) std::printf(" %d", t);
        std::printf("\n");
        if (placed && base) {
            print_cost("identity", qldpc::regular_place_cost(ident.data(), (int)P.block));
            print_cost("ordered", qldpc::regular_place_cost(rec.data(), (int)P.block));
        }
        print_table(own, qldpc::kRegOwnWords);
        print_table(minlast, qldpc::kRegOwnWords);
        if (placed && base) print_table(rec, qldpc::kRegPlaceWords);
    }
}
