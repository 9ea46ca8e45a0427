// Prints the LDS placement table of the regular (6,3) min-sum kernel (csrc/regular_place.h) and what its bank model charges, for every graph of standard
// input: "m n rst", then the m + 1 words of indptr, then indptr[m] column indices.  Arguments: force_S (0 = the plan's own S), max_iter of the plan
// (default 0), Kempe moves (default: the header's).  Per graph: "none" where the graph has no ownership table or no plan, else
//   "ok <S> <TS> <block> <offV> <offD> <span bytes: offV + S * n * 8> <placed: 1, or 0 where the header answered none and only the linear lines follow>"
//   "linear <gather> <post_store> <post_store_over6> <msg_store> <msg_store_over6> <the 14 per-stream cycles>"      today's addresses as a table
//   "own_cost <regular_own_cost of the ownership table at this plan>"
//   "placed <the same 19 figures>"                                                                                  only if placed
//   m lines of the 16 words of the ownership record, block lines of the 16 words of the linear record, then (if placed) block lines of the placed record.
// Host C++ only; tests/test_regular_place_cpu.py compiles it.
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
    const int moves = argc > 3 ? std::atoi(argv[3]) : qldpc::kRegPlaceKempeMoves;
    for (int m, n, rst; std::scanf("%d %d %d", &m, &n, &rst) == 3;) {
        if (m < 0 || m > (1 << 20)) return 1;
        std::vector<int32_t> indptr(m + 1), indices, own, lin, rec;
        for (int i = 0; i <= m; i++) if (std::scanf("%d", &indptr[i]) != 1) return 1;
        if (indptr[m] < 0 || indptr[m] > (1 << 24)) return 1;
        for (int i = 0; i < m; i++) if (indptr[i] < 0 || indptr[i] > indptr[i + 1]) return 1;
        indices.resize(indptr[m]);
        for (int e = 0; e < indptr[m]; e++) if (std::scanf("%d", &indices[e]) != 1) return 1;
        qldpc::RegPlan P{};
        if (!qldpc::regular_own_assign(m, n, indptr.data(), indices.data(), rst, own) ||
            !qldpc::plan_regular_shape(qldpc::kRegOwnCdeg, qldpc::kRegOwnVdeg, m, n, max_iter, qldpc::kRegOwnTeamThreads, force_S, P)) { std::printf("none\n"); continue; }
        qldpc::regular_place_linear(m, own.data(), P, rst, lin);
        const bool placed = qldpc::regular_place_build(m, own.data(), P, rst, rec, moves);
        std::printf("ok %d %d %u %d %d %d %d\n", P.S, P.TS, P.block, P.offV, P.offD, P.offV + P.S * n * 8, placed ? 1 : 0);
        print_cost("linear", qldpc::regular_place_cost(lin.data(), (int)P.block));
        std::printf("own_cost %lld\n", qldpc::regular_own_cost(m, own.data(), P, rst));
        if (placed) print_cost("placed", qldpc::regular_place_cost(rec.data(), (int)P.block));
        print_table(own, qldpc::kRegOwnWords);
        print_table(lin, qldpc::kRegPlaceWords);
        if (placed) print_table(rec, qldpc::kRegPlaceWords);
    }
}
