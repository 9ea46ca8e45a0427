// Prints which edge-ownership assignment the regular (6,3) min-sum kernel takes (csrc/regular_own.h) and what the bank model charges it, for every graph
// of standard input: "m n rst", then the m + 1 words of indptr, then indptr[m] column indices.  Per graph: "none", or
//   "ok <kind> <L> <M> <cyclic candidates priced> <S> <TS> <block> <offV> <offD>"      kind: kuhn, cyclic or searched; L x M: the torus of a cyclic choice
//   "kuhn <cost> <the eight per-stream costs>"                                         regular_own_cost of the assignment without search, one workgroup
//   "chosen <cost> <the eight per-stream costs>"
//   m lines of the 16 words of a record of the chosen table.
// An argument "0" asks for the table without search (regular_own_search 0).  Host C++ only; tests/test_regular_own_search_cpu.py compiles it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "regular_own.h"

int main(int argc, char **argv) {
    const int search = argc > 1 ? std::atoi(argv[1]) : 1;
    static const char *kinds[] = {"kuhn", "cyclic", "searched"};
    for (int m, n, rst; std::scanf("%d %d %d", &m, &n, &rst) == 3;) {
        if (m < 0 || m > (1 << 20)) return 1;
        std::vector<int32_t> indptr(m + 1), indices, tab;
        for (int i = 0; i <= m; i++) if (std::scanf("%d", &indptr[i]) != 1) return 1;
        if (indptr[m] < 0 || indptr[m] > (1 << 24)) return 1;
        for (int i = 0; i < m; i++) if (indptr[i] < 0 || indptr[i] > indptr[i + 1]) return 1;
        indices.resize(indptr[m]);
        for (int e = 0; e < indptr[m]; e++) if (std::scanf("%d", &indices[e]) != 1) return 1;
        qldpc::RegOwnChoice C;
        qldpc::RegPlan P{};
        if (!qldpc::regular_own_assign(m, n, indptr.data(), indices.data(), rst, tab, search, &C) || !qldpc::regular_own_plan(m, P)) { std::printf("none\n"); continue; }
        std::printf("ok %s %d %d %d %d %d %u %d %d\n", kinds[C.kind], C.L, C.M, C.candidates, P.S, P.TS, P.block, P.offV, P.offD);
        std::printf("kuhn %lld", C.kuhn_cost);
        for (int s = 0; s < qldpc::kRegOwnStreams; s++) std::printf(" %lld", C.kuhn_stream[s]);
        std::printf("\nchosen %lld", C.cost);
        for (int s = 0; s < qldpc::kRegOwnStreams; s++) std::printf(" %lld", C.stream[s]);
        std::printf("\n");
        for (int i = 0; i < m; i++)
            for (int w = 0; w < qldpc::kRegOwnWords; w++) std::printf("%d%c", tab[(size_t)i * qldpc::kRegOwnWords + w], w + 1 < qldpc::kRegOwnWords ? ' ' : '\n');
    }
}
