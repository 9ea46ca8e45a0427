// Prints the edge-ownership records of the regular (6,3) min-sum kernel (csrc/regular_own.h) for every graph of standard input: "m n rst", then the
// m + 1 words of indptr, then indptr[m] column indices.  Per graph: "none", or "ok" and m lines of the 16 words of a record.  Host C++ only;
// tests/test_regular_own_cpu.py compiles it and holds the records against the CSR.
#include <cstdio>
#include <vector>

#include "regular_own.h"

int main() {
    for (int m, n, rst; std::scanf("%d %d %d", &m, &n, &rst) == 3;) {
        if (m < 0 || m > (1 << 20)) return 1;
        std::vector<int32_t> indptr(m + 1), indices, tab;
        for (int i = 0; i <= m; i++) if (std::scanf("%d", &indptr[i]) != 1) return 1;
        if (indptr[m] < 0 || indptr[m] > (1 << 24)) return 1;
        indices.resize(indptr[m]);
        for (int e = 0; e < indptr[m]; e++) if (std::scanf("%d", &indices[e]) != 1) return 1;
        if (!qldpc::regular_own_assign(m, n, indptr.data(), indices.data(), rst, tab)) { std::printf("none\n"); continue; }
        std::printf("ok\n");
        for (int i = 0; i < m; i++)
            for (int w = 0; w < qldpc::kRegOwnWords; w++) std::printf("%d%c", tab[(size_t)i * qldpc::kRegOwnWords + w], w + 1 < qldpc::kRegOwnWords ? ' ' : '\n');
    }
}
