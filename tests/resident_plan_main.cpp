// Prints the resident min-sum kernel's plan (csrc/resident_plan.h) for every "m n nnz max_row_deg max_col_deg" line of standard input, one line
// each: ok cdeg vdeg cpt vpt TS S block lds.  Host C++ only; tests/test_resident_domain_cpu.py compiles it and compares with its own restatement.
#include <cstdio>

#include "resident_plan.h"

int main() {
    for (int m, n, rd, cd; ;) {
        long long nnz;
        if (std::scanf("%d %d %lld %d %d", &m, &n, &nnz, &rd, &cd) != 5) break;
        qldpc::ResidentPlan p{};
        if (!qldpc::plan_resident_shape(m, n, nnz, rd, cd, p)) { std::printf("0\n"); continue; }
        std::printf("1 %d %d %d %d %d %d %u %zu\n", p.cdeg, p.vdeg, p.cpt, p.vpt, p.TS, p.S, p.block, p.lds);
    }
}
