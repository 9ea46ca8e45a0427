// Prints the regular min-sum kernel's plan (csrc/regular_plan.h) for every "cdeg vdeg m n max_iter team_threads force_S" line of standard input, one
// line each: ok TS S block lds offV offE offL offI offA offT offD.  Host C++ only; tests/test_regular_plan_cpu.py compiles it and compares with its own carve.
#include <cstdio>

#include "regular_plan.h"

int main() {
    for (int cdeg, vdeg, m, n, max_iter, threads, force; std::scanf("%d %d %d %d %d %d %d", &cdeg, &vdeg, &m, &n, &max_iter, &threads, &force) == 7;) {
        qldpc::RegPlan p{};
        const bool ok = qldpc::plan_regular_shape(cdeg, vdeg, m, n, max_iter, threads, force, p);
        if (!ok) { std::printf("0\n"); continue; }
        std::printf("1 %d %d %u %zu %d %d %d %d %d %d %d\n", p.TS, p.S, p.block, p.lds, p.offV, p.offE, p.offL, p.offI, p.offA, p.offT, p.offD);
    }
}
