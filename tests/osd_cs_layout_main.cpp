// Prints the library's OSD-CS layout (osd_cs_layout, csrc/osd_plan.h) for every "m n order" line of standard input, one line each:
// lds global_sort block offUsed offPc offPr offR offTR offPf offMisc (lds 0: neither sort form fits).  Host C++ only; tests/test_osd_cs_domain_cpu.py
// compiles it and compares with osd_cs_shapes.
#include <cstdio>

#include "osd_plan.h"

struct Offsets { int offUsed, offPc, offPr, offR, offTR, offPf, offMisc; };

int main() {
    for (int m, n, order; std::scanf("%d %d %d", &m, &n, &order) == 3;) {
        Offsets o{};
        bool gsort = false;
        const size_t lds = qldpc::osd_cs_layout(m, n, order, o, gsort);
        std::printf("%zu %d %d %d %d %d %d %d %d %d\n", lds, (int)gsort, qldpc::osd_wide_block(m), o.offUsed, o.offPc, o.offPr, o.offR, o.offTR, o.offPf, o.offMisc);
    }
}
