// Prints the library's OSD-0 plan (csrc/osd_plan.h) for every "m n max_col_deg flags" line of standard input, one line each:
// path w16 block mode redo refused lds second-kernel second-block.  Host C++ only; tests/test_osd_plan_cpu.py compiles it and compares with osd_shapes.
#include <cstdio>

#include "osd_plan.h"

int main() {
    static const char *const names[] = {"NONE", "SMALL", "GJ", "GJG", "REFORDER_LDS", "REFORDER_UG", "GLOBAL"};
    for (int m, n, cdeg, flags; std::scanf("%d %d %d %d", &m, &n, &cdeg, &flags) == 4;) {
        const qldpc::Osd0Plan p = qldpc::osd0_plan(m, n, cdeg, flags);
        std::printf("%s %d %d %d %d %d %zu %s %d\n", names[p.path() + 1], (int)p.w16, p.first.block, p.detail() & QLDPC_OSD_DETAIL_MODE_MASK,
                    (p.detail() & QLDPC_OSD_DETAIL_REDO) != 0, p.refused != qldpc::kOsdAccepted, p.first.lds, names[p.second.kernel + 1], p.second.block);
    }
}
