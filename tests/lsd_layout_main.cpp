// Prints the library's LSD layout (lsd_layout and lsd_supported, csrc/lsd_plan.h) for every "m n cdeg max_rows" line of standard input, one line each:
// lds supported offMisc.  Host C++ only; tests/test_lsd_cpu.py compiles it and compares with the mirror in tests/lsd_shapes.py.
#include <cstdio>

#include "lsd_plan.h"

int main() {
    for (int m, n, cdeg, rows; std::scanf("%d %d %d %d", &m, &n, &cdeg, &rows) == 4;) {
        qldpc::LsdOffsets o{};
        const size_t lds = qldpc::lsd_layout(m, n, cdeg, rows, o);
        std::printf("%zu %d %d\n", lds, (int)(qldpc::lsd_supported(m, n, cdeg, rows) == qldpc::kLsdAccepted), o.offMisc);
    }
}
