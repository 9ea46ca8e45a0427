// Prints the layout HostStage gives a list of regions (csrc/stage_layout.h, the part of the helper that needs no device).  Every line of standard
// input is one list: "k" and then, k times, "nd d_1 ... d_nd elem" -- the element count as a product of nd signed dimensions, which is the form
// HostStage itself calls -- or "-1 count elem" with an unsigned count.  The answer is "ok total off_1 ... off_k", or "invalid" when a byte count does
// not fit size_t, a dimension is negative or there are more regions than the layout holds.  Host C++ only; tests/test_host_stage_cpu.py compiles it,
// also under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <initializer_list>

#include "stage_layout.h"

int main() {
    for (int k; std::scanf("%d", &k) == 1;) {
        qldpc::StageLayout L;
        for (int i = 0; i < k; i++) {
            int nd;
            long long d[4] = {1, 1, 1, 1};
            unsigned long long count = 0, elem;
            if (std::scanf("%d", &nd) != 1 || nd > 4) return 1;
            if (nd < 0 && std::scanf("%llu", &count) != 1) return 1;
            for (int j = 0; j < nd; j++) if (std::scanf("%lld", &d[j]) != 1) return 1;
            if (std::scanf("%llu", &elem) != 1) return 1;
            if (nd < 0) L.add((size_t)count, (size_t)elem);
            else if (nd == 0) L.add(std::initializer_list<int64_t>{}, (size_t)elem);
            else if (nd == 1) L.add({d[0]}, (size_t)elem);
            else if (nd == 2) L.add({d[0], d[1]}, (size_t)elem);
            else if (nd == 3) L.add({d[0], d[1], d[2]}, (size_t)elem);
            else L.add({d[0], d[1], d[2], d[3]}, (size_t)elem);
        }
        if (L.overflow) { std::printf("invalid\n"); continue; }
        std::printf("ok %zu", L.bytes());
        for (int i = 0; i < L.count; i++) std::printf(" %zu", L.regions[i].off);
        std::printf("\n");
    }
}
