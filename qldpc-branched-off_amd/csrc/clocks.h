// The clocks a kernel reads: the shader-clock probe of a production launch and the phase timers of the diagnostic build.
// Device header: only what can reach a kernel's instruction stream (device functions, kernel argument structs shared between files, constants
// and macros kernel bodies name).  Prototypes and host-only structs live in launchers.h; tools/isa_mix.py RECORDED lists this file per kernel.
#pragma once
#include <hip/hip_runtime.h>

// Phase timers of the OSD kernels exist only in the diagnostic build (`make timers` -> libqldpc_hip_timers.so, -DQLDPC_OSD_TIMERS);
// the default build carries no clock reads.  Counters (uint64[32]; [16..22] belong to the workgroup BP kernel: wave-iterations, check pass, its barrier, freeze, variable pass, its barrier): [0] shots, [1] chunks, [2] columns taken into blocks, [3] pivots,
// [4] cycles, [5] kill passes, [6] blocks, [8] sort, [9] phase 1 (reduce columns), [10] phase 2 (block pivots), [11] phase 3 (row updates),
// [12] dependent-column tests, [13] back-substitution.
#ifdef QLDPC_OSD_TIMERS
#define OSD_CLOCK() clock64()
#else
#define OSD_CLOCK() 0ll
#endif

namespace qldpc {

// Shader-clock probe (QLDPC_FLAG_CLOCK_PROBE): thread 0 of a workgroup stamps the shader-clock counter (s_memtime) and the constant
// 100 MHz counter (s_memrealtime) when it starts and when it ends; clock held under this kernel's load = delta ratio x 100 MHz
// (MI355X_MICROARCH.md, DVFS give-back item 6).  Buffer: kClkSlots pairs (delta memtime, delta memrealtime) indexed by blockIdx.x.
constexpr int kClkSlots = 512;
struct ClkStamp { unsigned long long t = 0, r = 0; };
__device__ __forceinline__ ClkStamp clk_begin(const unsigned long long *clk) {
    ClkStamp s;
    if (clk) { s.t = __builtin_amdgcn_s_memtime(); s.r = __builtin_amdgcn_s_memrealtime(); }
    return s;
}
__device__ __forceinline__ void clk_end(unsigned long long *clk, const ClkStamp &s) {
    if (clk && threadIdx.x == 0 && blockIdx.x < kClkSlots) {
        clk[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - s.t;
        clk[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - s.r;
    }
}

}  // namespace qldpc
