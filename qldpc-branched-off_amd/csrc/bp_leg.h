// What Relay-BP (relay_bp.hip) and BP with guided decimation (decimation.hip) share: the slot tables of the graph handle as kernel
// arguments, one leg of thread-per-row / thread-per-column min-sum over the 24-byte compressed check record, and the launch of a
// persistent shot-queue kernel on the handle's workspaces.  The other workgroup kernels (minsum_wg*.hip, minsum_f32.hip,
// minsum_layered.hip) keep loops of their own: each has hooks this one lacks (damping slab, f32 record, lanes that split a row).
// Both users are built with -ffp-contract=off; the order of every floating-point operation below is what their numpy models pin.
#pragma once
#include "common.h"
#include "minsum_common.h"

#include <algorithm>

namespace qldpc {

// degree-ordered (slot) views of the graph handle (common.h)
struct SlotGraph {
    int m, n, cdeg;
    const int32_t *row_of_slot, *col_of_slot;
    const uint8_t *degr;           // [m] degree of the row in slot s
    const uint16_t *ell_col;       // [round_up(rdeg, 8)][m] by row slot
    const uint32_t *ell_var;       // [cdeg][n] by column slot: (row slot << 8) | position in the row, ascending rows
};

inline SlotGraph slot_graph(const qldpc_graph *g) {
    return SlotGraph{g->m, g->n, g->max_col_deg, g->d_row_of_slot, g->d_col_of_slot, g->d_deg_of_rslot, g->d_ell_col_s, g->d_ell_var_s};
}

struct LegResult { bool conv; int itc; };

// One leg of at most T iterations on shot b, from the marginals V as they stand (the first check pass takes Q = V, nothing subtracted):
//     check pass it = 0 .. T (one thread per row slot; pass it >= 1 also tests the syndrome of the V the pass before left),
//     variable pass it = 0 .. T - 1 (one thread per column slot):  V_j = s_j + bias(j, V_j),  s_j = 0.0 + sum of R in ascending check order.
// F[0], F[1] are the alternating unsat flags: the caller zeroes them (and whatever else of its own the leg start resets) and has a
// barrier behind that.  Returns whether V reproduces the syndrome and after how many iterations (T when it does not); the trailing
// barrier means every thread has read the flags, so the caller may reset them.
template <class Bias>
__device__ __forceinline__ LegResult bp_leg(const SlotGraph &G, const int8_t *synd, int64_t b, int T, double alpha, double clip, double *V,
                                            double2 *SP, unsigned long long *SI, int *F, Bias bias) {
    const int m = G.m, n = G.n, tid = threadIdx.x, NT = blockDim.x;
    LegResult res{false, T};
    for (int it = 0; it <= T; it++) {
        // ---------------- check pass (minsum_wg_kernel's, constant alpha) ----------------
        for (int i = tid; i < m; i += NT) {                                  // i = row slot
            const int deg = G.degr[i];
            const bool csyn = synd[b * m + G.row_of_slot[i]] & 1;
            double p1p = 0.0, p2p = 0.0;
            unsigned long long ip = 0ull;
            if (it > 0 && deg > 0) { const double2 t = SP[i]; p1p = t.x; p2p = t.y; ip = SI[i]; }
            bool par = csyn, sp = csyn;
            double min1 = INFINITY, min2 = INFINITY;
            int arg = 127;
            unsigned long long negbits = 0ull;
            for (int k = 0; k < deg; k++) {
                const int col = G.ell_col[(size_t)k * m + i];
                const double v = V[col];
                par ^= (v < 0.0);
                double x = v;                                                // the leg's first pass: Q = V[col], nothing subtracted
                if (it > 0) x = clip_nan(v - rec_message(p1p, p2p, ip, k), clip);
                const bool neg = !(x >= 0.0);
                sp ^= neg;
                negbits |= (unsigned long long)neg << k;
                const double a = fabs(x);
                if (a < min1) { min2 = min1; min1 = a; arg = k; }
                else if (a < min2) { min2 = a; }
            }
            if (it >= 1 && par) F[it & 1] = 1;
            if (it < T && deg > 0) {
                SP[i] = make_double2(alpha * min1, alpha * min2);
                SI[i] = rec_pack(negbits, arg, sp);
            }
        }
        __syncthreads();
        if (it >= 1 && F[it & 1] == 0) { res.conv = true; res.itc = it; break; }     // V holds values_{it-1}: it reproduces the syndrome
        if (it == T) break;
        if (tid == 0) F[(it + 1) & 1] = 0;
        // ---------------- variable pass ----------------
        for (int c = tid; c < n; c += NT) {                                  // c = column slot
            const int j = G.col_of_slot[c];
            double s = 0.0;
            for (int d = 0; d < G.cdeg; d++) {
                const uint32_t e = G.ell_var[(size_t)d * n + c];
                if (e == 0xFFFFFFFFu) break;
                const int i = (int)(e >> 8), k = (int)(e & 255u);
                const double2 pp = SP[i];
                const unsigned long long inf = SI[i];
                s += rec_message(pp.x, pp.y, inf, k);                        // ascending check order
            }
            V[j] = s + bias(j, V[j]);
        }
        __syncthreads();
    }
    __syncthreads();                                                         // every thread has read the flags before the caller resets them
    return res;
}

// The common head of the two kernels' LDS layouts, V | SP | SI (V leaves it in the VG form); returns the first byte behind it.
inline int leg_lds_prefix(const qldpc_graph *g, bool vg, int &offP, int &offI) {
    offP = vg ? 0 : (int)round_up((int64_t)g->n * 8, 16);
    offI = offP + g->m * 16;
    return (int)round_up(offI + (int64_t)g->m * 8, 16);
}

// Enqueues a persistent shot-queue kernel for B shots on the graph handle's workspaces: sets A.queue (zeroed in stream order) and
// A.vglobal (vg: one V[n] slab per workgroup).  Callers hold g->mu; the workspaces are handed over in stream order (common.h).
template <class Args>
int shot_queue_launch(const qldpc_graph *g, int64_t B, void (*kern)(Args), Args &A, size_t lds, bool vg, hipStream_t stream) {
    const int block = (g->m > 512 || g->n > 4096) ? 1024 : 512;
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>((160 * 1024) / (int64_t)lds, 2048 / block));
    const unsigned grid = (unsigned)std::min<int64_t>(B, (int64_t)cu_count(g->device) * per_cu);
    int rc = g->ws_acquire(stream);
    if (rc != QLDPC_OK) return rc;
    auto launch = [&]() -> int {
        int rcl = g->ws_queue.ensure(16);
        if (rcl != QLDPC_OK) return rcl;
        QLDPC_HIP_TRY(hipMemsetAsync(g->ws_queue.p, 0, 16, stream));
        A.queue = g->ws_queue.as<int>();
        A.vglobal = nullptr;
        if (vg) {
            if ((rcl = g->ws_vals.ensure((size_t)grid * g->n * 8)) != QLDPC_OK) return rcl;
            A.vglobal = g->ws_vals.as<double>();
        }
        if ((rcl = ensure_max_lds(g->device, reinterpret_cast<const void *>(kern), 160 * 1024)) != QLDPC_OK) return rcl;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, A);
        QLDPC_HIP_TRY(hipGetLastError());
        return QLDPC_OK;
    };
    rc = launch();
    const int rel = g->ws_release(stream);          // always: a failing call may have enqueued launches the next stream has to wait for
    return rc != QLDPC_OK ? rc : rel;
}

}  // namespace qldpc
