// Which kernels an OSD-0 call takes, decided before anything is launched: osd0_plan is arithmetic on (m, n, max_col_deg, flags) and reads top to bottom
// as the rule (a table in DESIGN.md 4); osd0_listed_launch (gf2.hip) executes it.  The LDS layouts of the row-transform kernels are here too, each written
// once for plan and launcher.  No HIP header: a host program can include this.  Two routes the code does not show:
//   * a column so heavy that GJG's layout no longer fits LDS can still fit the reference-order kernel's mode 2 (2 m + 704 bytes smaller or more), which
//     then takes EVERY shot; GLOBAL follows one degree later;
//   * a free-pivot kernel with no reference-order form behind it would be followed by GLOBAL on every shot of the original list.  No shape reaches
//     that: GJ and GJG need m <= 4096 and n < 65535 as the reference-order kernel does, and both their layouts exceed mode 2's, so mode 2 fits
//     wherever they do (1.2 M random points of m <= 31 000, n <= 66 000, column degree <= 300 under every flag set never took it).  Kept as the rule has it.
#pragma once
#include <stddef.h>
#include "../../include/qldpc_hip.h"

namespace qldpc {

constexpr int kOsdLdsMax = 160 * 1024;        // what every OSD launcher allows itself of a CU's LDS
constexpr int kOsdElimMax = 150 * 1024;       // ... and the literal elimination (eliminate_packed, gf2.hip) for its scratch
constexpr int kOsdChunk = 1024;               // columns per chunk of the row-transform kernels
constexpr int kOsdSortCnt = 256 * 16 * 4 + 16 * 4 + 64;      // [256][waves] radix counters + per-wave sums (osd_radix_passes)
constexpr int kGjBlock = 16;                  // columns per block of the free-pivot kernels
#ifndef QLDPC_OSD_BLOCK
#define QLDPC_OSD_BLOCK 16
#endif
constexpr int kOsdBlock = QLDPC_OSD_BLOCK;    // ... and of the reference-order kernel (4 per register of the resolving wave)

constexpr size_t osd_align(size_t x, size_t q) { return (x + q - 1) / q * q; }
// threads of a workgroup that gives every row of the transform (m + 2 of them) a thread, in whole waves
inline int osd_wide_block(int m) { const int t = (int)osd_align(m + 2 > 256 ? m + 2 : 256, 64); return t < 1024 ? t : 1024; }
// columns of the sorted head of the free-pivot kernels; choice < 0 (option "osd_presort" unset) = automatic: about m columns, whole chunks
inline int osd_presort_columns(int m, int choice) { return choice < 0 ? (int)osd_align(m > kOsdChunk ? m : kOsdChunk, kOsdChunk) : choice; }
// U (m + 2 rows of mw words) in LDS, aliased by the scratch of the column sort
inline size_t osd_u_or_sort_bytes(int m, int n, int mw) {
    const size_t u = (size_t)(m + 2) * mw * 8, sort = (size_t)n * 12 + 16 + kOsdSortCnt;
    return osd_align(u > sort ? u : sort, 16);
}
// LDS scratch of eliminate_packed (carve_elim, gf2.hip), and the row words the global kernel calls it with
inline size_t elim_lds_bytes(int m, int nwords) { return 16 + (size_t)nwords * 8 + (size_t)m * 4 + 8 + (size_t)m + 16; }
inline int osd_global_nwords(int n) { return ((n + 7) / 8 + 7) / 8; }
// the one-wave kernels: the matrix in LDS unless n <= 256 keeps its rows in registers
inline size_t osd_small_lds(int m, int n) { return (n <= 256 ? 0 : (size_t)m * ((n + 63) / 64 + 1) * 8) + (size_t)n * 11 + (size_t)m * 2 + 16; }

// ---- dynamic LDS of the three row-transform kernels: a layout writes the byte offsets of the pieces, in order, into the off* fields of the kernel's
// own argument struct (the plan hands in an OsdOffsets it throws away, for GJG as both structs) and returns the total ----
struct OsdCarve { size_t off; int take(size_t bytes) { const int at = (int)off; off += bytes; return at; } };
struct OsdOffsets { int offSort, offIdx, offAlive, offRows, offPc, offPr, offR, offUsed, offBlk, offTl, offMisc; };
template <class Args> size_t osd_gj_layout(int m, int n, int cdeg, Args &P) {      // osd0_gj_kernel
    const int mw = (m + 63) / 64;
    OsdCarve c{osd_u_or_sort_bytes(m, n, mw)};
    P.offIdx = c.take(kOsdChunk * 2); P.offAlive = c.take(kOsdChunk); P.offRows = c.take(osd_align((size_t)kOsdChunk * cdeg * 2, 8));
    P.offPc = c.take(osd_align(m * 2, 8)); P.offPr = c.take(osd_align(m * 2, 8)); P.offR = c.take((size_t)3 * kGjBlock * mw * 8);
    P.offUsed = c.take(32 * 8); P.offBlk = c.take((4 + 5 * kGjBlock + 8) * 4); P.offTl = c.take(osd_align((size_t)(m + 2) * 4, 16));
    return c.off + 16;
}
template <class Args, class Outer> size_t osd_gjg_layout(int m, int cdeg, Args &P, Outer &PP) {      // osd0_gjg_kernel (n does not enter); PP: OsdGjgArgs around P
    const int mw = (m + 63) / 64;
    OsdCarve c{0};
    PP.offSort = c.take(osd_align(kOsdSortCnt, 16));
    P.offIdx = c.take(kOsdChunk * 2); PP.offAlive = c.take(kOsdChunk); P.offRows = c.take(osd_align((size_t)kOsdChunk * cdeg * 2, 8));
    P.offPc = c.take(osd_align(m * 2, 8)); P.offPr = c.take(osd_align(m * 2, 8)); P.offR = c.take((size_t)kGjBlock * mw * 8);
    P.offUsed = c.take(128 * 8); P.offBlk = c.take((4 + 2 * kGjBlock + 4) * 4);
    return c.off + 16;
}
template <class Args> size_t osd_ref_layout(int m, int n, int cdeg, int mode, Args &P) {      // osd0_lds_kernel: mode 1 U in LDS; mode 2 U and the sort's keys in HBM / L2
    const int mw = (m + 63) / 64;
    OsdCarve c{mode == 1 ? osd_u_or_sort_bytes(m, n, mw) : 0};
    P.offIdx = c.take(kOsdChunk * 2); P.offAlive = c.take(kOsdChunk); P.offRows = c.take((size_t)kOsdChunk * cdeg * 2);
    P.offPc = c.take(osd_align(m * 2, 8)); P.offR = c.take((size_t)kOsdBlock * mw * 8); P.offBlk = c.take((4 + 6 * kOsdBlock + 4) * 4);
    P.offMisc = c.take(64); P.offSort = c.take(mode == 2 ? kOsdSortCnt : 0);
    return c.off + 16;
}

// ---- OSD-CS (osd_cs.hip): one kernel, two forms of its column sort.  U (m + 2 rows) is aliased by the 12 n bytes of sort scratch while the whole layout
// still fits beside it; beyond that the sort runs in global memory and U stands alone (global_sort).  TR is carved per order, so the edge moves with it.
// Returns the dynamic LDS bytes of the form taken, 0 when neither fits ----
constexpr int kCsChunk = 64;                  // columns per chunk of the OSD-CS sweep
constexpr int kCsMaxOrder = 64;
template <class Args> size_t osd_cs_layout(int m, int n, int order, Args &P, bool &global_sort) {
    const int mw = (m + 63) / 64;
    for (int lsort = 1; lsort >= 0; lsort--) {
        OsdCarve c{lsort ? osd_u_or_sort_bytes(m, n, mw) : osd_align((size_t)(m + 2) * mw * 8, 16)};
        P.offUsed = c.take(16 * 8); P.offPc = c.take(osd_align(m * 2, 8)); P.offPr = c.take(osd_align(m * 2, 8));
        P.offR = c.take((size_t)kCsChunk * mw * 8);                // (>= m * 8: the signed pivot weights of the scoring phase)
        P.offTR = c.take((size_t)(order > 1 ? order : 1) * mw * 8); P.offPf = c.take(osd_align((size_t)((n + 31) / 32) * 4, 16)); P.offMisc = c.take(2048);
        if (c.off + 16 <= (size_t)kOsdLdsMax) { global_sort = !lsort; return c.off + 16; }
    }
    return 0;
}

// ---- the plan ----
struct OsdLaunch { int kernel = QLDPC_OSD_PATH_NONE, block = 0; size_t lds = 0; };      // QLDPC_OSD_PATH_* of the kernel, threads, dynamic LDS bytes
enum OsdRefusal { kOsdAccepted = 0, kOsdRefusedQueue, kOsdRefusedSize };
struct Osd0Plan {
    OsdLaunch first;               // the kernel that is given every listed shot (NONE: an empty matrix, or refused)
    OsdLaunch second;              // behind a free-pivot kernel: REFORDER_* on the shots of ws_redo, or GLOBAL on every shot of the original list
    bool w16 = false;              // GJ: rows of 16 words at 1024 threads, osd0_gj_kernel<true>
    bool queue_first = false;      // experiments build under QLDPC_FLAG_OSD_QUEUE: osd_gjq.hip is tried before that form (its launcher says whether it fits)
    int mode = 0;                  // the reference-order form planned: 0 none, 1 transform in LDS, 2 in HBM / L2
    OsdRefusal refused = kOsdAccepted;
    int path() const { return first.kernel; }      // what qldpc_osd0_last_path reports
    int detail() const { return (mode & QLDPC_OSD_DETAIL_MODE_MASK) | (second.kernel != QLDPC_OSD_PATH_NONE ? QLDPC_OSD_DETAIL_REDO : 0); }
};

inline Osd0Plan osd0_plan(int m, int n, int max_col_deg, int flags) {
    Osd0Plan p;
    if (m < 1 || n < 1) return p;
    const int cdeg = max_col_deg > 1 ? max_col_deg : 1, mw = (m + 63) / 64;
    const size_t fits = kOsdLdsMax, no = fits + 1;
    OsdOffsets o;
    if (!(flags & (QLDPC_FLAG_OSD_LDS | QLDPC_FLAG_OSD_UG | QLDPC_FLAG_OSD_GLOBAL)) && m <= 128 && n <= 1024) {      // REFORDER alone does not leave the one-wave kernel
        p.first = OsdLaunch{QLDPC_OSD_PATH_SMALL, 64, osd_small_lds(m, n)};
        return p;
    }
#ifndef QLDPC_EXPERIMENTS
    if (flags & QLDPC_FLAG_OSD_QUEUE) { p.refused = kOsdRefusedQueue; return p; }      // product build: here, after the one-wave kernel had its chance
#endif
    const bool transform = m <= 4096 && n < 65535;      // row-transform kernels: at most 64 row words (one per lane), uint16 column tables padded with 65535
    const bool lds_u = m <= 1024 && !(flags & QLDPC_FLAG_OSD_UG), free_pivot = transform && !(flags & (QLDPC_FLAG_OSD_REFORDER | QLDPC_FLAG_OSD_GLOBAL));
    const bool ref_order = transform && !(flags & QLDPC_FLAG_OSD_GLOBAL);
    const size_t gj = free_pivot && lds_u ? osd_gj_layout(m, n, cdeg, o) : no, gjg = free_pivot ? osd_gjg_layout(m, cdeg, o, o) : no;
    const size_t ref1 = ref_order && lds_u ? osd_ref_layout(m, n, cdeg, 1, o) : no, ref2 = ref_order ? osd_ref_layout(m, n, cdeg, 2, o) : no;
    if (gj <= fits) p.first = OsdLaunch{QLDPC_OSD_PATH_GJ, osd_wide_block(m), gj};
    else if (gjg <= fits) p.first = OsdLaunch{QLDPC_OSD_PATH_GJG, 1024, gjg};
    p.w16 = gj <= fits && mw == 16 && p.first.block == 1024;
    p.queue_first = p.w16 && (flags & QLDPC_FLAG_OSD_QUEUE);
    p.mode = ref1 <= fits ? 1 : ref2 <= fits ? 2 : 0;
    const OsdLaunch ref = p.mode == 1 ? OsdLaunch{QLDPC_OSD_PATH_REFORDER_LDS, osd_wide_block(m), ref1} : OsdLaunch{QLDPC_OSD_PATH_REFORDER_UG, 1024, ref2};
    const OsdLaunch global{QLDPC_OSD_PATH_GLOBAL, (m >= 512 || n >= 2048) ? 1024 : 256, elim_lds_bytes(m, osd_global_nwords(n))};
    if (p.first.kernel != QLDPC_OSD_PATH_NONE) p.second = p.mode ? ref : global;      // (GLOBAL here is the route no shape reaches)
    else if (p.mode) p.first = ref;
    else if (global.lds > (size_t)kOsdElimMax) p.refused = kOsdRefusedSize;
    else p.first = global;
    return p;
}

}  // namespace qldpc
