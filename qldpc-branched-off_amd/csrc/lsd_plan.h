// BP+LSD (lsd.hip): the LDS layout of the cluster kernel and the acceptance rule, written once for launcher, plan and tests (tests/test_lsd_cpu.py
// mirrors the arithmetic).  No HIP header: a host program can include this.  What sets the size is the row cap max_rows, not m: the local transform U has
// max_rows + 1 rows of ceil(max_rows / 64) words (the extra row carries the reduced right-hand side); m enters with two bytes per row (the local index of
// a row of H) and n with two bits per column (member of A; picked in the round in flight).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qldpc {

constexpr int kLsdLdsMax = 160 * 1024;        // what the launcher allows itself of a CU's LDS
constexpr int kLsdBlock = 256;                // threads of a workgroup (one shot in flight per workgroup)
constexpr int kLsdMaxRows = 1024;             // max_rows: 1 .. 1024 (at most 16 row words)
constexpr int kLsdMaxBits = 64;               // bits_per_step: 1 .. 64
constexpr int kLsdListCap = 128;              // columns of a round kept in LDS; a longer round sorts its list in the workgroup's global scratch
constexpr int kLsdGrid = 512;                 // workgroups of a launch at most (a ticket counter hands out the listed shots)

constexpr size_t lsd_align(size_t x, size_t q) { return (x + q - 1) / q * q; }

struct LsdOffsets {
    int offUsed, offMask, offBestKey, offBestJ, offLidx, offInA, offPicked, offLabel, offCache, offCand, offRowg, offPivcol, offLastJ, offInvalid,
        offColLab, offListK, offListJ, offListS, offMisc;
};

// byte offsets of the pieces behind U (which starts at 0), in order; returns the dynamic LDS bytes of a workgroup
inline size_t lsd_layout(int m, int n, int cdeg, int max_rows, LsdOffsets &o) {
    const size_t mr = (size_t)max_rows, w = (mr + 63) / 64;
    size_t at = lsd_align((mr + 1) * w * 8, 16);
    const auto take = [&at](size_t bytes) { const int here = (int)at; at += lsd_align(bytes, 16); return here; };
    o.offUsed = take(w * 8);                     // rows that have pivoted
    o.offMask = take(w * 8);                     // the reduced column of the column being added, its pivot bit cleared
    o.offBestKey = take(mr * 8);                 // per label: least |llr| key among the candidates of the cluster
    o.offBestJ = take(mr * 4);                   // ... and the least column index among those of that key
    o.offLidx = take((size_t)m * 2);             // local index of a row of H (0xFFFF: not in R)
    o.offInA = take((size_t)((n + 31) / 32) * 4);
    o.offPicked = take((size_t)((n + 31) / 32) * 4);
    o.offLabel = take(mr * 2);                   // cluster of a local row: the least local index in it
    o.offCache = take(mr * 2);                   // least key among the row's columns outside A (rescanned when that column is added)
    o.offCand = take(mr * 2);                    // the row's candidate of the selection pass in flight
    o.offRowg = take(mr * 2);                    // row of H behind a local index
    o.offPivcol = take(mr * 2);                  // column that pivoted on a local row
    o.offLastJ = take(mr * 2);                   // per label: the cluster's previous pick of the round
    o.offInvalid = take(mr);                     // per label: 0 valid, 1 picking, 2 out of candidates
    o.offColLab = take((size_t)(cdeg > 1 ? cdeg : 1) * 2);      // labels of the rows of the column being added
    o.offListK = take((size_t)kLsdListCap * 8);
    o.offListJ = take((size_t)kLsdListCap * 2);
    o.offListS = take((size_t)kLsdListCap * 2);
    o.offMisc = take(64 * 4);
    return at;
}

// per workgroup in global memory: the round's columns unsorted [n] and sorted [n] (uint16), their keys [n] (uint64)
inline size_t lsd_scratch_bytes(int n) { return lsd_align((size_t)n * 12, 16); }

enum LsdRefusal { kLsdAccepted = 0, kLsdRefusedColumns, kLsdRefusedRows, kLsdRefusedLds };
// the graph and the cap: n < 65535 (uint16 column tables with two reserved values), m <= 65535 (uint16 row tables padded with m), and the layout at max_rows
// within 160 KiB
inline LsdRefusal lsd_supported(int m, int n, int cdeg, int max_rows) {
    if (n >= 65535) return kLsdRefusedColumns;
    if (m > 65535) return kLsdRefusedRows;
    LsdOffsets o;
    return lsd_layout(m, n, cdeg, max_rows, o) <= (size_t)kLsdLdsMax ? kLsdAccepted : kLsdRefusedLds;
}

}  // namespace qldpc
