// Layered-schedule normalised min-sum (semantics: include/qldpc_hip.h, qldpc_layered_decoder_create).
//
// The flooding decoders read every posterior, then update every posterior.  Here the checks are cut into layers whose members share no column;
// a layer reads the posteriors the layers before it left, so one iteration carries information across the whole graph.  The state is the one
// minsum_wg*.hip keep: the posteriors V[n] and a 24-byte record per check (alpha*min1, alpha*min2, argmin, sign bits) from which the old
// message of an edge is rebuilt.  Inside a layer every V_j is touched by one check at most, so no floating-point sum has an order to choose and
// the kernel equals the numpy model (tests/layered_model.py) bit for bit whatever the lane assignment.
//
// One workgroup per shot, persistent grid over an atomic shot queue.  The host orders the non-empty rows by (layer, row) into SLOTS and gives
// every layer 2^lg lanes per check (at most 8 edges per lane, so a row's 56 edges need lg >= 3; more lanes while the layer still fits the
// workgroup).  A lane scans its edges k = sub, sub + 2^lg, ... with the reference's strict-< rule; the lanes of a check combine
// (min1, position) lexicographically through wave shuffles, so the argmin is the FIRST position of the minimum in ascending column order.
// One workgroup barrier per layer; the syndrome test after the last layer is one more (__syncthreads_or).
// LDS: V (or a per-workgroup slab in HBM/L2 when it does not fit: VG), the records, the slot edge offsets, the shot's syndrome bits by slot,
// the layer table and -- when n <= 65535 and they still fit -- the column indices as u16 in slot order (else int32 in L2).
// Every loop is bounded by the host tables and max_iter.
#include "common.h"
#include "launchers.h"
#include "minsum_common.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace qldpc {

constexpr int kLayeredLds = 160 * 1024 - 512;   // dynamic LDS of a workgroup: a CU's 160 KB less the kernel's static 256 bytes (__syncthreads_or), rounded
constexpr int kLayeredRowDeg = 56;        // sign bits of a record
constexpr int kLayeredLaneEdges = 8;      // edges a lane holds in registers

struct LayeredArgs {
    int m, n, nslots, nlayers, nnz;
    const uint32_t *layer;         // [nlayers + 1] first slot of the layer | lg << 24 (the last entry: nslots)
    const int32_t *slot_row;       // [m] row of slot s; the rows without entries follow the nslots others
    const uint32_t *estart;        // [nslots + 1] edge offsets in slot order
    const uint16_t *idx16;         // [nnz] columns in slot order (n <= 65535), copied to LDS by the IDXL form
    const int32_t *idx32;          // [nnz] the same as int32: read from HBM/L2 by the other form
    int64_t B;
    const int8_t *synd;
    const double *prior, *alpha;
    int max_iter;
    double clip;
    int8_t *out_err; double *out_llr; uint8_t *out_conv; int32_t *out_iter;
    int offP, offI, offE, offL, offS, offX, offF;
    double *vglobal;               // VG: V[n] per workgroup
    int *queue;                    // next shot (zeroed before the launch)
};

template <bool VG, bool IDXL>
__global__ __launch_bounds__(1024) void minsum_layered_kernel(LayeredArgs A) {
    extern __shared__ unsigned char lds[];
    double *V;
    if (VG) V = A.vglobal + (size_t)blockIdx.x * A.n; else V = reinterpret_cast<double *>(lds);
    double2 *SP = reinterpret_cast<double2 *>(lds + A.offP);                       // (alpha*min1, alpha*min2) per slot
    unsigned long long *SI = reinterpret_cast<unsigned long long *>(lds + A.offI); // bits 0-55 input signs, 56-62 argmin (127 = none), 63 total sign
    uint32_t *ES = reinterpret_cast<uint32_t *>(lds + A.offE);
    uint32_t *LY = reinterpret_cast<uint32_t *>(lds + A.offL);
    uint8_t *SY = lds + A.offS;
    const uint16_t *IX = reinterpret_cast<const uint16_t *>(lds + A.offX);
    int *F = reinterpret_cast<int *>(lds + A.offF);                                // [0] shot, [1] a row without entries has syndrome 1
    const int n = A.n, m = A.m, ns = A.nslots, tid = threadIdx.x, NT = blockDim.x;
    const double clip = A.clip;
    auto col_of = [&](uint32_t e) -> int { return IDXL ? (int)IX[e] : A.idx32[e]; };

    for (int i = tid; i <= ns; i += NT) ES[i] = A.estart[i];
    for (int i = tid; i <= A.nlayers; i += NT) LY[i] = A.layer[i];
    if (IDXL) {
        uint16_t *W = reinterpret_cast<uint16_t *>(lds + A.offX);
        for (int e = tid; e < A.nnz; e += NT) W[e] = A.idx16[e];
    }
    for (;;) {
        if (tid == 0) { F[0] = atomicAdd(A.queue, 1); F[1] = 0; }
        __syncthreads();
        const int64_t b = F[0];
        if (b >= A.B) break;
        const int8_t *syn = A.synd + b * m;
        for (int j = tid; j < n; j += NT) V[j] = A.prior[j];
        for (int i = tid; i < m; i += NT) {
            const int s = syn[A.slot_row[i]] & 1;
            if (i < ns) { SY[i] = (uint8_t)s; SP[i] = make_double2(0.0, 0.0); SI[i] = 0ull; }          // R = +0.0 on every edge
            else if (s) F[1] = 1;
        }
        __syncthreads();
        bool conv = false;
        int itc = A.max_iter - 1;
        for (int it = 0; it < A.max_iter; it++) {
            const double alpha = A.alpha[it];
            for (int L = 0; L < A.nlayers; L++) {
                const uint32_t w = LY[L];
                const int first = (int)(w & 0xFFFFFFu), cnt = (int)(LY[L + 1] & 0xFFFFFFu) - first, lg = (int)(w >> 24);
                const int lpc = 1 << lg, sub = tid & (lpc - 1), ngrp = NT >> lg;
                for (int c = tid >> lg; c < cnt; c += ngrp) {                        // (the lanes of a check share c)
                    const int slot = first + c;
                    const uint32_t e0 = ES[slot];
                    const int deg = (int)(ES[slot + 1] - e0);
                    const double2 old = SP[slot];
                    const unsigned long long ip = SI[slot];
                    const int argp = rec_argmin(ip);
                    const bool spp = (ip >> 63) & 1;                                 // (rec_total_sign / rec_message here change the compiler's schedule of the edge loop: spelled out)
                    double q[kLayeredLaneEdges];
                    int cols[kLayeredLaneEdges];
                    double min1 = INFINITY, min2 = INFINITY;
                    int pos = 127;
                    unsigned long long negbits = 0ull;
#pragma unroll
                    for (int t = 0; t < kLayeredLaneEdges; t++) {
                        const int k = sub + (t << lg);
                        if (k < deg) {
                            const int col = col_of(e0 + k);
                            const double mag = (k == argp) ? old.y : old.x;
                            const double rr = (spp != (bool)((ip >> k) & 1)) ? -mag : mag;
                            const double x = clip_nan(V[col] - rr, clip);
                            cols[t] = col; q[t] = x;
                            negbits |= (unsigned long long)(x < 0.0) << k;
                            const double a = fabs(x);
                            if (a < min1) { min2 = min1; min1 = a; pos = k; }
                            else if (a < min2) { min2 = a; }
                        }
                    }
                    for (int off = lpc >> 1; off > 0; off >>= 1) {                   // lexicographic (|Q|, position) over the check's lanes
                        const double o1 = __shfl_xor(min1, off, 64), o2 = __shfl_xor(min2, off, 64);
                        const int op = __shfl_xor(pos, off, 64);
                        negbits |= __shfl_xor(negbits, off, 64);
                        const bool take = o1 < min1 || (o1 == min1 && op < pos);
                        const double lose = take ? min1 : o1, w2 = take ? o2 : min2;
                        min1 = take ? o1 : min1;
                        pos = take ? op : pos;
                        min2 = lose < w2 ? lose : w2;
                    }
                    const bool sp = (bool)SY[slot] != (bool)(__popcll(negbits) & 1);
                    const double a1 = alpha * min1, a2 = alpha * min2;
                    if (sub == 0) {
                        SP[slot] = make_double2(a1, a2);
                        SI[slot] = rec_pack(negbits, pos, sp);
                    }
#pragma unroll
                    for (int t = 0; t < kLayeredLaneEdges; t++) {
                        const int k = sub + (t << lg);
                        if (k < deg) {
                            const double mag = (k == pos) ? a2 : a1;
                            const double r = (sp != (bool)((negbits >> k) & 1)) ? -mag : mag;
                            V[cols[t]] = q[t] + r;
                        }
                    }
                }
                __syncthreads();
            }
            int bad = F[1];
            for (int slot = tid; slot < ns; slot += NT) {
                int par = SY[slot];
                for (uint32_t e = ES[slot]; e < ES[slot + 1]; e++) par ^= (int)(V[col_of(e)] < 0.0);
                bad |= par;
            }
            if (!__syncthreads_or(bad)) { conv = true; itc = it; break; }
        }
        for (int j = tid; j < n; j += NT) {
            const double v = V[j];
            A.out_llr[b * n + j] = v;
            A.out_err[b * n + j] = (v < 0.0) ? 1 : 0;
        }
        if (tid == 0) { A.out_conv[b] = conv ? 1 : 0; A.out_iter[b] = itc; }
        __syncthreads();
    }
}

// Greedy colouring in ascending row order: the smallest layer no earlier row sharing a column holds (a row without entries: layer 0).
static int greedy_layers(const qldpc_graph *g, std::vector<int32_t> &layer) {
    const int m = g->m;
    layer.assign(m, 0);
    std::vector<int32_t> stamp(m + 1, -1);
    int layers = 0;
    for (int i = 0; i < m; i++) {
        for (int e = g->indptr[i]; e < g->indptr[i + 1]; e++) {
            const int j = g->indices[e];
            for (int k = g->colptr[j]; k < g->colptr[j + 1] && g->rowidx[k] < i; k++) stamp[layer[g->rowidx[k]]] = i;
        }
        int c = 0;
        while (stamp[c] == i) c++;
        layer[i] = c;
        layers = std::max(layers, c + 1);
    }
    return layers;
}

}  // namespace qldpc

using namespace qldpc;

struct qldpc_layered_decoder : DecoderBase {      // (the VG slab is handed from stream to stream with the queue word)
    int nnz = 0;
    double clip = 20;
    int nlayers = 0, nslots = 0, max_rows = 0, max_edges = 0;
    bool vg = false, idxl = false;
    int offP = 0, offI = 0, offE = 0, offL = 0, offS = 0, offX = 0, offF = 0;
    std::vector<int32_t> row_layer;
    DevBuf d_layer, d_slot_row, d_estart, d_idx16, d_idx32, d_vglobal;
    ~qldpc_layered_decoder() { quiesce(device, hand); }
    int launch(int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t s);
};

// Enqueues the decode of B shots on `s`.  Callers hold mu.
int qldpc_layered_decoder::launch(int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t s) {
    LayeredArgs A;
    A.m = m; A.n = n; A.nslots = nslots; A.nlayers = nlayers; A.nnz = nnz;
    A.layer = d_layer.as<uint32_t>(); A.slot_row = d_slot_row.as<int32_t>(); A.estart = d_estart.as<uint32_t>();
    A.idx16 = d_idx16.as<uint16_t>(); A.idx32 = d_idx32.as<int32_t>();
    A.B = B; A.synd = d_synd; A.prior = d_prior.as<double>(); A.alpha = d_alpha.as<double>(); A.max_iter = max_iter; A.clip = clip;
    A.out_err = d_err; A.out_llr = d_llr; A.out_conv = d_conv; A.out_iter = d_iter;
    A.offP = offP; A.offI = offI; A.offE = offE; A.offL = offL; A.offS = offS; A.offX = offX; A.offF = offF;
    A.vglobal = d_vglobal.as<double>(); A.queue = d_queue.as<int>();
    void (*kern)(LayeredArgs) = vg ? (idxl ? minsum_layered_kernel<true, true> : minsum_layered_kernel<true, false>)
                                   : (idxl ? minsum_layered_kernel<false, true> : minsum_layered_kernel<false, false>);
    return decoder_launch(*this, kern, kLayeredLds, A, B, s);
}

namespace qldpc {

static int ceil_log2(int x) { int l = 0; while ((1 << l) < x) l++; return l; }

// Creation on a ready alpha table (the circuit plan holds one per sector); the exported form builds the table from the alpha mode.
int layered_decoder_create_tab(const qldpc_graph *g, const int32_t *row_layer, const double *prior, int max_iter, const std::vector<double> &tab,
                               double clip_llr, int flags, qldpc_layered_decoder **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(g != nullptr && prior != nullptr, "NULL argument");
    QLDPC_REQUIRE(max_iter >= 1, "max_iter must be >= 1 (got %d)", max_iter);
    QLDPC_REQUIRE(clip_llr > 0.0, "clip_llr must be > 0 (got %g)", clip_llr);
    const int m = g->m, n = g->n;
    const int fb = flags & (QLDPC_FLAG_LAYERED_BLOCK_256 | QLDPC_FLAG_LAYERED_BLOCK_512 | QLDPC_FLAG_LAYERED_BLOCK_1024);
    QLDPC_REQUIRE((fb & (fb - 1)) == 0, "more than one QLDPC_FLAG_LAYERED_BLOCK_* flag");
    QLDPC_USE_DEVICE(g->device);                                    // ahead of D: a return deletes D on its device, then the caller's device comes back
    std::unique_ptr<qldpc_layered_decoder> D(new qldpc_layered_decoder());
    D->device = g->device;
    // ---- layers: the caller's (validated) or the greedy colouring, then compressed to 0 .. nlayers - 1 in ascending order
    if (row_layer) {
        for (int i = 0; i < m; i++) QLDPC_REQUIRE(row_layer[i] >= 0, "row_layer[%d] = %d is negative", i, row_layer[i]);
        D->row_layer.assign(row_layer, row_layer + m);
    } else {
        greedy_layers(g, D->row_layer);
    }
    std::vector<int32_t> order;                                     // the rows with entries by (layer, row)
    for (int i = 0; i < m; i++) if (g->indptr[i + 1] > g->indptr[i]) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return D->row_layer[a] < D->row_layer[b]; });
    if (row_layer) {                                                // two rows of one layer share no column
        std::vector<int32_t> seen_layer(n, -1), seen_row(n, -1);
        for (int i : order)
            for (int e = g->indptr[i]; e < g->indptr[i + 1]; e++) {
                const int j = g->indices[e];
                QLDPC_REQUIRE(seen_layer[j] != row_layer[i], "rows %d and %d are both in layer %d and share column %d", seen_row[j], i, row_layer[i], j);
                seen_layer[j] = row_layer[i]; seen_row[j] = i;
            }
    }
    // ---- what the kernel holds
    if (m < 1 || n < 1 || n >= (1 << 24) || m >= (1 << 24)) { set_error("the layered decoder needs 1 <= m, n < 2^24 (m=%d n=%d)", m, n); return QLDPC_ERR_UNSUPPORTED; }
    if (g->max_row_deg > kLayeredRowDeg) {
        set_error("the layered decoder supports row degree <= %d (this graph: %d)", kLayeredRowDeg, g->max_row_deg);
        return QLDPC_ERR_UNSUPPORTED;
    }
    const int ns = (int)order.size(), nnz = g->nnz;
    std::vector<int32_t> slot_row(order);
    for (int i = 0; i < m; i++) if (g->indptr[i + 1] == g->indptr[i]) slot_row.push_back(i);
    std::vector<uint32_t> estart(ns + 1, 0), layer;
    std::vector<int32_t> idx32;
    std::vector<uint16_t> idx16;
    idx32.reserve(nnz);
    std::vector<int> lfirst, lmaxdeg;
    for (int s = 0; s < ns; s++) {
        const int i = order[s], deg = g->indptr[i + 1] - g->indptr[i];
        if (s == 0 || D->row_layer[i] != D->row_layer[order[s - 1]]) { lfirst.push_back(s); lmaxdeg.push_back(0); }
        lmaxdeg.back() = std::max(lmaxdeg.back(), deg);
        idx32.insert(idx32.end(), g->indices.begin() + g->indptr[i], g->indices.begin() + g->indptr[i + 1]);
        estart[s + 1] = (uint32_t)idx32.size();
    }
    const int nl = (int)lfirst.size();
    lfirst.push_back(ns);
    for (int L = 0; L < nl; L++) {
        const int cnt = lfirst[L + 1] - lfirst[L];
        D->max_rows = std::max(D->max_rows, cnt);
        D->max_edges = std::max(D->max_edges, (int)(estart[lfirst[L + 1]] - estart[lfirst[L]]));
    }
    D->g = g; D->device = g->device; D->m = m; D->n = n; D->nnz = nnz; D->max_iter = max_iter; D->flags = flags & QLDPC_FLAG_PUBLIC_MASK; D->clip = clip_llr;
    D->nlayers = nl; D->nslots = ns;
    // workgroup size: by the edges of an average layer (a small layer leaves most of a large workgroup at the barrier for nothing)
    const int mean_edges = nl ? nnz / nl : 0;
    D->block = fb == QLDPC_FLAG_LAYERED_BLOCK_256 ? 256 : fb == QLDPC_FLAG_LAYERED_BLOCK_512 ? 512 : fb == QLDPC_FLAG_LAYERED_BLOCK_1024 ? 1024
               : mean_edges <= 512 ? 256 : mean_edges <= 1024 ? 512 : 1024;
    for (int L = 0; L < nl; L++) {      // lanes per check: at most 8 edges per lane; more lanes while the layer fits the workgroup and a lane has an edge
        const int cnt = lfirst[L + 1] - lfirst[L], lgmax = ceil_log2(std::max(lmaxdeg[L], 1));
        int lg = ceil_log2((lmaxdeg[L] + kLayeredLaneEdges - 1) / kLayeredLaneEdges);
        while (lg < lgmax && lg < 6 && ((int64_t)cnt << (lg + 1)) <= D->block) lg++;
        layer.push_back((uint32_t)lfirst[L] | ((uint32_t)lg << 24));
    }
    layer.push_back((uint32_t)ns);
    // LDS layout: [V] | records | edge offsets | layer table | syndrome bits | [column indices] | flags
    auto layout = [&](bool vg, bool idxl) {
        D->offP = vg ? 0 : (int)round_up((int64_t)n * 8, 16);
        int64_t o = D->offP;
        D->offI = (int)(o += (int64_t)ns * 16);
        D->offE = (int)(o += (int64_t)ns * 8);
        D->offL = (int)(o += (int64_t)(ns + 1) * 4);
        D->offS = (int)(o += (int64_t)(nl + 1) * 4);
        D->offX = (int)(o = round_up(o + ns, 16));
        D->offF = (int)(o = round_up(o + (idxl ? (int64_t)nnz * 2 : 0), 16));
        return o + 16;
    };
    const bool want_idxl = n <= 65535 && !(flags & QLDPC_FLAG_LAYERED_GLOBAL_IDX);
    int64_t bytes = 0;
    bool placed = false;
    for (int form = 0; form < 4 && !placed; form++) {               // V and indices in LDS; V only; indices only (VG); neither
        const bool vg = form >= 2, idxl = (form & 1) == 0;
        if ((idxl && !want_idxl) || (!vg && (flags & QLDPC_FLAG_LAYERED_VGLOBAL))) continue;
        bytes = layout(vg, idxl);
        if (bytes <= kLayeredLds) { D->vg = vg; D->idxl = idxl; placed = true; }
    }
    if (!placed) {
        set_error("the layered decoder keeps 29 bytes per non-empty row and 4 per layer in LDS: %d rows in %d layers need %lld bytes, more than %d", ns, nl,
                  (long long)bytes, kLayeredLds);
        return QLDPC_ERR_UNSUPPORTED;
    }
    D->lds = (int)bytes;
    D->grid_cap = cu_count(g->device) * (int)std::max<int64_t>(1, std::min<int64_t>(kLayeredLds / D->lds, 2048 / D->block));
    int rc;
    if (D->idxl) { idx16.assign(idx32.begin(), idx32.end()); if ((rc = upload(D->d_idx16, idx16)) != QLDPC_OK) return rc; }
    const std::vector<double> pv(prior, prior + n), av(tab.begin(), tab.begin() + max_iter);
    if ((rc = upload(D->d_prior, pv)) || (rc = upload(D->d_alpha, av)) || (rc = upload(D->d_layer, layer)) || (rc = upload(D->d_slot_row, slot_row)) ||
        (rc = upload(D->d_estart, estart)) || (rc = upload(D->d_idx32, idx32)) || (rc = D->d_queue.ensure(16)) ||
        (D->vg && (rc = D->d_vglobal.ensure((size_t)D->grid_cap * n * 8))))
        return rc;
    *out = D.release();
    return QLDPC_OK;
}

int layered_lock_and_launch(qldpc_layered_decoder *D, int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter,
                            hipStream_t s) {
    return decoder_lock_and_launch(D, B, d_synd, d_err, d_llr, d_conv, d_iter, s);
}

}  // namespace qldpc

QLDPC_EXPORT int qldpc_check_layers(const qldpc_graph *g, int32_t *row_layer, int *layers) {
    QLDPC_REQUIRE(g != nullptr && row_layer != nullptr, "NULL argument");
    std::vector<int32_t> lay;
    const int nl = greedy_layers(g, lay);
    std::copy(lay.begin(), lay.end(), row_layer);
    if (layers) *layers = nl;
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_layered_decoder_create(const qldpc_graph *g, const int32_t *row_layer, const double *prior, int max_iter, int alpha_mode,
                                              double alpha_val, const double *alpha_seq, int alpha_len, double clip_llr, int flags,
                                              qldpc_layered_decoder **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(max_iter >= 1, "max_iter must be >= 1 (got %d)", max_iter);
    std::vector<double> tab;
    const int rc = build_alpha_table(max_iter, alpha_mode, alpha_val, alpha_seq, alpha_len, tab);
    if (rc != QLDPC_OK) return rc;
    return layered_decoder_create_tab(g, row_layer, prior, max_iter, tab, clip_llr, flags, out);
}

QLDPC_EXPORT void qldpc_layered_decoder_destroy(qldpc_layered_decoder *D) { delete D; }

QLDPC_EXPORT int qldpc_layered_decoder_info(const qldpc_layered_decoder *D, int *layers, int *max_layer_rows, int *max_layer_edges, int *lds_bytes,
                                            int *form) {
    QLDPC_REQUIRE(D != nullptr, "decoder is NULL");
    if (layers) *layers = D->nlayers;
    if (max_layer_rows) *max_layer_rows = D->max_rows;
    if (max_layer_edges) *max_layer_edges = D->max_edges;
    if (lds_bytes) *lds_bytes = D->lds;
    if (form) *form = D->block | (D->vg ? QLDPC_LAYERED_FORM_VGLOBAL : 0) | (D->idxl ? QLDPC_LAYERED_FORM_LDS_INDICES : 0);
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_layered_decoder_layers(const qldpc_layered_decoder *D, int32_t *row_layer) {
    QLDPC_REQUIRE(D != nullptr && row_layer != nullptr, "NULL argument");
    std::copy(D->row_layer.begin(), D->row_layer.end(), row_layer);
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_layered_decode_batch_dev(qldpc_layered_decoder *D, int64_t B, const int8_t *d_syndromes, int8_t *d_err, double *d_llr,
                                                uint8_t *d_conv, int32_t *d_iter, void *stream) {
    return decoder_decode_dev(D, B, d_syndromes, d_err, d_llr, d_conv, d_iter, stream);
}

QLDPC_EXPORT int qldpc_layered_decode_batch(qldpc_layered_decoder *D, int64_t B, const int8_t *syndromes, int8_t *err, double *llr, uint8_t *conv,
                                            int32_t *iter) {
    return decoder_decode_host(D, "layered decode", B, syndromes, err, llr, conv, iter);
}
