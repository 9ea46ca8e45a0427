// Shared host-side infrastructure of libqldpc_hip (error reporting, device buffers, graph handle).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qldpc_hip.h"
#include "stage_layout.h"

#define QLDPC_EXPORT extern "C" __attribute__((visibility("default")))

namespace qldpc {

void set_error(const char *fmt, ...);

#define QLDPC_HIP_TRY(expr)                                                                     \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            qldpc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return QLDPC_ERR_HIP;                                                               \
        }                                                                                       \
    } while (0)

#define QLDPC_REQUIRE(cond, ...)                  \
    do {                                          \
        if (!(cond)) {                            \
            qldpc::set_error(__VA_ARGS__);        \
            return QLDPC_ERR_INVALID;             \
        }                                         \
    } while (0)

// Zeroes device memory and WAITS for it.  hipMemset returns once the fill is queued on the null stream, and the null stream is not ordered against
// hipStreamNonBlocking streams: a kernel enqueued on such a stream right after a bare hipMemset can start before the fill has run.  Round 4 found
// a lane's OSD-0 ticket counter zeroed in the middle of the lane's first launch that way (profiles/r04_experiments.txt, item 5; the hand-out in
// isolation: tools/microbench/ticket_race.hip).  Every "zero this before anyone uses it" in the library goes through here.
inline hipError_t zero_now(void *p, size_t bytes) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}

// Checks that a gfx9 device is present and selects it. Returns QLDPC_OK or QLDPC_ERR_NO_DEVICE.
int use_device(int device);

// Entry points select their handle's device for the calling thread and put the caller's current device back on return
// (a process that also drives the GPU through another runtime, e.g. torch, keeps its own current device).
struct DeviceScope {
    int prev = -1;
    int enter(int device);
    ~DeviceScope();
};
#define QLDPC_USE_DEVICE(dev)                                   \
    qldpc::DeviceScope _dev_scope;                              \
    {                                                           \
        const int _rc_dev = _dev_scope.enter(dev);              \
        if (_rc_dev != QLDPC_OK) return _rc_dev;                \
    }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute: set it once per (device, kernel), thread-safe.
int ensure_max_lds(int device, const void *func, int bytes);

// Grow-only device buffer (never shrinks).  It OWNS its allocation: freed when the object that holds it is deleted, so a handle that gains a buffer
// needs no line in its destroy function.  Move-only.  Every hipMalloc / hipFree of the library is in ensure() / release() (the process-lifetime
// timer buffer of gf2.hip aside), which keep the count behind qldpc_device_memory.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    int ensure(size_t bytes);
    void release();                                  // idempotent
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Pinned host memory with the same rules (grow-only, owning, move-only): every hipHostMalloc / hipHostFree of the library.
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    ~PinnedBuf() { release(); }
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    int ensure(size_t bytes);
    void release();
};

// unique_ptr to a library handle that its public destroy function releases: Handle<qldpc_graph, qldpc_graph_destroy>
template <auto Destroy> struct HandleDelete { template <class H> void operator()(H *h) const { Destroy(h); } };
template <class H, auto Destroy> using Handle = std::unique_ptr<H, HandleDelete<Destroy>>;

inline int64_t round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

// Replaces the contents of a device buffer with a host vector (synchronous copy; an empty vector still leaves an allocation).
template <class T>
int upload(DevBuf &b, const std::vector<T> &v) {
    int rc = b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (rc != QLDPC_OK) return rc;
    if (!v.empty()) QLDPC_HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return QLDPC_OK;
}

// Device staging of one host-pointer entry point.  A call declares its regions, stage() carves ONE allocation for all of them (stage_layout.h: 256-byte
// aligned, an address even for an empty region), uploads the inputs and zeroes what asked for it (zero_now), the call launches on the null stream under
// the lock it needs, and finish() waits and downloads every output that has a host pointer.  A declaration returns a typed handle: S[handle] is the
// region's device address after stage(), and the default handle stands for "no such buffer" (NULL).  Dimensions multiply to the element count; a byte
// count that does not fit size_t, a negative dimension or more than StageLayout::kMaxRegions regions make stage() fail with QLDPC_ERR_INVALID.
// Two backings.  HostStage S;                        one temporary allocation, freed with S.
//                HostStage S(g->ws_io, g->mu_io);    the regions live in a grow-only slab that stays allocated between calls; S holds the mutex.
template <class T> struct Staged { int id = -1; };
class HostStage {
  public:
    // kCopies: the blocking downloads are the wait (they run behind the null stream's work); kStream: hipStreamSynchronize(nullptr) first;
    // kDevice: hipDeviceSynchronize() first -- a launcher may use streams the null stream is not ordered against
    enum Wait { kCopies, kStream, kDevice };
    HostStage() = default;
    HostStage(DevBuf &slab, std::mutex &mu) : slab_(&slab), lock_(mu) {}
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;

    template <class T, class... N> Staged<T> in(const T *host, N... dims) { return {add(host, nullptr, false, sizeof(T), {(int64_t)dims...})}; }
    template <class T, class... N> Staged<T> out(T *host, N... dims) { return {add(nullptr, host, false, sizeof(T), {(int64_t)dims...})}; }          // host == NULL: stays on the device
    template <class T, class... N> Staged<T> out_zeroed(T *host, N... dims) { return {add(nullptr, host, true, sizeof(T), {(int64_t)dims...})}; }
    template <class T, class... N> Staged<T> inout(const T *from, T *to, N... dims) { return {add(from, to, false, sizeof(T), {(int64_t)dims...})}; }
    template <class T, class... N> Staged<T> scratch(N... dims) { return {add(nullptr, nullptr, false, sizeof(T), {(int64_t)dims...})}; }
    template <class T, class... N> Staged<T> zeroed(N... dims) { return {add(nullptr, nullptr, true, sizeof(T), {(int64_t)dims...})}; }
    template <class T> T *operator[](Staged<T> h) const { return h.id < 0 ? nullptr : reinterpret_cast<T *>(base_ + layout_.regions[h.id].off); }

    int stage();
    int finish(const char *what, Wait wait);        // a failed wait: "<what> failed: <hip error string>"
    // finish() for a latency-bound call: outputs of at most 1 MiB come back in ONE copy through the pinned buffer (grown here) and are scattered on the host
    int finish_pinned(const char *what, PinnedBuf &pin);
    // one region into a host array, for an output that the call downloads only once it has looked at another (declared as scratch)
    template <class T> int fetch(Staged<T> h, T *host) const { return fetch_bytes(h.id, host); }

  private:
    int fetch_bytes(int id, void *host) const;
    struct Copy { const void *in; void *out; bool zero; };
    int add(const void *in, void *out, bool zero, size_t elem, std::initializer_list<int64_t> dims) {
        const int id = layout_.add(dims, elem);
        if (id >= 0) copies_[id] = {in, out, zero};
        return id;
    }
    StageLayout layout_;
    Copy copies_[StageLayout::kMaxRegions];
    DevBuf own_, *slab_ = nullptr;                   // the temporary allocation, or the caller's slab
    std::unique_lock<std::mutex> lock_;
    unsigned char *base_ = nullptr;
};

// Compute units of a device (256 when the runtime does not say): what the persistent grids are sized by.
int cu_count(int device);

// Device state that one stream uses at a time, handed from stream to stream through an event: a user calls acquire(stream) before its
// launches (a launch on another stream first waits for the previous user to finish) and release(stream) after them -- on every path once
// anything may have been enqueued, failures included, since the next stream has to wait for those launches too.  The owner serialises the calls.
struct StreamHandover {
    hipEvent_t event = nullptr;
    hipStream_t stream = nullptr;
    bool used = false;
    StreamHandover() = default;
    ~StreamHandover();
    StreamHandover(const StreamHandover &) = delete;
    StreamHandover &operator=(const StreamHandover &) = delete;
    int acquire(hipStream_t s);
    int release(hipStream_t s);
};

// The destructor's body of a handle that has a hand-over: select its device and, when the hand-over was used, wait for what is in flight.  Members are
// destroyed after a destructor's body, so the buffers are freed only then.  (A base class's destructor runs AFTER the derived members are gone,
// which is why the decoder objects below call this from their own destructor.)
inline void quiesce(int device, const StreamHandover &hand) {
    (void)hipSetDevice(device);
    if (hand.used) (void)hipDeviceSynchronize();
}

// What the decoder objects with the outputs (err, llr, conv, iter) hold alike on the host: layered (minsum_layered.hip) and f32 (minsum_f32.hip).
// A decoder adds its tables, a destructor that calls quiesce(device, hand), and
//     int launch(int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t s);      callers hold mu
// which fills its kernel's argument struct, picks the instantiation and goes through decoder_launch.
struct DecoderBase {
    const qldpc_graph *g = nullptr;
    int device = 0, m = 0, n = 0, max_iter = 0, flags = 0;
    int block = 0, lds = 0, grid_cap = 0;
    DevBuf d_prior, d_alpha, d_queue;
    // the queue word (and a decoder's slabs) are handed from stream to stream like a graph handle's workspaces
    std::mutex mu;
    StreamHandover hand;
};

// Enqueues kern(A) for B shots on s: the queue word zeroed in stream order, min(B, grid_cap) workgroups of D.block threads and D.lds bytes.
template <class Args>
int decoder_launch(DecoderBase &D, void (*kern)(Args), int max_lds, const Args &A, int64_t B, hipStream_t s) {
    int rc = D.hand.acquire(s);
    if (rc != QLDPC_OK) return rc;
    auto launch = [&]() -> int {
        QLDPC_HIP_TRY(hipMemsetAsync(D.d_queue.p, 0, 16, s));
        const int rcl = ensure_max_lds(D.device, reinterpret_cast<const void *>(kern), max_lds);
        if (rcl != QLDPC_OK) return rcl;
        const unsigned grid = (unsigned)std::min<int64_t>(B, D.grid_cap);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(D.block), (size_t)D.lds, s, A);
        QLDPC_HIP_TRY(hipGetLastError());
        return QLDPC_OK;
    };
    rc = launch();
    const int rel = D.hand.release(s);              // always: a failing call may have enqueued work the next stream has to wait for
    return rc != QLDPC_OK ? rc : rel;
}

template <class D>
int decoder_lock_and_launch(D *dec, int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, hipStream_t s) {
    std::lock_guard<std::mutex> lk(dec->mu);
    return dec->launch(B, d_synd, d_err, d_llr, d_conv, d_iter, s);
}

// The call checks of the two entry points below.
int decoder_check_call(const void *decoder, int64_t B, const void *synd, const void *err, const void *llr, const void *conv, const void *iter);

// qldpc_*_decode_batch_dev of such a decoder: device pointers, enqueued on `stream`
template <class D>
int decoder_decode_dev(D *dec, int64_t B, const int8_t *d_synd, int8_t *d_err, double *d_llr, uint8_t *d_conv, int32_t *d_iter, void *stream) {
    const int rc = decoder_check_call(dec, B, d_synd, d_err, d_llr, d_conv, d_iter);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(dec->device);
    if (B == 0) return QLDPC_OK;
    return decoder_lock_and_launch(dec, B, d_synd, d_err, d_llr, d_conv, d_iter, reinterpret_cast<hipStream_t>(stream));
}

// qldpc_*_decode_batch: host pointers, staged, decoded on the null stream and waited for ("<what> failed: ..." when the wait fails)
template <class D>
int decoder_decode_host(D *dec, const char *what, int64_t B, const int8_t *synd, int8_t *err, double *llr, uint8_t *conv, int32_t *iter) {
    int rc = decoder_check_call(dec, B, synd, err, llr, conv, iter);
    if (rc != QLDPC_OK) return rc;
    QLDPC_USE_DEVICE(dec->device);
    if (B == 0) return QLDPC_OK;
    HostStage S;
    const auto ds = S.in(synd, B, dec->m);
    const auto de = S.out(err, B, dec->n);
    const auto dl = S.out(llr, B, dec->n);
    const auto dc = S.out(conv, B);
    const auto di = S.out(iter, B);
    if ((rc = S.stage()) != QLDPC_OK) return rc;
    rc = decoder_lock_and_launch(dec, B, S[ds], S[de], S[dl], S[dc], S[di], nullptr);
    return rc != QLDPC_OK ? rc : S.finish(what, HostStage::kStream);
}

// clocks.h: what the shader-clock probe stamped
double clock_probe_median(const unsigned long long *pairs, int slots);   // MHz; 0 when nothing was stamped


}  // namespace qldpc

// Tanner graph handle.  Host CSR/CSC plus device copies; immutable after create except the workspace cache.
struct qldpc_graph {
    int m = 0, n = 0, nnz = 0, device = 0;
    int max_row_deg = 0, max_col_deg = 0;
    std::vector<int32_t> indptr, indices;        // CSR (rows = checks), sorted columns
    std::vector<int32_t> colptr, rowidx, csc2csr; // CSC view: per column ascending check index; csc2csr[k] = CSR edge id
    std::vector<int32_t> csr2csc;                 // inverse permutation
    // device copies
    int32_t *d_indptr = nullptr, *d_indices = nullptr, *d_colptr = nullptr, *d_rowidx = nullptr, *d_csc2csr = nullptr,
            *d_csr2csc = nullptr;
    // ELL (slot-major) views for the workgroup-per-shot kernel: coalesced index loads across rows / columns
    uint16_t *d_ell_col = nullptr;   // [round_up(max_row_deg, 8)][m]  column of the k-th edge of row i; unused slots hold column 0
    uint32_t *d_ell_var = nullptr;   // [max_col_deg][n]  (row << 8) | position-in-row of the d-th edge of column j (ascending rows)
    // the same views with rows / columns handed to threads in DEGREE order (stable, descending): a wave's rows (columns) then have one
    // degree and its edge loop has no idle lanes.  Check state and index entries are in row-SLOT space; posteriors stay in column space.
    int32_t *d_row_of_slot = nullptr, *d_col_of_slot = nullptr;   // [m], [n]
    uint8_t *d_deg_of_rslot = nullptr, *d_deg_of_row = nullptr;      // [m]
    uint16_t *d_deg_of_cslot = nullptr, *d_deg_of_col = nullptr;     // [n]
    uint16_t *d_ell_col_s = nullptr; // [round_up(max_row_deg, 8)][m] indexed by row slot
    uint32_t *d_ell_var_s = nullptr; // [max_col_deg][n] indexed by column slot: (row slot << 8) | position-in-row, ascending ROW order
    int32_t *d_identity = nullptr;   // [max(m, n)] 0, 1, 2, ... (the natural-order "permutation")
    // The pointers above and below (and d_col_rows) are VIEWS that the launchers read; the memory behind them is owned here, so a table added to the
    // handle is freed with it.  own() uploads a host vector into a new owned buffer and sets the view (NULL when it fails).
    mutable std::vector<qldpc::DevBuf> owned;
    template <class T> int own(T **view, const std::vector<T> &v) const {
        qldpc::DevBuf b;
        const int rc = qldpc::upload(b, v);
        *view = rc == QLDPC_OK ? b.as<T>() : nullptr;
        if (rc == QLDPC_OK) owned.push_back(std::move(b));
        return rc;
    }
    int32_t *d_regown = nullptr;     // [m][16] edge-ownership records of the regular (6,3) kernel (regular_own.h), NULL where the graph has no assignment; built at creation
    // LDS place tables of that kernel (regular_place.h), one per workgroup shape: built and uploaded at the first launch with the shape and kept for the
    // handle's life (minsum_regular.hip: regular_place_table).  A shape is (S, block): "mc_list_shots" and a long iteration table change S on the same
    // graph.  placed = 0: today's linear addresses as a table, which also depend on where the dummy region lies (offD); 1: the placement of d_regown in
    // the identity thread order; 2: the placement of d_regown_minlast under the thread order of regular_place_order.  dev.p == NULL: placement
    // declined the shape.  Guarded by mu_place, which is held for the build and the upload only.
    std::vector<int32_t> regown;     // the host copy of d_regown the tables are built from
    // The min-last assignment (regular_own.h: the perfect assignment that owns the fewest `last` edges), for place tables with class-uniform waves: the
    // launches that read such a table read this ownership table with it; every other launch reads d_regown.  Built at creation next to d_regown.
    int32_t *d_regown_minlast = nullptr;
    std::vector<int32_t> regown_minlast;
    struct PlaceEntry { int S = 0, block = 0, placed = 0, offD = 0; qldpc::DevBuf dev; };
    mutable std::mutex mu_place;
    mutable std::vector<PlaceEntry> place_cache;
    // Device workspaces of the decode / OSD kernels.  `mu` guards the bookkeeping while launches are enqueued; the buffers themselves
    // are protected in STREAM order: every user calls ws_acquire(stream) before its launches and ws_release(stream) after them
    // (StreamHandover above).
    mutable std::mutex mu;
    mutable qldpc::DevBuf ws_msg, ws_qold, ws_vals, ws_misc, ws_queue, ws_list, ws_prior, ws_redo;
    mutable qldpc::DevBuf ws_cs;      // OSD-CS (osd_cs.hip): [0] count, [4..] shots whose right-hand side is outside the column space
    mutable qldpc::DevBuf ws_squeue;  // work queue of the one-wave OSD-0 kernels (osd_small.hip): zeroed once, the kernels reset it themselves
    mutable bool ws_private = false;  // the handle is used from ONE stream only (a private copy owned by a plan lane): no hand-over events
    mutable qldpc::StreamHandover ws_hand;
    int ws_acquire(hipStream_t stream) const;     // callers hold mu
    int ws_release(hipStream_t stream) const;
    mutable std::mutex mu_io;        // host-pointer entry points: serialises use of ws_io (taken before mu)
    mutable qldpc::DevBuf ws_io;
    // alpha tables already on the device (guarded by mu).  A table is uploaded once from a pinned host copy and never overwritten, so
    // the *_dev entry points stay pure enqueues (no synchronisation) however the alpha schedule changes between calls.
    struct AlphaEntry {                          // owns its pinned copy, its device copy and its event
        std::vector<double> host;
        qldpc::PinnedBuf pinned;
        qldpc::DevBuf dev;
        hipEvent_t ready = nullptr;
        hipStream_t stream = nullptr;
        AlphaEntry() = default;
        AlphaEntry(AlphaEntry &&o) noexcept : host(std::move(o.host)), pinned(std::move(o.pinned)), dev(std::move(o.dev)), ready(o.ready), stream(o.stream) { o.ready = nullptr; }
        ~AlphaEntry() { if (ready) (void)hipEventDestroy(ready); }
    };
    mutable std::vector<AlphaEntry> alpha_cache;
    int alpha_table(const std::vector<double> &tab, hipStream_t stream, const double **d_out) const;   // callers hold mu
    mutable qldpc::PinnedBuf pin;    // pinned host staging for small results
    mutable int gf2_rank = -1;       // rank of H over GF(2), computed on first OSD use
    mutable int osd_path = -1, osd_detail = 0;   // what the last OSD-0 launch on this handle took (QLDPC_OSD_PATH_*, QLDPC_OSD_DETAIL_*; guarded by mu)
    mutable uint16_t *d_col_rows = nullptr;   // [n][max_col_deg] rows of every column (ascending, padded with m), built on first OSD use
    mutable void *wg2_cache = nullptr;   // tables of the LDS-resident workgroup decoder per prior (minsum_wg2.hip), built on first use (guarded by mu)
    mutable unsigned long long *clk_probe = nullptr;   // set (under mu) by a plan created with QLDPC_FLAG_CLOCK_PROBE around one launch
};
