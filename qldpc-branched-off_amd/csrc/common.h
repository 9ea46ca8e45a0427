// Shared host-side infrastructure of libqldpc_hip (error reporting, device buffers, graph handle).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <functional>
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

// Grow-only device buffer (never shrinks; freed with the owner).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

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
    ~HostStage() { if (!slab_ && base_) (void)hipFree(base_); }
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
    int finish_pinned(const char *what, void *&pin, size_t &pin_cap);
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
    DevBuf *slab_ = nullptr;
    std::unique_lock<std::mutex> lock_;
    unsigned char *base_ = nullptr;
};

// The call checks shared by the decoder objects whose outputs are (err, llr, conv, iter): layered and f32.
int decoder_check_call(const void *decoder, int64_t B, const void *synd, const void *err, const void *llr, const void *conv, const void *iter);

// Compute units of a device (256 when the runtime does not say): what the persistent grids are sized by.
int cu_count(int device);

// Device state that one stream uses at a time, handed from stream to stream through an event: a user calls acquire(stream) before its
// launches (a launch on another stream first waits for the previous user to finish) and release(stream) after them -- on every path once
// anything may have been enqueued, failures included, since the next stream has to wait for those launches too.  The owner serialises the calls.
struct StreamHandover {
    hipEvent_t event = nullptr;
    hipStream_t stream = nullptr;
    bool used = false;
    int acquire(hipStream_t s);
    int release(hipStream_t s);
    void destroy();
};

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
    int32_t *d_regown = nullptr;     // [m][16] edge-ownership records of the regular (6,3) kernel (regular_own.h), NULL where the graph has no assignment; built at creation
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
    struct AlphaEntry { std::vector<double> host; double *pinned = nullptr; double *dev = nullptr; hipEvent_t ready = nullptr; hipStream_t stream = nullptr; };
    mutable std::vector<AlphaEntry> alpha_cache;
    int alpha_table(const std::vector<double> &tab, hipStream_t stream, const double **d_out) const;   // callers hold mu
    mutable void *pin = nullptr;     // pinned host staging for small results
    mutable size_t pin_cap = 0;
    mutable int gf2_rank = -1;       // rank of H over GF(2), computed on first OSD use
    mutable int osd_path = -1, osd_detail = 0;   // what the last OSD-0 launch on this handle took (QLDPC_OSD_PATH_*, QLDPC_OSD_DETAIL_*; guarded by mu)
    mutable uint16_t *d_col_rows = nullptr;   // [n][max_col_deg] rows of every column (ascending, padded with m), built on first OSD use
    mutable void *wg2_cache = nullptr;   // tables of the LDS-resident workgroup decoder per prior (minsum_wg2.hip), built on first use (guarded by mu)
    mutable unsigned long long *clk_probe = nullptr;   // set (under mu) by a plan created with QLDPC_FLAG_CLOCK_PROBE around one launch
};
