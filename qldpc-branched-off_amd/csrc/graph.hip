// Error state, device selection and the Tanner-graph handle of libqldpc_hip.
#include "common.h"
#include "launchers.h"
#include "regular_plan.h"
#include "regular_own.h"

#include <algorithm>
#include <atomic>
#include <cstring>

namespace qldpc {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int use_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s); libqldpc_hip has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        (void)hipGetLastError();
        return QLDPC_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (have %d)", device, count);
        return QLDPC_ERR_INVALID;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_error("hipSetDevice(%d) failed: %s", device, hipGetErrorString(e));
        return QLDPC_ERR_NO_DEVICE;
    }
    return QLDPC_OK;
}

int DeviceScope::enter(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
    const int rc = use_device(device);
    if (rc == QLDPC_OK && cur >= 0) prev = cur;        // recorded unconditionally: an entry point may walk through several devices (comm.hip)
    return rc;
}
DeviceScope::~DeviceScope() {
    int cur = -1;
    if (prev >= 0 && (hipGetDevice(&cur) != hipSuccess || cur != prev)) (void)hipSetDevice(prev);
}

int ensure_max_lds(int device, const void *func, int bytes) {
    static std::mutex mu;
    static std::vector<std::pair<int, const void *>> done;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &d : done) if (d.first == device && d.second == func) return QLDPC_OK;
    QLDPC_HIP_TRY(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.emplace_back(device, func);
    return QLDPC_OK;
}

double clock_probe_median(const unsigned long long *pairs, int slots) {
    std::vector<double> v;
    for (int i = 0; i < slots; i++)
        if (pairs[2 * i + 1] > 0) v.push_back(100.0 * (double)pairs[2 * i] / (double)pairs[2 * i + 1]);
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// what qldpc_device_memory reports: the DevBufs that hold an allocation, and their bytes
static std::atomic<int64_t> g_live_buffers{0}, g_live_bytes{0};

int DevBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return QLDPC_OK;
    release();
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        p = nullptr;
        return QLDPC_ERR_HIP;
    }
    cap = bytes;
    g_live_buffers += 1; g_live_bytes += (int64_t)bytes;
    return QLDPC_OK;
}

void DevBuf::release() {
    if (!p) return;
    (void)hipFree(p);
    g_live_buffers -= 1; g_live_bytes -= (int64_t)cap;
    p = nullptr;
    cap = 0;
}

int PinnedBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return QLDPC_OK;
    release();
    QLDPC_HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    cap = bytes;
    return QLDPC_OK;
}

void PinnedBuf::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

int cu_count(int device) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    return cus;
}

int StreamHandover::acquire(hipStream_t s) {
    if (used && s != stream && event) QLDPC_HIP_TRY(hipStreamWaitEvent(s, event, 0));
    return QLDPC_OK;
}
int StreamHandover::release(hipStream_t s) {
    if (!event) QLDPC_HIP_TRY(hipEventCreateWithFlags(&event, hipEventDisableTiming));
    QLDPC_HIP_TRY(hipEventRecord(event, s));
    stream = s; used = true;
    return QLDPC_OK;
}
StreamHandover::~StreamHandover() {
    if (event) (void)hipEventDestroy(event);
}

int HostStage::stage() {
    QLDPC_REQUIRE(!layout_.overflow, "a buffer's byte count does not fit size_t, a dimension is negative or there are more than %d buffers", StageLayout::kMaxRegions);
    DevBuf &b = slab_ ? *slab_ : own_;
    const int rc = b.ensure(layout_.bytes());
    if (rc != QLDPC_OK) return rc;
    base_ = b.as<unsigned char>();
    for (int i = 0; i < layout_.count; i++) {
        const StageLayout::Region &r = layout_.regions[i];
        if (r.bytes == 0) continue;
        // the slab serves latency-bound calls: its uploads are enqueued on the null stream, where the launch follows them
        if (copies_[i].in && slab_) QLDPC_HIP_TRY(hipMemcpyAsync(base_ + r.off, copies_[i].in, r.bytes, hipMemcpyHostToDevice, nullptr));
        else if (copies_[i].in) QLDPC_HIP_TRY(hipMemcpy(base_ + r.off, copies_[i].in, r.bytes, hipMemcpyHostToDevice));
        if (copies_[i].zero) QLDPC_HIP_TRY(zero_now(base_ + r.off, r.bytes));
    }
    return QLDPC_OK;
}

int HostStage::finish(const char *what, Wait wait) {
    const hipError_t e = wait == kDevice ? hipDeviceSynchronize() : wait == kStream ? hipStreamSynchronize(nullptr) : hipSuccess;
    if (e != hipSuccess) { set_error("%s failed: %s", what, hipGetErrorString(e)); return QLDPC_ERR_HIP; }
    for (int i = 0; i < layout_.count; i++) {
        const StageLayout::Region &r = layout_.regions[i];
        if (copies_[i].out && r.bytes) QLDPC_HIP_TRY(hipMemcpy(copies_[i].out, base_ + r.off, r.bytes, hipMemcpyDeviceToHost));
    }
    return QLDPC_OK;
}

int HostStage::fetch_bytes(int id, void *host) const {
    const StageLayout::Region &r = layout_.regions[id];
    if (r.bytes) QLDPC_HIP_TRY(hipMemcpy(host, base_ + r.off, r.bytes, hipMemcpyDeviceToHost));
    return QLDPC_OK;
}

int HostStage::finish_pinned(const char *what, PinnedBuf &pin) {
    const size_t kPin = (size_t)1 << 20;
    size_t lo = layout_.total, hi = 0;
    for (int i = 0; i < layout_.count; i++) {
        const StageLayout::Region &r = layout_.regions[i];
        if (copies_[i].out && r.bytes) { lo = std::min(lo, r.off); hi = std::max(hi, r.off + r.bytes); }
    }
    if (hi <= lo || hi - lo > kPin) return finish(what, kCopies);
    if (const int rc = pin.ensure(kPin); rc != QLDPC_OK) return rc;
    QLDPC_HIP_TRY(hipMemcpyAsync(pin.p, base_ + lo, hi - lo, hipMemcpyDeviceToHost, nullptr));
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { set_error("%s failed: %s", what, hipGetErrorString(e)); return QLDPC_ERR_HIP; }
    for (int i = 0; i < layout_.count; i++) {
        const StageLayout::Region &r = layout_.regions[i];
        if (copies_[i].out && r.bytes) std::memcpy(copies_[i].out, static_cast<const unsigned char *>(pin.p) + (r.off - lo), r.bytes);
    }
    return QLDPC_OK;
}

int decoder_check_call(const void *decoder, int64_t B, const void *synd, const void *err, const void *llr, const void *conv, const void *iter) {
    QLDPC_REQUIRE(decoder != nullptr, "decoder is NULL");
    QLDPC_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "batch out of range");
    if (B > 0) QLDPC_REQUIRE(synd && err && llr && conv && iter, "NULL buffer");
    return QLDPC_OK;
}

}  // namespace qldpc

using namespace qldpc;

int qldpc_graph::ws_acquire(hipStream_t stream) const { return ws_private ? QLDPC_OK : ws_hand.acquire(stream); }
int qldpc_graph::ws_release(hipStream_t stream) const { return ws_private ? QLDPC_OK : ws_hand.release(stream); }

int qldpc_graph::alpha_table(const std::vector<double> &tab, hipStream_t stream, const double **d_out) const {
    for (const AlphaEntry &e : alpha_cache)
        if (e.host == tab) {
            if (stream != e.stream) QLDPC_HIP_TRY(hipStreamWaitEvent(stream, e.ready, 0));   // uploaded on another stream: order behind it
            *d_out = e.dev.as<double>();
            return QLDPC_OK;
        }
    if (alpha_cache.size() >= 64) {            // a caller cycling through > 64 schedules: start over once everything in flight is done
        QLDPC_HIP_TRY(hipDeviceSynchronize());
        alpha_cache.clear();
    }
    AlphaEntry e;                               // a failure below releases what it made
    e.host = tab;
    const size_t bytes = std::max<size_t>(tab.size(), 1) * sizeof(double);
    int rc;
    if ((rc = e.pinned.ensure(bytes)) != QLDPC_OK || (rc = e.dev.ensure(bytes)) != QLDPC_OK) return rc;
    std::memcpy(e.pinned.p, tab.data(), tab.size() * sizeof(double));
    QLDPC_HIP_TRY(hipMemcpyAsync(e.dev.p, e.pinned.p, tab.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    QLDPC_HIP_TRY(hipEventCreateWithFlags(&e.ready, hipEventDisableTiming));
    QLDPC_HIP_TRY(hipEventRecord(e.ready, stream));
    e.stream = stream;
    *d_out = e.dev.as<double>();
    alpha_cache.push_back(std::move(e));
    return QLDPC_OK;
}

QLDPC_EXPORT const char *qldpc_last_error(void) { return g_last_error.c_str(); }
QLDPC_EXPORT int qldpc_version(void) { return 101; }

QLDPC_EXPORT int qldpc_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return count;
}

// A diagnostic of the library's own device allocations (include/qldpc_hip.h).
QLDPC_EXPORT int qldpc_device_memory(int64_t *buffers, int64_t *bytes) {
    if (buffers) *buffers = g_live_buffers.load();
    if (bytes) *bytes = g_live_bytes.load();
    return QLDPC_OK;
}

QLDPC_EXPORT int qldpc_graph_create(int m, int n, const int32_t *indptr, const int32_t *indices, int device, qldpc_graph **out) {
    QLDPC_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    QLDPC_REQUIRE(m >= 0 && n >= 0, "negative dimensions m=%d n=%d", m, n);
    QLDPC_REQUIRE(indptr != nullptr, "indptr is NULL");
    QLDPC_REQUIRE(indptr[0] == 0, "indptr[0] must be 0");
    for (int i = 0; i < m; i++) QLDPC_REQUIRE(indptr[i + 1] >= indptr[i], "indptr not monotone at row %d", i);
    const int nnz = indptr[m];
    QLDPC_REQUIRE(nnz == 0 || indices != nullptr, "indices is NULL");
    for (int i = 0; i < m; i++)
        for (int e = indptr[i]; e < indptr[i + 1]; e++) {
            QLDPC_REQUIRE(indices[e] >= 0 && indices[e] < n, "column index %d out of range in row %d", indices[e], i);
            QLDPC_REQUIRE(e == indptr[i] || indices[e] > indices[e - 1], "row %d: column indices must be strictly increasing (canonical CSR)", i);
        }
    int rc = use_device(device);
    if (rc != QLDPC_OK) return rc;

    Handle<qldpc_graph, qldpc_graph_destroy> G(new qldpc_graph());      // (the deleter selects the device)
    qldpc_graph *const g = G.get();
    g->m = m; g->n = n; g->nnz = nnz; g->device = device;
    g->indptr.assign(indptr, indptr + m + 1);
    g->indices.assign(indices, indices + nnz);
    // CSC view, per column in ascending check order (rows are visited in ascending i)
    g->colptr.assign(n + 1, 0);
    for (int e = 0; e < nnz; e++) g->colptr[indices[e] + 1]++;
    for (int j = 0; j < n; j++) g->colptr[j + 1] += g->colptr[j];
    g->rowidx.resize(nnz); g->csc2csr.resize(nnz); g->csr2csc.resize(nnz);
    std::vector<int32_t> fill(g->colptr.begin(), g->colptr.end() - 1);
    for (int i = 0; i < m; i++) {
        g->max_row_deg = std::max(g->max_row_deg, indptr[i + 1] - indptr[i]);
        for (int e = indptr[i]; e < indptr[i + 1]; e++) {
            const int k = fill[indices[e]]++;
            g->rowidx[k] = i; g->csc2csr[k] = e; g->csr2csc[e] = k;
        }
    }
    for (int j = 0; j < n; j++) g->max_col_deg = std::max(g->max_col_deg, g->colptr[j + 1] - g->colptr[j]);
    rc = g->own(&g->d_indptr, g->indptr);
    if (rc == QLDPC_OK) rc = g->own(&g->d_indices, g->indices);
    if (rc == QLDPC_OK) rc = g->own(&g->d_colptr, g->colptr);
    if (rc == QLDPC_OK) rc = g->own(&g->d_rowidx, g->rowidx);
    if (rc == QLDPC_OK) rc = g->own(&g->d_csc2csr, g->csc2csr);
    if (rc == QLDPC_OK) rc = g->own(&g->d_csr2csc, g->csr2csc);
    if (rc == QLDPC_OK && n < 65535 && m < (1 << 24) && g->max_row_deg < 256) {
        std::vector<uint16_t> ec((size_t)round_up(std::max(g->max_row_deg, 1), 8) * std::max(m, 1), 0);   // slots padded to 8 rows, column 0
        std::vector<uint32_t> ev((size_t)std::max(g->max_col_deg, 1) * std::max(n, 1), 0xFFFFFFFFu);
        for (int i = 0; i < m; i++)
            for (int e = indptr[i]; e < indptr[i + 1]; e++) ec[(size_t)(e - indptr[i]) * m + i] = (uint16_t)indices[e];
        for (int j = 0; j < n; j++)
            for (int k = g->colptr[j]; k < g->colptr[j + 1]; k++) {
                const int row = g->rowidx[k], pos = g->csc2csr[k] - indptr[row];
                ev[(size_t)(k - g->colptr[j]) * n + j] = ((uint32_t)row << 8) | (uint32_t)pos;
            }
        rc = g->own(&g->d_ell_col, ec);
        if (rc == QLDPC_OK) rc = g->own(&g->d_ell_var, ev);
        // degree-ordered views (stable sort, descending degree)
        std::vector<int32_t> ros(std::max(m, 1)), cos(std::max(n, 1)), slot_of_row(std::max(m, 1));
        for (int i = 0; i < m; i++) ros[i] = i;
        for (int j = 0; j < n; j++) cos[j] = j;
        std::stable_sort(ros.begin(), ros.begin() + m, [&](int a, int b) { return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b]; });
        std::stable_sort(cos.begin(), cos.begin() + n, [&](int a, int b) { return g->colptr[a + 1] - g->colptr[a] > g->colptr[b + 1] - g->colptr[b]; });
        for (int s = 0; s < m; s++) slot_of_row[ros[s]] = s;
        std::vector<uint8_t> drs(std::max(m, 1), 0), dr(std::max(m, 1), 0);
        std::vector<uint16_t> dcs(std::max(n, 1), 0), dc(std::max(n, 1), 0);
        for (int s = 0; s < m; s++) { drs[s] = (uint8_t)(indptr[ros[s] + 1] - indptr[ros[s]]); dr[s] = (uint8_t)(indptr[s + 1] - indptr[s]); }
        for (int s = 0; s < n; s++) { dcs[s] = (uint16_t)std::min(g->colptr[cos[s] + 1] - g->colptr[cos[s]], 65535); dc[s] = (uint16_t)std::min(g->colptr[s + 1] - g->colptr[s], 65535); }
        std::vector<uint16_t> ecs(ec.size(), 0);
        std::vector<uint32_t> evs(ev.size(), 0xFFFFFFFFu);
        for (int s = 0; s < m; s++) {
            const int i = ros[s];
            for (int e = indptr[i]; e < indptr[i + 1]; e++) ecs[(size_t)(e - indptr[i]) * m + s] = (uint16_t)indices[e];
        }
        for (int s = 0; s < n; s++) {
            const int j = cos[s];
            for (int k = g->colptr[j]; k < g->colptr[j + 1]; k++) {
                const int row = g->rowidx[k], pos = g->csc2csr[k] - indptr[row];
                evs[(size_t)(k - g->colptr[j]) * n + s] = ((uint32_t)slot_of_row[row] << 8) | (uint32_t)pos;
            }
        }
        std::vector<int32_t> ident(std::max(std::max(m, n), 1));
        for (size_t i = 0; i < ident.size(); i++) ident[i] = (int32_t)i;
        if (rc == QLDPC_OK) rc = g->own(&g->d_row_of_slot, ros);
        if (rc == QLDPC_OK) rc = g->own(&g->d_col_of_slot, cos);
        if (rc == QLDPC_OK) rc = g->own(&g->d_deg_of_rslot, drs);
        if (rc == QLDPC_OK) rc = g->own(&g->d_deg_of_cslot, dcs);
        if (rc == QLDPC_OK) rc = g->own(&g->d_deg_of_row, dr);
        if (rc == QLDPC_OK) rc = g->own(&g->d_deg_of_col, dc);
        if (rc == QLDPC_OK) rc = g->own(&g->d_ell_col_s, ecs);
        if (rc == QLDPC_OK) rc = g->own(&g->d_ell_var_s, evs);
        if (rc == QLDPC_OK) rc = g->own(&g->d_identity, ident);
    }
    if (rc == QLDPC_OK && g->max_row_deg == kRegOwnCdeg && g->max_col_deg == kRegOwnVdeg && n == 2 * m && m <= 1024) {
        // the regular (6,3) kernel's edge ownership: once per handle, here, where nothing is in flight and no lock is needed ("none" leaves the pointer NULL).
        // Which valid assignment it is changes LDS bank conflicts only, never a result ("regular_own_search", options.hip).
        std::vector<int32_t> own;
        if (regular_own_assign(m, n, indptr, indices, regular_row_stride(kRegOwnCdeg), own, regular_own_search_choice())) {
            rc = g->own(&g->d_regown, own); g->regown = std::move(own);
            // the assignment of the class-uniform waves (regular_place.h); it exists wherever the one above does
            std::vector<int32_t> minlast;
            if (rc == QLDPC_OK && regular_own_assign_minlast(m, n, indptr, indices, regular_row_stride(kRegOwnCdeg), minlast)) { rc = g->own(&g->d_regown_minlast, minlast); g->regown_minlast = std::move(minlast); }
        }
    }
    if (rc != QLDPC_OK) return rc;
    *out = G.release();
    return QLDPC_OK;
}

QLDPC_EXPORT void qldpc_graph_destroy(qldpc_graph *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->wg2_cache) qldpc::wg2_cache_free(g->wg2_cache);
    delete g;                                      // every buffer, alpha table and event of the handle releases itself
}

QLDPC_EXPORT int qldpc_graph_dims(const qldpc_graph *g, int *m, int *n, int *nnz) {
    QLDPC_REQUIRE(g != nullptr, "graph is NULL");
    if (m) *m = g->m;
    if (n) *n = g->n;
    if (nnz) *nnz = g->nnz;
    return QLDPC_OK;
}
