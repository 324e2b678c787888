// host_common.hip -- implementation of host_common.hpp and host_wait.hpp: the error text behind ldpc_last_error(), the
// bounded host-side waits with the stalled-device table, and the create-time scaffolding every decoder shares.  Host
// code only; it reads no environment variable, so the product and the experiments build link the same object.
#include "host_common.hpp"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

namespace ldpc_detail {

namespace {
thread_local std::string g_err;
}

ldpc_status set_error(ldpc_status st, const std::string &msg)
{
    g_err = msg;
    return st;
}
const std::string &last_error() { return g_err; }

// ---- bounded host-side waits (host_wait.hpp)
namespace {
std::atomic<int64_t> g_wait_limit_ms{600000};
constexpr int kMaxDev = 64;
std::atomic<bool> g_stalled[kMaxDev];
std::mutex g_stall_mu;
std::string g_stall_msg[kMaxDev];

ldpc_status expired(int device, const char *what, int64_t limit_ms)
{
    const std::string msg = std::string(what) + ": the device did not get there within " + std::to_string(limit_ms) +
                            " ms (ldpc_set_wait_limit_ms); device " + std::to_string(device) +
                            " is taken to be stalled: every later call on it fails with this message, and what it may still be "
                            "using is not freed";
    if (device >= 0 && device < kMaxDev) {
        std::lock_guard<std::mutex> lk(g_stall_mu);
        if (!g_stalled[device].load()) { g_stall_msg[device] = msg; g_stalled[device].store(true); }
    }
    return set_error(LDPC_ERR_HIP, msg);
}

template <class Query>
ldpc_status poll_until(Query &&query, int device, const char *what)
{
    if (device_stalled(device)) return stalled_error(device);
    const int64_t limit = g_wait_limit_ms.load(std::memory_order_relaxed);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = query();
        if (q == hipSuccess) return LDPC_OK;
        if (q != hipErrorNotReady) {
            (void)hipGetLastError();
            return set_error(LDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(q));
        }
        if (spins < 64) { __builtin_ia32_pause(); continue; }   // (a query is ~1 us: the first polls back to back)
        const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (limit > 0 && us > limit * 1000) return expired(device, what, limit);
        if (us < 300) __builtin_ia32_pause();                    // latency-bound calls (a small batch is ~100 us): keep polling
        else if (us < 5000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(us < 100000 ? 50 : 200));
    }
}
}  // namespace

int64_t wait_limit_ms() { return g_wait_limit_ms.load(std::memory_order_relaxed); }
bool device_stalled(int device) { return device >= 0 && device < kMaxDev && g_stalled[device].load(std::memory_order_acquire); }
ldpc_status stalled_error(int device)
{
    std::lock_guard<std::mutex> lk(g_stall_mu);
    return set_error(LDPC_ERR_HIP, (device >= 0 && device < kMaxDev) ? g_stall_msg[device] : std::string("device stalled"));
}
ldpc_status wait_event(hipEvent_t e, int device, const char *what)
{
    if (wait_limit_ms() == 0 && !device_stalled(device)) {       // unbounded, as before round 4
        const hipError_t q = hipEventSynchronize(e);
        if (q == hipSuccess) return LDPC_OK;
        (void)hipGetLastError();
        return set_error(LDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(q));
    }
    return poll_until([&] { return hipEventQuery(e); }, device, what);
}
ldpc_status wait_stream(hipStream_t s, int device, const char *what)
{
    if (wait_limit_ms() == 0 && !device_stalled(device)) {
        const hipError_t q = hipStreamSynchronize(s);
        if (q == hipSuccess) return LDPC_OK;
        (void)hipGetLastError();
        return set_error(LDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(q));
    }
    return poll_until([&] { return hipStreamQuery(s); }, device, what);
}
ldpc_status wait_expired(int device, const char *what)
{
    if (device_stalled(device)) return stalled_error(device);
    return expired(device, what, wait_limit_ms());
}
// hipDeviceSynchronize has no query form: it runs in a helper thread that the caller waits for with the deadline; a
// thread that never comes back is left behind (detached) with the state it shares with nobody else.
ldpc_status wait_device(int device, const char *what)
{
    if (device_stalled(device)) return stalled_error(device);
    const int64_t limit = wait_limit_ms();
    if (limit == 0) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        hipError_t q = hipSetDevice(device);
        if (q == hipSuccess) q = hipDeviceSynchronize();
        if (prev >= 0) (void)hipSetDevice(prev);
        if (q == hipSuccess) return LDPC_OK;
        (void)hipGetLastError();
        return set_error(LDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(q));
    }
    struct Shared { std::mutex m; std::condition_variable cv; bool done = false; hipError_t e = hipSuccess; };
    auto sh = std::make_shared<Shared>();
    std::thread([sh, device] {
        hipError_t q = hipSetDevice(device);
        if (q == hipSuccess) q = hipDeviceSynchronize();
        if (q != hipSuccess) (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(sh->m);
        sh->e = q; sh->done = true;
        sh->cv.notify_all();
    }).detach();
    std::unique_lock<std::mutex> lk(sh->m);
    if (!sh->cv.wait_for(lk, std::chrono::milliseconds(limit), [&] { return sh->done; })) {
        lk.unlock();
        return expired(device, what, limit);
    }
    if (sh->e == hipSuccess) return LDPC_OK;
    return set_error(LDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(sh->e));
}

// ---- what the creates share (host_common.hpp)
ldpc_status check_csc_args(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval, int64_t max_iters)
{
    if (s < 0 || n < 0 || nnz < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative dimension");
    if (!colptr || (nnz > 0 && !rowval)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "colptr/rowval is NULL");
    if (max_iters < 0 || max_iters > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "max_iters out of range");
    return LDPC_OK;
}

ldpc_status check_csc_pattern(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval)
{
    if (colptr[0] != 0 || colptr[n] != nnz)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "colptr[0] must be 0 and colptr[n] must equal nnz (zero-based CSC)");
    for (int64_t j = 0; j < n; ++j) {
        if (colptr[j + 1] < colptr[j]) return set_error(LDPC_ERR_INVALID_ARGUMENT, "colptr is not non-decreasing");
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
            if (rowval[k] < 0 || rowval[k] >= s)
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "rowval entry outside [0, s)");
            if (k > colptr[j] && rowval[k] <= rowval[k - 1])
                return set_error(LDPC_ERR_INVALID_ARGUMENT,
                                 "row indices must be strictly ascending inside each column (SparseMatrixCSC invariant)");
        }
    }
    return LDPC_OK;
}

ldpc_status select_device(int requested, int *device, hipDeviceProp_t *prop, const char *no_device_msg)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return set_error(LDPC_ERR_NO_DEVICE, no_device_msg);
    }
    if (requested < 0) LDPC_HIP_TRY(hipGetDevice(&requested));
    if (requested >= ndev) return set_error(LDPC_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    LDPC_HIP_TRY(hipSetDevice(requested));
    LDPC_HIP_TRY(hipGetDeviceProperties(prop, requested));
    if (!is_gfx950(*prop))
        return set_error(LDPC_ERR_NO_DEVICE, std::string("device is ") + prop->gcnArchName + ", this library is built for gfx950 only");
    if (device_stalled(requested)) return stalled_error(requested);
    *device = requested;
    return LDPC_OK;
}

// sparse(H') (belief_propagation.jl:64): CSR of H, bits ascending inside each check, plus for every CSC edge its
// position in that check-major order.
TannerGraph tanner_graph(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval)
{
    TannerGraph g;
    const size_t edges = (size_t)std::max<int64_t>(nnz, 1);
    g.row_ptr.assign((size_t)s + 1, 0);
    g.col_ptr.resize((size_t)n + 1);
    g.csr_col.resize(edges); g.csc_row.resize(edges); g.csc2csr.resize(edges);
    for (int64_t k = 0; k < nnz; ++k) g.row_ptr[(size_t)rowval[k] + 1]++;
    for (int64_t i = 0; i < s; ++i) {
        g.max_cdeg = std::max(g.max_cdeg, g.row_ptr[(size_t)i + 1]);
        g.row_ptr[(size_t)i + 1] += g.row_ptr[(size_t)i];
    }
    std::vector<int> fill(g.row_ptr.begin(), g.row_ptr.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
        g.col_ptr[(size_t)j] = (int)colptr[j];
        g.max_bdeg = std::max(g.max_bdeg, (int)(colptr[j + 1] - colptr[j]));
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
            const int q = fill[(size_t)rowval[k]]++;
            g.csr_col[(size_t)q] = (int)j;
            g.csc_row[(size_t)k] = (int)rowval[k];
            g.csc2csr[(size_t)k] = q;
        }
    }
    g.col_ptr[(size_t)n] = (int)nnz;
    return g;
}

ldpc_status grow_device_buffer(void **p, size_t *cap, size_t bytes, int device, const char *what)
{
    if (*cap >= bytes) return LDPC_OK;
    if (*p) {
        const ldpc_status ws = wait_device(device, what);
        if (ws != LDPC_OK) return ws;
        (void)hipFree(*p);
    }
    *p = nullptr; *cap = 0;
    LDPC_HIP_TRY(hipMalloc(p, bytes));
    *cap = bytes;
    return LDPC_OK;
}

int blocks_per_cu(const void *kernel, int threads, size_t lds)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds) != hipSuccess || nb <= 0) {
        (void)hipGetLastError();
        nb = 1;
    }
    return nb;
}

}  // namespace ldpc_detail

extern "C" {

const char *ldpc_last_error(void) { return ldpc_detail::g_err.c_str(); }

ldpc_status ldpc_set_wait_limit_ms(int64_t ms)
{
    if (ms < 0) return ldpc_detail::set_error(LDPC_ERR_INVALID_ARGUMENT, "negative wait limit");
    ldpc_detail::g_wait_limit_ms.store(ms);
    return LDPC_OK;
}
int64_t ldpc_get_wait_limit_ms(void) { return ldpc_detail::wait_limit_ms(); }

}  // extern "C"
