// host_common.hpp -- the host-side scaffolding that the C entry points of every decoder share (BP, the multi-GPU
// wrapper, BP-OTS, bit-flip, OSD on the device): the error text, the one "try a HIP call" macro, validation of the
// caller's CSC pattern, device selection, the Tanner graph in both orders, device-buffer growth, the staging layout
// (host_pipe_plan.hpp), the latency path's mapped image and flag spin and a few small helpers.  None of it has numerics or decides a kernel launch.
// Implemented in host_common.hip, except what is defined inline here.  The bounded waits: host_wait.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ldpc_mi355x.h"
#include "host_pipe_plan.hpp"
#include "host_wait.hpp"

namespace ldpc_detail {

// host_common.hip: records the calling thread's message (what ldpc_last_error() returns) and hands `st` back
ldpc_status set_error(ldpc_status st, const std::string &msg);
const std::string &last_error();                          // host_common.hip: that message

// The one macro that turns a failed HIP call into a status (out of memory apart) and returns it.
#define LDPC_HIP_TRY(expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            (void)hipGetLastError();                                                                         \
            return ldpc_detail::set_error(e_ == hipErrorOutOfMemory ? LDPC_ERR_OUT_OF_MEMORY : LDPC_ERR_HIP, \
                                          std::string(#expr) + ": " + hipGetErrorString(e_));                \
        }                                                                                                    \
    } while (0)

// Current device of the calling thread, put back when the scope ends (pool eviction and the multi-device entries
// switch devices; the caller's choice must survive them).
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; } }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ---- a create's arguments (host_common.hip).  Two steps, because a decoder's own size limit (LDPC_ERR_UNSUPPORTED)
// may stand between them: BP refuses a graph beyond 32-bit indexing before anything walks its arrays.
// dimensions >= 0, pattern pointers, 0 <= max_iters <= INT32_MAX
ldpc_status check_csc_args(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval, int64_t max_iters);
// zero-based CSC: colptr[0] = 0, colptr[n] = nnz, non-decreasing; every column's rows in range and in rising order, none twice
ldpc_status check_csc_pattern(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval);

inline bool is_gfx950(const hipDeviceProp_t &prop) { return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0; }

// host_common.hip: the device a handle is created on -- `requested`, or the calling thread's current one if negative --
// made current; it must exist, be a gfx950 and not have been marked stalled by a bounded wait (host_wait.hpp).
ldpc_status select_device(int requested, int *device, hipDeviceProp_t *prop, const char *no_device_msg);

// The caller's CSC pattern (bits -> checks) next to its CSR (checks -> bits, bits ascending inside a check), as 32-bit
// indices.  A decoder uploads the arrays its kernels read and drops the rest.
struct TannerGraph {
    std::vector<int> row_ptr, csr_col;    // CSR: edges of check i are [row_ptr[i], row_ptr[i + 1]), csr_col = their bits
    std::vector<int> col_ptr, csc_row;    // CSC: the caller's colptr / rowval
    std::vector<int> csc2csr;             // for every CSC edge, its position in the CSR order
    int max_cdeg = 0, max_bdeg = 0;       // largest check / bit degree
};
TannerGraph tanner_graph(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval);   // host_common.hip (validated pattern)

template <class V>
inline bool upload(V **dst, const std::vector<V> &v)   // hipMalloc (at least one element) + hipMemcpy
{
    if (hipMalloc((void **)dst, (v.empty() ? 1 : v.size()) * sizeof(V)) != hipSuccess) return false;
    return v.empty() || hipMemcpy(*dst, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice) == hipSuccess;
}

// host_common.hip: *p holds at least `bytes` afterwards.  A buffer that has to grow is freed only once the device has
// drained (bounded: `what` names that wait), and its contents are not kept.
ldpc_status grow_device_buffer(void **p, size_t *cap, size_t bytes, int device, const char *what);

// host_common.hip: workgroups of `kernel` a CU holds at once (1 if the runtime cannot tell)
int blocks_per_cu(const void *kernel, int threads, size_t lds);

// (Carve, the staging layout: host_pipe_plan.hpp)

// "Calls on a handle run in call order whatever streams they are given" (they share a workspace): a call enters by
// making its stream wait for the one before, if that ran on another stream, and leaves by recording itself.
struct CallOrder {
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool have = false;
    hipError_t create() { return hipEventCreateWithFlags(&done, hipEventDisableTiming); }
    void destroy() { if (done) (void)hipEventDestroy(done); done = nullptr; }
    ldpc_status enter(hipStream_t stream)
    {
        if (have && last != stream) LDPC_HIP_TRY(hipStreamWaitEvent(stream, done, 0));
        return LDPC_OK;
    }
    ldpc_status leave(hipStream_t stream)
    {
        LDPC_HIP_TRY(hipEventRecord(done, stream));
        last = stream; have = true;
        return LDPC_OK;
    }
};

// The latency paths' wait (DESIGN.md "Latency path"): spin on the host-mapped flag word until the last workgroup has
// stored `ticket` there.  Inline: it is the whole wait of a decode! at batch 1.
inline ldpc_status wait_flag(volatile unsigned int *flag, unsigned int ticket, hipStream_t stream, int device, const char *what)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 1;; ++spins) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return LDPC_OK;
        if ((spins & 0xffff) == 0) {   // every ~65k polls: is the kernel still alive?  (and the bound of host_wait.hpp)
            const int64_t lim = wait_limit_ms();
            if (lim > 0 && std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > lim)
                return wait_expired(device, what);   // (names the wait, marks the device; never LDPC_OK before the copy-out)
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ticket) return LDPC_OK;
                return set_error(LDPC_ERR_HIP, "latency path: the kernel finished without raising its flag");
            }
            if (q != hipErrorNotReady) {
                (void)hipGetLastError();
                return set_error(LDPC_ERR_HIP, std::string("latency path: ") + hipGetErrorString(q));
            }
        }
        __builtin_ia32_pause();
    }
}

// The latency paths' image: host memory mapped into the device, [flag header 256 B][staging image].  The kernel reads and
// writes the image in place and its last workgroup stores the call's ticket into the first word of the header, which
// wait_flag() spins on.  Tickets skip 0, the value of a fresh header.
struct LatencyImage {
    static constexpr size_t kHeader = 256;
    void *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    unsigned ticket = 0;
    ldpc_status ensure(size_t image_bytes)   // room for an image of that many bytes behind the header
    {
        if (cap >= kHeader + image_bytes) return LDPC_OK;
        release();
        LDPC_HIP_TRY(hipHostMalloc(&host, kHeader + image_bytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(host, 0, kHeader);
        LDPC_HIP_TRY(hipHostGetDevicePointer(&dev, host, 0));
        cap = kHeader + image_bytes;
        return LDPC_OK;
    }
    void release()
    {
        if (host) (void)hipHostFree(host);
        host = dev = nullptr; cap = 0;
    }
    char *image() const { return (char *)host + kHeader; }
    char *image_dev() const { return (char *)dev + kHeader; }
    volatile unsigned int *flag() const { return (volatile unsigned int *)host; }
    unsigned int *flag_dev() const { return (unsigned int *)dev; }
    unsigned next_ticket() { if (++ticket == 0) ticket = 1; return ticket; }
};

}  // namespace ldpc_detail
