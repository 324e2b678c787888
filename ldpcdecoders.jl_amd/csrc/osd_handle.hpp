// osd_handle.hpp -- the `ldpc_osd` handle, shared by its host step (osd_host.cpp, plain C++: it also builds
// without HIP, tests/native/osd_sanitize.cpp) and its opt-in device step (ldpc_osd_device.hip).
#pragma once
#include <stdint.h>

#include <vector>

// bounds of ldpc_osd_set_search: the order of each method, and n (a cost is a sum of at most 2^22 terms below 2^41)
constexpr int64_t kOsdSearchExhaustiveCap = 16, kOsdSearchSweepCap = 64, kOsdSearchMaxBits = (int64_t)1 << 22;

struct ldpc_osd {
    int64_t m = 0, n = 0;
    int64_t order = 0;
    int64_t nw = 0;                 // words per row
    std::vector<uint64_t> rows;     // m * nw, bit c of row i = H[i, c]
    // ldpc_osd_set_search: 0 = the reference rule, 1 = exhaustive, 2 = combination sweep (the standard rule, device
    // form only); q = the weight of each bit, empty for all ones
    int32_t method = 0;
    std::vector<int64_t> q;
    // device side: NULL until ldpc_osd_device_prepare; ldpc_osd_destroy releases it through dev_free
    void *dev = nullptr;
    void (*dev_free)(void *) = nullptr;
};
