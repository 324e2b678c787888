// osd_handle.hpp -- the `ldpc_osd` handle, shared by its host step (osd_host.cpp, plain C++: it also builds
// without HIP, tests/native/osd_sanitize.cpp) and its opt-in device step (ldpc_osd_device.hip).
#pragma once
#include <stdint.h>

#include <vector>

struct ldpc_osd {
    int64_t m = 0, n = 0;
    int64_t order = 0;
    int64_t nw = 0;                 // words per row
    std::vector<uint64_t> rows;     // m * nw, bit c of row i = H[i, c]
    // device side: NULL until ldpc_osd_device_prepare; ldpc_osd_destroy releases it through dev_free
    void *dev = nullptr;
    void (*dev_free)(void *) = nullptr;
};
