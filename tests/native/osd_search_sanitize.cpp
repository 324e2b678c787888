// osd_search_sanitize.cpp -- ldpc_osd_set_search (ldpcdecoders.jl_amd/csrc/osd_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: every argument check, the weight table q on the edge values of its formula, and the host
// entry's LDPC_ERR_UNSUPPORTED on a handle of the standard rule.  CPU build only; built and run by
// tests/test_osd_search_cpu.py::test_set_search_under_sanitizers.  Exit code 0 = all as stated.
#include "../../include/ldpc_mi355x.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace ldpc_detail {   // normally provided by host_common.hip
static std::string g_last;
ldpc_status set_error(ldpc_status st, const std::string &msg) { g_last = msg; return st; }
}  // namespace ldpc_detail

#define EXPECT(cond)                                                                          \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::printf("line %d: %s  (last error: %s)\n", __LINE__, #cond, ldpc_detail::g_last.c_str()); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

static ldpc_osd *make(int64_t s, int64_t n)
{
    std::vector<int64_t> colptr((size_t)n + 1), rowval((size_t)n);
    for (int64_t j = 0; j <= n; ++j) colptr[(size_t)j] = j;
    for (int64_t j = 0; j < n; ++j) rowval[(size_t)j] = j % s;
    ldpc_osd *h = nullptr;
    return ldpc_osd_create(s, n, n, colptr.data(), rowval.data(), 3, &h) == LDPC_OK ? h : nullptr;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double u = 1.0 / 65536.0;   // one unit of q
    // value -> weight: the clamps at +-2^24, halves to even on both sides of zero, plain values
    const double llr[] = {16777216.0, 1e9, -16777216.0, -1e9, 16777215.5, 0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u,
                          -2.5 * u, 0.0, -0.0, 1.0, -3.25, 0.49999 * u, 0.50001 * u, 2.0};
    const int64_t top = (int64_t)1 << 40;
    const int64_t want[] = {top, top, -top, -top, top - 32768, 0, 2, 2, 0, -2, -2, 0, 0, 65536, -212992, 0, 1, 131072};
    const int64_t n = (int64_t)(sizeof(llr) / sizeof(llr[0]));
    ldpc_osd *h = make(4, n);
    EXPECT(h);
    EXPECT(ldpc_osd_search_method(h) == 0 && ldpc_osd_search_method(nullptr) == 0);
    EXPECT(ldpc_osd_search_weight(h, 0) == 1);
    EXPECT(ldpc_osd_set_search(nullptr, 2, 10, n, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    for (int32_t method : {-1, 3, 7}) EXPECT(ldpc_osd_set_search(h, method, 0, n, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 1, -1, n, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 1, 17, n, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 2, 65, n, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 0, 41, n, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 2, 10, n + 1, nullptr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 2, 10, n - 1, llr) == LDPC_ERR_INVALID_ARGUMENT);
    EXPECT(ldpc_osd_set_search(h, 0, 3, n, llr) == LDPC_ERR_INVALID_ARGUMENT);
    for (double bad : {inf, -inf, nan}) {
        std::vector<double> v(llr, llr + n);
        v[(size_t)(n - 1)] = bad;
        EXPECT(ldpc_osd_set_search(h, 2, 10, n, v.data()) == LDPC_ERR_INVALID_ARGUMENT);
    }
    EXPECT(ldpc_osd_search_method(h) == 0 && ldpc_osd_search_weight(h, 1) == 1);   // a failed call changes nothing
    // the bounds themselves are accepted
    EXPECT(ldpc_osd_set_search(h, 1, 16, n, nullptr) == LDPC_OK && ldpc_osd_search_method(h) == 1);
    EXPECT(ldpc_osd_set_search(h, 2, 64, n, llr) == LDPC_OK && ldpc_osd_search_method(h) == 2);
    for (int64_t j = 0; j < n; ++j)
        if (ldpc_osd_search_weight(h, j) != want[j]) {
            std::printf("q[%lld] = %lld, expected %lld\n", (long long)j, (long long)ldpc_osd_search_weight(h, j), (long long)want[j]);
            return 1;
        }
    EXPECT(ldpc_osd_search_weight(h, -1) == 0 && ldpc_osd_search_weight(h, n) == 0 && ldpc_osd_search_weight(nullptr, 0) == 0);
    // the host entry has no form of the standard rule
    std::vector<uint8_t> syn(4), e((size_t)n), out((size_t)n);
    EXPECT(ldpc_osd_postprocess_batch(h, 1, syn.data(), e.data(), llr, out.data(), 1) == LDPC_ERR_UNSUPPORTED);
    EXPECT(ldpc_detail::g_last.find("ldpc_osd_postprocess_batch_device") != std::string::npos);
    // back to Hamming weights, then to the reference rule: the host entry works again
    EXPECT(ldpc_osd_set_search(h, 2, 0, n, nullptr) == LDPC_OK && ldpc_osd_search_weight(h, 0) == 1);
    EXPECT(ldpc_osd_set_search(h, 0, 2, n, nullptr) == LDPC_OK && ldpc_osd_search_method(h) == 0);
    EXPECT(ldpc_osd_postprocess_batch(h, 1, syn.data(), e.data(), llr, out.data(), 1) == LDPC_OK);
    ldpc_osd_destroy(h);
    // n beyond 2^22: a cost could leave int64
    const int64_t big = ((int64_t)1 << 22) + 1;
    h = make(1, big);
    EXPECT(h);
    EXPECT(ldpc_osd_set_search(h, 2, 10, big, nullptr) == LDPC_ERR_UNSUPPORTED);
    EXPECT(ldpc_osd_set_search(h, 0, 2, big, nullptr) == LDPC_OK);
    ldpc_osd_destroy(h);
    h = make(1, big - 1);
    EXPECT(h && ldpc_osd_set_search(h, 2, 10, big - 1, nullptr) == LDPC_OK);
    ldpc_osd_destroy(h);
    std::printf("OK\n");
    return 0;
}
