// bpots_plan_sanitize.cpp -- the HIP-free planner of the BP-OTS decoder (csrc/bpots_plan.hpp: ots_lds_bytes,
// ots_node_lds_bytes, ots_plan, ots_groups, ots_latency_ok, ots_queue_launch) under AddressSanitizer + UBSan on the CPU, over
// sizes from nothing to the largest create accepts, every bucket and every force_node.  Built and run by
// tests/test_bpots_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ldpcdecoders.jl_amd/csrc ...
#include <cstdint>
#include <cstdio>

#include "bpots_plan.hpp"

using namespace ldpc;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            return false;                                                         \
        }                                                                         \
    } while (0)

static bool plans(int *count)
{
    const int64_t top = kOtsMaxSize;
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)18, (int64_t)120, (int64_t)606, (int64_t)612, (int64_t)1500, (int64_t)1512,
                      (int64_t)23628, (int64_t)23634, (int64_t)65534, (int64_t)65535, top - 1, top})
        for (int64_t s : {(int64_t)0, (int64_t)1, n / 2, n})
            for (int64_t nnz : {(int64_t)0, n, 3 * n, top - 1, top})
                for (int cdeg : {0, 8, 9, 32, 33})
                    for (int bdeg : {0, 4, 5, 16, 17})
                        for (int force = 0; force < 3; ++force) {
                            OtsPlan p;
                            const bool ok = ots_plan(s, n, nnz, cdeg, bdeg, force, &p);
                            ++*count;
                            CHECK(ok == (s < top && n < top && nnz < top));
                            if (!ok) continue;
                            const bool wide = cdeg > 32 || bdeg > 16;
                            CHECK(p.kernel == 2 || p.kernel == 3 || p.kernel == 5);
                            CHECK((p.kernel == 2) == (p.logS >= 0) && p.logS <= 6);
                            if (wide || force >= 2) CHECK(p.kernel == 5);
                            if (force == 1) CHECK(p.kernel != 2);
                            if (p.kernel == 5) CHECK(p.DC == 0 && p.DV == 0 && p.lds_bytes == 0 && p.budget_kib == 0);
                            else CHECK(p.DC == (cdeg <= 8 ? 8 : 32) && p.DV == (bdeg <= 4 ? 4 : 16) && p.DC >= cdeg && p.DV >= bdeg);
                            if (p.kernel == 3) CHECK(p.lds_bytes == ots_node_lds_bytes((int)s, (int)n) && p.lds_bytes + 1024 <= kOtsLdsOne && p.budget_kib == 0);
                            if (p.kernel == 2) {
                                const int S = 1 << p.logS;
                                CHECK(s < 65535 && n < 65535 && nnz < 65535);
                                CHECK(p.lds_bytes == ots_lds_bytes((int)s, (int)n, (int)nnz, S));
                                const size_t need = p.lds_bytes + kOtsLdsStatic;
                                CHECK(p.budget_kib == (need <= kOtsLdsTwo ? 76 : 156) && need <= kOtsLdsOne);
                                if (p.budget_kib == 156) CHECK(S == 1);                       // the large budget only with S = 1
                                if (S < 64) CHECK(ots_lds_bytes((int)s, (int)n, (int)nnz, 2 * S) + kOtsLdsStatic > kOtsLdsTwo);   // the widest that fits 76 KiB
                                for (int64_t batch : {(int64_t)1, (int64_t)S, (int64_t)S + 1, (int64_t)8195, (int64_t)1 << 40}) {
                                    const int64_t g = ots_groups(batch, p.logS);
                                    CHECK(g * S >= batch && (g - 1) * S < batch);
                                    if (g > ((int64_t)1 << 30)) continue;                     // (refused by the decode entries)
                                    int grid = 0, chunk = 0;
                                    for (int per_cu : {1, 2, 4}) {
                                        ots_queue_launch(g, per_cu, 256, &grid, &chunk);
                                        CHECK(grid >= 1 && grid <= g && grid <= per_cu * 256 && chunk >= 1 && chunk <= 64);
                                        CHECK((chunk >= 2) == (g >= 32 * (int64_t)grid));
                                    }
                                    CHECK(ots_latency_ok(kOtsLatencyImage, g, 256) == (g <= 512) && !ots_latency_ok(kOtsLatencyImage + 1, 1, 256));
                                }
                            }
                        }
    return true;
}

int main()
{
    int n = 0;
    if (!plans(&n)) return 1;
    OtsPlan p;
    // (3,6)-regular: the two edges of the table in bytes
    if (!ots_plan(303, 606, 1818, 6, 3, 0, &p) || p.logS != 0 || p.lds_bytes + kOtsLdsStatic != 77774 || p.budget_kib != 76) return 2;
    if (!ots_plan(750, 1500, 4500, 6, 3, 0, &p) || p.logS != 0 || p.lds_bytes + kOtsLdsStatic != 159128 || p.budget_kib != 156) return 3;
    if (!ots_plan(756, 1512, 4536, 6, 3, 0, &p) || p.kernel != 3) return 4;
    std::printf("OK %d bpots plans\n", n);
    return 0;
}
