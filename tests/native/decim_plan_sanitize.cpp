// decim_plan_sanitize.cpp -- the HIP-free planner of the guided-decimation min-sum decoder (csrc/tile_plan.hpp:
// decim_state_bytes, decim_tile_plan) under AddressSanitizer + UBSan on the CPU, over sizes from nothing to the largest
// create accepts, every variant.  Built and run by tests/test_decim_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ldpcdecoders.jl_amd/csrc ...
#include <cstdint>
#include <cstdio>

#include "tile_plan.hpp"

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
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)31, (int64_t)32, (int64_t)33, (int64_t)72, (int64_t)150, (int64_t)240,
                      (int64_t)6144, (int64_t)10240, (int64_t)13824, (int64_t)16384, ((int64_t)1 << 28) - 1})
        for (int64_t s : {(int64_t)0, (int64_t)1, (int64_t)3, n / 2, n})
            for (int64_t rec : {(int64_t)0, 4 * s, ((int64_t)1 << 31) - 1})
                for (int variant = 0; variant < 3; ++variant) {
                    TilePlan pl, plain;
                    const size_t one = decim_state_bytes(s, n, rec, 1);
                    const bool ok = decim_tile_plan(s, n, rec, variant, &pl);
                    CHECK(ok == !(variant == 1 && one > kTileLdsOne));
                    ++*count;
                    if (!ok) continue;
                    CHECK(pl.S == 1 << pl.shift && pl.S >= 1 && pl.S <= 64 && (pl.tier == 1 || (pl.tier == 2 && pl.S == 64)));
                    CHECK(pl.tier == 2 || pl.state_bytes <= kTileLdsOne);
                    CHECK(variant == 0 || pl.tier == variant);
                    CHECK(pl.state_bytes % 256 == 0 && pl.state_bytes >= one && pl.state_bytes == decim_state_bytes(s, n, rec, pl.S));
                    // the four blocks end inside the slot: L, the records, D (a bit per bit, whole words), the syndromes
                    const size_t dw = (size_t)((n + 31) / 32);
                    CHECK(dw * 32 >= (size_t)n && (dw == 0 || (dw - 1) * 32 < (size_t)n));
                    const size_t raw = (((size_t)n + (size_t)rec + dw) * 4 + (size_t)s) * (size_t)pl.S;
                    CHECK(raw <= pl.state_bytes && pl.state_bytes < raw + 256);
                    // the state lies between the min-sum one (no D) and the relay one (a second float block as well)
                    CHECK(pl.state_bytes >= ms_state_bytes(s, n, rec, pl.S) && pl.state_bytes <= relay_state_bytes(s, n, rec, pl.S));
                    if (tile_plan(s, n, rec, false, variant, &plain) && plain.tier == 1 && pl.tier == 1) CHECK(pl.S <= plain.S);
                    if (variant == 0 && pl.tier == 1 && pl.S < 64)   // the widest that fits its budget
                        CHECK(decim_state_bytes(s, n, rec, pl.S * 2) > (pl.state_bytes <= kTileLdsTwo ? kTileLdsTwo : kTileLdsOne));
                    if (variant == 0 && pl.tier == 2) CHECK(one > kTileLdsOne);
                }
    return true;
}

int main()
{
    int n = 0;
    if (!plans(&n)) return 1;
    TilePlan a;
    if (!decim_tile_plan(36, 72, 144, 0, &a) || a.tier != 1 || a.S != 64 || a.state_bytes != 58368) return 2;      // BB-72
    if (!decim_tile_plan(120, 240, 480, 0, &a) || a.tier != 1 || a.S != 16 || a.state_bytes != 48640) return 3;    // (240, 8, 4): 3032 bytes a lane
    if (!decim_tile_plan(8192, 16384, 32768, 0, &a) || a.tier != 2 || a.S != 64) return 4;                        // 206848 bytes a lane
    if (decim_tile_plan(8192, 16384, 32768, 1, &a)) return 5;
    std::printf("OK %d decimation plans\n", n);
    return 0;
}
