// pauli_relay_plan_sanitize.cpp -- the HIP-free planner of the Pauli relay min-sum decoder (csrc/tile_plan.hpp:
// pauli_relay_state_bytes, pauli_relay_tile_plan) under AddressSanitizer + UBSan on the CPU, over sizes from nothing to the
// largest create accepts, every variant.  Built and run by tests/test_pauli_relay_cpu.py:
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
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)13, (int64_t)31, (int64_t)32, (int64_t)33, (int64_t)72, (int64_t)225,
                      (int64_t)2560, (int64_t)3328, (int64_t)6705, (int64_t)6784, (int64_t)1 << 22, ((int64_t)1 << 28) - 1})
        for (int64_t s : {(int64_t)0, (int64_t)2, (int64_t)3, n / 2, n})
            for (int64_t rec : {(int64_t)0, 4 * s, ((int64_t)1 << 31) - 1})
                for (int variant = 0; variant < 3; ++variant) {
                    TilePlan pl, pauli;
                    const size_t one = pauli_relay_state_bytes(s, n, rec, 1);
                    const bool ok = pauli_relay_tile_plan(s, n, rec, variant, &pl);
                    CHECK(ok == !(variant == 1 && one > kTileLdsOne));
                    ++*count;
                    if (!ok) continue;
                    CHECK(pl.S == 1 << pl.shift && pl.S >= 1 && pl.S <= 64 && (pl.tier == 1 || (pl.tier == 2 && pl.S == 64)));
                    CHECK(pl.tier == 2 || pl.state_bytes <= kTileLdsOne);
                    CHECK(variant == 0 || pl.tier == variant);
                    CHECK(pl.state_bytes % 256 == 0 && pl.state_bytes >= one && pl.state_bytes == pauli_relay_state_bytes(s, n, rec, pl.S));
                    // the five blocks end inside the slot: G and M (three beliefs each), the records, the two bit planes of
                    // best (whole words), the syndromes
                    const size_t bw = (size_t)((n + 31) / 32);
                    CHECK(bw * 32 >= (size_t)n && (bw == 0 || (bw - 1) * 32 < (size_t)n));
                    const size_t raw = ((6 * (size_t)n + (size_t)rec + 2 * bw) * 4 + (size_t)s) * (size_t)pl.S;
                    CHECK(raw <= pl.state_bytes && pl.state_bytes < raw + 256);
                    // the state holds the Pauli min-sum one (TX, TZ, the records) and the relay one (X, M, the records, one plane)
                    CHECK(pl.state_bytes >= pauli_state_bytes(s, n, rec, pl.S) && pl.state_bytes >= relay_state_bytes(s, n, rec, pl.S));
                    if (pauli_tile_plan(s, n, rec, variant, &pauli) && pauli.tier == 1 && pl.tier == 1) CHECK(pl.S <= pauli.S);
                    if (variant == 0 && pl.tier == 1 && pl.S < 64)   // the widest that fits its budget
                        CHECK(pauli_relay_state_bytes(s, n, rec, pl.S * 2) > (pl.state_bytes <= kTileLdsTwo ? kTileLdsTwo : kTileLdsOne));
                    if (variant == 0 && pl.tier == 2) CHECK(one > kTileLdsOne);
                }
    return true;
}

int main()
{
    int n = 0;
    if (!plans(&n)) return 1;
    TilePlan a;
    if (!pauli_relay_tile_plan(72, 72, 288, 0, &a) || a.tier != 1 || a.S != 16 || a.state_bytes != 47616) return 2;      // BB-72: 2976 bytes a lane
    if (!pauli_relay_tile_plan(72, 72, 288, 2, &a) || a.tier != 2 || a.S != 64 || a.state_bytes != 190464) return 3;
    if (!pauli_relay_tile_plan(12, 13, 48, 0, &a) || a.tier != 1 || a.S != 64 || a.state_bytes != 33536) return 4;       // 524 bytes a lane
    if (!pauli_relay_tile_plan(216, 225, 864, 0, &a) || a.tier != 1 || a.S != 8 || a.state_bytes != 73216) return 5;     // 9136 bytes a lane
    if (!pauli_relay_tile_plan(24, 6705, 48, 0, &a) || a.tier != 1 || a.S != 1 || a.state_bytes != kTileLdsOne) return 6;   // exactly 159 KiB
    if (!pauli_relay_tile_plan(25, 6705, 48, 0, &a) || a.tier != 2 || a.S != 64) return 7;
    if (pauli_relay_tile_plan(25, 6705, 48, 1, &a)) return 8;
    std::printf("OK %d Pauli relay plans\n", n);
    return 0;
}
