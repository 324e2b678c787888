// priors_plan_sanitize.cpp -- the HIP-free planner of the min-sum entries with per-syndrome priors (csrc/tile_plan.hpp:
// ms_priors_offset, ms_priors_state_bytes, priors_tile_plan) under AddressSanitizer + UBSan on the CPU, over sizes from
// nothing to the largest create accepts, both schedules, every variant.  Built and run by tests/test_priors_cpu.py:
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
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)72, (int64_t)96, (int64_t)6144, (int64_t)10240, (int64_t)13824, ((int64_t)1 << 28) - 1})
        for (int64_t s : {(int64_t)0, (int64_t)1, (int64_t)3, n / 2, n})
            for (int64_t rec : {(int64_t)0, 4 * s, ((int64_t)1 << 31) - 1})
                for (int variant = 0; variant < 3; ++variant) {
                    // the layered schedule keeps no priors block: the plain plan
                    TilePlan plain, lay;
                    const bool pok = tile_plan(s, n, rec, false, variant, &plain);
                    CHECK(priors_tile_plan(s, n, rec, true, variant, &lay) == pok);
                    if (pok) CHECK(lay.tier == plain.tier && lay.S == plain.S && lay.shift == plain.shift && lay.state_bytes == plain.state_bytes);
                    // the flooding schedule: the fourth block starts on a word behind the plain state and ends inside the slot
                    TilePlan pl;
                    const size_t one = ms_priors_state_bytes(s, n, rec, 1);
                    const bool ok = priors_tile_plan(s, n, rec, false, variant, &pl);
                    CHECK(ok == !(variant == 1 && one > kTileLdsOne));
                    ++*count;
                    if (!ok) continue;
                    CHECK(pl.S == 1 << pl.shift && pl.S >= 1 && pl.S <= 64 && (pl.tier == 1 || (pl.tier == 2 && pl.S == 64)));
                    CHECK(pl.tier == 2 || pl.state_bytes <= kTileLdsOne);
                    CHECK(pl.state_bytes % 256 == 0 && pl.state_bytes >= one);
                    const size_t off = ms_priors_offset(s, n, rec, pl.S);
                    const size_t raw = ((size_t)(n + rec) * 4 + (size_t)s) * (size_t)pl.S;
                    CHECK(off % 4 == 0 && off >= raw && off < raw + 4);
                    CHECK(off + (size_t)n * 4 * (size_t)pl.S <= pl.state_bytes);
                    CHECK(pl.state_bytes >= ms_state_bytes(s, n, rec, pl.S));
                    if (pok && plain.tier == 1 && pl.tier == 1) CHECK(pl.S <= plain.S);   // a larger state never widens the tile
                    if (variant == 0 && pl.tier == 1 && pl.S < 64)                        // the widest that fits its budget
                        CHECK(ms_priors_state_bytes(s, n, rec, pl.S * 2) > (pl.state_bytes <= kTileLdsTwo ? kTileLdsTwo : kTileLdsOne));
                }
    return true;
}

int main()
{
    int n = 0;
    if (!plans(&n)) return 1;
    // the shapes of the proposal: (8,4)-regular, s = n / 2, rec_words = 2 n
    TilePlan a, b;
    if (!tile_plan(48, 96, 192, false, 0, &a) || !priors_tile_plan(48, 96, 192, false, 0, &b) || a.S != 64 || b.S != 32 || b.tier != 1) return 2;
    if (!tile_plan(5120, 10240, 20480, false, 0, &a) || !priors_tile_plan(5120, 10240, 20480, false, 0, &b) || a.tier != 1 || a.S != 1 || b.tier != 2) return 3;
    if (priors_tile_plan(5120, 10240, 20480, false, 1, &b)) return 4;
    std::printf("OK %d priors plans\n", n);
    return 0;
}
