// tile_plan.hpp -- the tier and the tile width of the min-sum and the relay decoder (ldpc_minsum.hip, ldpc_relay.hip;
// device code: minsum_kernels.hpp, relay_kernels.hpp), and the sizes of a tile's state they are chosen from.  Pure host
// code over the standard library -- no HIP, no decoder handle, no environment -- so that it builds with a plain C++
// compiler and runs under the sanitizers on the CPU (tests/native/team_plan_sanitize.cpp).  Both `create` routines call
// tile_plan(); ldpc_debug_tile_plan (include/ldpc_mi355x_debug.h) hands it to the CPU tests.  At the end: the state size
// and the plan of the joint X/Z (Pauli) min-sum decoder (ldpc_pauli.hip), the same policy over another size.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace ldpc {

// words of check records for a check of degree `deg`
inline int ms_record_words(int deg) { return deg == 0 ? 0 : deg <= 32 ? 4 : deg <= 64 ? 5 : deg; }
// bytes of a min-sum tile's state: S lanes of (n + rec_words) words and s bytes, rounded up to 256
inline size_t ms_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(n + rec_words) * 4 + (size_t)s) * (size_t)S + 255) & ~(size_t)255;
}
// bytes of a relay tile's state: S lanes of (2 n + rec_words + ceil(n / 32)) words and s bytes, rounded up to 256
inline size_t relay_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(2 * n + rec_words + ((n + 31) >> 5)) * 4 + (size_t)s) * (size_t)S + 255) & ~(size_t)255;
}

constexpr size_t kTileLdsTwo = (size_t)79 * 1024, kTileLdsOne = (size_t)159 * 1024;   // two / one workgroup a CU

struct TilePlan {
    int tier = 0;             // 1 = on-chip (the state in LDS), 2 = unlimited (the state in a global workspace)
    int S = 64, shift = 6;    // syndromes per tile, S = 1 << shift
    size_t state_bytes = 0;   // of a tile of S syndromes: the dynamic LDS of tier 1, a workspace slot of tier 2
};

// syndromes per workgroup of the on-chip tier: the largest power of two <= 64 whose state fits `budget`; 0 = none
inline int tile_lds_syndromes(int64_t s, int64_t n, int64_t rec_words, bool relay, size_t budget)
{
    for (int S = 64; S >= 1; S >>= 1)
        if ((relay ? relay_state_bytes(s, n, rec_words, S) : ms_state_bytes(s, n, rec_words, S)) <= budget) return S;
    return 0;
}

// The choice.  On-chip with the largest S that leaves room for two workgroups a CU, else the largest that fits one; where
// not even one syndrome fits, the unlimited tier with S = 64.  variant 1 / 2 force a tier (0 = by size).  false: variant 1
// and nothing fits.
inline bool tile_plan(int64_t s, int64_t n, int64_t rec_words, bool relay, int variant, TilePlan *out)
{
    int S = tile_lds_syndromes(s, n, rec_words, relay, kTileLdsTwo);
    if (!S) S = tile_lds_syndromes(s, n, rec_words, relay, kTileLdsOne);
    if (variant == 1 && !S) return false;
    TilePlan p;
    p.tier = variant ? variant : S ? 1 : 2;
    p.S = p.tier == 1 ? S : 64;
    for (p.shift = 0; (1 << p.shift) < p.S; p.shift++) {}
    p.state_bytes = relay ? relay_state_bytes(s, n, rec_words, p.S) : ms_state_bytes(s, n, rec_words, p.S);
    *out = p;
    return true;
}

// ---- per-syndrome priors (the ldpc_minsum_decode_batch_priors / _given entries) ------------------------------------------
// The flooding schedule re-reads the prior in every bit sweep, so a tile keeps its priors as a fourth block P [n][S] f32
// behind the three of ms_state_bytes(); the block starts on a word: the S s syndrome bytes before it are rounded up to 4.
inline size_t ms_priors_offset(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(n + rec_words) * 4 + (size_t)s) * (size_t)S + 3) & ~(size_t)3;
}
// bytes of such a tile's state, rounded up to 256
inline size_t ms_priors_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (ms_priors_offset(s, n, rec_words, S) + (size_t)n * 4 * (size_t)S + 255) & ~(size_t)255;
}

// The plan of the priors entries: the policy of tile_plan() over the larger state.  The layered schedule reads the prior
// only when a tile starts and keeps no P, so its plan is tile_plan()'s.  false: variant 1 and nothing fits.
inline bool priors_tile_plan(int64_t s, int64_t n, int64_t rec_words, bool layered, int variant, TilePlan *out)
{
    if (layered) return tile_plan(s, n, rec_words, false, variant, out);
    int S = 0;
    for (size_t budget : {kTileLdsTwo, kTileLdsOne}) {
        for (int w = 64; w >= 1 && !S; w >>= 1)
            if (ms_priors_state_bytes(s, n, rec_words, w) <= budget) S = w;
        if (S) break;
    }
    if (variant == 1 && !S) return false;
    TilePlan p;
    p.tier = variant ? variant : S ? 1 : 2;
    p.S = p.tier == 1 ? S : 64;
    for (p.shift = 0; (1 << p.shift) < p.S; p.shift++) {}
    p.state_bytes = ms_priors_state_bytes(s, n, rec_words, p.S);
    *out = p;
    return true;
}

// ---- the joint X/Z (Pauli) min-sum decoder (ldpc_pauli.hip; device code: pauli_kernels.hpp) ------------------------------
// bytes of a Pauli tile's state: S lanes of (2 n + rec_words) words -- the two message totals TX, TZ and the check records of
// both sides -- and s = rx + rz syndrome bytes, rounded up to 256
inline size_t pauli_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(2 * n + rec_words) * 4 + (size_t)s) * (size_t)S + 255) & ~(size_t)255;
}

// Its plan: the policy of tile_plan() over that size (s = rx + rz, rec_words over the checks of both sides).  false:
// variant 1 and nothing fits.
inline bool pauli_tile_plan(int64_t s, int64_t n, int64_t rec_words, int variant, TilePlan *out)
{
    int S = 0;
    for (size_t budget : {kTileLdsTwo, kTileLdsOne}) {
        for (int w = 64; w >= 1 && !S; w >>= 1)
            if (pauli_state_bytes(s, n, rec_words, w) <= budget) S = w;
        if (S) break;
    }
    if (variant == 1 && !S) return false;
    TilePlan p;
    p.tier = variant ? variant : S ? 1 : 2;
    p.S = p.tier == 1 ? S : 64;
    for (p.shift = 0; (1 << p.shift) < p.S; p.shift++) {}
    p.state_bytes = pauli_state_bytes(s, n, rec_words, p.S);
    *out = p;
    return true;
}

}  // namespace ldpc
