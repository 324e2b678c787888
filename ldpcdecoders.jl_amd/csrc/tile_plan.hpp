// tile_plan.hpp -- what the host of every decoder of the min-sum family (ldpc_minsum.hip, ldpc_relay.hip, ldpc_pauli.hip,
// ldpc_decim.hip, ldpc_pauli_relay.hip, ldpc_stab.hip; device code: minsum_kernels.hpp, layered_kernels.hpp, relay_kernels.hpp,
// pauli_kernels.hpp, decim_kernels.hpp, pauli_relay_kernels.hpp, stab_kernels.hpp) derives from a graph's sizes
// alone: the sizes of a tile's state, the tier and the tile width chosen from them (the policy: plan_tiles(), the one
// place it is stated) and the check records of a Tanner graph (ms_records(), the one place they are laid out).  Pure host
// code over the standard library -- no HIP, no decoder handle, no environment -- so that it builds with a plain C++
// compiler and runs under the sanitizers on the CPU (tests/native/team_plan_sanitize.cpp, priors_plan_sanitize.cpp,
// records_sanitize.cpp).  The `create` routines call the plans; the ldpc_debug_*tile_plan entries
// (include/ldpc_mi355x_debug.h) hand them to the CPU tests.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

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

// The choice, over bytes(S) = the state of a tile of S syndromes.  On-chip with the largest power of two S <= 64 that
// leaves room for two workgroups a CU, else the largest that fits one; where not even one syndrome fits, the unlimited
// tier with S = 64.  variant 1 / 2 force a tier (0 = by size).  false: variant 1 and nothing fits.
template <class Bytes> inline bool plan_tiles(Bytes bytes, int variant, TilePlan *out)
{
    int S = 0;
    for (size_t budget : {kTileLdsTwo, kTileLdsOne})
        for (int w = 64; w >= 1 && !S; w >>= 1)
            if (bytes(w) <= budget) S = w;
    if (variant == 1 && !S) return false;
    TilePlan p;
    p.tier = variant ? variant : S ? 1 : 2;
    p.S = p.tier == 1 ? S : 64;
    for (p.shift = 0; (1 << p.shift) < p.S; p.shift++) {}
    p.state_bytes = bytes(p.S);
    *out = p;
    return true;
}

// the plan of the min-sum decoder (plain entries, both schedules) and of the relay decoder
inline bool tile_plan(int64_t s, int64_t n, int64_t rec_words, bool relay, int variant, TilePlan *out)
{
    return plan_tiles([=](int S) { return relay ? relay_state_bytes(s, n, rec_words, S) : ms_state_bytes(s, n, rec_words, S); }, variant, out);
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

// The plan of the priors entries.  The layered schedule reads the prior only when a tile starts and keeps no P, so its
// plan is tile_plan()'s.
inline bool priors_tile_plan(int64_t s, int64_t n, int64_t rec_words, bool layered, int variant, TilePlan *out)
{
    if (layered) return tile_plan(s, n, rec_words, false, variant, out);
    return plan_tiles([=](int S) { return ms_priors_state_bytes(s, n, rec_words, S); }, variant, out);
}

// ---- the joint X/Z (Pauli) min-sum decoder --------------------------------------------------------------------------------
// bytes of a Pauli tile's state: S lanes of (2 n + rec_words) words -- the two message totals TX, TZ and the check records of
// both sides -- and s = rx + rz syndrome bytes, rounded up to 256
inline size_t pauli_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(2 * n + rec_words) * 4 + (size_t)s) * (size_t)S + 255) & ~(size_t)255;
}

// Its plan (s = rx + rz, rec_words over the checks of both sides).
inline bool pauli_tile_plan(int64_t s, int64_t n, int64_t rec_words, int variant, TilePlan *out)
{
    return plan_tiles([=](int S) { return pauli_state_bytes(s, n, rec_words, S); }, variant, out);
}

// ---- the guided-decimation min-sum decoder ------------------------------------------------------------------------------------
// bytes of a decimation tile's state: S lanes of (n + rec_words + ceil(n / 32)) words -- L (the pins live in it), the check
// records and the set D of decimated bits, a bit each -- and s syndrome bytes, rounded up to 256
inline size_t decim_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(n + rec_words + ((n + 31) >> 5)) * 4 + (size_t)s) * (size_t)S + 255) & ~(size_t)255;
}

// Its plan.
inline bool decim_tile_plan(int64_t s, int64_t n, int64_t rec_words, int variant, TilePlan *out)
{
    return plan_tiles([=](int S) { return decim_state_bytes(s, n, rec_words, S); }, variant, out);
}

// ---- the Pauli relay min-sum decoder -------------------------------------------------------------------------------------------
// bytes of a Pauli relay tile's state: S lanes of (6 n + rec_words + 2 ceil(n / 32)) words -- the three beliefs the check
// sweep reads, the three posteriors, the check records of both sides, a bit plane each for the X part and the Z part of the
// lightest solution -- and s = rx + rz syndrome bytes, rounded up to 256
inline size_t pauli_relay_state_bytes(long long s, long long n, long long rec_words, int S)
{
    return (((size_t)(6 * n + rec_words + 2 * ((n + 31) >> 5)) * 4 + (size_t)s) * (size_t)S + 255) & ~(size_t)255;
}

// Its plan (s = rx + rz, rec_words over the checks of both sides).
inline bool pauli_relay_tile_plan(int64_t s, int64_t n, int64_t rec_words, int variant, TilePlan *out)
{
    return plan_tiles([=](int S) { return pauli_relay_state_bytes(s, n, rec_words, S); }, variant, out);
}

// ---- the stabilizer (non-CSS) min-sum decoder -----------------------------------------------------------------------------------
// bytes of a stabilizer tile's state: S lanes of (3 n + rec_words) words -- the message totals MX, MY, MZ of the three edge
// types and the check records -- and r syndrome bytes, rounded up to 256
inline size_t stab_state_bytes(long long r, long long n, long long rec_words, int S)
{
    return (((size_t)(3 * n + rec_words) * 4 + (size_t)r) * (size_t)S + 255) & ~(size_t)255;
}

// Its plan (r checks, rec_words over the checks of the union graph).
inline bool stab_tile_plan(int64_t r, int64_t n, int64_t rec_words, int variant, TilePlan *out)
{
    return plan_tiles([=](int S) { return stab_state_bytes(r, n, rec_words, S); }, variant, out);
}

// ---- the check records of a graph ------------------------------------------------------------------------------------------
constexpr int kMsPosEdge = (int)0x80000000;   // flag in edge_pos: the check keeps one message per edge (degree > 64)

struct MsRecords {
    std::vector<int> rec_off;    // [max(s, 1)]: first word of the check's record
    std::vector<int> edge_rec;   // [nnz], per CSC edge: rec_off of its check
    std::vector<int> edge_pos;   // [nnz], per CSC edge: position of the bit in its check (| kMsPosEdge)
    int64_t words = 0;           // of all records; a caller narrows it only after its own range check
};

// From the CSR row pointers [s + 1] and, per CSC edge, its check (csc_row) and its place in the CSR order (csc2csr): the
// arrays of ldpc_detail::TannerGraph (host_common.hpp).  words <= 4 s + nnz.
inline MsRecords ms_records(int64_t s, int64_t nnz, const int *row_ptr, const int *csc_row, const int *csc2csr)
{
    MsRecords r;
    r.rec_off.assign((size_t)(s > 1 ? s : 1), 0);
    r.edge_rec.assign((size_t)nnz, 0);
    r.edge_pos.assign((size_t)nnz, 0);
    for (int64_t i = 0; i < s; ++i) {
        r.rec_off[(size_t)i] = (int)r.words;
        r.words += ms_record_words(row_ptr[i + 1] - row_ptr[i]);
    }
    for (int64_t e = 0; e < nnz; ++e) {
        const int i = csc_row[e], k = csc2csr[e] - row_ptr[i];
        r.edge_rec[(size_t)e] = r.rec_off[(size_t)i];
        r.edge_pos[(size_t)e] = row_ptr[i + 1] - row_ptr[i] > 64 ? (k | kMsPosEdge) : k;
    }
    return r;
}

}  // namespace ldpc
