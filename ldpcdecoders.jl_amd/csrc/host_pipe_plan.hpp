// host_pipe_plan.hpp -- the arithmetic of the host staging of the BP decoder's host-pointer entries (ldpc_mi355x.hip:
// ldpc_bp_decode_batch and ldpc_bp_decode_batch_bits): how a staging image is carved, how a large batch is cut into the
// chunks of the 3-slot pipeline, and where a chunk of columns lies in a caller's bit-packed arrays.  Pure host code over the
// standard library -- no HIP, no decoder handle, no environment -- like team_plan.hpp and bpots_plan.hpp, so that it builds
// with a plain C++ compiler and runs under the sanitizers on the CPU (tests/native/host_pipe_plan_sanitize.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ldpc_detail {

// Carves a staging image into regions that each start on a 256-byte boundary: take() hands out the offset of the next
// region, `at` is the size of what has been taken so far.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

// The staging image of `rows` syndromes, [syndromes][errors][converged][iterations][LLRs]: the syndromes lie at 0, the
// other regions at the offsets below.  The entry says how many bytes its syndromes and errors take (bytes, or the
// words that cover bits: word_image_bytes()).
struct StageLayout {
    size_t o_err = 0, o_conv = 0, o_it = 0, o_llr = 0, total = 0;
};
inline StageLayout stage_layout(size_t rows, size_t syn_bytes, size_t err_bytes, bool want_llr, size_t n)
{
    Carve image;
    StageLayout L;
    image.take(syn_bytes);
    L.o_err = image.take(err_bytes);
    L.o_conv = image.take(rows);
    L.o_it = image.take(rows * sizeof(int32_t));
    L.o_llr = image.take(want_llr ? rows * n * sizeof(double) : 0);
    L.total = image.at;
    return L;
}

// bytes of the words covering nbits that start at any bit of a word
inline size_t word_image_bytes(size_t nbits) { return (((nbits + 63) >> 6) + 1) * sizeof(uint64_t); }

// Chunks of the large-batch pipeline: chunk_mb MiB worth of syndromes (`bps` bytes each), at least `floor` of them
// (enough to fill the chip), rounded up to 4096, and no trailing chunk under half a chunk.  override_syndromes > 0 sets
// the chunk outright (tests: chunk borders inside words, ring growth).
struct ChunkPlan {
    size_t cb = 0, nchunks = 0;   // syndromes per chunk; chunks
};
inline ChunkPlan pipe_chunks(size_t bps, size_t floor, size_t B, size_t chunk_mb = 24, size_t override_syndromes = 0)
{
    ChunkPlan c;
    c.cb = (std::max<size_t>(chunk_mb, 1) << 20) / std::max<size_t>(bps, 1);
    c.cb = std::max(c.cb, floor);
    c.cb = (c.cb + 4095) & ~(size_t)4095;
    if (B < c.cb + c.cb / 2) c.cb = B;
    if (override_syndromes) c.cb = override_syndromes;
    c.nchunks = c.cb ? (B + c.cb - 1) / c.cb : 0;
    return c;
}

// Columns [b0, b0 + nb) of r bits each in a caller's bit string that starts at bit `bit0`: the first word they touch,
// the offset of their first bit in it, and how many words cover them.
struct Span {
    size_t w0 = 0;
    int off = 0;
    size_t nwords = 0;
};
inline Span span_of(int64_t bit0, size_t b0, size_t nb, size_t r)
{
    const size_t lo = (size_t)bit0 + b0 * r;
    Span sp;
    sp.w0 = lo >> 6;
    sp.off = (int)(lo & 63);
    sp.nwords = nb * r ? ((size_t)sp.off + nb * r + 63) >> 6 : 0;
    return sp;
}

// Bits [off, off + nbits) of src -> the same bits of dst (word 0 of both holds bit 0 of the numbering).  Interior words
// are copied by `copy` (memcpy's signature); a partial first / last word is merged under its mask with atomic and / or
// on the word, because the shards of the multi-device entry merge from threads of their own and two neighbouring shards
// can share a word.
template <class Copy>
inline void merge_bit_range(uint64_t *dst, const uint64_t *src, int off, size_t nbits, Copy copy)
{
    if (!nbits) return;
    const size_t nw = ((size_t)off + nbits + 63) >> 6;
    const int end = (int)(((size_t)off + nbits) & 63);
    auto masked = [&](size_t q, uint64_t mask) {
        (void)__atomic_fetch_and(&dst[q], ~mask, __ATOMIC_RELAXED);
        (void)__atomic_fetch_or(&dst[q], src[q] & mask, __ATOMIC_RELAXED);
    };
    const uint64_t mfirst = ~(uint64_t)0 << off, mlast = end ? ((uint64_t)1 << end) - 1 : ~(uint64_t)0;
    if (nw == 1) { masked(0, mfirst & mlast); return; }
    size_t lo = 0, hi = nw;
    if (off) { masked(0, mfirst); lo = 1; }
    if (end) { masked(nw - 1, mlast); hi = nw - 1; }
    if (hi > lo) copy(dst + lo, src + lo, (hi - lo) * sizeof(uint64_t));
}
inline void merge_bit_range(uint64_t *dst, const uint64_t *src, int off, size_t nbits)
{
    merge_bit_range(dst, src, off, nbits, [](void *d, const void *s, size_t b) { std::memcpy(d, s, b); });
}

}  // namespace ldpc_detail
