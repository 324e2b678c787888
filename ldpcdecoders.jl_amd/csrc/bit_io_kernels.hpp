// bit_io_kernels.hpp -- bit-packed (Julia BitMatrix layout) <-> one-byte-per-bit conversion, gfx950.
//
// A BitMatrix of r x B keeps element (row, col) as bit k = col * r + row of a flat little-endian bit string
// (word k >> 6 of `chunks`, bit k & 63, columns not padded); the library's byte layout [batch][r] has that element at
// byte k.  Both conversions are therefore FLAT: bit bit0 + k <-> byte k, k in [0, nbytes), no per-column logic.
//
// Shape (both kernels): the byte side is the wide side, so a lane moves 16 contiguous bytes per access (1 KiB per wave
// instruction) and folds them to / from 16 bits with a multiply; four neighbouring lanes make one 64-bit word.  A bit
// offset (bit0 & 63 != 0) is a funnel shift of two neighbouring words on the bit side; the byte side stays aligned
// (`bytes` is the handle's staging buffer: 256-byte aligned, element 0 at its start).  The last, partial 16 bytes of the
// array take a byte-by-byte path.  `words` points at the word that holds bit bit0, `off` = bit0 & 63.
//
// Neither kernel reads or writes a word outside the ceil((off + nbytes) / 64) words that cover the range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc_bitio {

typedef unsigned long long bu64;
constexpr int kThreads = 256;

__host__ __device__ inline long long words_covering(int off, long long nbytes) { return (off + nbytes + 63) >> 6; }

// 8 bytes (0/1 in bit 0 of each) -> 8 bits, byte i -> bit i: the product moves bit 8i to bit 56 + i, no two terms meet
__device__ inline unsigned fold8(bu64 x) { return (unsigned)(((x & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56); }
// 8 bits -> 8 bytes of 0/1: bit i alone in byte i, then "non-zero byte -> 1" without carries between bytes
__device__ inline bu64 spread8(unsigned b)
{
    const bu64 one_hot = ((bu64)(b & 0xffu) * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((one_hot + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

// bit off + k of `words` -> bytes[k] (0 / 1), k in [0, nbytes).
// A wave writes 1 KiB of bytes per step = 16 words of the shifted bit string; lanes 0..16 load the 17 input words that
// cover them (coalesced), every lane takes the two it needs by shuffle.
__global__ __launch_bounds__(kThreads) void bits_to_bytes_kernel(const bu64 *__restrict__ words, int off,
                                                                 uint8_t *__restrict__ bytes, long long nbytes)
{
    const int lane = threadIdx.x & 63, g = lane >> 2, part = lane & 3;
    const long long nin = words_covering(off, nbytes);
    const long long ntiles = (nbytes + 1023) >> 10;
    const long long wave0 = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kThreads) >> 6;
    for (long long t = wave0; t < ntiles; t += nwaves) {
        const long long j0 = t << 4;   // first shifted word of the tile
        bu64 v = 0;
        if (lane <= 16 && j0 + lane < nin) v = words[j0 + lane];
        const bu64 lo = __shfl(v, g), hi = __shfl(v, g + 1);
        const bu64 w = off ? (lo >> off) | (hi << (64 - off)) : lo;
        const unsigned h = (unsigned)(w >> (16 * part)) & 0xffffu;
        const long long k = (j0 << 6) + 16 * lane;
        if (k + 16 <= nbytes) {
            uint4 o;
            const bu64 a = spread8(h), b = spread8(h >> 8);
            o.x = (unsigned)a; o.y = (unsigned)(a >> 32); o.z = (unsigned)b; o.w = (unsigned)(b >> 32);
            *reinterpret_cast<uint4 *>(bytes + k) = o;
        } else {
            for (int i = 0; i < 16 && k + i < nbytes; ++i) bytes[k + i] = (uint8_t)((h >> i) & 1u);
        }
    }
}

// bytes[k] & 1 -> bit off + k of `words`, k in [0, nbytes).  Exactly those bits change: words wholly inside the range
// are plain 8-byte stores, the (at most two) partial boundary words are read, merged under a mask and written by the ONE
// lane that owns them -- no other writer exists inside the launch, so no zero-fill of the output and no atomics.
// A wave reads 1 KiB of bytes per step = 16 byte-aligned words; the first is the neighbour below that the funnel shift
// needs, so a step produces 15 output words and steps overlap by 64 bytes.
__global__ __launch_bounds__(kThreads) void bytes_to_bits_kernel(const uint8_t *__restrict__ bytes, long long nbytes,
                                                                 bu64 *__restrict__ words, int off)
{
    const int lane = threadIdx.x & 63, g = lane >> 2, part = lane & 3;
    const long long nout = words_covering(off, nbytes);
    const long long ntiles = (nout + 14) / 15;
    const long long wave0 = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kThreads) >> 6;
    const int end_bit = (int)((off + nbytes) & 63);   // bits of the last word that belong to the range (0 = all)
    for (long long t = wave0; t < ntiles; t += nwaves) {
        const long long j = t * 15 - 1 + g;           // byte-aligned word of this lane group: bytes [64 j, 64 j + 64)
        const long long k = (j << 6) + 16 * part;
        unsigned h = 0;
        if (j >= 0 && k + 16 <= nbytes) {
            const uint4 x = *reinterpret_cast<const uint4 *>(bytes + k);
            h = fold8((bu64)x.x | ((bu64)x.y << 32)) | (fold8((bu64)x.z | ((bu64)x.w << 32)) << 8);
        } else if (j >= 0) {
            for (int i = 0; i < 16 && k + i < nbytes; ++i) h |= (unsigned)(bytes[k + i] & 1u) << i;
        }
        bu64 w = (bu64)h << (16 * part);
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        const bu64 below = __shfl_up(w, 4);           // (group 0 takes nothing from it: it only feeds group 1)
        const long long q = j;                        // output word of this group
        if (g > 0 && part == 0 && q < nout) {
            const bu64 val = off ? (w << off) | (below >> (64 - off)) : w;
            bu64 mask = ~0ull;
            if (q == 0) mask &= ~0ull << off;
            if (q == nout - 1 && end_bit) mask &= (1ull << end_bit) - 1;
            words[q] = mask == ~0ull ? val : (words[q] & ~mask) | (val & mask);
        }
    }
}

inline int grid_for(long long ntiles, int num_cus)
{
    const long long blocks = (ntiles + (kThreads / 64) - 1) / (kThreads / 64);
    const long long cap = (long long)(num_cus > 0 ? num_cus : 256) * 8;
    return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

}  // namespace ldpc_bitio
