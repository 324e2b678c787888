// trial_kernels.hpp -- the steps around a decode in a Monte-Carlo run, gfx950: sample errors (+ their syndromes),
// syndromes of given errors, score guesses against errors.  The rules are stated in include/ldpc_mi355x.h.
//
// One kernel template serves the three steps (MODE) and the two tiers (IMAGE):
//   phase A  the column's bytes are produced (sample) or read (syndromes, score), 16 contiguous bytes per lane and step:
//            one 16-byte vector access, folded to 16 bits with the multiply of bit_io_kernels.hpp.  The 16-byte pieces
//            are laid on the ADDRESS, not on the column: a column starts at byte i * n of the array, which is aligned
//            only by chance, so piece c covers the bytes [16 c - shift, 16 c - shift + 16) of the column, shift = the
//            column's address & 15.  The first and the last piece may hold fewer than 16 bytes of the column and go
//            byte by byte; every piece between them is an aligned vector access.  (score lays the pieces on `errors`;
//            where `guesses` differs from it in address mod 16 the guess of every piece is read as 16 single bytes:
//            correct, and 16 load instructions for one.  Arrays whose starts agree mod 16 never meet it.)
//            IMAGE: piece c becomes the 16-bit word c of the column's bit image in LDS (bit j of the column is bit
//            j + shift of the image): plain 2-byte LDS stores, no two lanes write one word, nothing to clear.
//   barrier
//   phase B  lanes walk the checks through the CSR and XOR the bits of their entries: out of the image (IMAGE), or the
//            bytes themselves out of global memory (the unlimited tier; the workgroup wrote or read them in phase A).
//            sample / syndromes: a lane takes `cpl` neighbouring checks (4 when there are enough checks to keep every
//            lane busy, else 1) and stores them as one 4-byte word, laid on the address like the pieces of phase A.
//            score: a lane ORs the parities of its checks of H and of L; the three flag bits of a column meet in an LDS
//            word, the workgroup keeps running counts in LDS and adds them to the caller's counters when it is done:
//            one 64-bit atomicAdd per workgroup and counter, from a vector lane.
//   barrier  (the image and the flag word are reused by the next column)
//
// Geometry: WPC waves work on a column.  WPC = 1: four columns per 256-thread workgroup, one wave each (short columns:
// BB-72 at batch 2^20 would otherwise be 2^20 workgroups of one busy wave); WPC = 4: the workgroup takes one column.
// The grid is persistent (workgroups stride over the column groups), so every wave reaches every barrier.
// With WPC = 1 a column of n bits has (n + 30) / 16 pieces at most, so in phase A only that many of the wave's 64 lanes
// work (BB-72: 5 or 6); columns of n < 1024 leave lanes idle there.  Dealing bits, not pieces, to the lanes would fill them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc_trials_k {

typedef unsigned long long tu64;
constexpr int kThreads = 256;
constexpr tu64 kGolden = 0x9E3779B97F4A7C15ull;
enum { kSample = 0, kSyndromes = 1, kScore = 2 };

// the SplitMix64 finaliser (include/ldpc_mi355x.h)
__host__ __device__ inline tu64 mix(tu64 z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// 8 bytes (0/1 in bit 0 of each) -> 8 bits and back, the multiplies of bit_io_kernels.hpp (whose header also defines its
// kernels, so it cannot be included by a second unit)
__device__ inline unsigned fold8(tu64 x) { return (unsigned)(((x & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56); }
__device__ inline tu64 spread8(unsigned b)
{
    const tu64 one_hot = ((tu64)(b & 0xffu) * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((one_hot + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

// 16-bit words a column's image takes: pieces 0 .. (shift + n + 15) / 16 - 1 with shift <= 15
__host__ __device__ inline int image_words(long long n) { return (int)((n + 30) >> 4) + 1; }

struct TrialParams {
    int s, n, nl, cpl;
    int image_stride;            // 16-bit words between the images of two columns of a workgroup
    int all_ones;                // per >= 1
    long long batch;
    tu64 column0, seed, threshold;
    uint8_t *err_out;            // sample
    const uint8_t *err;          // syndromes, score
    const uint8_t *guess;        // score
    uint8_t *syn;                // sample (may be NULL), syndromes
    uint8_t *flags;              // score (may be NULL)
    tu64 *counts;                // score
    const int *row_ptr, *csr_col;      // H, checks -> bits
    const int *lrow_ptr, *lcsr_col;    // L, logical rows -> bits
};

__device__ inline unsigned fold16(uint4 x)
{
    return fold8((tu64)x.x | ((tu64)x.y << 32)) | (fold8((tu64)x.z | ((tu64)x.w << 32)) << 8);
}

template <int WPC, int MODE, bool IMAGE>
__global__ __launch_bounds__(kThreads) void trial_kernel(TrialParams p)
{
    constexpr int GT = 64 * WPC, CPB = kThreads / GT;   // lanes per column, columns per workgroup
    extern __shared__ unsigned short image_all[];
    __shared__ unsigned int colflags[4], running[3];
    const int slot = threadIdx.x / GT, gl = threadIdx.x % GT;
    unsigned short *img = image_all + (size_t)slot * p.image_stride;
    const int n = p.n, s = p.s;
    if (MODE == kScore) {
        if (threadIdx.x < 4) colflags[threadIdx.x] = 0;
        if (threadIdx.x < 3) running[threadIdx.x] = 0;
        __syncthreads();
    }
    const long long ngroups = (p.batch + CPB - 1) / CPB;
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long col = g * CPB + slot;
        const bool live = col < p.batch;
        // the column's bytes; `piece0` is the 16-byte boundary at or below its first byte (only bytes of the column are touched)
        const uint8_t *ecol = (MODE == kSample ? (const uint8_t *)p.err_out : p.err) + (live ? col : 0) * (long long)n;
        const uint8_t *gcol = MODE == kScore ? p.guess + (live ? col : 0) * (long long)n : nullptr;
        const int shift = (int)((uintptr_t)ecol & 15);
        const uint8_t *piece0 = ecol - shift;
        unsigned nonzero = 0;
        if (live && (IMAGE || MODE != kSyndromes)) {
            const int npieces = (shift + n + 15) >> 4;
            const tu64 k = MODE == kSample ? mix(p.seed + kGolden * (p.column0 + (tu64)col + 1)) : 0;
            const bool guess_aligned = MODE == kScore && (((uintptr_t)gcol - (uintptr_t)ecol) & 15) == 0;
            for (int c = gl; c < npieces; c += GT) {
                const int j = 16 * c - shift;
                unsigned h = 0;
                if (j >= 0 && j + 16 <= n) {
                    if (MODE == kSample) {
#pragma unroll
                        for (int b = 0; b < 16; ++b) h |= (unsigned)(mix(k + (tu64)(j + b)) < p.threshold) << b;
                        if (p.all_ones) h = 0xffffu;
                        const tu64 lo = spread8(h), hi = spread8(h >> 8);
                        uint4 o;
                        o.x = (unsigned)lo; o.y = (unsigned)(lo >> 32); o.z = (unsigned)hi; o.w = (unsigned)(hi >> 32);
                        *reinterpret_cast<uint4 *>(p.err_out + col * (long long)n + j) = o;
                    } else {
                        uint4 x = *reinterpret_cast<const uint4 *>(piece0 + 16 * (long long)c);
                        if (MODE == kScore) {
                            if (guess_aligned) {
                                const uint4 y = *reinterpret_cast<const uint4 *>(gcol + j);
                                x.x ^= y.x; x.y ^= y.y; x.z ^= y.z; x.w ^= y.w;
                                h = fold16(x);
                            } else {
                                h = fold16(x);
                                for (int b = 0; b < 16; ++b) h ^= (unsigned)(gcol[j + b] & 1u) << b;
                            }
                        } else {
                            h = fold16(x);
                        }
                    }
                } else {
                    for (int b = 0; b < 16; ++b) {
                        const int jb = j + b;
                        if (jb < 0 || jb >= n) continue;
                        unsigned bit;
                        if (MODE == kSample) {
                            bit = p.all_ones ? 1u : (unsigned)(mix(k + (tu64)jb) < p.threshold);
                            p.err_out[col * (long long)n + jb] = (uint8_t)bit;
                        } else if (MODE == kScore) {
                            bit = (unsigned)((ecol[jb] ^ gcol[jb]) & 1u);
                        } else {
                            bit = (unsigned)(ecol[jb] & 1u);
                        }
                        h |= bit << b;
                    }
                }
                if (IMAGE) img[c] = (unsigned short)h;
                nonzero |= h;
            }
        }
        const bool walk = MODE == kScore || p.syn != nullptr;
        if (!walk) continue;                      // (the same for every thread of the grid)
        __syncthreads();
        auto bit_of = [&](int j) -> unsigned {
            if (IMAGE) {
                const int q = j + shift;
                return ((unsigned)img[q >> 4] >> (q & 15)) & 1u;
            }
            if (MODE == kScore) return (unsigned)((ecol[j] ^ gcol[j]) & 1u);
            return (unsigned)(ecol[j] & 1u);
        };
        auto parity_of = [&](const int *row_ptr, const int *csr_col, int r) -> unsigned {
            unsigned par = 0;
            for (int e = row_ptr[r], e1 = row_ptr[r + 1]; e < e1; ++e) par ^= bit_of(csr_col[e]);
            return par;
        };
        if (MODE != kScore) {
            if (live) {
                uint8_t *scol = p.syn + col * (long long)s;
                const int cpl = p.cpl, sshift = (int)((uintptr_t)scol & (uintptr_t)(cpl - 1));
                const int nwords = (sshift + s + cpl - 1) / cpl;
                for (int c = gl; c < nwords; c += GT) {
                    const int r0 = c * cpl - sshift;
                    unsigned w = 0;
                    for (int b = 0; b < cpl; ++b)
                        if (r0 + b >= 0 && r0 + b < s) w |= parity_of(p.row_ptr, p.csr_col, r0 + b) << (8 * b);
                    if (cpl == 4 && r0 >= 0 && r0 + 4 <= s) {
                        *reinterpret_cast<unsigned *>(scol + r0) = w;
                    } else {
                        for (int b = 0; b < cpl; ++b)
                            if (r0 + b >= 0 && r0 + b < s) scol[r0 + b] = (uint8_t)((w >> (8 * b)) & 0xffu);
                    }
                }
            }
        } else {
            unsigned bad = 0, badl = 0;
            if (live) {
                for (int r = gl; r < s; r += GT) bad |= parity_of(p.row_ptr, p.csr_col, r);
                for (int r = gl; r < p.nl; r += GT) badl |= parity_of(p.lrow_ptr, p.lcsr_col, r);
            }
            const unsigned f = (__any((int)nonzero) ? 1u : 0u) | (__any((int)bad) ? 2u : 0u) | (__any((int)badl) ? 4u : 0u);
            if ((threadIdx.x & 63) == 0 && f) atomicOr(&colflags[slot], f);
            __syncthreads();
            if (gl == 0 && live) {
                const unsigned cf = colflags[slot];
                colflags[slot] = 0;               // (the next column's waves meet here after the next barrier)
                if (p.flags) p.flags[col] = (uint8_t)cf;
                if (cf & 1u) atomicAdd(&running[0], 1u);
                if (cf & 2u) atomicAdd(&running[1], 1u);
                if (cf & 4u) atomicAdd(&running[2], 1u);
            }
        }
        __syncthreads();
    }
    if (MODE == kScore) {
        __syncthreads();
        // running[] is 32-bit: a call takes at most 2^36 columns and its grid has 32 workgroups or more once there are 32
        // column groups (ldpc_trials.hip), so a workgroup sees at most 2^31 + 4 columns
        if (threadIdx.x < 3 && running[threadIdx.x]) atomicAdd(&p.counts[1 + threadIdx.x], (tu64)running[threadIdx.x]);
        if (threadIdx.x == 3 && blockIdx.x == 0) atomicAdd(&p.counts[0], (tu64)p.batch);
    }
}

}  // namespace ldpc_trials_k
