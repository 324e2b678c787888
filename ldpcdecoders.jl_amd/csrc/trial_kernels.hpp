// trial_kernels.hpp -- the steps around a decode in a Monte-Carlo run, gfx950: sample errors (+ their syndromes),
// syndromes of given errors, score guesses against errors; for one check matrix (ldpc_trials_*) and for a CSS pair
// (ldpc_css_trials_*).  The rules are stated in include/ldpc_mi355x.h.
//
// A SIDE is a column of errors with the matrices that see it: its arrays (errors, guesses, syndromes), the CSR of its
// checks and of its logical rows, and the window [lo, hi) of the draw in which a bit of it is set.  The one-matrix trial
// is one side (errors / guesses / syndromes, H, L, window [0, threshold)); a CSS trial is two sides that share one draw
// per qubit and one flag word: side 0 = (ex, gx, sz) seen by Hz and Lz, window [0, tb); side 1 = (ez, gz, sx) seen by Hx
// and Lx, window [ta, tc).  Side 0's window starts at 0 in both uses and costs no compare.
//
// One kernel template serves the side counts (SIDES), the steps (MODE: sample, syndromes, score, and for one side the
// sample with a rate per bit) and the two tiers (IMAGE):
//   phase A  the column's bytes are produced (sample: ONE mix per bit position feeds every side) or read (syndromes,
//            score), 16 contiguous bytes per lane and step, folded to 16 bits with the multiply of bit_io_kernels.hpp.
//            The 16-byte pieces are laid on the ADDRESS of side 0's column, not on the column: a column starts at byte
//            i * n of the array, which is aligned only by chance, so piece c covers the bytes [16 c - shift,
//            16 c - shift + 16) of the column, shift = the column's address & 15.  The first and the last piece may hold
//            fewer than 16 bytes of the column and go byte by byte.  In every piece between them side 0's column is one
//            aligned vector access; each other array (side 0's guesses, everything of side 1) is a vector access too
//            where its column agrees with side 0's in address mod 16, and 16 single-byte accesses where it does not:
//            correct, and 16 instructions for one.
//            The per-bit sample (kSampleRates) compares the draw of bit j with entry j of a table of 64-bit thresholds
//            instead of side 0's `hi`: the 16 entries of a piece are 128 contiguous bytes at 8 j, read as eight 16-byte
//            loads where j is even and entry by entry where it is odd (8-byte aligned only: the compiler pairs the
//            inner fourteen into 16-byte loads all the same); the first and the last piece go entry by entry as they
//            go byte by byte.  Still one mix per bit.
//            IMAGE: piece c becomes the 16-bit word c of each side's bit image in LDS (bit j of a column is bit
//            j + shift of its image; a column owns SIDES neighbouring images): plain 2-byte LDS stores, no two lanes
//            write one word, nothing to clear.
//   barrier
//   phase B  lanes walk each side's checks through the CSR and XOR the bits of their entries: out of the side's image
//            (IMAGE), or the bytes themselves out of global memory (the unlimited tier; the workgroup wrote or read them
//            in phase A).
//            sample / syndromes: a lane takes `cpl` neighbouring checks (4 when the side has enough checks to keep every
//            lane busy, else 1) and stores them as one 4-byte word, laid on the address like the pieces of phase A.
//            score: a lane ORs the parities of its checks (all sides together) and of each side's logical rows; the flag
//            bits of a column (0: any side differs, 1: any side's checks violated, 2 + k: side k's logical rows
//            violated) meet in an LDS word, the workgroup keeps running counts in LDS and adds them to the caller's
//            counters when it is done: one 64-bit atomicAdd per workgroup and counter, from a vector lane.
//   barrier  (the images and the flag word are reused by the next column)
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
enum { kSample = 0, kSyndromes = 1, kScore = 2, kSampleRates = 3 };   // kSampleRates: sample, bit j at its own rate (one side only)

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

struct TrialSide {
    uint8_t *err_out;            // sample
    const uint8_t *err;          // syndromes, score
    const uint8_t *guess;        // score
    uint8_t *syn;                // sample (may be NULL), syndromes: what this side's checks say
    int rows, nl, cpl;           // checks, logical rows; checks a lane takes in the syndrome walk (4 or 1)
    const int *row_ptr, *csr_col;      // the checks that see this side -> bits
    const int *lrow_ptr, *lcsr_col;    // the logical rows that see this side -> bits
    tu64 lo, hi;                 // sample: the bit is set where lo <= r < hi (side 0: lo is 0 and is not read)
};

template <int SIDES>
struct TrialParams {
    int n;
    int image_stride;            // 16-bit words of ONE image; a column owns SIDES neighbouring ones
    int all_ones;                // per >= 1 (one matrix only)
    long long batch;
    tu64 column0, seed;
    uint8_t *flags;              // score (may be NULL)
    tu64 *counts;                // score: [trials, b0, b1, b2] or [trials, b0, b1, b2|b3, b2, b3]
    TrialSide side[SIDES];
    const tu64 *rates;           // kSampleRates: the threshold of every bit, [n]; all ones = always set (no rate below 1 gives it)
};

__device__ inline unsigned fold16(uint4 x)
{
    return fold8((tu64)x.x | ((tu64)x.y << 32)) | (fold8((tu64)x.z | ((tu64)x.w << 32)) << 8);
}

// 16 bytes at q -> their 16 low bits; `vec` says that q is 16-byte aligned
__device__ inline unsigned load16(const uint8_t *q, bool vec)
{
    if (vec) return fold16(*reinterpret_cast<const uint4 *>(q));
    unsigned h = 0;
    for (int b = 0; b < 16; ++b) h |= (unsigned)(q[b] & 1u) << b;
    return h;
}

// the low bits of 16 bytes at e ^ those at g; two aligned pieces are XORed as vectors and folded once
__device__ inline unsigned diff16(const uint8_t *e, bool evec, const uint8_t *g, bool gvec)
{
    if (!(evec && gvec)) return load16(e, evec) ^ load16(g, gvec);
    uint4 x = *reinterpret_cast<const uint4 *>(e);
    const uint4 y = *reinterpret_cast<const uint4 *>(g);
    x.x ^= y.x; x.y ^= y.y; x.z ^= y.z; x.w ^= y.w;
    return fold16(x);
}

// the thresholds of the 16 bits from bit j on: 128 contiguous bytes at 8 j; `vec` says that they are 16-byte aligned (j even)
__device__ inline void load_thresholds(const tu64 *q, bool vec, tu64 th[16])
{
    if (vec) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(q)[b];
            th[2 * b] = v.x; th[2 * b + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int b = 0; b < 16; ++b) th[b] = q[b];
    }
}

// is a bit of draw r set under threshold t of the rates table
__device__ inline unsigned under(tu64 r, tu64 t) { return (unsigned)(r < t) | (unsigned)(t == ~0ull); }

// 16 bits -> 16 bytes (0 / 1) at q
__device__ inline void store16(uint8_t *q, unsigned h, bool vec)
{
    const tu64 lo = spread8(h), hi = spread8(h >> 8);
    if (vec) {
        uint4 o;
        o.x = (unsigned)lo; o.y = (unsigned)(lo >> 32); o.z = (unsigned)hi; o.w = (unsigned)(hi >> 32);
        *reinterpret_cast<uint4 *>(q) = o;
    } else {
        for (int b = 0; b < 8; ++b) {
            q[b] = (uint8_t)((lo >> (8 * b)) & 0xffu);
            q[8 + b] = (uint8_t)((hi >> (8 * b)) & 0xffu);
        }
    }
}

// Every loop over the sides below is unrolled, so `k` is a constant wherever it indexes p.side[] or a per-side local.
// The two-sided score at one wave per column on the image tier asks for 8 waves/SIMD: left alone the scheduler spreads
// the byte path of a misaligned load16 over 69 VGPRs (7 waves, and a smaller persistent grid); asked, it takes 59 and
// keeps 12 SGPRs in the lanes of one VGPR outside the inner loops.  Every other instantiation gets the default (1).
template <int SIDES, int WPC, int MODE, bool IMAGE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(SIDES == 2 && WPC == 1 && MODE == kScore && IMAGE ? 8 : 1)))
void trial_kernel(TrialParams<SIDES> p)
{
    constexpr int GT = 64 * WPC, CPB = kThreads / GT;   // lanes per column, columns per workgroup
    constexpr int NRUN = SIDES == 1 ? 3 : 3 + SIDES;    // running counts: b0, b1, any logical; then each side's logical
    constexpr bool RATES = MODE == kSampleRates, SAMPLE = MODE == kSample || RATES;
    static_assert(!RATES || SIDES == 1, "per-bit rates: one side only");
    extern __shared__ unsigned short image_all[];
    __shared__ unsigned int colflags[4], running[NRUN];
    const int slot = threadIdx.x / GT, gl = threadIdx.x % GT;
    unsigned short *img[SIDES];                         // a column owns SIDES neighbouring images
#pragma unroll
    for (int k = 0; k < SIDES; ++k) img[k] = image_all + ((size_t)slot * SIDES + k) * p.image_stride;
    const int n = p.n;
    if (MODE == kScore) {
        if (threadIdx.x < 4) colflags[threadIdx.x] = 0;
        if (threadIdx.x < NRUN) running[threadIdx.x] = 0;
        __syncthreads();
    }
    bool walk = MODE == kScore;                         // (the same for every thread of the grid)
#pragma unroll
    for (int k = 0; k < SIDES; ++k) walk |= p.side[k].syn != nullptr;
    const long long ngroups = (p.batch + CPB - 1) / CPB;
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long col = g * CPB + slot;
        const bool live = col < p.batch;
        const long long base = (live ? col : 0) * (long long)n;
        // the column in every array (only bytes of the column are touched); the pieces are laid on ecol[0]
        const uint8_t *ecol[SIDES], *gcol[SIDES];
#pragma unroll
        for (int k = 0; k < SIDES; ++k) {
            ecol[k] = (SAMPLE ? (const uint8_t *)p.side[k].err_out : p.side[k].err) + base;
            gcol[k] = MODE == kScore ? p.side[k].guess + base : nullptr;
        }
        const int shift = (int)((uintptr_t)ecol[0] & 15);
        unsigned nonzero = 0;
        if (live && (IMAGE || MODE != kSyndromes)) {
            bool evec[SIDES], gvec[SIDES];              // an array's column agrees with ecol[0] in address mod 16
#pragma unroll
            for (int k = 0; k < SIDES; ++k) evec[k] = k == 0 || (((uintptr_t)ecol[k] - (uintptr_t)ecol[0]) & 15) == 0;
#pragma unroll
            for (int k = 0; k < SIDES; ++k) gvec[k] = MODE == kScore && (((uintptr_t)gcol[k] - (uintptr_t)ecol[0]) & 15) == 0;
            const int npieces = (shift + n + 15) >> 4;
            const tu64 key = SAMPLE ? mix(p.seed + kGolden * (p.column0 + (tu64)col + 1)) : 0;
            for (int c = gl; c < npieces; c += GT) {
                const int j = 16 * c - shift;
                unsigned h[SIDES] = {};
                if (j >= 0 && j + 16 <= n) {
                    if constexpr (RATES) {
                        tu64 th[16];
                        load_thresholds(p.rates + j, (j & 1) == 0, th);
#pragma unroll
                        for (int b = 0; b < 16; ++b) h[0] |= under(mix(key + (tu64)(j + b)), th[b]) << b;
                        store16(p.side[0].err_out + base + j, h[0], true);
                    } else if (MODE == kSample) {
#pragma unroll
                        for (int b = 0; b < 16; ++b) {
                            const tu64 r = mix(key + (tu64)(j + b));
#pragma unroll
                            for (int k = 0; k < SIDES; ++k)
                                h[k] |= (unsigned)((k == 0 || r >= p.side[k].lo) && r < p.side[k].hi) << b;
                        }
                        if (SIDES == 1 && p.all_ones) h[0] = 0xffffu;
#pragma unroll
                        for (int k = 0; k < SIDES; ++k) store16(p.side[k].err_out + base + j, h[k], evec[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < SIDES; ++k)
                            h[k] = MODE == kScore ? diff16(ecol[k] + j, evec[k], gcol[k] + j, gvec[k]) : load16(ecol[k] + j, evec[k]);
                    }
                } else {
                    for (int b = 0; b < 16; ++b) {
                        const int jb = j + b;
                        if (jb < 0 || jb >= n) continue;
                        const tu64 r = SAMPLE ? mix(key + (tu64)jb) : 0;
#pragma unroll
                        for (int k = 0; k < SIDES; ++k) {
                            unsigned bit;
                            if constexpr (RATES) {
                                bit = under(r, p.rates[jb]);
                                p.side[0].err_out[base + jb] = (uint8_t)bit;
                            } else if (MODE == kSample) {
                                bit = (unsigned)((k == 0 || r >= p.side[k].lo) && r < p.side[k].hi);
                                if (SIDES == 1 && p.all_ones) bit = 1u;
                                p.side[k].err_out[base + jb] = (uint8_t)bit;
                            } else if (MODE == kScore) {
                                bit = (unsigned)((ecol[k][jb] ^ gcol[k][jb]) & 1u);
                            } else {
                                bit = (unsigned)(ecol[k][jb] & 1u);
                            }
                            h[k] |= bit << b;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < SIDES; ++k) {
                    if (IMAGE) img[k][c] = (unsigned short)h[k];
                    nonzero |= h[k];
                }
            }
        }
        if (!walk) continue;
        __syncthreads();
        // bit j of side k, and row r of a CSR over side k's bits (k is a constant at every call)
        auto bit_of = [&](int k, int j) -> unsigned {
            if (IMAGE) {
                const int q = j + shift;
                return ((unsigned)img[k][q >> 4] >> (q & 15)) & 1u;
            }
            if (MODE == kScore) return (unsigned)((ecol[k][j] ^ gcol[k][j]) & 1u);
            return (unsigned)(ecol[k][j] & 1u);
        };
        auto parity_of = [&](int k, const int *row_ptr, const int *csr_col, int r) -> unsigned {
            unsigned par = 0;
            for (int e = row_ptr[r], e1 = row_ptr[r + 1]; e < e1; ++e) par ^= bit_of(k, csr_col[e]);
            return par;
        };
        if (MODE != kScore) {
#pragma unroll
            for (int k = 0; k < SIDES; ++k) {
                const TrialSide &sd = p.side[k];
                if (!live || (SIDES > 1 && !sd.syn)) continue;   // (one side: walk says that syn is there)
                const int s = sd.rows, cpl = sd.cpl;
                uint8_t *scol = sd.syn + col * (long long)s;
                const int sshift = (int)((uintptr_t)scol & (uintptr_t)(cpl - 1));
                const int nwords = (sshift + s + cpl - 1) / cpl;
                for (int c = gl; c < nwords; c += GT) {
                    const int r0 = c * cpl - sshift;
                    unsigned w = 0;
                    for (int b = 0; b < cpl; ++b)
                        if (r0 + b >= 0 && r0 + b < s) w |= parity_of(k, sd.row_ptr, sd.csr_col, r0 + b) << (8 * b);
                    if (cpl == 4 && r0 >= 0 && r0 + 4 <= s) {
                        *reinterpret_cast<unsigned *>(scol + r0) = w;
                    } else {
                        for (int b = 0; b < cpl; ++b)
                            if (r0 + b >= 0 && r0 + b < s) scol[r0 + b] = (uint8_t)((w >> (8 * b)) & 0xffu);
                    }
                }
            }
        } else {
            unsigned bad = 0, badl[SIDES] = {};
            if (live) {
#pragma unroll
                for (int k = 0; k < SIDES; ++k)
                    for (int r = gl; r < p.side[k].rows; r += GT) bad |= parity_of(k, p.side[k].row_ptr, p.side[k].csr_col, r);
#pragma unroll
                for (int k = 0; k < SIDES; ++k)
                    for (int r = gl; r < p.side[k].nl; r += GT) badl[k] |= parity_of(k, p.side[k].lrow_ptr, p.side[k].lcsr_col, r);
            }
            unsigned f = (__any((int)nonzero) ? 1u : 0u) | (__any((int)bad) ? 2u : 0u);
#pragma unroll
            for (int k = 0; k < SIDES; ++k) f |= __any((int)badl[k]) ? 4u << k : 0u;
            if ((threadIdx.x & 63) == 0 && f) atomicOr(&colflags[slot], f);
            __syncthreads();
            if (gl == 0 && live) {
                const unsigned cf = colflags[slot];
                colflags[slot] = 0;               // (the next column's waves meet here after the next barrier)
                if (p.flags) p.flags[col] = (uint8_t)cf;
                if (cf & 1u) atomicAdd(&running[0], 1u);
                if (cf & 2u) atomicAdd(&running[1], 1u);
                if (cf & (((1u << SIDES) - 1u) << 2)) atomicAdd(&running[2], 1u);
#pragma unroll
                for (int k = 0; k < NRUN - 3; ++k)
                    if (cf & (4u << k)) atomicAdd(&running[3 + k], 1u);
            }
        }
        __syncthreads();
    }
    if (MODE == kScore) {
        __syncthreads();
        // running[] is 32-bit: a call takes at most 2^36 columns and its grid has 32 workgroups or more once there are 32
        // column groups (ldpc_trials.hip), so a workgroup sees at most 2^31 + 4 columns
        if (threadIdx.x < NRUN && running[threadIdx.x]) atomicAdd(&p.counts[1 + threadIdx.x], (tu64)running[threadIdx.x]);
        if (threadIdx.x == NRUN && blockIdx.x == 0) atomicAdd(&p.counts[0], (tu64)p.batch);
    }
}

}  // namespace ldpc_trials_k
