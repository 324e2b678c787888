// css_trial_kernels.hpp -- the steps around the two decodes of a CSS-code Monte-Carlo run, gfx950: sample Pauli errors
// (+ both syndromes), syndromes of given errors, the joint score.  The rules are stated in include/ldpc_mi355x.h.
//
// The shape is that of trial_kernels.hpp, with two bit images per column (the X parts and the Z parts of the qubits'
// errors, or of d = guess ^ error) and four CSRs to walk:
//   phase A  the column's bytes are produced (sample: ONE mix per qubit feeds ex and ez) or read (syndromes, score) in
//            16-byte pieces laid on the ADDRESS of the column in `ex`: piece c covers the qubits [16 c - shift,
//            16 c - shift + 16), shift = that address & 15.  The first and the last piece may hold fewer than 16
//            qubits and go byte by byte.  In every piece between them `ex` is one aligned vector access; each other
//            array (ez; in score gx, gz) is a vector access too where its column agrees with ex's in address mod 16,
//            and 16 single-byte accesses where it does not: correct, and 16 instructions for one.
//            IMAGE: piece c becomes the 16-bit word c of BOTH images in LDS (qubit j is bit j + shift of either).
//   barrier
//   phase B  lanes walk the checks of Hz over the X image and those of Hx over the Z image (IMAGE), or over the bytes in
//            global memory (the unlimited tier).  sample / syndromes: a lane takes `cpl` neighbouring checks and stores
//            them as one word where that is 4 aligned bytes (cpl is chosen per matrix).  score: the same walks plus
//            Lz over the X image and Lx over the Z image; the four flag bits of a column meet in an LDS word, the
//            workgroup keeps five running counts in LDS and adds them to the caller's when it is done: one 64-bit
//            atomicAdd per workgroup and counter, from a vector lane.
//   barrier  (the images and the flag word are reused by the next column)
// Geometry as in trial_kernels.hpp: WPC waves per column (1: four columns per 256-thread workgroup; 4: one), persistent
// grid, every wave reaches every barrier.
#pragma once
#include "trial_kernels.hpp"   // mix, fold8, spread8, fold16, image_words, kThreads, kGolden, the MODE constants

namespace ldpc_css_k {

using ldpc_trials_k::tu64;
using ldpc_trials_k::kThreads;
using ldpc_trials_k::kGolden;
using ldpc_trials_k::kSample;
using ldpc_trials_k::kSyndromes;
using ldpc_trials_k::kScore;
using ldpc_trials_k::mix;
using ldpc_trials_k::fold16;
using ldpc_trials_k::spread8;
using ldpc_trials_k::image_words;

struct CssParams {
    int n, rows_x, rows_z, nlx, nlz;   // qubits; rows of Hx, Hz, Lx, Lz
    int cplx, cplz;                    // checks of Hx / of Hz a lane takes in the syndrome walks (4 or 1)
    int image_stride;                  // 16-bit words of ONE image; a column owns two neighbouring ones (X, then Z)
    long long batch;
    tu64 column0, seed;
    tu64 ta, tb, tc;                   // X: r < ta, Y: ta <= r < tb, Z: tb <= r < tc
    uint8_t *ex_out, *ez_out;          // sample
    const uint8_t *ex, *ez;            // syndromes, score
    const uint8_t *gx, *gz;            // score
    uint8_t *sx, *sz;                  // sample (both may be NULL: errors only), syndromes: sx = Hx ez, sz = Hz ex
    uint8_t *flags;                    // score (may be NULL)
    tu64 *counts;                      // score, [6]
    const int *hx_ptr, *hx_col, *hz_ptr, *hz_col;   // CSRs: checks -> qubits
    const int *lx_ptr, *lx_col, *lz_ptr, *lz_col;   // logical rows -> qubits
};

// 16 bytes at q -> their 16 low bits; `vec` says that q is 16-byte aligned
__device__ inline unsigned load16(const uint8_t *q, bool vec)
{
    if (vec) return fold16(*reinterpret_cast<const uint4 *>(q));
    unsigned h = 0;
    for (int b = 0; b < 16; ++b) h |= (unsigned)(q[b] & 1u) << b;
    return h;
}

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

template <int WPC, int MODE, bool IMAGE>
__global__ __launch_bounds__(kThreads) void css_trial_kernel(CssParams p)
{
    constexpr int GT = 64 * WPC, CPB = kThreads / GT;   // lanes per column, columns per workgroup
    extern __shared__ unsigned short css_images[];
    __shared__ unsigned int colflags[4], running[5];
    const int slot = threadIdx.x / GT, gl = threadIdx.x % GT;
    unsigned short *imgx = css_images + (size_t)slot * 2 * p.image_stride, *imgz = imgx + p.image_stride;
    const int n = p.n;
    if (MODE == kScore) {
        if (threadIdx.x < 4) colflags[threadIdx.x] = 0;
        if (threadIdx.x < 5) running[threadIdx.x] = 0;
        __syncthreads();
    }
    const bool walk = MODE == kScore || p.sx != nullptr || p.sz != nullptr;   // (the same for every thread of the grid)
    const long long ngroups = (p.batch + CPB - 1) / CPB;
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long col = g * CPB + slot;
        const bool live = col < p.batch;
        const long long base = (live ? col : 0) * (long long)n;
        // the column in the four arrays (only bytes of the column are touched); the pieces are laid on xcol
        const uint8_t *xcol = (MODE == kSample ? (const uint8_t *)p.ex_out : p.ex) + base;
        const uint8_t *zcol = (MODE == kSample ? (const uint8_t *)p.ez_out : p.ez) + base;
        const uint8_t *gxcol = MODE == kScore ? p.gx + base : nullptr;
        const uint8_t *gzcol = MODE == kScore ? p.gz + base : nullptr;
        const int shift = (int)((uintptr_t)xcol & 15);
        unsigned nonzero = 0;
        if (live && (IMAGE || MODE != kSyndromes)) {
            const int npieces = (shift + n + 15) >> 4;
            const tu64 k = MODE == kSample ? mix(p.seed + kGolden * (p.column0 + (tu64)col + 1)) : 0;
            const bool z_vec = (((uintptr_t)zcol - (uintptr_t)xcol) & 15) == 0;
            const bool gx_vec = MODE == kScore && (((uintptr_t)gxcol - (uintptr_t)xcol) & 15) == 0;
            const bool gz_vec = MODE == kScore && (((uintptr_t)gzcol - (uintptr_t)xcol) & 15) == 0;
            for (int c = gl; c < npieces; c += GT) {
                const int j = 16 * c - shift;
                unsigned hx = 0, hz = 0;
                if (j >= 0 && j + 16 <= n) {
                    if (MODE == kSample) {
#pragma unroll
                        for (int b = 0; b < 16; ++b) {
                            const tu64 r = mix(k + (tu64)(j + b));
                            hx |= (unsigned)(r < p.tb) << b;
                            hz |= (unsigned)(r >= p.ta && r < p.tc) << b;
                        }
                        store16(p.ex_out + base + j, hx, true);
                        store16(p.ez_out + base + j, hz, z_vec);
                    } else {
                        hx = load16(xcol + j, true);
                        hz = load16(zcol + j, z_vec);
                        if (MODE == kScore) {
                            hx ^= load16(gxcol + j, gx_vec);
                            hz ^= load16(gzcol + j, gz_vec);
                        }
                    }
                } else {
                    for (int b = 0; b < 16; ++b) {
                        const int jb = j + b;
                        if (jb < 0 || jb >= n) continue;
                        unsigned bx, bz;
                        if (MODE == kSample) {
                            const tu64 r = mix(k + (tu64)jb);
                            bx = (unsigned)(r < p.tb);
                            bz = (unsigned)(r >= p.ta && r < p.tc);
                            p.ex_out[base + jb] = (uint8_t)bx;
                            p.ez_out[base + jb] = (uint8_t)bz;
                        } else if (MODE == kScore) {
                            bx = (unsigned)((xcol[jb] ^ gxcol[jb]) & 1u);
                            bz = (unsigned)((zcol[jb] ^ gzcol[jb]) & 1u);
                        } else {
                            bx = (unsigned)(xcol[jb] & 1u);
                            bz = (unsigned)(zcol[jb] & 1u);
                        }
                        hx |= bx << b;
                        hz |= bz << b;
                    }
                }
                if (IMAGE) {
                    imgx[c] = (unsigned short)hx;
                    imgz[c] = (unsigned short)hz;
                }
                nonzero |= hx | hz;
            }
        }
        if (!walk) continue;
        __syncthreads();
        auto bit_x = [&](int j) -> unsigned {
            if (IMAGE) {
                const int q = j + shift;
                return ((unsigned)imgx[q >> 4] >> (q & 15)) & 1u;
            }
            if (MODE == kScore) return (unsigned)((xcol[j] ^ gxcol[j]) & 1u);
            return (unsigned)(xcol[j] & 1u);
        };
        auto bit_z = [&](int j) -> unsigned {
            if (IMAGE) {
                const int q = j + shift;
                return ((unsigned)imgz[q >> 4] >> (q & 15)) & 1u;
            }
            if (MODE == kScore) return (unsigned)((zcol[j] ^ gzcol[j]) & 1u);
            return (unsigned)(zcol[j] & 1u);
        };
        auto parity_of = [&](auto &bit, const int *row_ptr, const int *csr_col, int r) -> unsigned {
            unsigned par = 0;
            for (int e = row_ptr[r], e1 = row_ptr[r + 1]; e < e1; ++e) par ^= bit(csr_col[e]);
            return par;
        };
        if (MODE != kScore) {
            // the s checks of one matrix over one image -> the column's s bytes at scol, cpl checks per lane and word
            auto syndromes_of = [&](auto &bit, const int *row_ptr, const int *csr_col, uint8_t *scol, int s, int cpl) {
                const int sshift = (int)((uintptr_t)scol & (uintptr_t)(cpl - 1));
                const int nwords = (sshift + s + cpl - 1) / cpl;
                for (int c = gl; c < nwords; c += GT) {
                    const int r0 = c * cpl - sshift;
                    unsigned w = 0;
                    for (int b = 0; b < cpl; ++b)
                        if (r0 + b >= 0 && r0 + b < s) w |= parity_of(bit, row_ptr, csr_col, r0 + b) << (8 * b);
                    if (cpl == 4 && r0 >= 0 && r0 + 4 <= s) {
                        *reinterpret_cast<unsigned *>(scol + r0) = w;
                    } else {
                        for (int b = 0; b < cpl; ++b)
                            if (r0 + b >= 0 && r0 + b < s) scol[r0 + b] = (uint8_t)((w >> (8 * b)) & 0xffu);
                    }
                }
            };
            if (live) {
                if (p.sz) syndromes_of(bit_x, p.hz_ptr, p.hz_col, p.sz + col * (long long)p.rows_z, p.rows_z, p.cplz);
                if (p.sx) syndromes_of(bit_z, p.hx_ptr, p.hx_col, p.sx + col * (long long)p.rows_x, p.rows_x, p.cplx);
            }
        } else {
            unsigned bad = 0, badx = 0, badz = 0;
            if (live) {
                for (int r = gl; r < p.rows_z; r += GT) bad |= parity_of(bit_x, p.hz_ptr, p.hz_col, r);
                for (int r = gl; r < p.rows_x; r += GT) bad |= parity_of(bit_z, p.hx_ptr, p.hx_col, r);
                for (int r = gl; r < p.nlz; r += GT) badx |= parity_of(bit_x, p.lz_ptr, p.lz_col, r);
                for (int r = gl; r < p.nlx; r += GT) badz |= parity_of(bit_z, p.lx_ptr, p.lx_col, r);
            }
            const unsigned f = (__any((int)nonzero) ? 1u : 0u) | (__any((int)bad) ? 2u : 0u) | (__any((int)badx) ? 4u : 0u) |
                               (__any((int)badz) ? 8u : 0u);
            if ((threadIdx.x & 63) == 0 && f) atomicOr(&colflags[slot], f);
            __syncthreads();
            if (gl == 0 && live) {
                const unsigned cf = colflags[slot];
                colflags[slot] = 0;               // (the next column's waves meet here after the next barrier)
                if (p.flags) p.flags[col] = (uint8_t)cf;
                if (cf & 1u) atomicAdd(&running[0], 1u);
                if (cf & 2u) atomicAdd(&running[1], 1u);
                if (cf & 12u) atomicAdd(&running[2], 1u);
                if (cf & 4u) atomicAdd(&running[3], 1u);
                if (cf & 8u) atomicAdd(&running[4], 1u);
            }
        }
        __syncthreads();
    }
    if (MODE == kScore) {
        __syncthreads();
        // running[] is 32-bit: a call takes at most 2^36 columns and its grid has 32 workgroups or more once there are 32
        // column groups (ldpc_css_trials.hip), so a workgroup sees at most 2^31 + 4 columns
        if (threadIdx.x < 5 && running[threadIdx.x]) atomicAdd(&p.counts[1 + threadIdx.x], (tu64)running[threadIdx.x]);
        if (threadIdx.x == 5 && blockIdx.x == 0) atomicAdd(&p.counts[0], (tu64)p.batch);
    }
}

}  // namespace ldpc_css_k
