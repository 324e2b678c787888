// window_kernels.hpp -- the step between two windows of a sliding-window decode, gfx950 (ldpc_windows_* of
// include/ldpc_mi355x.h, where the rule is stated): commit the first mechanisms of window k's guess, push their effect
// into the residual syndrome, hand window k + 1 its syndromes.  Memory-bound glue around the decoders: per column it
// reads the window's guess, writes |commit_k| guess bytes, reads and writes |U_k| residual bytes.
//
// The tables (window_plan.hpp) make every output byte the business of ONE thread: committed position t of the window
// owns guess byte c_mech[t]; entry u of U_k owns residual byte u_det[u] and, where that detector is in det_{k+1}, byte
// u_next[u] of the next window's syndromes -- the thread reads the residual byte, XORs the committed bits of the
// detector's row, stores it and stores the same value as the next window's syndrome.  So there is no atomic, and no
// thread reads a byte that another thread of the launch writes (the caller's arrays must not overlap).  A detector that
// is in U_k through det_{k+1} alone has an empty range: it is read and copied, the residual byte is left as it is.
// The gather is the same kernel with nothing committed: U = det_k, every range empty (u_ptr = NULL), entry u copies to
// place u (u_next = NULL).
//
// Geometry and the staging of the guess are those of trial_kernels.hpp: WPC waves work on a column (1: four columns per
// 256-thread workgroup, one wave each; 4: the workgroup takes one column), the grid is persistent, so every wave
// reaches every barrier.  IMAGE: the column of the window's guess is read once, 16 contiguous bytes per lane laid on its
// ADDRESS (first and last piece byte by byte), and folded into a bit image in LDS, 16 bits per piece; the walks over the
// rows of U_k and the committed positions read bits out of the image.  !IMAGE (a guess column beyond the LDS budget):
// the walks read the guess bytes themselves out of global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trial_kernels.hpp"   // load16, image_words: the piece loads of the trial steps

namespace ldpc_windows_k {

constexpr int kThreads = 256;

struct WindowParams {
    long long batch;
    const uint8_t *win_guess;    // [batch][nmech], NULL when nothing is committed
    int nmech, image_stride;     // 16-bit words of one column's image
    int nc;                      // committed positions
    const int *c_pos, *c_mech;   // [nc]
    uint8_t *guess;              // [batch][N]
    int N, D;
    uint8_t *residual;           // [batch][D]; the gather only reads it
    int nu;
    const int *u_det, *u_ptr, *u_pos, *u_next;   // u_ptr NULL: every range empty; u_next NULL: entry u copies to place u
    uint8_t *next;               // [batch][nnext], may be NULL
    int nnext;
    int first;                   // window 0: the flag starts at 1
    const uint8_t *win_conv;     // [batch]; conv and win_conv are both given or both NULL
    uint8_t *conv;
};

template <int WPC, bool IMAGE>
__global__ __launch_bounds__(kThreads) void window_kernel(WindowParams p)
{
    constexpr int GT = 64 * WPC, CPB = kThreads / GT;   // lanes per column, columns per workgroup
    extern __shared__ unsigned short window_images[];
    const int slot = threadIdx.x / GT, gl = threadIdx.x % GT;
    unsigned short *img = window_images + (size_t)slot * p.image_stride;
    const bool commits = p.nc > 0;                      // (the same for every thread of the grid)
    const long long ngroups = (p.batch + CPB - 1) / CPB;
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long col = g * CPB + slot;
        const bool live = col < p.batch;
        const uint8_t *wg = commits ? p.win_guess + (live ? col : 0) * (long long)p.nmech : nullptr;
        const int shift = (int)((uintptr_t)wg & 15);
        if (IMAGE && commits) {
            if (live) {
                const int npieces = (shift + p.nmech + 15) >> 4;
                for (int c = gl; c < npieces; c += GT) {
                    const int j = 16 * c - shift;
                    unsigned h = 0;
                    if (j >= 0 && j + 16 <= p.nmech) {
                        h = ldpc_trials_k::load16(wg + j, true);
                    } else {
                        for (int b = 0; b < 16; ++b)
                            if (j + b >= 0 && j + b < p.nmech) h |= (unsigned)(wg[j + b] & 1u) << b;
                    }
                    img[c] = (unsigned short)h;
                }
            }
            __syncthreads();
        }
        auto bit_of = [&](int c) -> unsigned {          // position c of the window's guess
            if constexpr (IMAGE) {
                const int q = c + shift;
                return ((unsigned)img[q >> 4] >> (q & 15)) & 1u;
            } else {
                return (unsigned)(wg[c] & 1u);
            }
        };
        if (live) {
            uint8_t *gcol = p.guess + col * (long long)p.N;
            for (int t = gl; t < p.nc; t += GT) gcol[p.c_mech[t]] = (uint8_t)bit_of(p.c_pos[t]);
            uint8_t *rcol = p.residual + col * (long long)p.D;
            uint8_t *ncol = p.next ? p.next + col * (long long)p.nnext : nullptr;
            for (int u = gl; u < p.nu; u += GT) {
                const int e0 = p.u_ptr ? p.u_ptr[u] : 0, e1 = p.u_ptr ? p.u_ptr[u + 1] : 0;
                const int place = !ncol ? -1 : p.u_next ? p.u_next[u] : u;
                if (e0 == e1 && place < 0) continue;    // owned through det_{k+1} alone, and no next window is asked for
                const int d = p.u_det[u];
                unsigned r = (unsigned)(rcol[d] & 1u);
                if (e0 < e1) {
                    for (int e = e0; e < e1; ++e) r ^= bit_of(p.u_pos[e]);
                    rcol[d] = (uint8_t)r;
                }
                if (place >= 0) ncol[place] = (uint8_t)r;
            }
            if (gl == 0 && p.conv) p.conv[col] = (uint8_t)((p.first ? 1u : (unsigned)(p.conv[col] != 0)) & (unsigned)(p.win_conv[col] != 0));
        }
        if (IMAGE && commits) __syncthreads();          // (the image is reused by the next column)
    }
}

}  // namespace ldpc_windows_k
