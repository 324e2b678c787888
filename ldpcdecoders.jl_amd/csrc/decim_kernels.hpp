// decim_kernels.hpp -- device code of the guided-decimation min-sum decoder (ldpc_decim_* of include/ldpc_mi355x.h, where
// the rule is stated; host side: ldpc_decim.hip).  Binary32 throughout, one rounding per operation, no contraction.
//
// A SYNDROME IN A LANE, tiles of S <= 64 syndromes, rows S words wide, check records (alpha m1, alpha m2, a, sign bits):
// all as in minsum_kernels.hpp, whose ms_clamp and ms_message are used here and whose flooding sweeps these are.  State of
// a tile:
//   L    [n][S]              f32  the posterior LLRs; a decimated bit holds its pin, +-2 clip, here and nowhere else
//   rec  [rec_words][S]      u32  the check-to-bit messages (forms: minsum_kernels.hpp)
//   D    [ceil(n / 32)][S]   u32  the decimated bits, bit j % 32 of word j / 32
//   syn  [s][S]              u8
// GLOBAL = false: the workgroup's dynamic LDS for the whole decode; GLOBAL = true: a slot of a global workspace per
// workgroup of the persistent grid (S = 64); same code.
//
// The stop test of iteration t rides on check sweep t + 1 as in the min-sum kernel, so a round that ends with iteration t
// is known to have failed only after check sweep t + 1 has read the L of bit sweep t: the decimation sits between check
// sweep t + 1 and bit sweep t + 1, which is the order THE RULE states.  The bit sweep leaves a bit of D alone.
// All lanes of a tile start together and a round has round_iters iterations, so the end of a round is uniform across the
// workgroup: every thread scans its share of the bits for (|L| as its bit pattern, 0xffffffff - j) over the bits not in D,
// a 64-bit LDS word per lane takes the largest (atomicMax: the order is free), and one thread per lane sets the bit of D
// and writes the pin.  A lane that has stopped is frozen: its L and D are not written again.  The tile ends with its last
// lane.  my_iters, my_dec and my_conv are equal copies in the T / S threads that share a lane.
#pragma once
#include "minsum_kernels.hpp"

namespace ldpc {

struct DecimParams {
    int s, n, round_iters, max_dec;   // round_iters >= 1
    int total_iters;                  // round_iters * (max_dec + 1)
    int S, shift;                     // syndromes per tile, S = 1 << shift
    long long batch;
    float alpha, clip, pin;           // pin = 2 clip
    const uint8_t *syn;               // [batch][s]
    uint8_t *err, *conv;              // [batch][n], [batch]
    double *llr;                      // [batch][n] or NULL
    int32_t *iters, *decimated;       // [batch] or NULL
    const float *prior;               // [n]
    const int *row_ptr, *csr_col, *rec_off, *col_ptr, *edge_rec, *edge_pos;   // as MsParams
    int rec_words;
    unsigned char *ws;                // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

// (decim_state_bytes() -- the bytes of a tile's state, S lanes of (n + rec_words + ceil(n / 32)) words and s bytes: tile_plan.hpp)

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void decim_kernel(DecimParams p)
{
    constexpr int T = TW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char decim_lds[];
    // (bytes: with what __syncthreads_or keeps, the static LDS stays within the 1 KiB that the 79 / 159 KiB budgets of the
    // dynamic part leave of a CU's 160 KiB)
    __shared__ unsigned long long sh_key[64];
    __shared__ unsigned char sh_bad[64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, s = p.s, dw = (n + 31) >> 5;
    const float alpha = p.alpha, clip = p.clip;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = decim_lds;
    float *L = (float *)base;
    unsigned *R = (unsigned *)base + ((size_t)n << sh);
    unsigned *D = R + ((size_t)p.rec_words << sh);
    unsigned char *Y = (unsigned char *)(D + ((size_t)dw << sh));
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ edge_rec = p.edge_rec, *__restrict__ edge_pos = p.edge_pos;
    const float *__restrict__ prior = p.prior;
    const long long tiles = (p.batch + S - 1) >> sh;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long col0 = tile << sh;
        const int valid = (int)((p.batch - col0) < (long long)S ? (p.batch - col0) : (long long)S);
        // ---- state of iteration 0: L = channel_llr, every message +0, D empty; the syndromes, a wave per column
        for (int j = q; j < n; j += Q) L[((size_t)j << sh) + l] = prior[j];
        for (int w = q; w < p.rec_words + dw; w += Q) R[((size_t)w << sh) + l] = 0u;   // (D follows the records)
        ms_stage_syndromes<TW>(Y, s, S, sh, valid, wave, lane, [&](int c, int i) { return p.syn[(col0 + c) * s + i]; });
        if (t < 64) { sh_bad[t] = 0; sh_key[t] = 0ull; }
        bool active = l < valid;
        int my_iters = 0, my_dec = 0, my_conv = 0;
        int t_in = 0;   // iterations of the current round that have run
        __syncthreads();

        for (int done = 0;; ++done) {   // done: the bit sweeps so far
            const bool test_only = done == p.total_iters;
            // ---- check sweep done + 1, and H * err == syndrome on the L it reads (the stop test of iteration `done`)
            if (active) {
                int bad = 0;
                for (int i = q; i < s; i += Q) {
                    const int ra = row_ptr[i], deg = row_ptr[i + 1] - ra;
                    const unsigned y = Y[((size_t)i << sh) + l];
                    unsigned hard = 0;
                    if (deg == 0) {   // an empty check sends nothing and is matched only by a 0 entry
                        bad |= (int)y;
                        continue;
                    }
                    ms_check_update(R + ((size_t)rec_off[i] << sh) + l, deg, sh, alpha, clip, y, false, !test_only, [&](int k, float c, bool test) {
                        const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                        if (test) hard ^= (unsigned)(Lj <= 0.0f);
                        return ms_clamp(Lj - c, clip);   // (a pinned bit: exactly +-clip, never below m1)
                    });
                    bad |= (int)(hard ^ y);
                }
                if (bad) sh_bad[l] = 1;
            }
            __syncthreads();
            // ---- what the test means for the lane; at the end of a round a lane that has no decimation left gives up
            const bool round_end = t_in == p.round_iters;   // (the same in every thread: done = a multiple of round_iters, > 0)
            if (active && done > 0) {
                if (!sh_bad[l]) {   // the L of bit sweep `done` reproduces the syndrome
                    active = false;
                    my_conv = 1;
                    my_iters = done;
                } else if (round_end && my_dec == p.max_dec) {
                    active = false;
                    my_iters = done;
                }
            }
            const int any = __syncthreads_or(active);
            if (t < 64) sh_bad[t] = 0;
            if (!any || test_only) break;
            if (round_end) {
                // ---- decimation: the bit outside D of largest |L|, the lowest index on a tie; D gets it, L[j] its pin
                t_in = 0;
                if (active) {
                    unsigned long long key = 0ull;
                    for (int j = q; j < n; j += Q) {
                        if ((D[((size_t)(j >> 5) << sh) + l] >> (j & 31)) & 1u) continue;
                        const unsigned mag = __float_as_uint(L[((size_t)j << sh) + l]) & 0x7fffffffu;
                        const unsigned long long k = ((unsigned long long)mag << 32) | (unsigned long long)(0xffffffffu - (unsigned)j);
                        key = k > key ? k : key;
                    }
                    if (key) atomicMax(&sh_key[l], key);
                }
                __syncthreads();
                if (active) {
                    const unsigned j = 0xffffffffu - (unsigned)(sh_key[l] & 0xffffffffull);
                    if (q == 0 && j < (unsigned)n) {   // (my_dec < max_dec <= n: a bit outside D exists, so the key is one)
                        D[((size_t)(j >> 5) << sh) + l] |= 1u << (j & 31);
                        float *Lj = L + ((size_t)j << sh) + l;
                        *Lj = *Lj <= 0.0f ? -p.pin : p.pin;
                    }
                    my_dec += 1;
                }
                __syncthreads();
                if (t < 64) sh_key[t] = 0ull;
            }
            // ---- bit sweep done + 1: channel_llr plus the messages in ascending check order; a bit of D keeps its pin
            if (active) {
                for (int j = q; j < n; j += Q) {
                    if ((D[((size_t)(j >> 5) << sh) + l] >> (j & 31)) & 1u) continue;
                    float acc = prior[j];
                    const int eb = col_ptr[j + 1];
                    for (int e = col_ptr[j]; e < eb; ++e) {
                        acc = acc + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                    }
                    L[((size_t)j << sh) + l] = acc;
                }
            }
            t_in += 1;
            __syncthreads();
        }

        // ---- results, a wave per column: err = (L <= 0), llr = L widened
        ms_write_results<TW>(L, n, sh, valid, wave, lane, p.err + col0 * n, p.llr ? p.llr + col0 * n : nullptr);
        if (q == 0 && l < valid) {
            p.conv[col0 + l] = (uint8_t)my_conv;
            if (p.iters) p.iters[col0 + l] = my_iters;
            if (p.decimated) p.decimated[col0 + l] = my_dec;
        }
        __syncthreads();
    }
}

}  // namespace ldpc
