// relay_kernels.hpp -- device code of the relay min-sum decoder (ldpc_relay_* of include/ldpc_mi355x.h, where the rule
// is stated; host side: ldpc_relay.hip).  Binary32 throughout, one rounding per operation, no contraction.
//
// A SYNDROME IN A LANE, tiles of S <= 64 syndromes, rows S words wide, check records (alpha m1, alpha m2, a, sign bits):
// all as in minsum_kernels.hpp, whose ms_clamp and ms_message are used here.  State of a tile:
//   X    [n][S]              f32  what the check sweep reads
//   M    [n][S]              f32  the posterior
//   rec  [rec_words][S]      u32  the check-to-bit messages (forms: minsum_kernels.hpp)
//   best [ceil(n / 32)][S]   u32  the lightest solution so far, bit j % 32 of word j / 32
//   syn  [s][S]              u8
// GLOBAL = false: the workgroup's dynamic LDS for the whole decode; GLOBAL = true: a slot of a global workspace per
// workgroup of the persistent grid (S = 64); same code.
//
// The lanes of a tile are in different legs, so every thread keeps its lane's (leg, iteration in the leg, found, best_w,
// ...) in registers -- the T / S threads that share a lane hold equal copies -- and reads gammas / g0 rows of ITS leg.
// One round of the loop is a check sweep and a bit sweep for every running lane:
//   * the test of iteration t (H * err == syndrome on the M of bit sweep t) rides on the next check sweep, which reads M
//     next to X for it;
//   * "every c <- +0" of a leg start is the per-lane predicate `fresh` inside the check sweep: the old record reads as
//     all-zero words; there is no zeroing pass;
//   * a leg that uses up its iterations ends in its last bit sweep, which writes the NEXT leg's X = g0 + gamma * M at once,
//     so the sweep that tests that M is the first check sweep of the next leg;
//   * a lane whose test finds a solution in the middle of a leg (and that goes on) has swept with the old leg's X: it
//     spends the round's bit sweep on X = g0 + gamma * M of the next leg instead and sweeps again in the next round;
//   * the weight of a solution is summed in int64 per lane over the threads that share it, through an LDS word per lane.
// A lane that has stopped is frozen: its M and best are not written again.  The tile ends with its last lane.
#pragma once
#include "minsum_kernels.hpp"

namespace ldpc {

struct RelayParams {
    int s, n, legs, stop_after;     // legs: those with leg_iters > 0, at least one
    int S, shift;                   // syndromes per tile, S = 1 << shift
    long long batch;
    float alpha, clip;
    const uint8_t *syn;             // [batch][s]
    uint8_t *err, *conv;            // [batch][n], [batch]
    double *llr;                    // [batch][n] or NULL
    int32_t *iters, *solutions;     // [batch] or NULL
    const float *prior;             // [n]
    const float *gammas, *g0;       // [legs][n]
    const int *leg_iters;           // [legs], each >= 1
    const long long *weight;        // [n]: q of the rule
    const int *row_ptr, *csr_col, *rec_off, *col_ptr, *edge_rec, *edge_pos;   // as MsParams
    int rec_words;
    unsigned char *ws;              // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

// (relay_state_bytes() -- the bytes of a tile's state, S lanes of (2 n + rec_words + ceil(n / 32)) words and s bytes: tile_plan.hpp)

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void relay_kernel(RelayParams p)
{
    constexpr int T = TW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char relay_lds[];
    // (bytes: with the weights and what __syncthreads_or keeps, the static LDS stays within the 1 KiB that the 79 / 159 KiB
    // budgets of the dynamic part leave of a CU's 160 KiB)
    __shared__ unsigned long long sh_w[64];
    __shared__ unsigned char sh_bad[64], sh_have[64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, s = p.s, bw = (n + 31) >> 5;
    const float alpha = p.alpha, clip = p.clip;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = relay_lds;
    float *X = (float *)base;
    float *M = X + ((size_t)n << sh);
    unsigned *R = (unsigned *)(M + ((size_t)n << sh));
    unsigned *Bst = R + ((size_t)p.rec_words << sh);
    unsigned char *Y = (unsigned char *)(Bst + ((size_t)bw << sh));
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ edge_rec = p.edge_rec, *__restrict__ edge_pos = p.edge_pos;
    const float *__restrict__ prior = p.prior, *__restrict__ gammas = p.gammas, *__restrict__ g0 = p.g0;
    const int *__restrict__ leg_iters = p.leg_iters;
    const long long *__restrict__ weight = p.weight;
    const long long tiles = (p.batch + S - 1) >> sh;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long col0 = tile << sh;
        const int valid = (int)((p.batch - col0) < (long long)S ? (p.batch - col0) : (long long)S);
        // ---- leg 0 starts: M = channel_llr, X = g0 + gamma * M, every message +0 (`fresh`); the syndromes, a wave per column
        for (int j = q; j < n; j += Q) {
            const float m = prior[j];
            M[((size_t)j << sh) + l] = m;
            X[((size_t)j << sh) + l] = g0[j] + gammas[j] * m;
        }
        for (int c = wave; c < S; c += TW) {
            if (c < valid) {
                const uint8_t *src = p.syn + (col0 + c) * s;
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = src[i] != 0;
            } else {   // a lane past the batch reads nothing and never becomes active
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = 0;
            }
        }
        if (t < 64) { sh_bad[t] = 0; sh_have[t] = 0; sh_w[t] = 0ull; }
        bool active = l < valid, fresh = true, pending = false, last = false;
        int leg = 0, t_in = 0, my_iters = 0, my_found = 0;
        long long best_w = 0;
        __syncthreads();

        for (;;) {
            // ---- check sweep on X, and H * err == syndrome on the M next to it (the test of the bit sweep before)
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
                    unsigned *rec = R + ((size_t)rec_off[i] << sh) + l;
                    float m1 = clip, m2 = clip;
                    unsigned a = kMsNone, par = y;
                    if (deg <= 64) {
                        const float o1 = fresh ? 0.0f : __uint_as_float(rec[0]);
                        const float o2 = fresh ? 0.0f : __uint_as_float(rec[(size_t)1 << sh]);
                        const unsigned oa = rec[(size_t)2 << sh];
                        unsigned sg = fresh ? 0u : rec[(size_t)3 << sh], neg_lo = 0, neg_hi = 0;
                        const int d0 = deg < 32 ? deg : 32;
                        for (int k = 0; k < d0; ++k) {
                            const size_t at = ((size_t)csr_col[ra + k] << sh) + l;
                            hard ^= (unsigned)(M[at] <= 0.0f);
                            const float cm = (unsigned)k == oa ? o2 : o1;
                            const float c = (sg >> k) & 1u ? -cm : cm;
                            const float b = ms_clamp(X[at] - c, clip);
                            const unsigned ng = b < 0.0f;
                            const float mag = fabsf(b);
                            neg_lo |= ng << k;
                            par ^= ng;
                            if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                            else if (mag < m2) m2 = mag;
                        }
                        if (deg > 32) {
                            sg = fresh ? 0u : rec[(size_t)4 << sh];
                            for (int k = 32; k < deg; ++k) {
                                const size_t at = ((size_t)csr_col[ra + k] << sh) + l;
                                hard ^= (unsigned)(M[at] <= 0.0f);
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float c = (sg >> (k - 32)) & 1u ? -cm : cm;
                                const float b = ms_clamp(X[at] - c, clip);
                                const unsigned ng = b < 0.0f;
                                const float mag = fabsf(b);
                                neg_hi |= ng << (k - 32);
                                par ^= ng;
                                if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                                else if (mag < m2) m2 = mag;
                            }
                        }
                        const unsigned flip = par ? 0xffffffffu : 0u;   // negative iff par XOR neg_k
                        rec[0] = __float_as_uint(alpha * m1);
                        rec[(size_t)1 << sh] = __float_as_uint(alpha * m2);
                        rec[(size_t)2 << sh] = a;
                        rec[(size_t)3 << sh] = (neg_lo ^ flip) & (d0 == 32 ? 0xffffffffu : (1u << d0) - 1u);
                        if (deg > 32) rec[(size_t)4 << sh] = (neg_hi ^ flip) & (deg == 64 ? 0xffffffffu : (1u << (deg - 32)) - 1u);
                    } else {
                        // per-edge record: the minima first, then every edge's b once more for its sign
                        for (int k = 0; k < deg; ++k) {
                            const size_t at = ((size_t)csr_col[ra + k] << sh) + l;
                            hard ^= (unsigned)(M[at] <= 0.0f);
                            const float old = fresh ? 0.0f : __uint_as_float(rec[(size_t)k << sh]);
                            const float b = ms_clamp(X[at] - old, clip);
                            const float mag = fabsf(b);
                            par ^= (unsigned)(b < 0.0f);
                            if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                            else if (mag < m2) m2 = mag;
                        }
                        const float n1 = alpha * m1, n2 = alpha * m2;
                        for (int k = 0; k < deg; ++k) {
                            const float old = fresh ? 0.0f : __uint_as_float(rec[(size_t)k << sh]);
                            const float b = ms_clamp(X[((size_t)csr_col[ra + k] << sh) + l] - old, clip);
                            const float cm = (unsigned)k == a ? n2 : n1;
                            rec[(size_t)k << sh] = __float_as_uint((par ^ (unsigned)(b < 0.0f)) ? -cm : cm);
                        }
                    }
                    bad |= (int)(hard ^ y);
                }
                if (bad) sh_bad[l] = 1;
            }
            __syncthreads();
            const bool was_fresh = fresh;
            const bool sol = active && pending && !sh_bad[l];   // the M of the bit sweep before reproduces the syndrome
            fresh = false;
            // ---- a solution: its weight, summed per lane over the threads that share it; the lighter one is kept
            if (__syncthreads_or(sol)) {
                if (sol) {
                    long long part = 0;
                    for (int w = q; w < bw; w += Q) {
                        const int je = (w << 5) + 32 < n ? (w << 5) + 32 : n;
                        for (int j = w << 5; j < je; ++j)
                            if (M[((size_t)j << sh) + l] <= 0.0f) part += weight[j];
                    }
                    if (part) atomicAdd(&sh_w[l], (unsigned long long)part);
                }
                __syncthreads();
                if (sol) {
                    const long long w_now = (long long)sh_w[l];
                    if (my_found == 0 || w_now < best_w) {   // a tie keeps the earlier solution
                        best_w = w_now;
                        for (int w = q; w < bw; w += Q) {
                            const int je = (w << 5) + 32 < n ? (w << 5) + 32 : n;
                            unsigned bits = 0;
                            for (int j = w << 5; j < je; ++j) bits |= (unsigned)(M[((size_t)j << sh) + l] <= 0.0f) << (j & 31);
                            Bst[((size_t)w << sh) + l] = bits;
                        }
                    }
                    my_found += 1;
                }
                __syncthreads();
                if (t < 64) sh_w[t] = 0ull;
            }
            if (t < 64) sh_bad[t] = 0;
            // ---- what the test means for the lane: stop, go on, or start the next leg from this M
            bool restart = false;
            if (active && pending) {
                bool stop = last;   // the last leg has used up its iterations
                if (sol) {
                    if (my_found == p.stop_after) stop = true;
                    else if (was_fresh) {}   // the leg ended with this iteration anyway: the next one has started
                    else if (leg + 1 < p.legs) { leg += 1; t_in = 0; fresh = true; restart = true; }
                    else stop = true;
                }
                if (stop) {
                    active = false;
                    if (q == 0) sh_have[l] = my_found > 0;
                }
                pending = false;
            }
            if (!__syncthreads_or(active)) break;
            if (active) {
                const size_t row = (size_t)leg * (size_t)n;
                if (restart) {
                    // ---- leg start in the middle of the old leg: X = g0 + gamma * M; the next round sweeps it (`fresh`)
                    for (int j = q; j < n; j += Q) {
                        const size_t at = ((size_t)j << sh) + l;
                        X[at] = g0[row + j] + gammas[row + j] * M[at];
                    }
                } else {
                    // ---- bit sweep: M = (g0 + gamma * M) + messages; X = (g0 + gamma * new M) + messages, or, where the leg
                    // ends with this iteration, the next leg's start X = g0' + gamma' * new M
                    const bool ends = t_in + 1 == leg_iters[leg], next = ends && leg + 1 < p.legs;
                    const size_t row2 = row + (size_t)n;
                    for (int j = q; j < n; j += Q) {
                        const size_t at = ((size_t)j << sh) + l;
                        const float g = gammas[row + j], h = g0[row + j];
                        const int ea = col_ptr[j], eb = col_ptr[j + 1];
                        float acc = h + g * M[at];
                        for (int e = ea; e < eb; ++e) acc = acc + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                        M[at] = acc;
                        float x;
                        if (next) {
                            x = g0[row2 + j] + gammas[row2 + j] * acc;
                        } else {
                            x = h + g * acc;
                            for (int e = ea; e < eb; ++e) x = x + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                        }
                        X[at] = x;
                    }
                    t_in += 1;
                    my_iters += 1;
                    pending = true;
                    if (next) { leg += 1; t_in = 0; fresh = true; }
                    else if (ends) last = true;
                }
            }
            __syncthreads();
        }

        // ---- results, a wave per column: err = best where a solution was found, else (M <= 0); llr = M widened
        for (int c = wave; c < valid; c += TW) {
            uint8_t *eo = p.err + (col0 + c) * n;
            double *lo = p.llr ? p.llr + (col0 + c) * n : nullptr;
            const bool have = sh_have[c] != 0;
            for (int j = lane; j < n; j += 64) {
                const float v = M[((size_t)j << sh) + c];
                eo[j] = have ? (uint8_t)((Bst[((size_t)(j >> 5) << sh) + c] >> (j & 31)) & 1u) : (uint8_t)(v <= 0.0f);
                if (lo) lo[j] = (double)v;
            }
        }
        if (q == 0 && l < valid) {
            p.conv[col0 + l] = (uint8_t)(my_found > 0);
            if (p.iters) p.iters[col0 + l] = my_iters;
            if (p.solutions) p.solutions[col0 + l] = my_found;
        }
        __syncthreads();
    }
}

}  // namespace ldpc
