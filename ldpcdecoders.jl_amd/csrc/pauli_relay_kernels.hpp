// pauli_relay_kernels.hpp -- device code of the Pauli relay min-sum decoder: the joint X/Z min-sum of pauli_kernels.hpp
// run with the memory legs of relay_kernels.hpp (ldpc_pauli_relay_* of include/ldpc_mi355x.h, where the rule is stated; host
// side: ldpc_pauli_relay.hip).  Binary32 throughout, one rounding per operation, no contraction.
//
// A SYNDROME IN A LANE, tiles of S <= 64 syndromes, rows S words wide, check records (alpha m1, alpha m2, a, sign bits) as in
// minsum_kernels.hpp, whose ms_clamp and ms_message are used here; the checks of both sides are one graph, Hx rows first
// (they see the Z parts), then Hz rows (they see the X parts), and pauli_decide is the rule's decision.  State of a tile:
//   G    [3 n][S]                f32  GX, GY, GZ as the check sweep reads them: Lambda of the CURRENT M plus the totals
//   M    [3 n][S]                f32  MX, MY, MZ, the posteriors
//   rec  [rec_words][S]          u32  the check-to-qubit messages (forms: minsum_kernels.hpp)
//   best [2 ceil(n / 32)][S]     u32  the lightest solution so far: a bit plane for the X part, then one for the Z part
//   syn  [rx + rz][S]            u8
// = 4 (6 n + rec_words + 2 ceil(n / 32)) + rx + rz bytes a syndrome (pauli_relay_state_bytes(), tile_plan.hpp).  The totals
// TX, TZ are not stored: the bit sweep sums them in registers and writes both triples, M = Lambda(old M) + T and
// G = Lambda(new M) + T, so the check sweep -- six reads an edge -- touches no table.  gamma and the three g0 of a qubit and
// leg are gathered once per qubit in the bit sweep (tab, four rows a leg).
// GLOBAL = false: the workgroup's dynamic LDS for the whole decode; GLOBAL = true: a slot of a global workspace per
// workgroup of the persistent grid (S = 64); same code.
//
// The legs are handled as in relay_kernels.hpp: the lanes of a tile are in different legs, every thread keeps its lane's
// (leg, iteration in the leg, found, best_w, ...) in registers, and one round of the loop is a check sweep and a bit sweep
// for every running lane:
//   * the test of iteration t (Hz ex == sz and Hx ez == sx on the M of bit sweep t) rides on the next check sweep, which
//     reads M next to G for it;
//   * "every c <- +0" of a leg start is the per-lane predicate `fresh` inside the check sweep; there is no zeroing pass;
//   * a leg that uses up its iterations ends in its last bit sweep, which writes the NEXT leg's start G = Lambda' + 0 at
//     once, so the sweep that tests that M is the first check sweep of the next leg;
//   * a lane whose test finds a solution in the middle of a leg (and that goes on) has swept with the old leg's G: it
//     spends the round's bit sweep on the next leg's start G instead and sweeps again in the next round;
//   * the weight of a solution is summed in int64 per lane over the threads that share it, through an LDS word per lane.
// A lane that has stopped is frozen: its M and best are not written again.  The tile ends with its last lane.
#pragma once
#include "pauli_kernels.hpp"   // pauli_decide; minsum_kernels.hpp: ms_clamp, ms_message, kMsNone

namespace ldpc {

struct PauliRelayParams {
    int rx, s, n, legs, stop_after;   // s = rx + rz; legs: those with leg_iters > 0, at least one
    int S, shift;                     // syndromes per tile, S = 1 << shift
    long long batch;
    float alpha, clip;
    const uint8_t *sx, *sz;           // [batch][rx], [batch][s - rx]
    uint8_t *gx, *gz, *conv;          // [batch][n], [batch][n], [batch]
    double *llr;                      // [batch][3][n] or NULL
    int32_t *iters, *solutions;       // [batch] or NULL
    const float *prior;               // [3][n]: prior_x, prior_y, prior_z
    const float *tab;                 // [legs][4][n]: gammas, g0X, g0Y, g0Z of the leg
    const int *leg_iters;             // [legs], each >= 1
    const long long *weight;          // [3][n]: qX, qY, qZ of the rule
    const int *row_ptr, *csr_col, *rec_off, *col_ptr, *col_mid, *edge_rec, *edge_pos;   // as PauliParams
    int rec_words;
    unsigned char *ws;                // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void pauli_relay_kernel(PauliRelayParams p)
{
    constexpr int T = TW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char pauli_relay_lds[];
    // (bytes: with the weights and what __syncthreads_or keeps, the static LDS stays within the 1 KiB that the 79 / 159 KiB
    // budgets of the dynamic part leave of a CU's 160 KiB)
    __shared__ unsigned long long sh_w[64];
    __shared__ unsigned char sh_bad[64], sh_have[64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, s = p.s, rx = p.rx, rz = p.s - p.rx, bw = (n + 31) >> 5;
    const float alpha = p.alpha, clip = p.clip;
    const size_t plane = (size_t)n << sh;   // words of one belief of a tile
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = pauli_relay_lds;
    float *G = (float *)base;            // GX at 0, GY at plane, GZ at 2 plane
    float *M = G + 3 * plane;            // MX, MY, MZ alike
    unsigned *R = (unsigned *)(M + 3 * plane);
    unsigned *Bst = R + ((size_t)p.rec_words << sh);
    unsigned char *Y = (unsigned char *)(Bst + ((size_t)2 * bw << sh));
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ col_mid = p.col_mid;
    const int *__restrict__ edge_rec = p.edge_rec, *__restrict__ edge_pos = p.edge_pos;
    const float *__restrict__ prior = p.prior, *__restrict__ tab = p.tab;
    const int *__restrict__ leg_iters = p.leg_iters;
    const long long *__restrict__ weight = p.weight;
    const long long tiles = (p.batch + S - 1) >> sh;

    // the decision of the rule on the posteriors of qubit j in lane c
    auto decide_at = [&](size_t at) -> unsigned { return pauli_decide(M[at], M[plane + at], M[2 * plane + at]); };

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long col0 = tile << sh;
        const int valid = (int)((p.batch - col0) < (long long)S ? (p.batch - col0) : (long long)S);
        // ---- leg 0 starts: M = the priors, G = Lambda + (+0) totals, every message +0 (`fresh`); the syndromes, a wave per column
        for (int j = q; j < n; j += Q) {
            const size_t at = ((size_t)j << sh) + l;
            const float g = tab[j];
            const float mx = prior[j], my = prior[(size_t)n + j], mz = prior[(size_t)2 * n + j];
            M[at] = mx;
            M[plane + at] = my;
            M[2 * plane + at] = mz;
            G[at] = (tab[(size_t)n + j] + g * mx) + 0.0f;
            G[plane + at] = ((tab[(size_t)2 * n + j] + g * my) + 0.0f) + 0.0f;
            G[2 * plane + at] = (tab[(size_t)3 * n + j] + g * mz) + 0.0f;
        }
        for (int c = wave; c < S; c += TW) {
            if (c < valid) {
                const uint8_t *ax = p.sx + (col0 + c) * rx, *az = p.sz + (col0 + c) * rz;
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = (i < rx ? ax[i] : az[i - rx]) != 0;
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
            // ---- check sweep on G, and Hz ex == sz, Hx ez == sx on the M next to it (the test of the bit sweep before)
            if (active) {
                int bad = 0;
                for (int i = q; i < s; i += Q) {
                    const int ra = row_ptr[i], deg = row_ptr[i + 1] - ra;
                    const unsigned y = Y[((size_t)i << sh) + l];
                    if (deg == 0) {   // an empty check sends nothing and is matched only by a 0 entry
                        bad |= (int)y;
                        continue;
                    }
                    const bool zrow = i >= rx;   // an Hz row: it sees the X parts
                    unsigned hard = 0;
                    // b_k of the check's k-th qubit against its old message c
                    auto edge = [&](int k, float c) -> float {
                        const size_t at = ((size_t)csr_col[ra + k] << sh) + l;
                        const float gx = G[at], gy = G[plane + at], gz = G[2 * plane + at];
                        const float own = zrow ? gx : gz, other = zrow ? gz : gx;
                        const float u = gy < own ? gy : own;            // min(GY, own)
                        const float w = other < 0.0f ? other : 0.0f;
                        return ms_clamp((u - c) - w, clip);
                    };
                    // the part of the k-th qubit's decision (on M) that the check sees
                    auto seen = [&](int k) -> unsigned {
                        const unsigned E = decide_at(((size_t)csr_col[ra + k] << sh) + l);
                        return zrow ? (E & 1u) : (E >> 1);
                    };
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
                            hard ^= seen(k);
                            const float cm = (unsigned)k == oa ? o2 : o1;
                            const float b = edge(k, (sg >> k) & 1u ? -cm : cm);
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
                                hard ^= seen(k);
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float b = edge(k, (sg >> (k - 32)) & 1u ? -cm : cm);
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
                            hard ^= seen(k);
                            const float b = edge(k, fresh ? 0.0f : __uint_as_float(rec[(size_t)k << sh]));
                            const float mag = fabsf(b);
                            par ^= (unsigned)(b < 0.0f);
                            if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                            else if (mag < m2) m2 = mag;
                        }
                        const float n1 = alpha * m1, n2 = alpha * m2;
                        for (int k = 0; k < deg; ++k) {
                            const float b = edge(k, fresh ? 0.0f : __uint_as_float(rec[(size_t)k << sh]));
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
            const bool sol = active && pending && !sh_bad[l];   // the M of the bit sweep before reproduces both syndromes
            fresh = false;
            // ---- a solution: its weight, summed per lane over the threads that share it; the lighter one is kept
            if (__syncthreads_or(sol)) {
                if (sol) {
                    long long part = 0;
                    for (int w = q; w < bw; w += Q) {
                        const int je = (w << 5) + 32 < n ? (w << 5) + 32 : n;
                        for (int j = w << 5; j < je; ++j) {
                            const unsigned E = decide_at(((size_t)j << sh) + l);   // 1 = X, 3 = Y, 2 = Z
                            if (E) part += weight[(size_t)(E == 1u ? 0 : E == 3u ? 1 : 2) * n + j];
                        }
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
                            unsigned bx = 0, bz = 0;
                            for (int j = w << 5; j < je; ++j) {
                                const unsigned E = decide_at(((size_t)j << sh) + l);
                                bx |= (E & 1u) << (j & 31);
                                bz |= (E >> 1) << (j & 31);
                            }
                            Bst[((size_t)w << sh) + l] = bx;
                            Bst[((size_t)(bw + w) << sh) + l] = bz;
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
                const float *__restrict__ row = tab + (size_t)leg * 4 * (size_t)n;   // gamma, g0X, g0Y, g0Z of the lane's leg
                if (restart) {
                    // ---- leg start in the middle of the old leg: G = Lambda + (+0) totals; the next round sweeps it (`fresh`)
                    for (int j = q; j < n; j += Q) {
                        const size_t at = ((size_t)j << sh) + l;
                        const float g = row[j];
                        G[at] = (row[(size_t)n + j] + g * M[at]) + 0.0f;
                        G[plane + at] = ((row[(size_t)2 * n + j] + g * M[plane + at]) + 0.0f) + 0.0f;
                        G[2 * plane + at] = (row[(size_t)3 * n + j] + g * M[2 * plane + at]) + 0.0f;
                    }
                } else {
                    // ---- bit sweep: TZ over the qubit's Hx checks, TX over its Hz checks, each from +0 in ascending order;
                    // M = Lambda(old M) + T; G = Lambda(new M) + T, or, where the leg ends with this iteration, the next
                    // leg's start G = Lambda'(new M) + (+0)
                    const bool ends = t_in + 1 == leg_iters[leg], next = ends && leg + 1 < p.legs;
                    const float *__restrict__ row2 = row + (size_t)4 * n;
                    for (int j = q; j < n; j += Q) {
                        const size_t at = ((size_t)j << sh) + l;
                        const float g = row[j], hx = row[(size_t)n + j], hy = row[(size_t)2 * n + j], hz = row[(size_t)3 * n + j];
                        const int ea = col_ptr[j], em = col_mid[j], eb = col_ptr[j + 1];
                        float tz = 0.0f, tx = 0.0f;
                        for (int e = ea; e < em; ++e) tz = tz + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                        for (int e = em; e < eb; ++e) tx = tx + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                        const float mx = (hx + g * M[at]) + tx;
                        const float my = ((hy + g * M[plane + at]) + tx) + tz;
                        const float mz = (hz + g * M[2 * plane + at]) + tz;
                        M[at] = mx;
                        M[plane + at] = my;
                        M[2 * plane + at] = mz;
                        if (next) {
                            const float g2 = row2[j];
                            G[at] = (row2[(size_t)n + j] + g2 * mx) + 0.0f;
                            G[plane + at] = ((row2[(size_t)2 * n + j] + g2 * my) + 0.0f) + 0.0f;
                            G[2 * plane + at] = (row2[(size_t)3 * n + j] + g2 * mz) + 0.0f;
                        } else {
                            G[at] = (hx + g * mx) + tx;
                            G[plane + at] = ((hy + g * my) + tx) + tz;
                            G[2 * plane + at] = (hz + g * mz) + tz;
                        }
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

        // ---- results, a wave per column: best where a solution was found, else the decision on M; llr = M widened
        for (int c = wave; c < valid; c += TW) {
            uint8_t *ox = p.gx + (col0 + c) * n, *oz = p.gz + (col0 + c) * n;
            double *lo = p.llr ? p.llr + (col0 + c) * 3 * n : nullptr;
            const bool have = sh_have[c] != 0;
            for (int j = lane; j < n; j += 64) {
                const size_t at = ((size_t)j << sh) + c;
                const float mx = M[at], my = M[plane + at], mz = M[2 * plane + at];
                unsigned E = pauli_decide(mx, my, mz);
                if (have)
                    E = ((Bst[((size_t)(j >> 5) << sh) + c] >> (j & 31)) & 1u) | (((Bst[((size_t)(bw + (j >> 5)) << sh) + c] >> (j & 31)) & 1u) << 1);
                ox[j] = (uint8_t)(E & 1u);
                oz[j] = (uint8_t)(E >> 1);
                if (lo) {
                    lo[j] = (double)mx;
                    lo[(size_t)n + j] = (double)my;
                    lo[(size_t)2 * n + j] = (double)mz;
                }
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
