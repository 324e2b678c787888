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
#include "pauli_kernels.hpp"   // pauli_decide; minsum_kernels.hpp: ms_clamp, ms_message, ms_check_update

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

// ---- the legs of a lane, as named steps (relay_kernel of relay_kernels.hpp spells the same steps inline: with these
// functions it measured about 1 % slower, profiles/check_update_refactor_probe.txt).  Every thread of a lane keeps an equal copy.
struct RelayLeg {
    bool fresh = true, pending = false, last = false;   // fresh: the leg starts with the next check sweep; pending: a bit sweep awaits its test
    int leg = 0, t_in = 0, my_iters = 0, my_found = 0;   // t_in: iterations of the leg that have run
    long long best_w = 0;
};

// A solution (`sol`: the lane's test found one): its weight, summed per lane over the threads that share it through sh_w;
// the lighter one is kept in best, PLANES bit planes of bw words.  decision(j): bit p of it goes into plane p;
// weight_of(j, E): the weight of decision E at j.  Every thread of the workgroup calls this: one barrier where no lane has
// a solution, three where one has.
template <int PLANES, class Decision, class WeightOf>
__device__ inline void relay_keep_lighter(RelayLeg &g, bool sol, unsigned long long *sh_w, unsigned *best, int n, int sh, int l, int q, int Q, int t,
                                          Decision decision, WeightOf weight_of)
{
    const int bw = (n + 31) >> 5;
    if (!__syncthreads_or(sol)) return;
    if (sol) {
        long long part = 0;
        for (int w = q; w < bw; w += Q) {
            const int je = (w << 5) + 32 < n ? (w << 5) + 32 : n;
            for (int j = w << 5; j < je; ++j) part += weight_of(j, decision(j));
        }
        if (part) atomicAdd(&sh_w[l], (unsigned long long)part);
    }
    __syncthreads();
    if (sol) {
        const long long w_now = (long long)sh_w[l];
        if (g.my_found == 0 || w_now < g.best_w) {   // a tie keeps the earlier solution
            g.best_w = w_now;
            for (int w = q; w < bw; w += Q) {
                const int je = (w << 5) + 32 < n ? (w << 5) + 32 : n;
                unsigned bits[PLANES] = {};
                for (int j = w << 5; j < je; ++j) {
                    const unsigned E = decision(j);
#pragma unroll
                    for (int pl = 0; pl < PLANES; ++pl) bits[pl] |= ((E >> pl) & 1u) << (j & 31);
                }
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl) best[((size_t)(pl * bw + w) << sh) + l] = bits[pl];
            }
        }
        g.my_found += 1;
    }
    __syncthreads();
    if (t < 64) sh_w[t] = 0ull;
}

// What the test means for a lane whose bit sweep awaited it: stop (false goes into `active`), go on, or start the next leg
// from this M in the middle of the old one -- then true is returned, and the lane spends the round's bit sweep on that start.
// A lane that stops leaves in sh_have whether the write-out takes best.
__device__ inline bool relay_after_test(RelayLeg &g, bool &active, bool sol, int legs, int stop_after, unsigned char *sh_have, int l, int q)
{
    const bool was_fresh = g.fresh;
    bool restart = false;
    g.fresh = false;
    if (active && g.pending) {
        bool stop = g.last;   // the last leg has used up its iterations
        if (sol) {
            if (g.my_found == stop_after) stop = true;
            else if (was_fresh) {}   // the leg ended with this iteration anyway: the next one has started
            else if (g.leg + 1 < legs) { g.leg += 1; g.t_in = 0; g.fresh = true; restart = true; }
            else stop = true;
        }
        if (stop) {
            active = false;
            if (q == 0) sh_have[l] = g.my_found > 0;
        }
        g.pending = false;
    }
    return restart;
}

// A bit sweep has run: the iteration counts; `next`: it wrote the next leg's start, `ends`: the leg ended with it.
__device__ inline void relay_after_sweep(RelayLeg &g, bool ends, bool next)
{
    g.t_in += 1;
    g.my_iters += 1;
    g.pending = true;
    if (next) { g.leg += 1; g.t_in = 0; g.fresh = true; }
    else if (ends) g.last = true;
}

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
        ms_stage_syndromes<TW>(Y, s, S, sh, valid, wave, lane,
                               [&](int c, int i) { return i < rx ? p.sx[(col0 + c) * rx + i] : p.sz[(col0 + c) * rz + (i - rx)]; });
        if (t < 64) { sh_bad[t] = 0; sh_have[t] = 0; sh_w[t] = 0ull; }
        bool active = l < valid;
        RelayLeg lg;
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
                    // b_k of the check's k-th qubit (on G) against its old message c; where tested, the part of the qubit's
                    // decision (on M) that the check sees goes into `hard`
                    ms_check_update(R + ((size_t)rec_off[i] << sh) + l, deg, sh, alpha, clip, y, lg.fresh, true, [&](int k, float c, bool test) {
                        const size_t at = ((size_t)csr_col[ra + k] << sh) + l;
                        if (test) {
                            const unsigned E = decide_at(at);
                            hard ^= zrow ? (E & 1u) : (E >> 1);
                        }
                        const float gx = G[at], gy = G[plane + at], gz = G[2 * plane + at];
                        const float own = zrow ? gx : gz, other = zrow ? gz : gx;
                        const float u = gy < own ? gy : own;            // min(GY, own)
                        const float w = other < 0.0f ? other : 0.0f;
                        return ms_clamp((u - c) - w, clip);
                    });
                    bad |= (int)(hard ^ y);
                }
                if (bad) sh_bad[l] = 1;
            }
            __syncthreads();
            const bool sol = active && lg.pending && !sh_bad[l];   // the M of the bit sweep before reproduces both syndromes
            relay_keep_lighter<2>(lg, sol, sh_w, Bst, n, sh, l, q, Q, t,
                                  [&](int j) -> unsigned { return decide_at(((size_t)j << sh) + l); },   // 1 = X, 3 = Y, 2 = Z
                                  [&](int j, unsigned E) -> long long { return E ? weight[(size_t)(E == 1u ? 0 : E == 3u ? 1 : 2) * n + j] : 0; });
            if (t < 64) sh_bad[t] = 0;
            const bool restart = relay_after_test(lg, active, sol, p.legs, p.stop_after, sh_have, l, q);
            if (!__syncthreads_or(active)) break;
            if (active) {
                const float *__restrict__ row = tab + (size_t)lg.leg * 4 * (size_t)n;   // gamma, g0X, g0Y, g0Z of the lane's leg
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
                    const bool ends = lg.t_in + 1 == leg_iters[lg.leg], next = ends && lg.leg + 1 < p.legs;
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
                    relay_after_sweep(lg, ends, next);
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
            p.conv[col0 + l] = (uint8_t)(lg.my_found > 0);
            if (p.iters) p.iters[col0 + l] = lg.my_iters;
            if (p.solutions) p.solutions[col0 + l] = lg.my_found;
        }
        __syncthreads();
    }
}

}  // namespace ldpc
