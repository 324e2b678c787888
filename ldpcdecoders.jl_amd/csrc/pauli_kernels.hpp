// pauli_kernels.hpp -- device code of the joint X/Z (Pauli) min-sum decoder of CSS codes (ldpc_pauli_minsum_* of
// include/ldpc_mi355x.h, where the rule is stated; host side: ldpc_pauli.hip).  Binary32 throughout, one rounding per
// operation, no contraction.
//
// The design of minsum_kernel (minsum_kernels.hpp): A SYNDROME IN A LANE, a workgroup decodes a tile of S syndromes (S a
// power of two, <= 64); thread t works for syndrome t % S and takes the nodes t / S, t / S + T / S, ... of each sweep.
// The checks of both sides form ONE graph over the n qubits: Hx rows first (0 .. rx - 1: they see the Z parts), then Hz
// rows (rx .. rx + rz - 1: they see the X parts).
//
// State of a tile, every row S words wide:
//   TX   [n][S]          f32  per qubit the sum of the messages of its Hz checks
//   TZ   [n][S]          f32  ... of its Hx checks
//   rec  [rec_words][S]  u32  the check-to-qubit messages, one record per check of either side, in the three forms of
//                             ms_record_words() (tile_plan.hpp; what the words hold: minsum_kernels.hpp)
//   syn  [rx + rz][S]    u8   the syndrome entries of both sides as 0 / 1
// The three beliefs of a qubit are not kept: GX = prior_x + TX, GZ = prior_z + TZ, GY = (prior_y + TX) + TZ are formed
// wherever they are read, from the two totals and the three prior tables in global memory (wave-uniform for S = 64).
// GLOBAL = false: the state is the workgroup's dynamic LDS.  GLOBAL = true: a slot of a global workspace per workgroup of
// the persistent grid (S = 64); same code.
//
// The stop test of iteration t rides on check sweep t + 1: that sweep loads TX and TZ of each of its qubits anyway, forms
// the three G and with them the decision of the rule; an Hx check XORs the Z parts of its qubits, an Hz check the X parts.
// A last sweep that only tests follows bit sweep max_iters.  A syndrome that has stopped is frozen: TX and TZ are not
// written again.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minsum_kernels.hpp"   // ms_clamp, ms_message, kMsNone

namespace ldpc {

struct PauliParams {
    int rx, s, n, max_iters;      // s = rx + rz
    int S, shift;                 // syndromes per tile, S = 1 << shift
    long long batch;
    float alpha, clip;
    const uint8_t *sx, *sz;       // [batch][rx], [batch][s - rx]
    uint8_t *gx, *gz, *conv;      // [batch][n], [batch][n], [batch]
    double *llr;                  // [batch][3][n] or NULL
    int32_t *iters;               // [batch] or NULL
    const float *prior_x, *prior_y, *prior_z;   // [n] each
    const int *row_ptr, *csr_col; // checks (Hx rows, then Hz rows) -> qubits, ascending
    const int *rec_off;           // [s]: first word of the check's record
    const int *col_ptr;           // qubits -> edges in ascending check order: the Hx checks [col_ptr[j], col_mid[j]),
    const int *col_mid;           //   then the Hz checks [col_mid[j], col_ptr[j + 1])
    const int *edge_rec;          // per CSC edge: rec_off of its check
    const int *edge_pos;          // per CSC edge: position of the qubit in its check (| kMsPosEdge: per-edge record)
    int rec_words;
    unsigned char *ws;            // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

// The decision of the rule's bit sweep: bit 0 = the X part (E is X or Y), bit 1 = the Z part (E is Z or Y).
__device__ inline unsigned pauli_decide(float gx, float gy, float gz)
{
    unsigned best = 1u;
    float g = gx;
    if (gz < g) { best = 2u; g = gz; }
    if (gy < g) { best = 3u; g = gy; }
    return g <= 0.0f ? best : 0u;
}

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void pauli_minsum_kernel(PauliParams p)
{
    constexpr int T = TW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char pauli_lds[];
    __shared__ int sh_bad[64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, s = p.s, rx = p.rx, rz = p.s - p.rx;
    const float alpha = p.alpha, clip = p.clip;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = pauli_lds;
    float *TX = (float *)base;
    float *TZ = TX + ((size_t)n << sh);
    unsigned *R = (unsigned *)base + ((size_t)2 * n << sh);
    unsigned char *Y = base + (((size_t)2 * n + (size_t)p.rec_words) << sh) * 4;
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ col_mid = p.col_mid;
    const int *__restrict__ edge_rec = p.edge_rec, *__restrict__ edge_pos = p.edge_pos;
    const float *__restrict__ prior_x = p.prior_x, *__restrict__ prior_y = p.prior_y, *__restrict__ prior_z = p.prior_z;
    const long long tiles = (p.batch + S - 1) >> sh;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long col0 = tile << sh;
        const int valid = (int)((p.batch - col0) < (long long)S ? (p.batch - col0) : (long long)S);
        // ---- state of iteration 0: TX = TZ = +0 and every message +0 (all-zero words); the syndromes, a wave per column
        for (int w = q; w < 2 * n + p.rec_words; w += Q) ((unsigned *)base)[((size_t)w << sh) + l] = 0u;   // TX, TZ, rec: one block
        for (int c = wave; c < S; c += TW) {
            if (c < valid) {
                const uint8_t *ax = p.sx + (col0 + c) * rx, *az = p.sz + (col0 + c) * rz;
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = (i < rx ? ax[i] : az[i - rx]) != 0;
            } else {   // a lane past the batch reads nothing and never becomes active
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = 0;
            }
        }
        if (t < 64) sh_bad[t] = 0;
        bool active = l < valid;
        int my_iters = p.max_iters, my_conv = 0;
        __syncthreads();

        for (int it = 1;; ++it) {
            const bool test_only = it > p.max_iters;
            // ---- check sweep `it`, and the stop test of iteration it - 1 on the TX, TZ it reads
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
                    // b_k of the check's k-th qubit against its old message c; the qubit's decision goes into `hard`
                    auto edge = [&](int k, float c) -> float {
                        const int j = csr_col[ra + k];
                        const float tx = TX[((size_t)j << sh) + l], tz = TZ[((size_t)j << sh) + l];
                        const float gx = prior_x[j] + tx, gz = prior_z[j] + tz, gy = (prior_y[j] + tx) + tz;
                        const unsigned E = pauli_decide(gx, gy, gz);
                        hard ^= zrow ? (E & 1u) : (E >> 1);
                        const float own = zrow ? gx : gz, other = zrow ? gz : gx;
                        const float u = gy < own ? gy : own;            // min(GY, own)
                        const float w = other < 0.0f ? other : 0.0f;
                        return ms_clamp((u - c) - w, clip);
                    };
                    unsigned *rec = R + ((size_t)rec_off[i] << sh) + l;
                    float m1 = clip, m2 = clip;
                    unsigned a = kMsNone, par = y;
                    if (deg <= 64) {
                        const float o1 = __uint_as_float(rec[0]), o2 = __uint_as_float(rec[(size_t)1 << sh]);
                        const unsigned oa = rec[(size_t)2 << sh];
                        unsigned sg = rec[(size_t)3 << sh], neg_lo = 0, neg_hi = 0;
                        const int d0 = deg < 32 ? deg : 32;
                        for (int k = 0; k < d0; ++k) {
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
                            sg = rec[(size_t)4 << sh];
                            for (int k = 32; k < deg; ++k) {
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
                        if (!test_only) {
                            const unsigned flip = par ? 0xffffffffu : 0u;   // negative iff par XOR neg_k
                            rec[0] = __float_as_uint(alpha * m1);
                            rec[(size_t)1 << sh] = __float_as_uint(alpha * m2);
                            rec[(size_t)2 << sh] = a;
                            rec[(size_t)3 << sh] = (neg_lo ^ flip) & (d0 == 32 ? 0xffffffffu : (1u << d0) - 1u);
                            if (deg > 32) rec[(size_t)4 << sh] = (neg_hi ^ flip) & (deg == 64 ? 0xffffffffu : (1u << (deg - 32)) - 1u);
                        }
                    } else {
                        // per-edge record: the minima first, then every edge's b once more for its sign
                        for (int k = 0; k < deg; ++k) {
                            const float b = edge(k, __uint_as_float(rec[(size_t)k << sh]));
                            const float mag = fabsf(b);
                            par ^= (unsigned)(b < 0.0f);
                            if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                            else if (mag < m2) m2 = mag;
                        }
                        if (!test_only) {
                            const unsigned tested = hard;   // (the second pass runs every decision into `hard` again)
                            const float n1 = alpha * m1, n2 = alpha * m2;
                            for (int k = 0; k < deg; ++k) {
                                const float b = edge(k, __uint_as_float(rec[(size_t)k << sh]));
                                const float cm = (unsigned)k == a ? n2 : n1;
                                rec[(size_t)k << sh] = __float_as_uint((par ^ (unsigned)(b < 0.0f)) ? -cm : cm);
                            }
                            hard = tested;
                        }
                    }
                    bad |= (int)(hard ^ y);
                }
                if (bad) sh_bad[l] = 1;
            }
            __syncthreads();
            if (active && it > 1 && !sh_bad[l]) {   // the decision of bit sweep it - 1 reproduces both syndromes
                active = false;
                my_conv = 1;
                my_iters = it - 1;
            }
            const int any = __syncthreads_or(active);
            if (t < 64) sh_bad[t] = 0;
            if (!any || test_only) break;
            // ---- bit sweep `it`: TZ over the qubit's Hx checks, TX over its Hz checks, each from +0 in ascending order
            if (active) {
                for (int j = q; j < n; j += Q) {
                    const int ea = col_ptr[j], em = col_mid[j], eb = col_ptr[j + 1];
                    float tz = 0.0f, tx = 0.0f;
                    for (int e = ea; e < em; ++e) tz = tz + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                    for (int e = em; e < eb; ++e) tx = tx + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                    TX[((size_t)j << sh) + l] = tx;
                    TZ[((size_t)j << sh) + l] = tz;
                }
            }
            __syncthreads();
        }

        // ---- results, a wave per column: the decision on the final TX, TZ; llr = the planes GX, GY, GZ widened
        for (int c = wave; c < valid; c += TW) {
            uint8_t *ox = p.gx + (col0 + c) * n, *oz = p.gz + (col0 + c) * n;
            double *lo = p.llr ? p.llr + (col0 + c) * 3 * n : nullptr;
            for (int j = lane; j < n; j += 64) {
                const float tx = TX[((size_t)j << sh) + c], tz = TZ[((size_t)j << sh) + c];
                const float gx = prior_x[j] + tx, gz = prior_z[j] + tz, gy = (prior_y[j] + tx) + tz;
                const unsigned E = pauli_decide(gx, gy, gz);
                ox[j] = (uint8_t)(E & 1u);
                oz[j] = (uint8_t)(E >> 1);
                if (lo) {
                    lo[j] = (double)gx;
                    lo[(size_t)n + j] = (double)gy;
                    lo[(size_t)2 * n + j] = (double)gz;
                }
            }
        }
        if (q == 0 && l < valid) {
            p.conv[col0 + l] = (uint8_t)my_conv;
            if (p.iters) p.iters[col0 + l] = my_iters;
        }
        __syncthreads();
    }
}

}  // namespace ldpc
