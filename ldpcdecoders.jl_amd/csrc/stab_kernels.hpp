// stab_kernels.hpp -- device code of the joint Pauli min-sum decoder of a general (non-CSS) stabilizer code
// (ldpc_stab_minsum_* of include/ldpc_mi355x_stab.h, where the rule is stated; host side: ldpc_stab.hip).  Binary32
// throughout, one rounding per operation, no contraction.
//
// The design of pauli_minsum_kernel (pauli_kernels.hpp): A SYNDROME IN A LANE, a workgroup decodes a tile of S syndromes (S
// a power of two, <= 64); thread t works for syndrome t % S and takes the nodes t / S, t / S + T / S, ... of each sweep.
// One graph of r checks over the n qubits: edge (i, j) where stabilizer i has X, Y or Z on qubit j, and that Pauli is the
// edge's TYPE, two bits: bit 0 = the stabilizer has an X part there (X or Y), bit 1 = a Z part (Z or Y); so 1 = X, 2 = Z,
// 3 = Y.  The type is graph data and costs no load of its own: it rides in bits 28 .. 29 of the word the sweep reads
// anyway -- csr_col in the check sweep, edge_pos in the bit sweep (qubits and positions stay below 2^28; bit 31 of edge_pos
// is kMsPosEdge).
//
// State of a tile, every row S words wide:
//   MX, MY, MZ [3 n][S]       f32  per qubit the sum of the messages of its X-, Y- and Z-type edges
//   rec        [rec_words][S] u32  the check-to-qubit messages, one record per check, in the three forms of
//                                  ms_record_words() (tile_plan.hpp; what the words hold: minsum_kernels.hpp)
//   syn        [r][S]         u8   the syndrome entries as 0 / 1
// The three beliefs of a qubit are not kept: GX = (prior_x + MZ) + MY, GY = (prior_y + MZ) + MX, GZ = (prior_z + MX) + MY
// are formed wherever they are read.  GLOBAL = false: the state is the workgroup's dynamic LDS.  GLOBAL = true: a slot of a
// global workspace per workgroup of the persistent grid (S = 64); same code.
//
// With S < 64 the lanes of one wave work on different checks, so on edges of different types: the operands of u and w are
// SELECTED by the type (conditional moves), never branched on.  The bit sweep walks a qubit's edges once, in ascending
// check order, and adds each message into the total its type selects -- per total that is the order the rule states.
//
// The stop test of iteration t rides on check sweep t + 1: that sweep loads the three totals of each of its qubits anyway,
// forms the three G and with them the decision of the rule; an edge XORs in whether that decision anticommutes with its
// type.  A last sweep that only tests follows bit sweep max_iters.  A syndrome that has stopped is frozen: its totals are
// not written again.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minsum_kernels.hpp"   // ms_clamp, ms_message, kMsNone
#include "pauli_kernels.hpp"    // pauli_decide

namespace ldpc {

constexpr int kStabTypeShift = 28;                    // the edge type in csr_col and edge_pos
constexpr int kStabIndexMask = (1 << kStabTypeShift) - 1;
constexpr int kStabTypeMask = 3 << kStabTypeShift;

struct StabParams {
    int r, n, max_iters;
    int S, shift;                 // syndromes per tile, S = 1 << shift
    long long batch;
    float alpha, clip;
    const uint8_t *syn;           // [batch][r]
    uint8_t *gx, *gz, *conv;      // [batch][n], [batch][n], [batch]
    double *llr;                  // [batch][3][n] or NULL
    int32_t *iters;               // [batch] or NULL
    const float *prior_x, *prior_y, *prior_z;   // [n] each
    const int *row_ptr, *csr_col; // checks -> qubits, ascending; csr_col = qubit | type << 28
    const int *rec_off;           // [r]: first word of the check's record
    const int *col_ptr;           // qubits -> edges in ascending check order
    const int *edge_rec;          // per CSC edge: rec_off of its check
    const int *edge_pos;          // per CSC edge: position of the qubit in its check (| kMsPosEdge: per-edge record) | type << 28
    int rec_words;
    unsigned char *ws;            // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void stab_minsum_kernel(StabParams p)
{
    constexpr int T = TW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char stab_lds[];
    __shared__ int sh_bad[64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, r = p.r;
    const float alpha = p.alpha, clip = p.clip;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = stab_lds;
    float *MX = (float *)base;
    float *MY = MX + ((size_t)n << sh);
    float *MZ = MY + ((size_t)n << sh);
    unsigned *R = (unsigned *)base + ((size_t)3 * n << sh);
    unsigned char *Y = base + (((size_t)3 * n + (size_t)p.rec_words) << sh) * 4;
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ edge_rec = p.edge_rec, *__restrict__ edge_pos = p.edge_pos;
    const float *__restrict__ prior_x = p.prior_x, *__restrict__ prior_y = p.prior_y, *__restrict__ prior_z = p.prior_z;
    const long long tiles = (p.batch + S - 1) >> sh;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long col0 = tile << sh;
        const int valid = (int)((p.batch - col0) < (long long)S ? (p.batch - col0) : (long long)S);
        // ---- state of iteration 0: the totals +0 and every message +0 (all-zero words); the syndromes, a wave per column
        for (int w = q; w < 3 * n + p.rec_words; w += Q) ((unsigned *)base)[((size_t)w << sh) + l] = 0u;   // MX, MY, MZ, rec: one block
        for (int c = wave; c < S; c += TW) {
            if (c < valid) {
                const uint8_t *a = p.syn + (col0 + c) * r;
                for (int i = lane; i < r; i += 64) Y[((size_t)i << sh) + c] = a[i] != 0;
            } else {   // a lane past the batch reads nothing and never becomes active
                for (int i = lane; i < r; i += 64) Y[((size_t)i << sh) + c] = 0;
            }
        }
        if (t < 64) sh_bad[t] = 0;
        bool active = l < valid;
        int my_iters = p.max_iters, my_conv = 0;
        __syncthreads();

        for (int it = 1;; ++it) {
            const bool test_only = it > p.max_iters;
            // ---- check sweep `it`, and the stop test of iteration it - 1 on the totals it reads
            if (active) {
                int bad = 0;
                for (int i = q; i < r; i += Q) {
                    const int ra = row_ptr[i], deg = row_ptr[i + 1] - ra;
                    const unsigned y = Y[((size_t)i << sh) + l];
                    if (deg == 0) {   // an empty check sends nothing and is matched only by a 0 entry
                        bad |= (int)y;
                        continue;
                    }
                    unsigned hard = 0;
                    // b_k of the check's k-th qubit against its old message c; whether the qubit's decision anticommutes with
                    // the edge's Pauli goes into `hard`.  Everything by type is a select.
                    auto edge = [&](int k, float c) -> float {
                        const int jt = csr_col[ra + k], j = jt & kStabIndexMask;
                        const unsigned ty = (unsigned)jt >> kStabTypeShift;
                        const float mx = MX[((size_t)j << sh) + l], my = MY[((size_t)j << sh) + l], mz = MZ[((size_t)j << sh) + l];
                        const float gx = (prior_x[j] + mz) + my, gy = (prior_y[j] + mz) + mx, gz = (prior_z[j] + mx) + my;
                        const unsigned E = pauli_decide(gx, gy, gz);
                        hard ^= ((E & 1u) & (ty >> 1)) ^ ((E >> 1) & (ty & 1u));   // ex where the edge has a Z part, ez where an X part
                        const float ua = ty == 3u ? gx : gy, ub = ty == 2u ? gx : gz;   // X: (GY, GZ)  Z: (GY, GX)  Y: (GX, GZ)
                        const float other = ty == 1u ? gx : ty == 2u ? gz : gy;
                        const float u = ua < ub ? ua : ub;
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
            if (active && it > 1 && !sh_bad[l]) {   // the decision of bit sweep it - 1 reproduces the syndrome
                active = false;
                my_conv = 1;
                my_iters = it - 1;
            }
            const int any = __syncthreads_or(active);
            if (t < 64) sh_bad[t] = 0;
            if (!any || test_only) break;
            // ---- bit sweep `it`: one walk over the qubit's edges in ascending check order, each message into its type's total
            if (active) {
                for (int j = q; j < n; j += Q) {
                    const int ea = col_ptr[j], eb = col_ptr[j + 1];
                    float mx = 0.0f, my = 0.0f, mz = 0.0f;
                    for (int e = ea; e < eb; ++e) {
                        const int pt = edge_pos[e];
                        const unsigned ty = ((unsigned)pt >> kStabTypeShift) & 3u;
                        const float m = ms_message(R + ((size_t)edge_rec[e] << sh) + l, pt & ~kStabTypeMask, sh);
                        const float sx = mx + m, sy = my + m, sz = mz + m;
                        mx = ty == 1u ? sx : mx;
                        my = ty == 3u ? sy : my;
                        mz = ty == 2u ? sz : mz;
                    }
                    MX[((size_t)j << sh) + l] = mx;
                    MY[((size_t)j << sh) + l] = my;
                    MZ[((size_t)j << sh) + l] = mz;
                }
            }
            __syncthreads();
        }

        // ---- results, a wave per column: the decision on the final totals; llr = the planes GX, GY, GZ widened
        for (int c = wave; c < valid; c += TW) {
            uint8_t *ox = p.gx + (col0 + c) * n, *oz = p.gz + (col0 + c) * n;
            double *lo = p.llr ? p.llr + (col0 + c) * 3 * n : nullptr;
            for (int j = lane; j < n; j += 64) {
                const float mx = MX[((size_t)j << sh) + c], my = MY[((size_t)j << sh) + c], mz = MZ[((size_t)j << sh) + c];
                const float gx = (prior_x[j] + mz) + my, gy = (prior_y[j] + mz) + mx, gz = (prior_z[j] + mx) + my;
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
