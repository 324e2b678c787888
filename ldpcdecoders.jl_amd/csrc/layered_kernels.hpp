// layered_kernels.hpp -- device code of the LAYERED schedule of the normalised min-sum decoder (THE LAYERED RULE of
// include/ldpc_mi355x.h, the ldpc_minsum_* section; host side: ldpc_minsum.hip, the layers: layer_plan.hpp).  Binary32
// throughout, one rounding per operation, no contraction.
//
// The mapping and the state of a tile are those of minsum_kernels.hpp: a syndrome in a lane, thread t works for syndrome
// t % S; L [n][S], the check records rec [rec_words][S] in the same three forms, syn [s][S]; GLOBAL = false keeps the state
// in the workgroup's dynamic LDS, GLOBAL = true in a slot of a global workspace (S = 64).  What differs is the sweep:
//
// "Serial over the checks" is serial inside a lane.  The threads that share a lane work side by side on checks that share
// no bit -- a LAYER (first fit, layer_plan.hpp; create verifies the property before the upload, a slip would be a data
// race here).  In layer l thread t takes the checks layer_checks[layer_ptr[l] + t / S + m (T / S)], m = 0, 1, ...; one
// workgroup barrier follows every layer.  A check's new messages are known only after its minima, so its L write-back is a
// second pass over its bits that forms b_k once more from L and the OLD record: up to degree 64 the old record stays in
// registers (o1, o2, oa and the sign words) while the new one is stored; in the per-edge form the old message word is read
// before it is overwritten.  There is no bit sweep: L[j_k] = b_k + new c[i][j_k].
//
// The stop test is a pass of its own after the last layer (L moves inside a sweep, so it cannot ride on the next one):
// each thread XORs (L <= 0) over its share of ALL checks against the syndrome byte; an empty check only compares its
// entry.  A syndrome that has stopped is frozen.  An iteration has K + 2 barriers.  Layers of fewer than T / S checks
// leave thread groups idle.
#pragma once
#include "minsum_kernels.hpp"

namespace ldpc {

struct LayeredParams {
    MsParams ms;
    int K;                        // layers
    const int *layer_ptr;         // [K + 1]
    const int *layer_checks;      // [layer_ptr[K]]: the non-empty checks, layer by layer
};
struct LayeredPriorsParams : LayeredParams {   // (the table instantiations keep LayeredParams as their argument)
    MsPriorSource src;
};
template <int SRC> struct LayeredParamsOf { typedef LayeredPriorsParams type; };
template <> struct LayeredParamsOf<kMsPriorTable> { typedef LayeredParams type; };

// SRC (minsum_kernels.hpp): per-syndrome priors are read only here, when a tile starts, so they are staged straight into L
// and the state of a tile is the same for every SRC.
template <int TW, bool GLOBAL, int SRC = kMsPriorTable>
__global__ __launch_bounds__(TW * 64) void layered_minsum_kernel(typename LayeredParamsOf<SRC>::type lp)
{
    constexpr int T = TW * 64;
    constexpr bool STAGED = SRC != kMsPriorTable;
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    __shared__ int sh_bad[STAGED ? 128 : 64];   // STAGED: [64 + c] = column c of the tile holds a non-finite prior
    const MsParams &p = lp.ms;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, s = p.s, K = lp.K;
    const float alpha = p.alpha, clip = p.clip;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = ms_lds;
    float *L = (float *)base;
    unsigned *R = (unsigned *)base + ((size_t)n << sh);
    unsigned char *Y = base + (((size_t)n + (size_t)p.rec_words) << sh) * 4;
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ layer_ptr = lp.layer_ptr, *__restrict__ layer_checks = lp.layer_checks;
    const float *__restrict__ prior = p.prior;
    const long long tiles = (p.batch + S - 1) >> sh;

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long col0 = tile << sh;
        const int valid = (int)((p.batch - col0) < (long long)S ? (p.batch - col0) : (long long)S);
        // ---- state of iteration 0: L = channel_llr, every message +0; the syndromes, a wave per column
        if constexpr (!STAGED)
            for (int j = q; j < n; j += Q) L[((size_t)j << sh) + l] = prior[j];
        for (int w = q; w < p.rec_words; w += Q) R[((size_t)w << sh) + l] = 0u;
        for (int c = wave; c < S; c += TW) {
            if (c < valid) {
                const uint8_t *src = p.syn + (col0 + c) * s;
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = src[i] != 0;
                if constexpr (STAGED) {   // ... and the column's priors, all of L[.][c]
                    const bool skip = ms_stage_priors<SRC>(lp.src, col0 + c, n, lane, [&](int j, float v) { L[((size_t)j << sh) + c] = v; });
                    if (lane == 0) sh_bad[64 + c] = skip;
                }
            } else {   // a lane past the batch reads nothing and never becomes active
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = 0;
                if constexpr (STAGED)
                    for (int j = lane; j < n; j += 64) L[((size_t)j << sh) + c] = 0.0f;
            }
        }
        if (t < 64) sh_bad[t] = 0;
        bool active = l < valid;
        int my_iters = p.max_iters, my_conv = 0;
        __syncthreads();
        if constexpr (STAGED) {
            if (active && sh_bad[64 + l]) {   // a column with a non-finite prior stays out
                active = false;
                my_iters = 0;
            }
        }

        for (int it = 1; it <= p.max_iters; ++it) {
            // ---- the layers in order; the checks of a layer share no bit
            for (int ly = 0; ly < K; ++ly) {
                if (active) {
                    const int qe = layer_ptr[ly + 1];
                    for (int qi = layer_ptr[ly] + q; qi < qe; qi += Q) {
                        const int i = layer_checks[qi];
                        const int ra = row_ptr[i], deg = row_ptr[i + 1] - ra;   // >= 1: an empty check is in no layer
                        // (a writer of the record forms of its own, next to ms_check_update of minsum_kernels.hpp: the write-back needs
                        // the old and the new record in registers at once, and the per-edge form fuses its store with L = b + c)
                        unsigned *rec = R + ((size_t)rec_off[i] << sh) + l;
                        float m1 = clip, m2 = clip;
                        unsigned a = kMsNone, par = Y[((size_t)i << sh) + l];
                        if (deg <= 64) {
                            const float o1 = __uint_as_float(rec[0]), o2 = __uint_as_float(rec[(size_t)1 << sh]);
                            const unsigned oa = rec[(size_t)2 << sh];
                            const unsigned og_lo = rec[(size_t)3 << sh], og_hi = deg > 32 ? rec[(size_t)4 << sh] : 0u;
                            unsigned neg_lo = 0, neg_hi = 0;
                            const int d0 = deg < 32 ? deg : 32;
                            for (int k = 0; k < d0; ++k) {
                                const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float c = (og_lo >> k) & 1u ? -cm : cm;
                                const float b = ms_clamp(Lj - c, clip);
                                const unsigned ng = b < 0.0f;
                                const float mag = fabsf(b);
                                neg_lo |= ng << k;
                                par ^= ng;
                                if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                                else if (mag < m2) m2 = mag;
                            }
                            for (int k = 32; k < deg; ++k) {
                                const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float c = (og_hi >> (k - 32)) & 1u ? -cm : cm;
                                const float b = ms_clamp(Lj - c, clip);
                                const unsigned ng = b < 0.0f;
                                const float mag = fabsf(b);
                                neg_hi |= ng << (k - 32);
                                par ^= ng;
                                if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                                else if (mag < m2) m2 = mag;
                            }
                            const unsigned flip = par ? 0xffffffffu : 0u;   // negative iff par XOR neg_k
                            const float n1 = alpha * m1, n2 = alpha * m2;
                            const unsigned ng_lo = (neg_lo ^ flip) & (d0 == 32 ? 0xffffffffu : (1u << d0) - 1u);
                            const unsigned ng_hi = deg > 32 ? (neg_hi ^ flip) & (deg == 64 ? 0xffffffffu : (1u << (deg - 32)) - 1u) : 0u;
                            rec[0] = __float_as_uint(n1);
                            rec[(size_t)1 << sh] = __float_as_uint(n2);
                            rec[(size_t)2 << sh] = a;
                            rec[(size_t)3 << sh] = ng_lo;
                            if (deg > 32) rec[(size_t)4 << sh] = ng_hi;
                            // the write-back: b_k once more from L and the old record, then L = b_k + the new message
                            for (int k = 0; k < d0; ++k) {
                                float *Lp = L + ((size_t)csr_col[ra + k] << sh) + l;
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float c = (og_lo >> k) & 1u ? -cm : cm;
                                const float b = ms_clamp(*Lp - c, clip);
                                const float nm = (unsigned)k == a ? n2 : n1;
                                *Lp = b + ((ng_lo >> k) & 1u ? -nm : nm);
                            }
                            for (int k = 32; k < deg; ++k) {
                                float *Lp = L + ((size_t)csr_col[ra + k] << sh) + l;
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float c = (og_hi >> (k - 32)) & 1u ? -cm : cm;
                                const float b = ms_clamp(*Lp - c, clip);
                                const float nm = (unsigned)k == a ? n2 : n1;
                                *Lp = b + ((ng_hi >> (k - 32)) & 1u ? -nm : nm);
                            }
                        } else {
                            // per-edge record: the minima first, then every edge's b once more for its message and its L
                            for (int k = 0; k < deg; ++k) {
                                const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                                const float b = ms_clamp(Lj - __uint_as_float(rec[(size_t)k << sh]), clip);
                                const float mag = fabsf(b);
                                par ^= (unsigned)(b < 0.0f);
                                if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                                else if (mag < m2) m2 = mag;
                            }
                            const float n1 = alpha * m1, n2 = alpha * m2;
                            for (int k = 0; k < deg; ++k) {
                                float *Lp = L + ((size_t)csr_col[ra + k] << sh) + l;
                                const float old = __uint_as_float(rec[(size_t)k << sh]);   // read before it is overwritten
                                const float b = ms_clamp(*Lp - old, clip);
                                const float nm = (unsigned)k == a ? n2 : n1;
                                const float c = (par ^ (unsigned)(b < 0.0f)) ? -nm : nm;
                                rec[(size_t)k << sh] = __float_as_uint(c);
                                *Lp = b + c;
                            }
                        }
                    }
                }
                __syncthreads();
            }
            // ---- the stop test: H * err == syndrome on the L the last layer left
            if (active) {
                int bad = 0;
                for (int i = q; i < s; i += Q) {
                    const int ra = row_ptr[i], rb = row_ptr[i + 1];
                    unsigned hard = Y[((size_t)i << sh) + l];   // an empty check is matched only by a 0 entry
                    for (int e = ra; e < rb; ++e) hard ^= (unsigned)(L[((size_t)csr_col[e] << sh) + l] <= 0.0f);
                    bad |= (int)hard;
                }
                if (bad) sh_bad[l] = 1;
            }
            __syncthreads();
            if (active && !sh_bad[l]) {
                active = false;
                my_conv = 1;
                my_iters = it;
            }
            const int any = __syncthreads_or(active);
            if (t < 64) sh_bad[t] = 0;
            if (!any) break;
            if (K == 0) __syncthreads();   // no layer barrier stands between this reset and the next test's flags
        }

        // ---- results, a wave per column: err = (L <= 0), llr = L widened
        for (int c = wave; c < valid; c += TW) {
            uint8_t *eo = p.err + (col0 + c) * n;
            double *lo = p.llr ? p.llr + (col0 + c) * n : nullptr;
            if constexpr (STAGED) {
                if (sh_bad[64 + c]) {   // not decoded: what max_iters = 0 writes
                    for (int j = lane; j < n; j += 64) {
                        eo[j] = 0;
                        if (lo) lo[j] = 0.0;
                    }
                    continue;
                }
            }
            for (int j = lane; j < n; j += 64) {
                const float v = L[((size_t)j << sh) + c];
                eo[j] = v <= 0.0f;
                if (lo) lo[j] = (double)v;
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
