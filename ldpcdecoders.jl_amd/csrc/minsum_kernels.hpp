// minsum_kernels.hpp -- device code of the normalised min-sum decoder (ldpc_minsum_* of include/ldpc_mi355x.h, where the
// rule is stated; host side: ldpc_minsum.hip).  Binary32 throughout, one rounding per operation, no contraction.
//
// A SYNDROME IN A LANE, as in the sum-product kernels: a workgroup decodes a tile of S syndromes (S a power of two,
// <= 64); thread t works for syndrome t % S and takes the nodes t / S, t / S + T / S, ... of each sweep.  With S = 64 a
// wave's lanes are the 64 syndromes of the tile and its nodes are wave-uniform.
//
// State of a tile, every row S words wide so that the lanes of a wave read one contiguous row:
//   L    [n][S]          f32  the posterior LLRs
//   rec  [rec_words][S]  u32  the check-to-bit messages, one record per check at rec_off[i]:
//          degree 1..32    m1a, m2a, a, signs              (4 words)
//          degree 33..64   m1a, m2a, a, signs lo, signs hi (5 words)
//          degree > 64     one f32 message per edge        (the per-edge fallback)
//        m1a = alpha * m1, m2a = alpha * m2; a = position of the smallest magnitude in the check (kMsNone: none was
//        below clip); bit k of signs: the message to the check's k-th bit is negative.  The message to bit k is
//        (k == a ? m2a : m1a) with that sign -- what the rule's step 1 defines.  All-zero words are the initial +0.
//   syn  [s][S]          u8   the syndrome entries as 0 / 1
//   P    [n][S]          f32  only with per-syndrome priors (SRC below): the tile's priors, on the next word boundary
// GLOBAL = false: the state is the workgroup's dynamic LDS and stays there for the whole decode.  GLOBAL = true: a slot
// of a global workspace per workgroup of the persistent grid (S = 64); same code.
//
// The stop test of iteration t (H * err == syndrome on the L of bit sweep t) rides on check sweep t + 1, which reads
// every L of every check anyway; a last sweep that only tests follows bit sweep max_iters.  A syndrome that has stopped
// is frozen: its L is not written again (what its records hold no longer matters).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_plan.hpp"

namespace ldpc {

constexpr unsigned kMsNone = 0xffffffffu;
// (kMsPosEdge, the flag in edge_pos of a check that keeps one message per edge: tile_plan.hpp, with the host code that sets it)

struct MsParams {
    int s, n, max_iters;
    int S, shift;                 // syndromes per tile, S = 1 << shift
    long long batch;
    float alpha, clip;
    const uint8_t *syn;           // [batch][s]
    uint8_t *err, *conv;          // [batch][n], [batch]
    double *llr;                  // [batch][n] or NULL
    int32_t *iters;               // [batch] or NULL
    const float *prior;           // [n]
    const int *row_ptr, *csr_col; // checks -> bits, ascending
    const int *rec_off;           // [s]: first word of the check's record
    const int *col_ptr;           // bits -> edges in ascending check order
    const int *edge_rec;          // per CSC edge: rec_off of its check
    const int *edge_pos;          // per CSC edge: position of the bit in its check (| kMsPosEdge: per-edge record)
    int rec_words;
    unsigned char *ws;            // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

// (ms_record_words(), ms_state_bytes() -- the words of a check record, the bytes of a tile's state: tile_plan.hpp, host code)

// Where a syndrome's prior comes from (the third template argument of both kernels).  kMsPriorTable: prior[n] of the
// handle, shared by the batch -- the plain entries.  The other two are the per-syndrome priors of the header:
// kMsPriorFloats reads priors [batch][n] f32, kMsPriorGiven forms (given[i][j] & 1) ? llr_if1[j] : llr_if0[j] from
// given [batch][n] u8.  Both are staged once per tile, a wave per column with its lanes along j (a coalesced read, every
// float or byte read once): into a fourth block P [n][S] f32 behind syn (at ms_priors_offset(), tile_plan.hpp) in the
// flooding kernel, whose bit sweep reads the prior again in every iteration, and straight into L in the layered one.  A
// column in which the staging meets a non-finite prior never becomes active and is written out as zeros.
constexpr int kMsPriorTable = 0, kMsPriorFloats = 1, kMsPriorGiven = 2;

struct MsPriorSource {
    const float *priors;            // kMsPriorFloats: [batch][n]
    const uint8_t *given;           // kMsPriorGiven: [batch][n]
    const float *llr_if0, *llr_if1; // kMsPriorGiven: [n] each
};
struct MsPriorsParams : MsParams {   // (the table instantiations keep MsParams as their argument)
    MsPriorSource src;
};
template <int SRC> struct MsParamsOf { typedef MsPriorsParams type; };
template <> struct MsParamsOf<kMsPriorTable> { typedef MsParams type; };

// One column's priors, lanes along j: store(j, value) for every bit; true in every lane if one of them is not finite.
template <int SRC, class Store>
__device__ inline bool ms_stage_priors(const MsPriorSource &src, long long column, int n, int lane, Store store)
{
    static_assert(SRC == kMsPriorFloats || SRC == kMsPriorGiven, "the table is not staged");
    int bad = 0;
    for (int j = lane; j < n; j += 64) {
        float v;
        if constexpr (SRC == kMsPriorFloats) v = src.priors[column * n + j];
        else v = (src.given[column * n + j] & 1) ? src.llr_if1[j] : src.llr_if0[j];
        bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;   // infinity or NaN
        store(j, v);
    }
    return __any(bad) != 0;
}

__device__ inline float ms_clamp(float x, float clip)
{
    x = x < -clip ? -clip : x;    // max(x, -clip)
    return x > clip ? clip : x;   // min(., clip)
}

// The message of a bit's edge out of its check's record (rec: the record's first word in the bit's lane; k: edge_pos): the
// one reader of the record forms in the bit sweeps of the flooding, relay and Pauli kernels.
__device__ inline float ms_message(const unsigned *rec, int k, int sh)
{
    if (k < 0) return __uint_as_float(rec[(size_t)(k & 0x7fffffff) << sh]);
    const unsigned a = rec[(size_t)2 << sh];
    const float cm = __uint_as_float(rec[(size_t)((unsigned)k == a ? 1 : 0) << sh]);
    const unsigned sg = rec[(size_t)(3 + (k >> 5)) << sh];
    return (sg >> (k & 31)) & 1u ? -cm : cm;
}

// The update of one check's record in the thread's lane (rec: the record's first word there): the minima and the parity
// (from the syndrome entry y) of the check's b_k, then, if `write`, the new record -- the writer of the record forms in
// decim_kernel and pauli_relay_kernel.  minsum_kernel below, relay_kernel and pauli_minsum_kernel keep the same text inline:
// with this function each had a probe row beyond the parent's spread (profiles/check_update_refactor_probe.txt), and
// layered_minsum_kernel needs the old and the new record at once.  A fix to a record form is made here and in those four.
// `fresh`: the old record reads as all-zero words.  edge(k, c, test) is the kernel's part: the clamped b_k of the check's
// k-th bit against its old message c; where `test` it also folds the bit's hard decision into the caller's stop test (the
// per-edge form forms every b_k twice and tests once).  A strict < in the minima: a tie keeps the earlier position.
template <class Edge>
__device__ inline void ms_check_update(unsigned *rec, int deg, int sh, float alpha, float clip, unsigned y, bool fresh, bool write, Edge edge)
{
    float m1 = clip, m2 = clip;
    unsigned a = kMsNone, par = y;
    auto least = [&](int k, float mag) {
        if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
        else if (mag < m2) m2 = mag;
    };
    if (deg <= 64) {
        const float o1 = fresh ? 0.0f : __uint_as_float(rec[0]), o2 = fresh ? 0.0f : __uint_as_float(rec[(size_t)1 << sh]);
        const unsigned oa = rec[(size_t)2 << sh];
        // the edges k0 .. k1 - 1 against their old sign word sg; their new sign bits before the parity is known
        auto word = [&](int k0, int k1, unsigned sg) -> unsigned {
            unsigned neg = 0;
            for (int k = k0; k < k1; ++k) {
                const float cm = (unsigned)k == oa ? o2 : o1;
                const float b = edge(k, (sg >> (k - k0)) & 1u ? -cm : cm, true);
                const unsigned ng = b < 0.0f;
                neg |= ng << (k - k0);
                par ^= ng;
                least(k, fabsf(b));
            }
            return neg;
        };
        const int d0 = deg < 32 ? deg : 32;
        const unsigned neg_lo = word(0, d0, fresh ? 0u : rec[(size_t)3 << sh]);
        const unsigned neg_hi = deg > 32 ? word(32, deg, fresh ? 0u : rec[(size_t)4 << sh]) : 0u;
        if (write) {
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
            const float b = edge(k, fresh ? 0.0f : __uint_as_float(rec[(size_t)k << sh]), true);
            par ^= (unsigned)(b < 0.0f);
            least(k, fabsf(b));
        }
        if (write) {
            const float n1 = alpha * m1, n2 = alpha * m2;
            for (int k = 0; k < deg; ++k) {
                const float b = edge(k, fresh ? 0.0f : __uint_as_float(rec[(size_t)k << sh]), false);
                const float cm = (unsigned)k == a ? n2 : n1;
                rec[(size_t)k << sh] = __float_as_uint((par ^ (unsigned)(b < 0.0f)) ? -cm : cm);
            }
        }
    }
}

// The syndromes of a tile into Y [s][S], a wave per column with its lanes along the checks: entry(c, i) is entry i of the
// tile's column c.  A lane past the batch reads nothing, gets zeros and never becomes active.
template <int TW, class Entry>
__device__ inline void ms_stage_syndromes(unsigned char *Y, int s, int S, int sh, int valid, int wave, int lane, Entry entry)
{
    for (int c = wave; c < S; c += TW) {
        if (c < valid)
            for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = entry(c, i) != 0;
        else
            for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = 0;
    }
}

// The plain results of a tile, a wave per column: err = (L <= 0), llr = L widened (err, llr: at the tile's first column,
// llr may be null).
template <int TW>
__device__ inline void ms_write_results(const float *L, int n, int sh, int valid, int wave, int lane, uint8_t *err, double *llr)
{
    for (int c = wave; c < valid; c += TW) {
        uint8_t *eo = err + (long long)c * n;
        double *lo = llr ? llr + (long long)c * n : nullptr;
        for (int j = lane; j < n; j += 64) {
            const float v = L[((size_t)j << sh) + c];
            eo[j] = v <= 0.0f;
            if (lo) lo[j] = (double)v;
        }
    }
}

template <int TW, bool GLOBAL, int SRC = kMsPriorTable>
__global__ __launch_bounds__(TW * 64) void minsum_kernel(typename MsParamsOf<SRC>::type kp)
{
    constexpr int T = TW * 64;
    constexpr bool STAGED = SRC != kMsPriorTable;
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    __shared__ int sh_bad[STAGED ? 128 : 64];   // STAGED: [64 + c] = column c of the tile holds a non-finite prior
    const MsParams &p = kp;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = p.S, sh = p.shift, l = t & (S - 1), q = t >> sh, Q = T >> sh;
    const int n = p.n, s = p.s;
    const float alpha = p.alpha, clip = p.clip;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = ms_lds;
    float *L = (float *)base;
    unsigned *R = (unsigned *)base + ((size_t)n << sh);
    unsigned char *Y = base + (((size_t)n + (size_t)p.rec_words) << sh) * 4;
    float *P = nullptr;   // STAGED: the tile's priors [n][S]
    if constexpr (STAGED) P = (float *)(base + ((((((size_t)n + (size_t)p.rec_words) << sh) * 4 + ((size_t)s << sh)) + 3) & ~(size_t)3));
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col, *__restrict__ rec_off = p.rec_off;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ edge_rec = p.edge_rec, *__restrict__ edge_pos = p.edge_pos;
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
                if constexpr (STAGED) {   // ... and the column's priors, all of P[.][c] anew
                    const bool skip = ms_stage_priors<SRC>(kp.src, col0 + c, n, lane, [&](int j, float v) { P[((size_t)j << sh) + c] = v; });
                    if (lane == 0) sh_bad[64 + c] = skip;
                }
            } else {   // a lane past the batch reads nothing and never becomes active
                for (int i = lane; i < s; i += 64) Y[((size_t)i << sh) + c] = 0;
                if constexpr (STAGED)
                    for (int j = lane; j < n; j += 64) P[((size_t)j << sh) + c] = 0.0f;
            }
        }
        if (t < 64) sh_bad[t] = 0;
        bool active = l < valid;
        int my_iters = p.max_iters, my_conv = 0;
        __syncthreads();
        if constexpr (STAGED) {   // L = the staged priors, rows along the lanes; a column with a non-finite one stays out
            for (int j = q; j < n; j += Q) L[((size_t)j << sh) + l] = P[((size_t)j << sh) + l];
            if (active && sh_bad[64 + l]) {
                active = false;
                my_iters = 0;
            }
            __syncthreads();
        }

        for (int it = 1;; ++it) {
            const bool test_only = it > p.max_iters;
            // ---- check sweep `it`, and H * err == syndrome on the L it reads (the stop test of iteration it - 1)
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
                        const float o1 = __uint_as_float(rec[0]), o2 = __uint_as_float(rec[(size_t)1 << sh]);
                        const unsigned oa = rec[(size_t)2 << sh];
                        unsigned sg = rec[(size_t)3 << sh], neg_lo = 0, neg_hi = 0;
                        const int d0 = deg < 32 ? deg : 32;
                        for (int k = 0; k < d0; ++k) {
                            const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                            hard ^= (unsigned)(Lj <= 0.0f);
                            const float cm = (unsigned)k == oa ? o2 : o1;
                            const float c = (sg >> k) & 1u ? -cm : cm;
                            const float b = ms_clamp(Lj - c, clip);
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
                                const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                                hard ^= (unsigned)(Lj <= 0.0f);
                                const float cm = (unsigned)k == oa ? o2 : o1;
                                const float c = (sg >> (k - 32)) & 1u ? -cm : cm;
                                const float b = ms_clamp(Lj - c, clip);
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
                            const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                            hard ^= (unsigned)(Lj <= 0.0f);
                            const float b = ms_clamp(Lj - __uint_as_float(rec[(size_t)k << sh]), clip);
                            const float mag = fabsf(b);
                            par ^= (unsigned)(b < 0.0f);
                            if (mag < m1) { m2 = m1; m1 = mag; a = (unsigned)k; }
                            else if (mag < m2) m2 = mag;
                        }
                        if (!test_only) {
                            const float n1 = alpha * m1, n2 = alpha * m2;
                            for (int k = 0; k < deg; ++k) {
                                const float Lj = L[((size_t)csr_col[ra + k] << sh) + l];
                                const float b = ms_clamp(Lj - __uint_as_float(rec[(size_t)k << sh]), clip);
                                const float cm = (unsigned)k == a ? n2 : n1;
                                rec[(size_t)k << sh] = __float_as_uint((par ^ (unsigned)(b < 0.0f)) ? -cm : cm);
                            }
                        }
                    }
                    bad |= (int)(hard ^ y);
                }
                if (bad) sh_bad[l] = 1;
            }
            __syncthreads();
            if (active && it > 1 && !sh_bad[l]) {   // the L of bit sweep it - 1 reproduces the syndrome
                active = false;
                my_conv = 1;
                my_iters = it - 1;
            }
            const int any = __syncthreads_or(active);
            if (t < 64) sh_bad[t] = 0;
            if (!any || test_only) break;
            // ---- bit sweep `it`: channel_llr plus the messages in ascending check order
            if (active) {
                for (int j = q; j < n; j += Q) {
                    float acc;
                    if constexpr (STAGED) acc = P[((size_t)j << sh) + l];
                    else acc = prior[j];
                    const int eb = col_ptr[j + 1];
                    for (int e = col_ptr[j]; e < eb; ++e) {
                        acc = acc + ms_message(R + ((size_t)edge_rec[e] << sh) + l, edge_pos[e], sh);
                    }
                    L[((size_t)j << sh) + l] = acc;
                }
            }
            __syncthreads();
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
