// osd_kernels.hpp -- device code of the opt-in device form of the BP+OSD ordered-statistics step
// (ldpc_osd_device_prepare / ldpc_osd_postprocess_batch_device of include/ldpc_mi355x.h; host side:
// ldpc_osd_device.hip).  Replaces belief_propagation_osd.jl:52-60 and osd (:63-125 order 0, :127-209 order > 0)
// for a batch, like osd_host.cpp, but with the mechanics the algebra allows on a GPU.
//
// ONE WORKGROUP OF TW WAVES PER SYNDROME, THREAD = ROW.  Thread t owns the rows t, t + 64 TW, ...; the working rows are
// 64-bit packed in the ORIGINAL column order, `st` words apart (st = nw + 1 made odd: word nw carries the syndrome bit of
// the row along, and an odd stride keeps the lanes of a wave, which all test the same column of their own rows, on
// different LDS banks).
//
//   keys       p = pm_exp(llr) (portable_math.h: the same bits on host and device), key = p > 1-p ? p : 1-p.  Keys are
//              doubles >= 0.5, so their bit patterns order like unsigned integers; a NaN key becomes 0 and so orders
//              LAST, among the NaNs by ascending index.  The order is (key descending, index ascending): rank by counting.
//   elimination  columns in that order.  The result of OSD does not depend on WHICH row serves as the pivot of a column
//              (the pivot COLUMNS are the greedy independent set in reliability order, the solved bits are unique), so
//              there are no row swaps: the pivot of a column is the lowest row not yet used that has the bit (one ballot
//              per wave, one atomicMin per workgroup), and it is XORed into EVERY other row that has the bit
//              (Gauss-Jordan: a thread only ever writes its own rows, and no back-substitution / diagonalisation pass
//              remains).  One barrier per column: the pivot slot is one of three that rotate.
//   order 0    the syndrome bit carried along is the RESIDUAL syn + H bp_err; all zero -> the output is the BP estimate
//              (:72-74).  The loop stops as soon as no unused row has its residual bit set (:82: the residual lies in
//              the span of the pivot columns so far), and the estimate is bp_err with bit c flipped for every pivot
//              (row, c) whose residual bit ended up set.
//   order > 0  full elimination with the syndrome itself carried along; the first w = min(order, n - rank) non-pivot
//              columns in reliability order are the search set (:174-181).  Lanes across the 2^w candidates: with bpx =
//              the BP bits of the search set, candidate x means the pattern eff = (x == 0 ? bpx : x) on the search set
//              (the reference leaves them at their BP values for x = 0 and overwrites all of them for x >= 1, :187-192);
//              its pivot bits are base + the XOR of the diagonalised columns of the bits of eff + bpx, as bitsets over
//              the rows; weight by popcount; arg-min of (weight, x) -- the lowest x wins a tie (the reference's strict <).
//
// A syndrome entry that is not 0 counts as 1.  bp_err entries are 0 or 1 (what BP writes).  A syndrome outside the
// column space of H has no solution; the estimate returned for it then depends on the pivot rows and is not specified.
//
// GLOBAL = false: the state of the syndrome lives in the workgroup's dynamic LDS.  GLOBAL = true: in a slot of a global
// workspace, one slot per workgroup of the persistent grid; same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "portable_math.h"

namespace ldpc {

typedef unsigned long long osd_u64;

constexpr int kOsdMaxOrder = 16;   // the device entry runs at most 2^16 candidates per syndrome

struct OsdParams {
    int m, n, nw, st, mw, order;   // st: words between rows; mw = words of a bitset over the rows
    long long batch;
    const uint8_t *syn, *bp;
    const double *llr;
    uint8_t *out;                  // may alias bp
    const osd_u64 *rows;           // [m][nw] packed H
    unsigned char *ws;             // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

__host__ __device__ inline size_t osd_up16(size_t v) { return (v + 15) & ~(size_t)15; }
__host__ __device__ inline long long osd_stride(long long nw) { return (nw + 1) | 1; }
// bytes of one syndrome's state: rows, keys, order, pivot column of each row, BP bits, pivot column mask,
// base + search columns as row bitsets, search set
__host__ __device__ inline size_t osd_state_bytes(long long m, long long n)
{
    const size_t nw = (size_t)((n + 63) >> 6), mw = (size_t)((m + 63) >> 6), st = (size_t)osd_stride((long long)nw);
    return osd_up16((size_t)m * st * 8) + osd_up16((size_t)n * 8) + osd_up16((size_t)n * 4) + osd_up16((size_t)m * 4) +
           2 * osd_up16((nw + 1) * 8) + osd_up16((size_t)(kOsdMaxOrder + 1) * (mw + 1) * 8) + osd_up16((size_t)kOsdMaxOrder * 4);
}

__device__ inline osd_u64 osd_wave_min(osd_u64 v)
{
    for (int d = 32; d; d >>= 1) {
        const osd_u64 o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void osd_kernel(OsdParams p)
{
    constexpr int T = TW * 64;
    constexpr int kNone = 0x7FFFFFFF;
    extern __shared__ __attribute__((aligned(16))) unsigned char osd_lds[];
    __shared__ int sh_piv[3], sh_any[3];
    __shared__ osd_u64 sh_best;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = p.m, n = p.n, nw = p.nw, st = p.st, mw = p.mw;
    const int RB = (m + T - 1) / T;   // rows a thread owns
    unsigned char *base_ptr;
    if constexpr (GLOBAL) base_ptr = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base_ptr = osd_lds;
    osd_u64 *W = (osd_u64 *)base_ptr;
    osd_u64 *keys = (osd_u64 *)((unsigned char *)W + osd_up16((size_t)m * st * 8));
    int *perm = (int *)((unsigned char *)keys + osd_up16((size_t)n * 8));
    int *pcol = (int *)((unsigned char *)perm + osd_up16((size_t)n * 4));
    osd_u64 *ebits = (osd_u64 *)((unsigned char *)pcol + osd_up16((size_t)m * 4));
    osd_u64 *pmask = (osd_u64 *)((unsigned char *)ebits + osd_up16((size_t)(nw + 1) * 8));
    osd_u64 *cand = (osd_u64 *)((unsigned char *)pmask + osd_up16((size_t)(nw + 1) * 8));   // [0]: base, [1 + q]: column q
    int *mrc = (int *)((unsigned char *)cand + osd_up16((size_t)(kOsdMaxOrder + 1) * (mw + 1) * 8));
    const int cstride = mw + 1;

    for (long long col = blockIdx.x; col < p.batch; col += gridDim.x) {
        __syncthreads();   // the previous syndrome's state is no longer read
        const uint8_t *syn = p.syn + col * m, *bp = p.bp + col * n;
        const double *llr = p.llr + col * n;
        uint8_t *out = p.out + col * n;
        // ---- BP hard decisions as a bitset, no pivot column yet
        for (int g = wave; g < nw; g += TW) {
            const int j = g * 64 + lane;
            const osd_u64 b = __ballot(j < n && bp[j] == 1);
            if (lane == 0) { ebits[g] = b; pmask[g] = 0; }
        }
        if (t == 0) { sh_piv[0] = kNone; sh_any[0] = 0; sh_best = ~0ull; }
        __syncthreads();
        // ---- working rows; carried along: order 0 the residual syn + H bp_err (:66-71), order > 0 the syndrome (:136)
        int any = 0;
        for (int row = t; row < m; row += T) {
            const osd_u64 *h = p.rows + (long long)row * nw;
            osd_u64 *wr = W + (long long)row * st;
            osd_u64 acc = 0;
            for (int w = 0; w < nw; ++w) {
                const osd_u64 v = h[w];
                wr[w] = v;
                acc ^= v & ebits[w];
            }
            int sb = syn[row] != 0;
            if (p.order == 0) sb ^= __popcll(acc) & 1;
            wr[nw] = (osd_u64)sb;
            pcol[row] = -1;
            any |= sb;
        }
        if (p.order == 0 && !__syncthreads_or(any)) {   // :72-74: BP's estimate reproduces the syndrome
            for (int j = t; j < n; j += T) out[j] = (uint8_t)((ebits[j >> 6] >> (j & 63)) & 1u);
            continue;
        }
        // ---- reliability order (:53-55 with the stated key)
        for (int j = t; j < n; j += T) {
            const double pr = pm_exp(llr[j]);
            const double q = 1.0 - pr;
            const double k = pr > q ? pr : q;
            keys[j] = k != k ? 0ull : (osd_u64)pm_to_bits(k);
        }
        __syncthreads();
        for (int j = t; j < n; j += T) {
            const osd_u64 kj = keys[j];
            int r = 0;
            for (int k = 0; k < n; ++k) {
                const osd_u64 kk = keys[k];
                r += (kk > kj) || (kk == kj && k < j);
            }
            perm[r] = j;
        }
        __syncthreads();
        // ---- elimination over the columns in that order (:81-108 / :140-172)
        int npiv = 0;
        for (int jj = 0; jj < n && npiv < m; ++jj) {
            const int slot = jj % 3, next = (jj + 1) % 3;
            const int c = perm[jj], cw = c >> 6, cb = c & 63;
            if (t == 0) { sh_piv[next] = kNone; sh_any[next] = 0; }
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rb * T + t;
                bool has = false, res = false;
                if (row < m && pcol[row] < 0) {
                    const osd_u64 *wr = W + (long long)row * st;
                    has = (wr[cw] >> cb) & 1u;
                    res = wr[nw] & 1u;
                }
                const osd_u64 bh = __ballot(has);
                if (bh && lane == __ffsll(bh) - 1) atomicMin(&sh_piv[slot], row);
                if (p.order == 0) {
                    const osd_u64 br = __ballot(res);
                    if (br && lane == 0) atomicOr(&sh_any[slot], 1);
                }
            }
            __syncthreads();
            const int piv = sh_piv[slot];
            if (p.order == 0 && !sh_any[slot]) break;   // :82-84
            if (piv == kNone) continue;                  // dependent on the pivot columns so far
            const osd_u64 *ri = W + (long long)piv * st;
            for (int row = t; row < m; row += T) {
                osd_u64 *wr = W + (long long)row * st;
                if (row == piv) {
                    pcol[row] = c;
                    atomicOr(&pmask[cw], 1ull << cb);
                } else if ((wr[cw] >> cb) & 1u) {
                    for (int w = 0; w <= nw; ++w) wr[w] ^= ri[w];
                }
            }
            ++npiv;
        }
        __syncthreads();
        if (p.order == 0) {
            // the solved pivot bits, as flips of the BP estimate (:111-122)
            for (int row = t; row < m; row += T) {
                const int c = pcol[row];
                if (c >= 0 && (W[(long long)row * st + nw] & 1u)) atomicXor(&ebits[c >> 6], 1ull << (c & 63));
            }
            __syncthreads();
            for (int j = t; j < n; j += T) out[j] = (uint8_t)((ebits[j >> 6] >> (j & 63)) & 1u);
            continue;
        }
        // ---- order > 0: the search set = the first `ord` non-pivot columns in reliability order (:174-181)
        int ord = p.order;
        if (ord > n - npiv) ord = n - npiv;
        if (wave == 0) {
            int cnt = 0;
            for (int pos0 = 0; pos0 < n && cnt < ord; pos0 += 64) {
                const int pos = pos0 + lane;
                int c = 0;
                bool np = false;
                if (pos < n) {
                    c = perm[pos];
                    np = !((pmask[c >> 6] >> (c & 63)) & 1u);
                }
                const osd_u64 b = __ballot(np);
                const int k = cnt + __popcll(b & ((1ull << lane) - 1ull));
                if (np && k < ord) mrc[k] = c;
                cnt += __popcll(b);
            }
        }
        __syncthreads();
        unsigned bpx = 0;
        for (int q = 0; q < ord; ++q) bpx |= (unsigned)((ebits[mrc[q] >> 6] >> (mrc[q] & 63)) & 1u) << q;
        // weight of the non-pivot BP bits outside the search set
        int wrest = -__popc(bpx);
        for (int w = 0; w < nw; ++w) wrest += __popcll(ebits[w] & ~pmask[w]);
        // base = the pivot bits with every non-pivot bit at its BP value, and the search columns, as bitsets over the rows
        for (int rb = 0; rb < RB; ++rb) {
            const int row = rb * T + t, word = rb * TW + wave;
            const bool used = row < m && pcol[row] >= 0;
            const osd_u64 *wr = W + (long long)(used ? row : 0) * st;
            bool b = false;
            if (used) {
                osd_u64 acc = 0;
                for (int w = 0; w < nw; ++w) acc ^= wr[w] & ebits[w] & ~pmask[w];
                b = ((unsigned)wr[nw] ^ (unsigned)__popcll(acc)) & 1u;
            }
            const osd_u64 bb = __ballot(b);
            if (lane == 0 && word < mw) cand[word] = bb;
            for (int q = 0; q < ord; ++q) {
                const int c = mrc[q];
                const osd_u64 bq = __ballot(used && ((wr[c >> 6] >> (c & 63)) & 1u));
                if (lane == 0 && word < mw) cand[(1 + q) * cstride + word] = bq;
            }
        }
        __syncthreads();
        // ---- candidates across the lanes (:184-206)
        osd_u64 best = ~0ull;
        for (unsigned x = (unsigned)t; x < (1u << ord); x += T) {
            const unsigned eff = x ? x : bpx, d = eff ^ bpx;
            int wt = wrest + __popc(eff);
            for (int w = 0; w < mw; ++w) {
                osd_u64 v = cand[w];
                for (int q = 0; q < ord; ++q)
                    if ((d >> q) & 1u) v ^= cand[(1 + q) * cstride + w];
                wt += __popcll(v);
            }
            const osd_u64 key = ((osd_u64)(unsigned)wt << 32) | x;
            best = key < best ? key : best;
        }
        best = osd_wave_min(best);
        if (lane == 0) atomicMin(&sh_best, best);
        __syncthreads();
        const unsigned xs = (unsigned)(sh_best & 0xFFFFFFFFull);
        const unsigned eff = xs ? xs : bpx, d = eff ^ bpx;
        // ---- the winner's bits into the BP bitset: the search set, then the pivot bits
        if (t < ord) {
            const int c = mrc[t];
            const osd_u64 bit = 1ull << (c & 63);
            if ((eff >> t) & 1u) atomicOr(&ebits[c >> 6], bit);
            else atomicAnd(&ebits[c >> 6], ~bit);
        }
        for (int row = t; row < m; row += T) {
            const int c = pcol[row];
            if (c < 0) continue;
            const int word = row >> 6, rbit = row & 63;
            osd_u64 v = cand[word];
            for (int q = 0; q < ord; ++q)
                if ((d >> q) & 1u) v ^= cand[(1 + q) * cstride + word];
            const osd_u64 bit = 1ull << (c & 63);
            if ((v >> rbit) & 1u) atomicOr(&ebits[c >> 6], bit);
            else atomicAnd(&ebits[c >> 6], ~bit);
        }
        __syncthreads();
        for (int j = t; j < n; j += T) out[j] = (uint8_t)((ebits[j >> 6] >> (j & 63)) & 1u);
    }
}

}  // namespace ldpc
