// osd_search_kernels.hpp -- device code of the STANDARD RULE of the ordered-statistics step (ldpc_osd_set_search of
// include/ldpc_mi355x.h, where the rule is stated; host side: ldpc_osd_device.hip): least reliable column first, the
// exhaustive or the combination-sweep search, an integer cost with one weight per bit.  Device form only.
//
// Shared with osd_kernel (osd_kernels.hpp), because it does not depend on the rule: ONE WORKGROUP OF TW WAVES PER
// SYNDROME, THREAD = ROW; the working rows 64-bit packed in the original column order at an odd stride, word nw carrying
// the syndrome bit along; the pivot of a column = the lowest unused row that has the bit (a ballot per wave, one atomicMin
// per workgroup, three rotating slots, one barrier per column); Gauss-Jordan without swaps.  New here:
//
//   step 1     the residual syn + H bp_err is formed while the rows are loaded; all zero -> the output is bp_err, at every
//              order.  The syndrome itself is what the rows carry along.
//   order      key = the sortable-integer form of the double (negative: all bits flipped; else the sign bit set), with
//              -0.0 read as +0.0 and a NaN as the all-ones key, which no other double has.  (key ascending, index
//              ascending), rank by counting.  No exp, no transform.
//   elimination  FULL, over the columns in that order until the rank is reached; the non-pivot columns t_0 .. t_{K-1}, in
//              that order, are listed by wave 0 (ballot + prefix popcount).
//   candidates  spread across the threads.  Candidate 0 (F empty) has the carried syndrome bits as its pivot bits: `base`,
//              a bitset over the rows.  Every other candidate is costed as a DELTA against it: + q of its own columns, and
//              for each pivot row where the XOR of its columns has a bit, + rowq[row] where base has 0 and - rowq[row] where
//              base has 1 (rowq[row] = q[pcol[row]], 0 for an unused row).  With all-ones weights two popcounts a word.
//              The column bitsets over the rows are HELD for the first w = min(order, K) non-pivot columns only, at most
//              64 of them (the pairs of the sweep, every subset of the exhaustive search); a single flip t_k reads its
//              column from the working rows instead (m words, all lanes of a wave in the same row: broadcasts).  Holding
//              all K would cost K (mw + 1) 8 bytes -- 100 KiB for the 900 x 1000 test code -- for K candidates that are
//              each costed once.
//   winner     arg-min over (int64 delta, index): a two-word compare in the wave's butterfly and across the waves (one
//              slot per wave in LDS).  A thread meets its candidates in ascending index, so strict < keeps the lowest.
//   output     the winner's columns are read from the working rows once more: pivot bit = base + their XOR.
//
// STATE of one syndrome (osd_search_state_bytes), each part rounded up to 16 bytes: the working rows m (nw + 1 made odd)
// 8; keys 8 n; order 4 n; non-pivot list 4 n; pivot column 4 m and weight 8 m of each row; BP / output bits and pivot
// mask 2 (nw + 1) 8; base and the 64 held columns 65 (mw + 1) 8.  That is 148 m + 16 n + 8.7 KiB for the 900 x 1000 code.
//
// GLOBAL = false: the state lives in the workgroup's dynamic LDS.  GLOBAL = true: in a slot of a global workspace.
#pragma once
#include "osd_kernels.hpp"

namespace ldpc {

constexpr int kOsdSearchExhaustive = 1, kOsdSearchSweep = 2;
constexpr int kOsdSearchCols = 64;      // column bitsets held per syndrome: the largest order of either method (osd_handle.hpp)

struct OsdSearchParams {
    int m, n, nw, st, mw, method, order;
    long long batch;
    const uint8_t *syn, *bp;
    const double *llr;
    uint8_t *out;                  // may alias bp
    const osd_u64 *rows;           // [m][nw] packed H
    const long long *q;            // [n] weight of each bit; NULL: all 1
    unsigned char *ws;             // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

__host__ __device__ inline size_t osd_search_state_bytes(long long m, long long n)
{
    const size_t nw = (size_t)((n + 63) >> 6), mw = (size_t)((m + 63) >> 6), st = (size_t)osd_stride((long long)nw);
    return osd_up16((size_t)m * st * 8) + osd_up16((size_t)n * 8) + 2 * osd_up16((size_t)n * 4) + osd_up16((size_t)m * 4) +
           osd_up16((size_t)m * 8) + 2 * osd_up16((nw + 1) * 8) + osd_up16((size_t)(kOsdSearchCols + 1) * (mw + 1) * 8);
}

__device__ inline osd_u64 osd_sort_key(double x)
{
    if (x != x) return ~0ull;
    const osd_u64 b = x == 0.0 ? 0ull : (osd_u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

template <int TW, bool GLOBAL>
__global__ __launch_bounds__(TW * 64) void osd_search_kernel(OsdSearchParams p)
{
    constexpr int T = TW * 64;
    constexpr int kNone = 0x7FFFFFFF;
    extern __shared__ __attribute__((aligned(16))) unsigned char osd_search_lds[];
    __shared__ int sh_piv[3], sh_idx[TW];
    __shared__ long long sh_cost[TW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = p.m, n = p.n, nw = p.nw, st = p.st, mw = p.mw;
    const int RB = (m + T - 1) / T;   // rows a thread owns
    unsigned char *base_ptr;
    if constexpr (GLOBAL) base_ptr = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base_ptr = osd_search_lds;
    osd_u64 *W = (osd_u64 *)base_ptr;
    osd_u64 *keys = (osd_u64 *)((unsigned char *)W + osd_up16((size_t)m * st * 8));
    int *perm = (int *)((unsigned char *)keys + osd_up16((size_t)n * 8));
    int *npc = (int *)((unsigned char *)perm + osd_up16((size_t)n * 4));          // t_0 .. t_{K-1}
    int *pcol = (int *)((unsigned char *)npc + osd_up16((size_t)n * 4));
    long long *rowq = (long long *)((unsigned char *)pcol + osd_up16((size_t)m * 4));
    osd_u64 *ebits = (osd_u64 *)((unsigned char *)rowq + osd_up16((size_t)m * 8));
    osd_u64 *pmask = (osd_u64 *)((unsigned char *)ebits + osd_up16((size_t)(nw + 1) * 8));
    osd_u64 *base = (osd_u64 *)((unsigned char *)pmask + osd_up16((size_t)(nw + 1) * 8));
    const int cstride = mw + 1;
    osd_u64 *cand = base + cstride;   // [k]: column t_k over the rows, k < w

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
        if (t == 0) sh_piv[0] = kNone;
        __syncthreads();
        // ---- working rows, the syndrome bit carried along; step 1: the residual syn + H bp_err
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
            const int sb = syn[row] != 0;
            wr[nw] = (osd_u64)sb;
            pcol[row] = -1;
            any |= sb ^ (__popcll(acc) & 1);
        }
        if (!__syncthreads_or(any)) {   // BP's estimate reproduces the syndrome: returned unchanged
            for (int j = t; j < n; j += T) out[j] = (uint8_t)((ebits[j >> 6] >> (j & 63)) & 1u);
            continue;
        }
        // ---- step 2: ascending llr, ties by index
        for (int j = t; j < n; j += T) keys[j] = osd_sort_key(llr[j]);
        __syncthreads();
        for (int j = t; j < n; j += T) {
            const osd_u64 kj = keys[j];
            int r = 0;
            for (int k = 0; k < n; ++k) {
                const osd_u64 kk = keys[k];
                r += (kk < kj) || (kk == kj && k < j);
            }
            perm[r] = j;
        }
        __syncthreads();
        // ---- step 3: full elimination over the columns in that order
        int npiv = 0;
        for (int jj = 0; jj < n && npiv < m; ++jj) {
            const int slot = jj % 3, next = (jj + 1) % 3;
            const int c = perm[jj], cw = c >> 6, cb = c & 63;
            if (t == 0) sh_piv[next] = kNone;
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rb * T + t;
                bool has = false;
                if (row < m && pcol[row] < 0) has = (W[(long long)row * st + cw] >> cb) & 1u;
                const osd_u64 bh = __ballot(has);
                if (bh && lane == __ffsll(bh) - 1) atomicMin(&sh_piv[slot], row);
            }
            __syncthreads();
            const int piv = sh_piv[slot];
            if (piv == kNone) continue;   // dependent on the pivot columns so far
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
        const int K = n - npiv;
        const int w = p.order < K ? p.order : K;
        if (wave == 0) {
            int cnt = 0;
            for (int pos0 = 0; pos0 < n; pos0 += 64) {
                const int pos = pos0 + lane;
                int c = 0;
                bool np = false;
                if (pos < n) {
                    c = perm[pos];
                    np = !((pmask[c >> 6] >> (c & 63)) & 1u);
                }
                const osd_u64 b = __ballot(np);
                if (np) npc[cnt + __popcll(b & ((1ull << lane) - 1ull))] = c;
                cnt += __popcll(b);
            }
        }
        __syncthreads();
        // ---- step 4, F empty: the pivot bits are the carried syndrome bits; the held columns; the weight of each row
        for (int rb = 0; rb < RB; ++rb) {
            const int row = rb * T + t, word = rb * TW + wave;
            const bool used = row < m && pcol[row] >= 0;
            const osd_u64 *wr = W + (long long)(used ? row : 0) * st;
            const osd_u64 bb = __ballot(used && (wr[nw] & 1u));
            if (lane == 0 && word < mw) base[word] = bb;
            if (row < m) rowq[row] = used ? (p.q ? p.q[pcol[row]] : 1ll) : 0ll;
            for (int k = 0; k < w && k < kOsdSearchCols; ++k) {
                const int c = npc[k];
                const osd_u64 bk = __ballot(used && ((wr[c >> 6] >> (c & 63)) & 1u));
                if (lane == 0 && word < mw) cand[k * cstride + word] = bk;
            }
        }
        __syncthreads();
        // ---- steps 5 and 6: the candidates across the threads, each a delta against candidate 0
        auto qof = [&](int c) -> long long { return p.q ? p.q[c] : 1ll; };
        auto rows_delta = [&](osd_u64 v, int word) -> long long {
            const osd_u64 b = base[word];
            if (!p.q) return (long long)__popcll(v & ~b) - (long long)__popcll(v & b);
            long long d = 0;
            for (; v; v &= v - 1) {
                const int r = __ffsll(v) - 1;
                const long long q = rowq[word * 64 + r];
                d += ((b >> r) & 1u) ? -q : q;
            }
            return d;
        };
        const bool sweep = p.method == kOsdSearchSweep;
        const int total = sweep ? 1 + K + w * (w - 1) / 2 : 1 << w;
        long long bestc = 0x7FFFFFFFFFFFFFFFll;
        int besti = kNone;
        for (int idx = t; idx < total; idx += T) {
            long long d = 0;
            if (!sweep) {
                for (int k = 0; k < w; ++k)
                    if ((idx >> k) & 1) d += qof(npc[k]);
                for (int word = 0; word < mw; ++word) {
                    osd_u64 v = 0;
                    for (int k = 0; k < w; ++k)
                        if ((idx >> k) & 1) v ^= cand[k * cstride + word];
                    d += rows_delta(v, word);
                }
            } else if (idx > K) {
                int a = 0, rest = idx - 1 - K;   // pairs a < b < w, a ascending then b ascending
                while (rest >= w - 1 - a) { rest -= w - 1 - a; ++a; }
                const int b = a + 1 + rest;
                d = qof(npc[a]) + qof(npc[b]);
                for (int word = 0; word < mw; ++word) d += rows_delta(cand[a * cstride + word] ^ cand[b * cstride + word], word);
            } else if (idx > 0) {
                const int c = npc[idx - 1], cw = c >> 6, cb = c & 63;
                d = qof(c);
                for (int row = 0; row < m; ++row)
                    if ((W[(long long)row * st + cw] >> cb) & 1u) {
                        const long long q = rowq[row];
                        d += ((base[row >> 6] >> (row & 63)) & 1u) ? -q : q;
                    }
            }
            if (d < bestc) { bestc = d; besti = idx; }
        }
        for (int s = 32; s; s >>= 1) {
            const long long oc = __shfl_xor(bestc, s);
            const int oi = __shfl_xor(besti, s);
            if (oc < bestc || (oc == bestc && oi < besti)) { bestc = oc; besti = oi; }
        }
        if (lane == 0) { sh_cost[wave] = bestc; sh_idx[wave] = besti; }
        for (int g = t; g < nw; g += T) ebits[g] = 0;   // the BP bits are used no further
        __syncthreads();
        for (int v = 0; v < TW; ++v) {
            const long long oc = sh_cost[v];
            const int oi = sh_idx[v];
            if (oc < bestc || (oc == bestc && oi < besti)) { bestc = oc; besti = oi; }
        }
        // ---- the winner's F: positions below 64 as a mask, a single flip beyond as its column
        osd_u64 fmask = 0;
        int fsingle = -1;
        if (!sweep) fmask = (osd_u64)(unsigned)besti;
        else if (besti > K) {
            int a = 0, rest = besti - 1 - K;
            while (rest >= w - 1 - a) { rest -= w - 1 - a; ++a; }
            fmask = (1ull << a) | (1ull << (a + 1 + rest));
        } else if (besti > 0) fsingle = npc[besti - 1];
        if (t < 64 && ((fmask >> t) & 1u)) atomicOr(&ebits[npc[t] >> 6], 1ull << (npc[t] & 63));
        if (t == 0 && fsingle >= 0) atomicOr(&ebits[fsingle >> 6], 1ull << (fsingle & 63));
        for (int row = t; row < m; row += T) {
            const int c = pcol[row];
            if (c < 0) continue;
            const osd_u64 *wr = W + (long long)row * st;
            unsigned v = (unsigned)(wr[nw] & 1u);
            if (fsingle >= 0) v ^= (unsigned)((wr[fsingle >> 6] >> (fsingle & 63)) & 1u);
            for (osd_u64 f = fmask; f; f &= f - 1) {
                const int cf = npc[__ffsll(f) - 1];
                v ^= (unsigned)((wr[cf >> 6] >> (cf & 63)) & 1u);
            }
            if (v) atomicOr(&ebits[c >> 6], 1ull << (c & 63));
        }
        __syncthreads();
        for (int j = t; j < n; j += T) out[j] = (uint8_t)((ebits[j >> 6] >> (j & 63)) & 1u);
    }
}

}  // namespace ldpc
