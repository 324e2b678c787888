// bitflip_kernels.hpp -- device code of the bit-flip decoder (ldpc_bitflip_* of include/ldpc_mi355x.h; host side:
// ldpc_bitflip.hip).  Replaces decode! of src/decoders/iterative_bitflip.jl:116-157 for a batch.
//
// LANES ACROSS THE BITS OF ONE SYNDROME (every BP kernel of this library puts a syndrome in a lane): a team of TW waves
// -- one workgroup -- decodes one syndrome; thread t owns the bits t, t + 64 TW, t + 128 TW, ..., so the 64 bits of
// "group" g = j / 64 sit in the 64 lanes of wave g % TW in bit order, and a ballot over a group is a bit mask in
// candidate order (candidates are ordered by ascending bit index: include/ldpc_mi355x.h "The tie rule").
//
// The reference recomputes H * err and every vote from scratch in each iteration (O(nnz)).  Here the state of a
// syndrome is kept incrementally; it is integer-identical:
//   err[j]    the error bit
//   chk[i]    bit 0: check i is mismatched now, bit 1: its syndrome entry is neither 0 nor 1 (never matches, never toggles)
//   M         number of mismatched checks (a workgroup-shared word)
//   w[j]      2 u[j] - deg[j], u[j] = mismatched checks of bit j: what one iteration adds to votes[j]
//   votes[j]  accumulated over the iterations (the reference's reset! runs once per syndrome)
// One iteration: M == 0 -> matched; votes += w and the maximum (VALU + wave reduction, across waves through LDS); < 0 ->
// stop; per-group candidate counts (ballot + popcount); a wave-wide prefix scan finds the group and the lane of the
// chosen rank; the flip toggles the (<= deg) checks of the bit and adds -+2 to w of the bits of those checks, one lane
// per (check, bit) pair, with atomics (LDS or global).
//
// GLOBAL = false: the state lives in the workgroup's LDS (dynamic), the graph is read from global memory through the
// caches.  GLOBAL = true: the state lives in a slot of a global workspace, one slot per workgroup of the persistent
// grid; same code.  VT = type of the vote accumulators (int; long long when max_iters * max bit degree >= 2^31).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <limits>

namespace ldpc {

struct BfParams {
    int s, n, max_iters, tie_break;   // tie_break: 0 random, 1 first, 2 last
    int rw_shift;                     // 1 << rw_shift >= the largest check degree: a (check, bit) pair is index >> / & of it
    long long batch, column0;
    unsigned long long seed;
    const uint8_t *syn;
    uint8_t *err, *conv, *stop;
    int32_t *iters;
    const int *row_ptr, *csr_col, *col_ptr, *csc_row;
    unsigned char *ws;                // GLOBAL: [grid][slot_bytes]
    long long slot_bytes;
};

__host__ __device__ inline size_t bf_up16(size_t v) { return (v + 15) & ~(size_t)15; }
// bytes of one syndrome's state: votes, w, group counts, err, chk (each part 16-byte aligned)
__host__ __device__ inline size_t bf_state_bytes(long long s, long long n, size_t vote_bytes)
{
    const size_t G = (size_t)((n + 63) >> 6);
    return bf_up16((size_t)n * vote_bytes) + bf_up16((size_t)n * 4) + bf_up16(G * 4) + bf_up16((size_t)n) + bf_up16((size_t)s);
}

__host__ __device__ inline unsigned long long bf_mix(unsigned long long z)   // the SplitMix64 finaliser
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// candidate of `k` that the RANDOM rule takes for column `column` (column0 + index in the call) in iteration `iter` (1-based)
__host__ __device__ inline unsigned bf_pick(unsigned long long seed, long long column, int iter, unsigned k)
{
    const unsigned long long r = bf_mix(bf_mix(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(column + 1)) + (unsigned long long)iter);
    return (unsigned)(((r >> 32) * (unsigned long long)k) >> 32);
}

template <typename VT>
__device__ inline VT bf_wave_max(VT v)
{
    for (int d = 32; d; d >>= 1) {
        const VT o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline int bf_wave_sum(int v)
{
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <int TW, bool GLOBAL, typename VT>
__global__ __launch_bounds__(TW * 64) void bitflip_kernel(BfParams p)
{
    constexpr int T = TW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[];
    __shared__ VT sh_red[TW];
    __shared__ int sh_M;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = p.n, s = p.s, G = (n + 63) >> 6;
    unsigned char *base;
    if constexpr (GLOBAL) base = p.ws + (long long)blockIdx.x * p.slot_bytes;
    else base = bf_lds;
    VT *votes = (VT *)base;
    int *w = (int *)(base + bf_up16((size_t)n * sizeof(VT)));
    int *grpcnt = (int *)((unsigned char *)w + bf_up16((size_t)n * 4));
    unsigned char *err = (unsigned char *)grpcnt + bf_up16((size_t)G * 4);
    unsigned char *chk = err + bf_up16((size_t)n);
    const int *__restrict__ row_ptr = p.row_ptr, *__restrict__ csr_col = p.csr_col;
    const int *__restrict__ col_ptr = p.col_ptr, *__restrict__ csc_row = p.csc_row;
    const int C = (G + 63) >> 6;   // groups a lane sums in the rank search

    for (long long col = blockIdx.x; col < p.batch; col += gridDim.x) {
        // ---- reset! + the state of err = 0: a check is mismatched iff its syndrome entry is not 0
        const uint8_t *syn = p.syn + col * s;
        int mloc = 0;
        for (int i = t; i < s; i += T) {
            const uint8_t v = syn[i];
            const unsigned char f = v == 0 ? 0 : v == 1 ? 1 : 3;
            chk[i] = f;
            mloc += f & 1;
        }
        if (t == 0) sh_M = 0;
        __syncthreads();
        mloc = bf_wave_sum(mloc);
        if (lane == 0 && mloc) atomicAdd(&sh_M, mloc);
        for (int j = t; j < n; j += T) {
            const int a = col_ptr[j], b = col_ptr[j + 1];
            int u = 0;
            for (int k = a; k < b; ++k) u += chk[csc_row[k]] & 1;
            w[j] = 2 * u - (b - a);
            votes[j] = 0;
            err[j] = 0;
        }
        __syncthreads();

        int stop = 0, it = 1;
        for (; it <= p.max_iters; ++it) {
            if (sh_M == 0) { stop = 1; break; }                     // syn == syndrome (:124)
            // ---- every check votes (:131-143), and the maximum (:145)
            VT lmax = std::numeric_limits<VT>::min();
            for (int j = t; j < n; j += T) {
                const VT v = votes[j] + (VT)w[j];
                votes[j] = v;
                lmax = v > lmax ? v : lmax;
            }
            lmax = bf_wave_max(lmax);
            if (lane == 0) sh_red[wave] = lmax;
            __syncthreads();
            VT gmax = sh_red[0];
#pragma unroll
            for (int q = 1; q < TW; ++q) gmax = sh_red[q] > gmax ? sh_red[q] : gmax;
            if (gmax < 0) { stop = 2; break; }                      // :150-152 (n = 0: no bit at all)
            // ---- candidates per 64-bit group, in bit order
            for (int g = wave; g < G; g += TW) {
                const int j = g * 64 + lane;
                const unsigned long long m = __ballot(j < n && votes[j] == gmax);
                if (lane == 0) grpcnt[g] = __popcll(m);
            }
            __syncthreads();
            // ---- (every wave, redundantly) the number of candidates, the rank the tie rule takes, its group and lane
            int lsum = 0;
            for (int c = 0; c < C; ++c) {
                const int g = lane * C + c;
                if (g < G) lsum += grpcnt[g];
            }
            int incl = lsum;
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            const int k = __shfl(incl, 63);
            const int r = p.tie_break == 1 ? 0 : p.tie_break == 2 ? k - 1 : (int)bf_pick(p.seed, p.column0 + col, it, (unsigned)k);
            const int L = __ffsll((unsigned long long)__ballot(r < incl)) - 1;
            int rr = r - __shfl(incl - lsum, L);
            int g = L * C;
            for (int c = 0; c < C && g < G - 1; ++c, ++g) {
                const int cnt = grpcnt[g];
                if (rr < cnt) break;
                rr -= cnt;
            }
            int jstar;
            {
                const int j = g * 64 + lane;
                const bool cand = j < n && votes[j] == gmax;
                const unsigned long long m = __ballot(cand);
                const int below = __popcll(m & ((1ull << lane) - 1ull));
                jstar = g * 64 + __ffsll((unsigned long long)__ballot(cand && below == rr)) - 1;
            }
            if ((unsigned)jstar >= (unsigned)n) { stop = 3; break; }   // (cannot happen: k >= 1 candidates exist; keeps a fault in here from indexing out of bounds)
            // ---- flip (:149): the bit, then those of its checks that can toggle, and M
            const int a = col_ptr[jstar], deg = col_ptr[jstar + 1] - a;
            if (t == 0) err[jstar] ^= 1;
            int dm = 0;
            for (int c = t; c < deg; c += T) {
                const int i = csc_row[a + c];
                const unsigned char f = chk[i];
                if (!(f & 2)) {
                    chk[i] = f ^ 1;
                    dm += (f & 1) ? -1 : 1;
                }
            }
            if (dm) atomicAdd(&sh_M, dm);
            __syncthreads();
            // ---- one lane per (check, bit) pair: a check that is mismatched now gives each of its bits one more
            // mismatched check (w += 2), one that is matched now one fewer
            const long long P = (long long)deg << p.rw_shift;
            const int qmask = (1 << p.rw_shift) - 1;
            for (long long pp = t; pp < P; pp += T) {
                const int i = csc_row[a + (int)(pp >> p.rw_shift)], q = (int)pp & qmask;
                const int ra = row_ptr[i], rl = row_ptr[i + 1] - ra;
                const unsigned char f = chk[i];
                if (q < rl && !(f & 2)) atomicAdd(&w[csr_col[ra + q]], (f & 1) ? 2 : -2);
            }
            __syncthreads();
        }
        // ---- (err, converged) (:156); iterations entered and why the loop ended
        uint8_t *out = p.err + col * n;
        for (int j = t; j < n; j += T) out[j] = err[j];
        if (t == 0) {
            p.conv[col] = stop != 0;
            if (p.iters) p.iters[col] = stop ? it : p.max_iters;
            if (p.stop) p.stop[col] = (uint8_t)stop;
        }
        __syncthreads();
    }
}

}  // namespace ldpc
