// bpots_plan.hpp -- what the host of the BP-OTS decoder (ldpc_bpots.hip; device code: bpots_kernels.hpp) derives from a
// graph's sizes and largest degrees alone: the bytes each kernel keeps in LDS, which of the three kernels decodes the graph,
// the tile width and LDS budget of the LDS-resident one, the register buckets of the instantiation (ots_plan(), the one
// place the choice is stated) and how a batch is launched (ots_latency_ok(), ots_queue_launch()).  Pure host code over the
// standard library -- no HIP, no decoder handle, no environment -- like tile_plan.hpp, so that it builds with a plain C++
// compiler and runs under the sanitizers on the CPU (tests/native/bpots_plan_sanitize.cpp).  ldpc_bpots_create and the decode
// entries call it; ldpc_debug_bpots_plan (include/ldpc_mi355x_debug.h) hands it to the CPU tests.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ldpc {

constexpr int kOtsThreads = 512;        // of a workgroup of bpots_lds_kernel
constexpr int kOtsNodeThreads = 1024;   // ... of bpots_node_kernel / bpots_big_kernel

// dynamic LDS of bpots_lds_kernel for a tile of S syndromes
inline size_t ots_lds_bytes(int s, int n, int nnz, int S)
{
    size_t b = (size_t)nnz * S * 8;                 // messages (in place: cv <-> vc)
    b += (size_t)n * S * 8;                         // llrs
    b += (size_t)n * S * 4;                         // oscillation counters
    b += 3 * (size_t)n * 8;                         // decision / prior / best masks
    b += 4 * (size_t)s * 8;                         // sign, target, never, parity masks
    b += 8 * 64 * 4 + 64;                           // per-syndrome words
    b += (size_t)kOtsThreads * 24;                  // arg-min partials (one double key + three ints per thread)
    b += 2 * ((size_t)s + 1 + (size_t)n + 1 + 2 * (size_t)nnz) + 32;   // graph (uint16)
    return b;
}

// dynamic LDS of bpots_node_kernel: syndrome codes, decisions and parities of one syndrome, the arg-min partials
inline size_t ots_node_lds_bytes(int s, int n)
{
    return (((size_t)s + 3 * (size_t)n + 15) & ~(size_t)15) + 4 * (size_t)s + (size_t)kOtsNodeThreads * 28 + 64;
}

constexpr size_t kOtsLdsTwo = (size_t)76 * 1024, kOtsLdsOne = (size_t)156 * 1024;   // two / one workgroup a CU
constexpr size_t kOtsLdsStatic = 8192;   // counted on top of ots_lds_bytes(): the kernel's static LDS (the second key array, 4 KiB, and the group word) and headroom
constexpr int64_t kOtsMaxSize = (int64_t)1 << 28;   // s, n, nnz below this: 32-bit indexing of [edge][syndrome] slots

struct OtsPlan {
    int kernel = 0;         // 2 = bpots_lds_kernel, 3 = bpots_node_kernel, 5 = bpots_big_kernel (what ldpc_bpots_kernel reports)
    int logS = -1;          // kernel 2: S = 1 << logS syndromes per workgroup; -1 otherwise
    size_t lds_bytes = 0;   // the dynamic LDS the kernel is launched with (0 for kernel 5)
    int budget_kib = 0;     // kernel 2: 76 or 156, the budget lds_bytes + kOtsLdsStatic fits; 0 otherwise
    int DC = 0, DV = 0;     // register buckets of the instantiation: checks up to 8 or 32 edges, bits up to 4 or 16; 0 for kernel 5
};

inline int ots_bucket_dc(int max_cdeg) { return max_cdeg <= 8 ? 8 : 32; }
inline int ots_bucket_dv(int max_bdeg) { return max_bdeg <= 4 ? 4 : 16; }

// The choice.  LDS-resident with the largest S = 1 ... 64 whose state fits 76 KiB, else S = 1 where that fits 156 KiB (the
// second clause below holds only while nothing is chosen yet, and the widths are tried upwards: the large budget is only
// ever taken with S = 1); graphs with s, n or nnz >= 65535 (uint16 graph copies in LDS), nodes wider than the register
// buckets (`wide`) and force_node != 0 never take it.  Else the node kernel, unless `wide`, force_node >= 2 or the bytes of
// one syndrome are past 156 KiB: the unlimited kernel.  false: a size at or past kOtsMaxSize (create: LDPC_ERR_UNSUPPORTED).
inline bool ots_plan(int64_t s, int64_t n, int64_t nnz, int max_cdeg, int max_bdeg, int force_node, OtsPlan *out)
{
    if (nnz >= kOtsMaxSize || s >= kOtsMaxSize || n >= kOtsMaxSize) return false;
    OtsPlan p;
    const bool wide = max_cdeg > 32 || max_bdeg > 16;   // beyond the register buckets of the two fast kernels
    if (!force_node && !wide && nnz < 65535 && s < 65535 && n < 65535)   // (uint16 graph copies in LDS)
        for (int l = 0; l <= 6; ++l) {
            const size_t b = ots_lds_bytes((int)s, (int)n, (int)nnz, 1 << l) + kOtsLdsStatic;
            if (b <= kOtsLdsTwo || (p.logS < 0 && b <= kOtsLdsOne)) p.logS = l;
            else if (b > kOtsLdsOne) break;
        }
    if (p.logS >= 0) {
        p.kernel = 2;
        p.lds_bytes = ots_lds_bytes((int)s, (int)n, (int)nnz, 1 << p.logS);
        p.budget_kib = p.lds_bytes + kOtsLdsStatic <= kOtsLdsTwo ? 76 : 156;
    } else {
        // beyond the LDS kernel: one workgroup per syndrome, messages in a global slot, bytes / parities in LDS ... and when
        // even the bytes and parities of one syndrome do not fit the LDS, or nodes are wider than the register buckets:
        // everything in the global slot, any degree (the reference's BPOTSDecoder has no limit either)
        const bool big = wide || force_node >= 2 || ots_node_lds_bytes((int)s, (int)n) + 1024 > kOtsLdsOne;
        p.kernel = big ? 5 : 3;
        p.lds_bytes = big ? 0 : ots_node_lds_bytes((int)s, (int)n);
    }
    if (p.kernel != 5) { p.DC = ots_bucket_dc(max_cdeg); p.DV = ots_bucket_dv(max_bdeg); }
    *out = p;
    return true;
}

// ---- how a batch is launched ---------------------------------------------------------------------------------------------
struct OtsLaunch {
    int path = 0;         // 0 = nothing launched (no decode yet, or max_iters == 0), 1 = latency path, 2 = queue
    int64_t groups = 0;   // tiles of S syndromes (kernel 2) or syndromes (kernels 3, 5) of the batch
    int grid = 0;         // workgroups launched
    int chunk = 0;        // groups a workgroup takes from the queue at a time (1 on the latency path)
    int per_cu = 0;       // workgroups a CU holds, as the occupancy query answered (kernel 2; 0 = never asked)
};

constexpr size_t kOtsLatencyImage = (size_t)256 << 10;   // bytes of the host-mapped I/O image of the latency path

inline int64_t ots_groups(int64_t batch, int logS) { return (batch + ((int64_t)1 << logS) - 1) >> logS; }

// The host entry takes the latency path (one workgroup per group, no queue, results through a host-mapped image) for a
// batch of the LDS kernel whose image [syndromes][errors][converged][iterations] fits and that has at most two groups a CU.
inline bool ots_latency_ok(size_t image_bytes, int64_t groups, int num_cus)
{
    return image_bytes <= kOtsLatencyImage && groups <= 2 * (int64_t)num_cus;
}

// The queue path of the LDS kernel: a grid that fills the device once, groups dealt in chunks of up to 64 once there are 32 a workgroup.
inline void ots_queue_launch(int64_t ngroups, int per_cu, int num_cus, int *grid, int *chunk)
{
    *grid = (int)std::min<int64_t>(ngroups, (int64_t)per_cu * num_cus);
    *chunk = (int)std::max<int64_t>(1, std::min<int64_t>(64, ngroups / ((int64_t)*grid * 16)));
}

}  // namespace ldpc
