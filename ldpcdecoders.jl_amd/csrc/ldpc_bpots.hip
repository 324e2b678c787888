// ldpc_bpots.hip -- host side of the BP-OTS decoder: the ldpc_bpots_* entry points
// of include/ldpc_mi355x.h.  Replaces BPOTSDecoder / decode! / batchdecode! of
// src/decoders/bpots_decoder.jl:39-115, 225-340.  Device code: bpots_kernels.hpp; the choice of kernel, tile width and
// launch path: bpots_plan.hpp (HIP-free; ldpc_debug_bpots_plan hands it to the CPU tests).
// Three kernels: LDS-resident (S syndromes per workgroup; every code of the reference's BP-OTS tests); for graphs
// whose messages do not fit a CU's LDS, node-parallel with the messages in a global slot (one workgroup per
// syndrome); and beyond s + 3n + 4s bytes of LDS (n ~ 23,600 for a rate-1/2 code), check degree 32 or bit degree 16, the
// unlimited kernel with everything in the global slot and nodes of any degree.  Only a graph of 2^28 or more checks, bits or
// edges answers LDPC_ERR_UNSUPPORTED.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "../../include/ldpc_mi355x_debug.h"
#include "bpots_kernels.hpp"
#include "host_env.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

struct ldpc_bpots_decoder {
    int64_t s = 0, n = 0, nnz = 0, max_iters = 0, T = 9;
    double per = 0.0, C = 2.0;
    int device = 0, num_cus = 0, logS = 0, max_cdeg = 0, max_bdeg = 0, DC = 0, DV = 0;   // DC, DV: the plan's register buckets
    int *row_ptr = nullptr, *csc_row = nullptr, *col_ptr = nullptr, *csc2csr = nullptr;
    unsigned int *queue = nullptr;
    void *stage = nullptr;      // device staging for the host-pointer entry
    size_t stage_cap = 0;
    // latency path of the host-pointer entry (DESIGN.md "Latency path"): host-mapped I/O image with a flag word
    unsigned int *done_ctr = nullptr;
    ldpc_detail::LatencyImage lat;
    bool kernel_ready = false;  // dynamic-LDS limit set, occupancy known
    int per_cu = 1;
    bool node_mode = false;     // the graph is beyond the LDS kernel: bpots_node_kernel, messages in a global slot
    bool big_mode = false;      // ... and beyond that one too (bytes of a syndrome past the LDS, or nodes wider than the
                                // register buckets): bpots_big_kernel, everything in the global slot, any degree
    double *node_ws = nullptr;  // [grid][slot] of the node kernel
    size_t node_ws_cap = 0;
    OtsLaunch last;             // how the most recent decode was launched (ldpc_debug_bpots_last_launch)
    ~ldpc_bpots_decoder()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {row_ptr, csc_row, col_ptr, csc2csr, queue, stage, done_ctr, node_ws};
        for (void *q : all)
            if (q) (void)hipFree(q);
        lat.release();
    }
};

typedef void (*ots_kernel_t)(OtsParams, const int *, const int *, const int *, const int *);

// by the register buckets of the plan (bpots_plan.hpp: DC 8 or 32, DV 4 or 16)
static ots_kernel_t pick_ots(int DC, int DV)
{
    if (DC == 8) return DV == 4 ? bpots_lds_kernel<8, 4> : bpots_lds_kernel<8, 16>;
    return DV == 4 ? bpots_lds_kernel<32, 4> : bpots_lds_kernel<32, 16>;
}

typedef void (*ots_node_kernel_t)(OtsNodeParams, const int *, const int *, const int *, const int *);

static ots_node_kernel_t pick_ots_node(int DC, int DV)
{
    if (DC == 8) return DV == 4 ? bpots_node_kernel<8, 4> : bpots_node_kernel<8, 16>;
    return DV == 4 ? bpots_node_kernel<32, 4> : bpots_node_kernel<32, 16>;
}

extern "C" {

ldpc_status ldpc_bpots_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                              double per, int64_t max_iters, int64_t T, double C, int32_t device,
                              ldpc_bpots_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, max_iters);
    if (st != LDPC_OK) return st;
    if (T < 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, "T must be >= 1 (iter % T, bpots_decoder.jl:295)");
    if ((st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;

    ldpc_bpots_decoder *d = new (std::nothrow) ldpc_bpots_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->max_iters = max_iters; d->T = T; d->per = per; d->C = C;
    d->device = device; d->num_cus = prop.multiProcessorCount;
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    d->max_cdeg = g.max_cdeg; d->max_bdeg = g.max_bdeg;
    // tests (experiments build, read at create): LDPC_BPOTS_FORCE_NODE = 1 sends small graphs through the node kernel, 2 through the unlimited one
    const int force_node = exp_env("LDPC_BPOTS_FORCE_NODE") ? std::max(1, std::atoi(exp_env("LDPC_BPOTS_FORCE_NODE"))) : 0;
    OtsPlan plan;   // bpots_plan.hpp: the kernel, the tile width and the buckets, from the sizes and largest degrees
    if (!ots_plan(s, n, nnz, d->max_cdeg, d->max_bdeg, force_node, &plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "BP-OTS kernels: graph too large for 32-bit edge indexing");
    }
    d->logS = plan.logS; d->DC = plan.DC; d->DV = plan.DV;
    d->node_mode = plan.kernel != 2;   // bpots_node_kernel: one workgroup per syndrome, messages in a global slot
    d->big_mode = plan.kernel == 5;    // bpots_big_kernel: everything in the global slot, any degree
    using ldpc_detail::upload;
    if (!upload(&d->row_ptr, g.row_ptr) || !upload(&d->csc_row, g.csc_row) || !upload(&d->col_ptr, g.col_ptr) ||
        !upload(&d->csc2csr, g.csc2csr) ||
        hipMalloc((void **)&d->queue, 64) != hipSuccess || hipMalloc((void **)&d->done_ctr, 64) != hipSuccess ||
        hipMemset(d->done_ctr, 0, 64) != hipSuccess) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

int32_t ldpc_bpots_kernel(const ldpc_bpots_decoder *d) { return d ? (d->big_mode ? 5 : d->node_mode ? 3 : 2) : 0; }

ldpc_status ldpc_bpots_destroy(ldpc_bpots_decoder *d)
{
    if (!d) return LDPC_OK;
    (void)hipSetDevice(d->device);
    const ldpc_status st = ldpc_detail::wait_device(d->device, "ldpc_bpots_destroy (device synchronise)");
    delete d;
    return st;
}

}  // extern "C"

struct OtsLatencyCtl {
    unsigned int *flag;
    unsigned int ticket;
};

static ldpc_status bpots_decode_impl(ldpc_bpots_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                     uint8_t *d_conv, int32_t *d_iters, void *stream_v, const OtsLatencyCtl *lat)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !d_syn) || (d->n > 0 && !d_err) || !d_conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(d->device));
    if (ldpc_detail::device_stalled(d->device)) return ldpc_detail::stalled_error(d->device);
    d->last = OtsLaunch();
    if (d->max_iters == 0) {   // the loop at :239 never runs: best_decisions = 0, converged = false
        if (d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        return LDPC_OK;
    }
    if (d->node_mode) {
        if (batch > (1ll << 30)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
        ots_node_kernel_t nk = d->big_mode ? (ots_node_kernel_t)bpots_big_kernel : pick_ots_node(d->DC, d->DV);
        const size_t nlds = d->big_mode ? 0 : ots_node_lds_bytes((int)d->s, (int)d->n);
        if (!d->kernel_ready) {
            if (nlds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)nk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)nlds));
            d->kernel_ready = true;
        }
        const int grid = (int)std::min<int64_t>(batch, d->num_cus);
        const size_t slot = d->big_mode ? ots_big_slot_doubles((int)d->s, (int)d->n, (int)d->nnz) : ots_node_slot_doubles((int)d->n, (int)d->nnz);
        const ldpc_status ws = ldpc_detail::grow_device_buffer((void **)&d->node_ws, &d->node_ws_cap, (size_t)grid * slot * sizeof(double), d->device,
                                                               "BP-OTS workspace regrow (device synchronise before the free)");
        if (ws != LDPC_OK) return ws;
        OtsNodeParams np{};
        np.s = (int)d->s; np.n = (int)d->n; np.nnz = (int)d->nnz; np.max_iters = (int)d->max_iters; np.T = (int)d->T;
        np.batch = batch;
        np.prior = std::log((1 - (2 * d->per / 3)) / (2 * d->per / 3));   // bpots_decoder.jl:231
        np.C = d->C;
        np.syn = d_syn; np.err = d_err; np.conv = d_conv; np.iters = d_iters; np.queue = d->queue;
        np.ws = d->node_ws; np.slot_doubles = (long long)slot;
        LDPC_HIP_TRY(hipMemsetAsync(d->queue, 0, 64, stream));
        hipLaunchKernelGGL(nk, dim3((unsigned)grid), dim3(kOtsNodeThreads), nlds, stream, np, (const int *)d->row_ptr,
                           (const int *)d->csc_row, (const int *)d->col_ptr, (const int *)d->csc2csr);
        LDPC_HIP_TRY(hipGetLastError());
        d->last.path = 2; d->last.groups = batch; d->last.grid = grid; d->last.chunk = 1;
        return LDPC_OK;
    }
    const int64_t ngroups = ots_groups(batch, d->logS);
    if (ngroups > (1ll << 30)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    OtsParams p;
    p.s = (int)d->s; p.n = (int)d->n; p.nnz = (int)d->nnz; p.max_iters = (int)d->max_iters; p.T = (int)d->T;
    p.logS = d->logS; p.ngroups = (int)ngroups; p.batch = batch;
    p.prior = std::log((1 - (2 * d->per / 3)) / (2 * d->per / 3));   // bpots_decoder.jl:231
    p.C = d->C;
    p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.iters = d_iters; p.queue = d->queue;
    const size_t lds = ots_lds_bytes((int)d->s, (int)d->n, (int)d->nnz, 1 << d->logS);
    ots_kernel_t k = pick_ots(d->DC, d->DV);
    if (!d->kernel_ready) {
        LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        d->per_cu = ldpc_detail::blocks_per_cu((const void *)k, kOtsThreads, lds);
        d->kernel_ready = true;
    }
    p.done_count = d->done_ctr; p.done_flag = nullptr; p.done_ticket = 0;
    if (lat) {   // one workgroup per group, no queue to reset: the launch is the only runtime call
        p.queue = nullptr; p.chunk = 1;
        p.done_flag = lat->flag; p.done_ticket = lat->ticket;
        hipLaunchKernelGGL(k, dim3((unsigned)ngroups), dim3(kOtsThreads), lds, stream, p, (const int *)d->row_ptr,
                           (const int *)d->csc_row, (const int *)d->col_ptr, (const int *)d->csc2csr);
        LDPC_HIP_TRY(hipGetLastError());
        d->last.path = 1; d->last.groups = ngroups; d->last.grid = (int)ngroups; d->last.chunk = 1; d->last.per_cu = d->per_cu;
        return LDPC_OK;
    }
    int grid = 0;
    ots_queue_launch(ngroups, d->per_cu, d->num_cus, &grid, &p.chunk);
    LDPC_HIP_TRY(hipMemsetAsync(d->queue, 0, 64, stream));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kOtsThreads), lds, stream, p, (const int *)d->row_ptr,
                       (const int *)d->csc_row, (const int *)d->col_ptr, (const int *)d->csc2csr);
    LDPC_HIP_TRY(hipGetLastError());
    d->last.path = 2; d->last.groups = ngroups; d->last.grid = grid; d->last.chunk = p.chunk; d->last.per_cu = d->per_cu;
    return LDPC_OK;
}

extern "C" {

ldpc_status ldpc_debug_bpots_plan(int64_t s, int64_t n, int64_t nnz, int32_t max_cdeg, int32_t max_bdeg, int32_t force_node,
                                  int32_t *kernel, int32_t *logS, int64_t *lds_bytes, int32_t *budget_kib, int32_t *dc, int32_t *dv)
{
    if (s < 0 || n < 0 || nnz < 0 || max_cdeg < 0 || max_bdeg < 0 || force_node < 0)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "ldpc_debug_bpots_plan: negative size, degree or force_node");
    OtsPlan plan;
    if (!ots_plan(s, n, nnz, max_cdeg, max_bdeg, force_node, &plan))
        return set_error(LDPC_ERR_UNSUPPORTED, "BP-OTS kernels: graph too large for 32-bit edge indexing");
    if (kernel) *kernel = plan.kernel;
    if (logS) *logS = plan.logS;
    if (lds_bytes) *lds_bytes = (int64_t)plan.lds_bytes;
    if (budget_kib) *budget_kib = plan.budget_kib;
    if (dc) *dc = plan.DC;
    if (dv) *dv = plan.DV;
    return LDPC_OK;
}

ldpc_status ldpc_debug_bpots_last_launch(const ldpc_bpots_decoder *d, int32_t *path, int64_t *groups, int32_t *grid, int32_t *chunk,
                                         int32_t *per_cu)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (path) *path = d->last.path;
    if (groups) *groups = d->last.groups;
    if (grid) *grid = d->last.grid;
    if (chunk) *chunk = d->last.chunk;
    if (per_cu) *per_cu = d->last.per_cu;
    return LDPC_OK;
}

ldpc_status ldpc_bpots_decode_batch_device(ldpc_bpots_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                           uint8_t *d_conv, int32_t *d_iters, void *stream_v)
{
    return bpots_decode_impl(d, batch, d_syn, d_err, d_conv, d_iters, stream_v, nullptr);
}

ldpc_status ldpc_bpots_decode_batch(ldpc_bpots_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err,
                                    uint8_t *conv, int32_t *iters)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    LDPC_HIP_TRY(hipSetDevice(d->device));
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    const ldpc_detail::StageLayout L = ldpc_detail::stage_layout(B, B * s, B * n, false, n);   // [syndromes][errors][converged][iterations]
    const size_t o_err = L.o_err, o_conv = L.o_conv, o_it = L.o_it, total = L.total;
    static const bool lat_off = exp_env("LDPC_NO_LATENCY_PATH") != nullptr;
    if (!d->node_mode && !lat_off && d->max_iters > 0 && ots_latency_ok(total, ots_groups(batch, d->logS), d->num_cus)) {
        const ldpc_status ist = d->lat.ensure(kOtsLatencyImage);
        if (ist != LDPC_OK) return ist;
        char *hp = d->lat.image(), *dp = d->lat.image_dev();
        const OtsLatencyCtl lc{d->lat.flag_dev(), d->lat.next_ticket()};
        std::memcpy(hp, syn, B * s);
        ldpc_status lst = bpots_decode_impl(d, batch, (const uint8_t *)dp, (uint8_t *)(dp + o_err), (uint8_t *)(dp + o_conv),
                                            (int32_t *)(dp + o_it), nullptr, &lc);
        if (lst != LDPC_OK) return lst;
        if ((lst = ldpc_detail::wait_flag(d->lat.flag(), lc.ticket, nullptr, d->device, "BP-OTS latency path (flag of the last workgroup)")) != LDPC_OK) return lst;
        std::memcpy(err, hp + o_err, B * n);
        std::memcpy(conv, hp + o_conv, B);
        if (iters) std::memcpy(iters, hp + o_it, B * sizeof(int32_t));
        return LDPC_OK;
    }
    const ldpc_status gs = ldpc_detail::grow_device_buffer(&d->stage, &d->stage_cap, total, d->device, "BP-OTS staging regrow (device synchronise before the free)");
    if (gs != LDPC_OK) return gs;
    char *dp = (char *)d->stage;
    if (s > 0) LDPC_HIP_TRY(hipMemcpyAsync(dp, syn, B * s, hipMemcpyHostToDevice, nullptr));
    ldpc_status st = ldpc_bpots_decode_batch_device(d, batch, (const uint8_t *)dp, (uint8_t *)(dp + o_err),
                                                    (uint8_t *)(dp + o_conv), (int32_t *)(dp + o_it), nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) LDPC_HIP_TRY(hipMemcpyAsync(err, dp + o_err, B * n, hipMemcpyDeviceToHost, nullptr));
    LDPC_HIP_TRY(hipMemcpyAsync(conv, dp + o_conv, B, hipMemcpyDeviceToHost, nullptr));
    if (iters) LDPC_HIP_TRY(hipMemcpyAsync(iters, dp + o_it, B * 4, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, d->device, "ldpc_bpots_decode_batch (stream synchronise)");
}

}  // extern "C"
