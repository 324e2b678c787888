// ldpc_bitflip.hip -- host side of the bit-flip decoder: the ldpc_bitflip_* entry points of include/ldpc_mi355x.h.
// Replaces BitFlipDecoder / decode! / batchdecode! of src/decoders/iterative_bitflip.jl:61-68, 116-201.
// Device code: bitflip_kernels.hpp.  Tiers (ldpc_bitflip_kernel):
//   1  on-chip, one wave per syndrome          n <= 2048 and <= 40 KiB of state (four workgroups a CU and more)
//   2  on-chip, one 16-wave workgroup per syndrome   state up to 159 KiB of LDS
//   3  unlimited: the state in a global workspace, one slot per workgroup of a persistent grid
//   4  unlimited with 64-bit vote accumulators (max_iters * max bit degree >= 2^31)
// No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "bitflip_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr size_t kBfWaveLds = (size_t)40 * 1024, kBfGroupLds = (size_t)159 * 1024;
static constexpr int kBfGroupWaves = 16;
static constexpr size_t kBfWorkspaceCap = (size_t)1 << 30;   // the unlimited tier's grid shrinks to keep its slots below this

struct ldpc_bitflip_decoder {
    int64_t s = 0, n = 0, nnz = 0, max_iters = 0;
    double per = 0.0;
    int device = 0, num_cus = 0, max_cdeg = 0, max_bdeg = 0, tier = 0, tie_break = 0, rw_shift = 0;
    uint64_t seed = 0;
    int *row_ptr = nullptr, *csr_col = nullptr, *col_ptr = nullptr, *csc_row = nullptr;
    void *stage = nullptr;      // device staging for the host-pointer entry
    size_t stage_cap = 0;
    unsigned char *ws = nullptr;   // tiers 3, 4: [grid][slot]
    size_t ws_cap = 0;
    bool kernel_ready = false;
    int per_cu = 1;
    ldpc_detail::CallOrder calls;   // calls on a handle run in call order whatever streams they are given (they share the workspace)
    ~ldpc_bitflip_decoder()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {row_ptr, csr_col, col_ptr, csc_row, stage, ws};
        for (void *q : all)
            if (q) (void)hipFree(q);
        calls.destroy();
    }
};

typedef void (*bf_kernel_t)(BfParams);

static bf_kernel_t bf_kernel_of(int tier)
{
    switch (tier) {
    case 1: return bitflip_kernel<1, false, int>;
    case 2: return bitflip_kernel<kBfGroupWaves, false, int>;
    case 3: return bitflip_kernel<kBfGroupWaves, true, int>;
    default: return bitflip_kernel<kBfGroupWaves, true, long long>;
    }
}

extern "C" {

ldpc_status ldpc_bitflip_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                                double per, int64_t max_iters, const ldpc_bitflip_options *options,
                                ldpc_bitflip_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, max_iters);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    const int tie = options ? options->tie_break : LDPC_BF_TIE_RANDOM, variant = options ? options->kernel_variant : 0;
    int device = options ? options->device : -1;
    if (tie < 0 || tie > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "tie_break must be LDPC_BF_TIE_RANDOM, _FIRST or _LAST");
    if (variant < 0 || variant > 3) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1, 2 or 3");
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "bit-flip kernels: graph too large for 32-bit edge indexing");

    ldpc_bitflip_decoder *d = new (std::nothrow) ldpc_bitflip_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->max_iters = max_iters; d->per = per;
    d->device = device; d->num_cus = prop.multiProcessorCount;
    d->tie_break = tie; d->seed = options ? options->seed : 0;
    // CSR (checks -> bits, ascending) next to the caller's CSC
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    d->max_cdeg = g.max_cdeg; d->max_bdeg = g.max_bdeg;
    while ((1 << d->rw_shift) < d->max_cdeg) d->rw_shift++;
    // |votes[j]| <= max_iters * deg[j]: 32-bit accumulators are exact below 2^31, beyond that the 64-bit kernel decodes
    const bool wide_votes = max_iters * (int64_t)d->max_bdeg >= ((int64_t)1 << 31);
    const size_t state = bf_state_bytes(s, n, 4);
    const bool fits1 = !wide_votes && n <= 2048 && state <= kBfWaveLds, fits2 = !wide_votes && state <= kBfGroupLds;
    if ((variant == 1 && !fits1) || (variant == 2 && !fits2)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant: the state of a syndrome does not fit that on-chip tier");
    }
    d->tier = wide_votes ? 4 : variant ? variant : fits1 ? 1 : fits2 ? 2 : 3;
    using ldpc_detail::upload;
    if (!upload(&d->row_ptr, g.row_ptr) || !upload(&d->csr_col, g.csr_col) || !upload(&d->col_ptr, g.col_ptr) ||
        !upload(&d->csc_row, g.csc_row) || d->calls.create() != hipSuccess) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

int32_t ldpc_bitflip_kernel(const ldpc_bitflip_decoder *d) { return d ? d->tier : 0; }

ldpc_status ldpc_bitflip_destroy(ldpc_bitflip_decoder *d)
{
    if (!d) return LDPC_OK;
    (void)hipSetDevice(d->device);
    const ldpc_status st = ldpc_detail::wait_device(d->device, "ldpc_bitflip_destroy (device synchronise)");
    delete d;
    return st;
}

ldpc_status ldpc_bitflip_decode_batch_device(ldpc_bitflip_decoder *d, int64_t batch, int64_t column0, const uint8_t *d_syn,
                                             uint8_t *d_err, uint8_t *d_conv, int32_t *d_iters, uint8_t *d_stop,
                                             void *stream_v)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (column0 < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative column0");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !d_syn) || (d->n > 0 && !d_err) || !d_conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(d->device));
    if (ldpc_detail::device_stalled(d->device)) return ldpc_detail::stalled_error(d->device);
    ldpc_status st = d->calls.enter(stream);
    if (st != LDPC_OK) return st;
    if (d->max_iters == 0) {   // the loop at :121 never runs: err = 0, converged = false
        if (d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        if (d_stop) LDPC_HIP_TRY(hipMemsetAsync(d_stop, 0, (size_t)batch, stream));
    } else {
        const bool global = d->tier >= 3;
        const int threads = d->tier == 1 ? 64 : kBfGroupWaves * 64;
        const size_t state = bf_state_bytes(d->s, d->n, d->tier == 4 ? 8 : 4);
        const size_t lds = global ? 0 : state;
        bf_kernel_t k = bf_kernel_of(d->tier);
        if (!d->kernel_ready) {
            if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            d->per_cu = ldpc_detail::blocks_per_cu((const void *)k, threads, lds);
            d->kernel_ready = true;
        }
        int64_t grid = std::min<int64_t>(batch, (int64_t)d->per_cu * d->num_cus);
        if (global) {
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(kBfWorkspaceCap / state)));
            st = ldpc_detail::grow_device_buffer((void **)&d->ws, &d->ws_cap, (size_t)grid * state, d->device,
                                                 "bit-flip workspace regrow (device synchronise before the free)");
            if (st != LDPC_OK) return st;
        }
        BfParams p{};
        p.s = (int)d->s; p.n = (int)d->n; p.max_iters = (int)d->max_iters; p.tie_break = d->tie_break; p.rw_shift = d->rw_shift;
        p.batch = batch; p.column0 = column0; p.seed = d->seed;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.stop = d_stop; p.iters = d_iters;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.col_ptr = d->col_ptr; p.csc_row = d->csc_row;
        p.ws = d->ws; p.slot_bytes = (long long)state;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
    }
    return d->calls.leave(stream);
}

ldpc_status ldpc_bitflip_decode_batch(ldpc_bitflip_decoder *d, int64_t batch, int64_t column0, const uint8_t *syn,
                                      uint8_t *err, uint8_t *conv, int32_t *iters, uint8_t *stop)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (column0 < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative column0");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    LDPC_HIP_TRY(hipSetDevice(d->device));
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [syndromes][errors][converged][iterations][stopped]
    image.take(B * s);
    const size_t o_err = image.take(B * n), o_conv = image.take(B), o_it = image.take(B * 4), o_stop = image.take(B), total = image.at;
    ldpc_status st = ldpc_detail::grow_device_buffer(&d->stage, &d->stage_cap, total, d->device, "bit-flip staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    char *dp = (char *)d->stage;
    if (s > 0) LDPC_HIP_TRY(hipMemcpyAsync(dp, syn, B * s, hipMemcpyHostToDevice, nullptr));
    st = ldpc_bitflip_decode_batch_device(d, batch, column0, (const uint8_t *)dp, (uint8_t *)(dp + o_err),
                                                      (uint8_t *)(dp + o_conv), (int32_t *)(dp + o_it), (uint8_t *)(dp + o_stop), nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) LDPC_HIP_TRY(hipMemcpyAsync(err, dp + o_err, B * n, hipMemcpyDeviceToHost, nullptr));
    LDPC_HIP_TRY(hipMemcpyAsync(conv, dp + o_conv, B, hipMemcpyDeviceToHost, nullptr));
    if (iters) LDPC_HIP_TRY(hipMemcpyAsync(iters, dp + o_it, B * 4, hipMemcpyDeviceToHost, nullptr));
    if (stop) LDPC_HIP_TRY(hipMemcpyAsync(stop, dp + o_stop, B, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, d->device, "ldpc_bitflip_decode_batch (stream synchronise)");
}

}  // extern "C"
