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

#include "host_wait.hpp"   // set_error, and the bounded forms of every host-side wait
using ldpc_detail::set_error;

#define BF_TRY(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (void)hipGetLastError();                                                         \
            return set_error(e_ == hipErrorOutOfMemory ? LDPC_ERR_OUT_OF_MEMORY : LDPC_ERR_HIP, \
                             std::string(#expr) + ": " + hipGetErrorString(e_));             \
        }                                                                                    \
    } while (0)

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
    // calls on a handle run in call order whatever streams they are given (they share the workspace)
    hipEvent_t last_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    ~ldpc_bitflip_decoder()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {row_ptr, csr_col, col_ptr, csc_row, stage, ws};
        for (void *q : all)
            if (q) (void)hipFree(q);
        if (last_done) (void)hipEventDestroy(last_done);
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
    if (s < 0 || n < 0 || nnz < 0 || !colptr || (nnz > 0 && !rowval) || max_iters < 0 || max_iters > INT32_MAX)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "bad dimensions / NULL pattern / max_iters");
    if (colptr[0] != 0 || colptr[n] != nnz) return set_error(LDPC_ERR_INVALID_ARGUMENT, "colptr is not a zero-based CSC pointer array");
    for (int64_t j = 0; j < n; ++j) {
        if (colptr[j + 1] < colptr[j]) return set_error(LDPC_ERR_INVALID_ARGUMENT, "colptr is not non-decreasing");
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
            if (rowval[k] < 0 || rowval[k] >= s) return set_error(LDPC_ERR_INVALID_ARGUMENT, "rowval entry outside [0, s)");
            if (k > colptr[j] && rowval[k] <= rowval[k - 1])
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "row indices must be strictly ascending inside each column");
        }
    }
    const int tie = options ? options->tie_break : LDPC_BF_TIE_RANDOM, variant = options ? options->kernel_variant : 0;
    int device = options ? options->device : -1;
    if (tie < 0 || tie > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "tie_break must be LDPC_BF_TIE_RANDOM, _FIRST or _LAST");
    if (variant < 0 || variant > 3) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1, 2 or 3");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return set_error(LDPC_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    }
    if (device < 0) BF_TRY(hipGetDevice(&device));
    if (device >= ndev) return set_error(LDPC_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    BF_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    BF_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(LDPC_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "bit-flip kernels: graph too large for 32-bit edge indexing");

    ldpc_bitflip_decoder *d = new (std::nothrow) ldpc_bitflip_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->max_iters = max_iters; d->per = per;
    d->device = device; d->num_cus = prop.multiProcessorCount;
    d->tie_break = tie; d->seed = options ? options->seed : 0;
    // CSR (checks -> bits, ascending) next to the caller's CSC
    std::vector<int> row_ptr((size_t)s + 1, 0), col_ptr((size_t)n + 1), csr_col((size_t)std::max<int64_t>(nnz, 1)),
        csc_row((size_t)std::max<int64_t>(nnz, 1));
    for (int64_t k = 0; k < nnz; ++k) row_ptr[(size_t)rowval[k] + 1]++;
    for (int64_t i = 0; i < s; ++i) {
        d->max_cdeg = std::max(d->max_cdeg, row_ptr[(size_t)i + 1]);
        row_ptr[(size_t)i + 1] += row_ptr[(size_t)i];
    }
    {
        std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1);
        for (int64_t j = 0; j < n; ++j) {
            col_ptr[(size_t)j] = (int)colptr[j];
            d->max_bdeg = std::max(d->max_bdeg, (int)(colptr[j + 1] - colptr[j]));
            for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
                csr_col[(size_t)fill[(size_t)rowval[k]]++] = (int)j;
                csc_row[(size_t)k] = (int)rowval[k];
            }
        }
        col_ptr[(size_t)n] = (int)nnz;
    }
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
    auto up = [&](int *&dst, const std::vector<int> &v) -> bool {
        if (hipMalloc((void **)&dst, std::max<size_t>(v.size(), 1) * sizeof(int)) != hipSuccess) return false;
        return hipMemcpy(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(d->row_ptr, row_ptr) || !up(d->csr_col, csr_col) || !up(d->col_ptr, col_ptr) || !up(d->csc_row, csc_row) ||
        hipEventCreateWithFlags(&d->last_done, hipEventDisableTiming) != hipSuccess) {
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
    BF_TRY(hipSetDevice(d->device));
    if (ldpc_detail::device_stalled(d->device)) return ldpc_detail::stalled_error(d->device);
    if (d->have_last && d->last_stream != stream) BF_TRY(hipStreamWaitEvent(stream, d->last_done, 0));
    if (d->max_iters == 0) {   // the loop at :121 never runs: err = 0, converged = false
        if (d->n > 0) BF_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        BF_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_iters) BF_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        if (d_stop) BF_TRY(hipMemsetAsync(d_stop, 0, (size_t)batch, stream));
    } else {
        const bool global = d->tier >= 3;
        const int threads = d->tier == 1 ? 64 : kBfGroupWaves * 64;
        const size_t state = bf_state_bytes(d->s, d->n, d->tier == 4 ? 8 : 4);
        const size_t lds = global ? 0 : state;
        bf_kernel_t k = bf_kernel_of(d->tier);
        if (!d->kernel_ready) {
            if (lds) BF_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k, threads, lds) != hipSuccess || per_cu <= 0) {
                (void)hipGetLastError();
                per_cu = 1;
            }
            d->per_cu = per_cu;
            d->kernel_ready = true;
        }
        int64_t grid = std::min<int64_t>(batch, (int64_t)d->per_cu * d->num_cus);
        if (global) {
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(kBfWorkspaceCap / state)));
            if (d->ws_cap < (size_t)grid * state) {
                if (d->ws) {
                    const ldpc_status ws = ldpc_detail::wait_device(d->device, "bit-flip workspace regrow (device synchronise before the free)");
                    if (ws != LDPC_OK) return ws;
                    (void)hipFree(d->ws);
                }
                d->ws = nullptr; d->ws_cap = 0;
                BF_TRY(hipMalloc((void **)&d->ws, (size_t)grid * state));
                d->ws_cap = (size_t)grid * state;
            }
        }
        BfParams p{};
        p.s = (int)d->s; p.n = (int)d->n; p.max_iters = (int)d->max_iters; p.tie_break = d->tie_break; p.rw_shift = d->rw_shift;
        p.batch = batch; p.column0 = column0; p.seed = d->seed;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.stop = d_stop; p.iters = d_iters;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.col_ptr = d->col_ptr; p.csc_row = d->csc_row;
        p.ws = d->ws; p.slot_bytes = (long long)state;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        BF_TRY(hipGetLastError());
    }
    BF_TRY(hipEventRecord(d->last_done, stream));
    d->last_stream = stream; d->have_last = true;
    return LDPC_OK;
}

ldpc_status ldpc_bitflip_decode_batch(ldpc_bitflip_decoder *d, int64_t batch, int64_t column0, const uint8_t *syn,
                                      uint8_t *err, uint8_t *conv, int32_t *iters, uint8_t *stop)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (column0 < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative column0");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    BF_TRY(hipSetDevice(d->device));
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_err = up(B * s), o_conv = o_err + up(B * n), o_it = o_conv + up(B), o_stop = o_it + up(B * 4),
                 total = o_stop + up(B);
    if (d->stage_cap < total) {
        if (d->stage) {
            const ldpc_status ws = ldpc_detail::wait_device(d->device, "bit-flip staging regrow (device synchronise before the free)");
            if (ws != LDPC_OK) return ws;
            (void)hipFree(d->stage);
        }
        d->stage = nullptr; d->stage_cap = 0;
        BF_TRY(hipMalloc(&d->stage, total));
        d->stage_cap = total;
    }
    char *dp = (char *)d->stage;
    if (s > 0) BF_TRY(hipMemcpyAsync(dp, syn, B * s, hipMemcpyHostToDevice, nullptr));
    ldpc_status st = ldpc_bitflip_decode_batch_device(d, batch, column0, (const uint8_t *)dp, (uint8_t *)(dp + o_err),
                                                      (uint8_t *)(dp + o_conv), (int32_t *)(dp + o_it), (uint8_t *)(dp + o_stop), nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) BF_TRY(hipMemcpyAsync(err, dp + o_err, B * n, hipMemcpyDeviceToHost, nullptr));
    BF_TRY(hipMemcpyAsync(conv, dp + o_conv, B, hipMemcpyDeviceToHost, nullptr));
    if (iters) BF_TRY(hipMemcpyAsync(iters, dp + o_it, B * 4, hipMemcpyDeviceToHost, nullptr));
    if (stop) BF_TRY(hipMemcpyAsync(stop, dp + o_stop, B, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, d->device, "ldpc_bitflip_decode_batch (stream synchronise)");
}

}  // extern "C"
