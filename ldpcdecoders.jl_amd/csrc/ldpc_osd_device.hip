// ldpc_osd_device.hip -- host side of the opt-in DEVICE form of the BP+OSD ordered-statistics step: the
// ldpc_osd_device_* / ldpc_osd_postprocess_batch_device entry points of include/ldpc_mi355x.h, on the `ldpc_osd`
// handle of osd_host.cpp (whose host form stays the default).  Device code and the rule it states: osd_kernels.hpp.
// Tiers (ldpc_osd_device_kernel), by the state of one syndrome (osd_state_bytes: the working rows, (n/64 + 1 made odd)
// words each, + 12 n + 4 s bytes + the candidate bitsets):
//   1  on-chip, one wave per syndrome            s <= 128, n <= 512 (<= 17 KiB of LDS: nine workgroups a CU and more)
//   2  on-chip, one 16-wave workgroup per syndrome   state up to 159 KiB of LDS
//   3  unlimited: the state in a global workspace, one slot per workgroup of a persistent grid, slots capped at 1 GiB
// A handle on the standard rule (ldpc_osd_set_search, method 1 or 2) runs osd_search_kernel (osd_search_kernels.hpp) in the
// same three tiers, bounded by ITS state (osd_search_state_bytes: 16 n + 12 s bytes + 65 row bitsets beside the rows).
// No CPU path behind these entries.
#include "../../include/ldpc_mi355x.h"
#include "osd_handle.hpp"
#include "osd_kernels.hpp"
#include "osd_search_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, select_device, CallOrder and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr int64_t kOsdWaveRows = 128, kOsdWaveCols = 512;
static constexpr size_t kOsdGroupLds = (size_t)159 * 1024;
static constexpr int kOsdGroupWaves = 16;
static constexpr size_t kOsdWorkspaceCap = (size_t)1 << 30;   // the unlimited tier's grid shrinks to keep its slots below this

namespace {

struct OsdDevice {
    int device = 0, num_cus = 0, tier = 0, per_cu = 1, threads = 64;
    size_t state = 0, lds = 0;
    osd_u64 *rows = nullptr;
    long long *q = nullptr;        // standard rule with weights: [n]
    unsigned char *ws = nullptr;   // tier 3: [grid][state]
    int64_t ws_grid = 0;
    ldpc_detail::CallOrder calls;   // calls on a handle run in call order whatever streams they are given (tier 3: they share the workspace)
};

typedef void (*osd_kernel_t)(OsdParams);

osd_kernel_t osd_kernel_of(int tier)
{
    switch (tier) {
    case 1: return osd_kernel<1, false>;
    case 2: return osd_kernel<kOsdGroupWaves, false>;
    default: return osd_kernel<kOsdGroupWaves, true>;
    }
}

static_assert(kOsdSearchExhaustiveCap <= 16 && kOsdSearchSweepCap <= kOsdSearchCols, "the search kernel holds 64 column bitsets and counts 2^16 subsets");
typedef void (*osd_search_kernel_t)(OsdSearchParams);

osd_search_kernel_t osd_search_kernel_of(int tier)
{
    switch (tier) {
    case 1: return osd_search_kernel<1, false>;
    case 2: return osd_search_kernel<kOsdGroupWaves, false>;
    default: return osd_search_kernel<kOsdGroupWaves, true>;
    }
}

void osd_device_free(void *v)
{
    OsdDevice *dv = (OsdDevice *)v;
    if (!dv) return;
    // (host_wait.hpp: nothing a stalled device may still use is freed)
    if (!ldpc_detail::device_stalled(dv->device) &&
        ldpc_detail::device_idle_for_release(dv->device, "ldpc_osd_destroy (device synchronise)")) {
        if (dv->rows) (void)hipFree(dv->rows);
        if (dv->q) (void)hipFree(dv->q);
        if (dv->ws) (void)hipFree(dv->ws);
        dv->calls.destroy();
    }
    delete dv;
}

}  // namespace

extern "C" {

int32_t ldpc_osd_device_kernel(const ldpc_osd *d) { return d && d->dev ? ((const OsdDevice *)d->dev)->tier : 0; }

ldpc_status ldpc_osd_device_prepare(ldpc_osd *d, int32_t device, int32_t kernel_variant)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "osd handle is NULL");
    if (kernel_variant < 0 || kernel_variant > 3) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1, 2 or 3");
    if (d->dev) return set_error(LDPC_ERR_INVALID_ARGUMENT, "osd handle is already prepared for a device");
    const bool search = d->method != 0;   // (ldpc_osd_set_search has bounded its order and n)
    if (!search && d->order > kOsdMaxOrder)
        return set_error(LDPC_ERR_UNSUPPORTED, "device OSD runs osd_order <= 16 (2^16 candidates per syndrome); use the host entry beyond");
    if (d->m >= ((int64_t)1 << 24) || d->n >= ((int64_t)1 << 24))
        return set_error(LDPC_ERR_UNSUPPORTED, "device OSD: graph too large for 32-bit row indexing");
    const size_t state = search ? osd_search_state_bytes(d->m, d->n) : osd_state_bytes(d->m, d->n);
    const bool fits1 = d->m <= kOsdWaveRows && d->n <= kOsdWaveCols, fits2 = state <= kOsdGroupLds;
    if ((kernel_variant == 1 && !fits1) || (kernel_variant == 2 && !fits2))
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant: the state of a syndrome does not fit that on-chip tier");
    if (state > kOsdWorkspaceCap) return set_error(LDPC_ERR_UNSUPPORTED, "device OSD: the state of one syndrome exceeds the workspace cap");
    hipDeviceProp_t prop;
    const ldpc_status sel = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (the device OSD entries have no CPU fallback)");
    if (sel != LDPC_OK) return sel;

    OsdDevice *dv = new (std::nothrow) OsdDevice();
    if (!dv) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    dv->device = device; dv->num_cus = prop.multiProcessorCount; dv->state = state;
    dv->tier = kernel_variant ? kernel_variant : fits1 ? 1 : fits2 ? 2 : 3;
    dv->threads = dv->tier == 1 ? 64 : kOsdGroupWaves * 64;
    dv->lds = dv->tier == 3 ? 0 : state;
    auto fail = [&](ldpc_status st, const std::string &msg) {
        (void)hipGetLastError();
        osd_device_free(dv);
        return set_error(st, msg);
    };
    const size_t row_bytes = std::max<size_t>(d->rows.size(), 1) * sizeof(osd_u64);
    if (hipMalloc((void **)&dv->rows, row_bytes) != hipSuccess) return fail(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the packed rows failed");
    if (!d->rows.empty() && hipMemcpy(dv->rows, d->rows.data(), d->rows.size() * sizeof(osd_u64), hipMemcpyHostToDevice) != hipSuccess)
        return fail(LDPC_ERR_HIP, "upload of the packed rows failed");
    if (dv->calls.create() != hipSuccess) return fail(LDPC_ERR_HIP, "hipEventCreate failed");
    if (search && !d->q.empty()) {
        if (hipMalloc((void **)&dv->q, d->q.size() * sizeof(long long)) != hipSuccess) return fail(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the weights failed");
        if (hipMemcpy(dv->q, d->q.data(), d->q.size() * sizeof(long long), hipMemcpyHostToDevice) != hipSuccess)
            return fail(LDPC_ERR_HIP, "upload of the weights failed");
    }
    const void *k = search ? (const void *)osd_search_kernel_of(dv->tier) : (const void *)osd_kernel_of(dv->tier);
    if (dv->lds && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dv->lds) != hipSuccess)
        return fail(LDPC_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    const int per_cu = dv->per_cu = ldpc_detail::blocks_per_cu(k, dv->threads, dv->lds);
    if (dv->tier == 3) {
        dv->ws_grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)per_cu * dv->num_cus, (int64_t)(kOsdWorkspaceCap / state)));
        if (hipMalloc((void **)&dv->ws, (size_t)dv->ws_grid * state) != hipSuccess)
            return fail(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the OSD workspace failed");
    }
    d->dev = dv;
    d->dev_free = osd_device_free;
    return LDPC_OK;
}

ldpc_status ldpc_osd_postprocess_batch_device(ldpc_osd *d, int64_t batch, const uint8_t *d_syndromes,
                                              const uint8_t *d_bp_errors, const double *d_llr, uint8_t *d_errors,
                                              void *stream_v)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "osd handle is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (!d->dev) return set_error(LDPC_ERR_INVALID_ARGUMENT, "osd handle is not prepared (ldpc_osd_device_prepare)");
    if (batch == 0) return LDPC_OK;
    if ((d->m > 0 && !d_syndromes) || (d->n > 0 && (!d_bp_errors || !d_llr || !d_errors)))
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    if (d->n == 0) return LDPC_OK;   // nothing to write
    OsdDevice *dv = (OsdDevice *)d->dev;
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(dv->device));
    if (ldpc_detail::device_stalled(dv->device)) return ldpc_detail::stalled_error(dv->device);
    const ldpc_status ent = dv->calls.enter(stream);
    if (ent != LDPC_OK) return ent;
    int64_t grid = std::min<int64_t>(batch, (int64_t)dv->per_cu * dv->num_cus);
    if (dv->tier == 3) grid = std::min<int64_t>(grid, dv->ws_grid);
    if (d->method != 0) {
        OsdSearchParams p{};
        p.m = (int)d->m; p.n = (int)d->n; p.nw = (int)d->nw; p.st = (int)osd_stride(d->nw); p.mw = (int)((d->m + 63) >> 6);
        p.method = (int)d->method; p.order = (int)d->order; p.batch = batch;
        p.syn = d_syndromes; p.bp = d_bp_errors; p.llr = d_llr; p.out = d_errors;
        p.rows = dv->rows; p.q = dv->q; p.ws = dv->ws; p.slot_bytes = (long long)dv->state;
        hipLaunchKernelGGL(osd_search_kernel_of(dv->tier), dim3((unsigned)grid), dim3((unsigned)dv->threads), dv->lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
        return dv->calls.leave(stream);
    }
    OsdParams p{};
    p.m = (int)d->m; p.n = (int)d->n; p.nw = (int)d->nw; p.st = (int)osd_stride(d->nw); p.mw = (int)((d->m + 63) >> 6);
    p.order = (int)d->order; p.batch = batch;
    p.syn = d_syndromes; p.bp = d_bp_errors; p.llr = d_llr; p.out = d_errors;
    p.rows = dv->rows; p.ws = dv->ws; p.slot_bytes = (long long)dv->state;
    hipLaunchKernelGGL(osd_kernel_of(dv->tier), dim3((unsigned)grid), dim3((unsigned)dv->threads), dv->lds, stream, p);
    LDPC_HIP_TRY(hipGetLastError());
    return dv->calls.leave(stream);
}

}  // extern "C"
