// ldpc_trials.hip -- host side of the Monte-Carlo trial steps: the ldpc_trials_* entry points of include/ldpc_mi355x.h.
// What the reference does around every decode on the host (test/test_bp_decoder.jl:19-30: rand(n, B) .< per,
// H * errors .% 2, guesses[:, i] == errors[:, i]) as device-resident steps.  Device code: trial_kernels.hpp.
// Tiers (ldpc_trials_kernel): 1 = a column's bits in an LDS image while its checks are walked, 2 = unlimited.
// No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "trial_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

using namespace ldpc_trials_k;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr size_t kTrialsImageLds = (size_t)159 * 1024;
static constexpr int kTrialsWaveColumn = 4096;   // columns up to this many bits take one wave each, four to a workgroup

struct ldpc_trials {
    int64_t s = 0, n = 0, nl = 0;
    int device = 0, num_cus = 0, tier = 0, wpc = 1, cpl = 1, image_stride = 0;
    int *row_ptr = nullptr, *csr_col = nullptr, *lrow_ptr = nullptr, *lcsr_col = nullptr;   // CSR of H and of L (the walks go check by check)
    void *stage = nullptr;      // device staging for the host-pointer entries
    size_t stage_cap = 0;
    int per_cu[3] = {0, 0, 0};  // workgroups a CU holds, per step (0 = not asked yet)
    ldpc_detail::CallOrder calls;
    ~ldpc_trials()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {row_ptr, csr_col, lrow_ptr, lcsr_col, stage};
        for (void *q : all)
            if (q) (void)hipFree(q);
        calls.destroy();
    }
};

typedef void (*trial_kernel_t)(TrialParams);

template <int MODE>
static trial_kernel_t trial_kernel_of(int wpc, bool image)
{
    if (wpc == 1) return image ? trial_kernel<1, MODE, true> : trial_kernel<1, MODE, false>;
    return image ? trial_kernel<4, MODE, true> : trial_kernel<4, MODE, false>;
}

static trial_kernel_t trial_kernel_of(int mode, int wpc, bool image)
{
    switch (mode) {
    case kSample: return trial_kernel_of<kSample>(wpc, image);
    case kSyndromes: return trial_kernel_of<kSyndromes>(wpc, image);
    default: return trial_kernel_of<kScore>(wpc, image);
    }
}

// One step: the arguments are checked, the handle is not NULL, batch > 0.
static ldpc_status trials_launch(ldpc_trials *t, int mode, TrialParams p, int64_t batch, hipStream_t stream)
{
    // (2^36: with the grid below, no workgroup's 32-bit running counts of the score step can wrap)
    if (batch > ((int64_t)1 << 36)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call (more than 2^36 columns)");
    LDPC_HIP_TRY(hipSetDevice(t->device));
    if (ldpc_detail::device_stalled(t->device)) return ldpc_detail::stalled_error(t->device);
    ldpc_status st = t->calls.enter(stream);
    if (st != LDPC_OK) return st;
    const bool image = t->tier == 1;
    const int cpb = kThreads / (64 * t->wpc);
    const size_t lds = image ? (size_t)cpb * t->image_stride * sizeof(unsigned short) : 0;
    trial_kernel_t k = trial_kernel_of(mode, t->wpc, image);
    if (!t->per_cu[mode]) {
        // always the whole budget, never this handle's own size: the cap belongs to the kernel, not to the handle, and a
        // later handle of a smaller n must not lower it under an earlier, larger one
        if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrialsImageLds));
        t->per_cu[mode] = std::min(8, ldpc_detail::blocks_per_cu((const void *)k, kThreads, lds));
    }
    p.s = (int)t->s; p.n = (int)t->n; p.nl = (int)t->nl; p.cpl = t->cpl; p.image_stride = t->image_stride; p.batch = batch;
    p.row_ptr = t->row_ptr; p.csr_col = t->csr_col; p.lrow_ptr = t->lrow_ptr; p.lcsr_col = t->lcsr_col;
    const int64_t ngroups = (batch + cpb - 1) / cpb;
    const int64_t grid = std::min<int64_t>(ngroups, (int64_t)t->per_cu[mode] * std::max(t->num_cus, 32));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)kThreads), lds, stream, p);
    LDPC_HIP_TRY(hipGetLastError());
    return t->calls.leave(stream);
}

static ldpc_status check_sample_args(int64_t batch, int64_t column0, double per, const void *errors)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (column0 < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative column0");
    if (!(per >= 0.0 && per <= 1.0)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "per must lie in [0, 1] (and not be NaN)");
    if (batch > 0 && !errors) return set_error(LDPC_ERR_INVALID_ARGUMENT, "errors pointer is NULL");
    return LDPC_OK;
}

static ldpc_status check_score_args(int64_t batch, const void *guesses, const void *errors, const void *counts)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch > 0 && !guesses) return set_error(LDPC_ERR_INVALID_ARGUMENT, "guesses pointer is NULL");
    if (batch > 0 && !errors) return set_error(LDPC_ERR_INVALID_ARGUMENT, "errors pointer is NULL");
    if (batch > 0 && !counts) return set_error(LDPC_ERR_INVALID_ARGUMENT, "counts pointer is NULL");
    return LDPC_OK;
}

extern "C" {

ldpc_status ldpc_trials_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                               int64_t nl, int64_t lnnz, const int64_t *lcolptr, const int64_t *lrowval,
                               const ldpc_trials_options *options, ldpc_trials **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, 0);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    if (nl < 0 || lnnz < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative dimension of the logical rows (nl, lnnz)");
    const bool have_l = nl > 0;
    if (!have_l && lnnz != 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "lnnz must be 0 when nl is 0");
    if (have_l) {
        if (!lcolptr || (lnnz > 0 && !lrowval)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "lcolptr/lrowval is NULL although nl > 0");
        if ((st = ldpc_detail::check_csc_pattern(nl, n, lnnz, lcolptr, lrowval)) != LDPC_OK)
            return set_error(st, "logical rows: " + ldpc_detail::last_error());
    }
    const int variant = options ? options->kernel_variant : 0;
    int device = options ? options->device : -1;
    if (variant < 0 || variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    const int64_t lim = (int64_t)1 << 28;
    if (nnz >= lim || s >= lim || n >= lim || nl >= lim || lnnz >= lim)
        return set_error(LDPC_ERR_UNSUPPORTED, "trial kernels: graph too large for 32-bit edge indexing");

    ldpc_trials *t = new (std::nothrow) ldpc_trials();
    if (!t) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    t->s = s; t->n = n; t->nl = nl; t->device = device; t->num_cus = prop.multiProcessorCount;
    t->wpc = n <= kTrialsWaveColumn ? 1 : 4;
    t->image_stride = (image_words(n) + 7) & ~7;   // (16-byte granules)
    t->cpl = s >= 4 * 64 * (int64_t)t->wpc ? 4 : 1;
    const bool fits = (size_t)(kThreads / (64 * t->wpc)) * t->image_stride * sizeof(unsigned short) <= kTrialsImageLds;
    if (variant == 1 && !fits) {
        delete t;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the bit image of a column does not fit the LDS");
    }
    t->tier = variant ? variant : fits ? 1 : 2;
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    using ldpc_detail::upload_ints;
    bool ok = upload_ints(&t->row_ptr, g.row_ptr) && upload_ints(&t->csr_col, g.csr_col);
    if (ok && have_l) {
        const ldpc_detail::TannerGraph gl = ldpc_detail::tanner_graph(nl, n, lnnz, lcolptr, lrowval);
        ok = upload_ints(&t->lrow_ptr, gl.row_ptr) && upload_ints(&t->lcsr_col, gl.csr_col);
    }
    if (!ok || t->calls.create() != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = t;
    return LDPC_OK;
}

int32_t ldpc_trials_kernel(const ldpc_trials *t) { return t ? t->tier : 0; }

ldpc_status ldpc_trials_destroy(ldpc_trials *t)
{
    if (!t) return LDPC_OK;
    (void)hipSetDevice(t->device);
    const ldpc_status st = ldpc_detail::wait_device(t->device, "ldpc_trials_destroy (device synchronise)");
    delete t;
    return st;
}

ldpc_status ldpc_trials_sample_device(ldpc_trials *t, int64_t batch, int64_t column0, double per, uint64_t seed,
                                      uint8_t *d_errors, uint8_t *d_syndromes, void *stream)
{
    const ldpc_status st = check_sample_args(batch, column0, per, d_errors);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    TrialParams p{};
    p.column0 = (tu64)column0; p.seed = seed;
    p.all_ones = per >= 1.0;
    p.threshold = per >= 1.0 ? ~0ull : (tu64)(per * 18446744073709551616.0);
    p.err_out = d_errors; p.syn = t->s > 0 ? d_syndromes : nullptr;
    return trials_launch(t, kSample, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_syndromes_device(ldpc_trials *t, int64_t batch, const uint8_t *d_errors, uint8_t *d_syndromes,
                                         void *stream)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch > 0 && !d_errors) return set_error(LDPC_ERR_INVALID_ARGUMENT, "errors pointer is NULL");
    if (batch > 0 && !d_syndromes) return set_error(LDPC_ERR_INVALID_ARGUMENT, "syndromes pointer is NULL");
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0 || t->s == 0) return LDPC_OK;
    TrialParams p{};
    p.err = d_errors; p.syn = d_syndromes;
    return trials_launch(t, kSyndromes, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_score_device(ldpc_trials *t, int64_t batch, const uint8_t *d_guesses, const uint8_t *d_errors,
                                     uint8_t *d_flags, int64_t *d_counts, void *stream)
{
    const ldpc_status st = check_score_args(batch, d_guesses, d_errors, d_counts);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    TrialParams p{};
    p.guess = d_guesses; p.err = d_errors; p.flags = d_flags; p.counts = (tu64 *)d_counts;
    return trials_launch(t, kScore, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_sample(ldpc_trials *t, int64_t batch, int64_t column0, double per, uint64_t seed, uint8_t *errors,
                               uint8_t *syndromes)
{
    ldpc_status st = check_sample_args(batch, column0, per, errors);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(t->device));
    const size_t s = (size_t)t->s, n = (size_t)t->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [errors][syndromes]
    image.take(B * n);
    const size_t o_syn = image.take(B * s);
    st = ldpc_detail::grow_device_buffer(&t->stage, &t->stage_cap, std::max<size_t>(image.at, 256), t->device,
                                         "trials staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    uint8_t *dp = (uint8_t *)t->stage;
    const bool want_syn = syndromes && s > 0;
    st = ldpc_trials_sample_device(t, batch, column0, per, seed, dp, want_syn ? dp + o_syn : nullptr, nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) LDPC_HIP_TRY(hipMemcpyAsync(errors, dp, B * n, hipMemcpyDeviceToHost, nullptr));
    if (want_syn) LDPC_HIP_TRY(hipMemcpyAsync(syndromes, dp + o_syn, B * s, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, t->device, "ldpc_trials_sample (stream synchronise)");
}

ldpc_status ldpc_trials_score(ldpc_trials *t, int64_t batch, const uint8_t *guesses, const uint8_t *errors, uint8_t *flags,
                              int64_t counts[4])
{
    ldpc_status st = check_score_args(batch, guesses, errors, counts);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(t->device));
    const size_t n = (size_t)t->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [guesses][errors][flags][counts]
    image.take(B * n);
    const size_t o_err = image.take(B * n), o_flags = image.take(B), o_counts = image.take(4 * sizeof(int64_t));
    st = ldpc_detail::grow_device_buffer(&t->stage, &t->stage_cap, image.at, t->device,
                                         "trials staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    uint8_t *dp = (uint8_t *)t->stage;
    if (n > 0) {
        LDPC_HIP_TRY(hipMemcpyAsync(dp, guesses, B * n, hipMemcpyHostToDevice, nullptr));
        LDPC_HIP_TRY(hipMemcpyAsync(dp + o_err, errors, B * n, hipMemcpyHostToDevice, nullptr));
    }
    LDPC_HIP_TRY(hipMemcpyAsync(dp + o_counts, counts, 4 * sizeof(int64_t), hipMemcpyHostToDevice, nullptr));
    st = ldpc_trials_score_device(t, batch, dp, dp + o_err, dp + o_flags, (int64_t *)(dp + o_counts), nullptr);
    if (st != LDPC_OK) return st;
    if (flags) LDPC_HIP_TRY(hipMemcpyAsync(flags, dp + o_flags, B, hipMemcpyDeviceToHost, nullptr));
    LDPC_HIP_TRY(hipMemcpyAsync(counts, dp + o_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, t->device, "ldpc_trials_score (stream synchronise)");
}

}  // extern "C"
