// ldpc_css_trials.hip -- host side of the CSS-code Monte-Carlo trial steps: the ldpc_css_trials_* entry points of
// include/ldpc_mi355x.h.  Pauli errors on n qubits (one draw per qubit gives its X part and its Z part), the two
// syndromes sz = Hz ex and sx = Hx ez, and the joint score with logical X and logical Z failures, as device-resident
// steps around two decodes.  Device code: css_trial_kernels.hpp.
// Tiers (ldpc_css_trials_kernel): 1 = a column's two bit images in LDS while the checks are walked, 2 = unlimited.
// No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "css_trial_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

using namespace ldpc_css_k;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr size_t kCssImageLds = (size_t)159 * 1024;
static constexpr int kCssWaveColumn = 4096;   // columns up to this many qubits take one wave each, four to a workgroup

struct CssGraph {
    int64_t rows = 0;
    int *row_ptr = nullptr, *csr_col = nullptr;
};

struct ldpc_css_trials {
    int64_t n = 0;
    CssGraph hx, hz, lx, lz;    // CSRs on the device (the walks go check by check)
    int device = 0, num_cus = 0, tier = 0, wpc = 1, cplx = 1, cplz = 1, image_stride = 0;
    void *stage = nullptr;      // device staging for the host-pointer entries
    size_t stage_cap = 0;
    int per_cu[3] = {0, 0, 0};  // workgroups a CU holds, per step (0 = not asked yet)
    ldpc_detail::CallOrder calls;
    ~ldpc_css_trials()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {hx.row_ptr, hx.csr_col, hz.row_ptr, hz.csr_col, lx.row_ptr, lx.csr_col, lz.row_ptr, lz.csr_col, stage};
        for (void *q : all)
            if (q) (void)hipFree(q);
        calls.destroy();
    }
};

typedef void (*css_kernel_t)(CssParams);

template <int MODE>
static css_kernel_t css_kernel_of(int wpc, bool image)
{
    if (wpc == 1) return image ? css_trial_kernel<1, MODE, true> : css_trial_kernel<1, MODE, false>;
    return image ? css_trial_kernel<4, MODE, true> : css_trial_kernel<4, MODE, false>;
}

static css_kernel_t css_kernel_of(int mode, int wpc, bool image)
{
    switch (mode) {
    case kSample: return css_kernel_of<kSample>(wpc, image);
    case kSyndromes: return css_kernel_of<kSyndromes>(wpc, image);
    default: return css_kernel_of<kScore>(wpc, image);
    }
}

// One step: the arguments are checked, the handle is not NULL, batch > 0.
static ldpc_status css_launch(ldpc_css_trials *t, int mode, CssParams p, int64_t batch, hipStream_t stream)
{
    // (2^36: with the grid below, no workgroup's 32-bit running counts of the score step can wrap)
    if (batch > ((int64_t)1 << 36)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call (more than 2^36 columns)");
    LDPC_HIP_TRY(hipSetDevice(t->device));
    if (ldpc_detail::device_stalled(t->device)) return ldpc_detail::stalled_error(t->device);
    ldpc_status st = t->calls.enter(stream);
    if (st != LDPC_OK) return st;
    const bool image = t->tier == 1;
    const int cpb = kThreads / (64 * t->wpc);
    const size_t lds = image ? (size_t)cpb * 2 * t->image_stride * sizeof(unsigned short) : 0;
    css_kernel_t k = css_kernel_of(mode, t->wpc, image);
    if (!t->per_cu[mode]) {
        // always the whole budget, never this handle's own size: the cap belongs to the kernel, not to the handle, and a
        // later handle of a smaller n must not lower it under an earlier, larger one
        if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCssImageLds));
        t->per_cu[mode] = std::min(8, ldpc_detail::blocks_per_cu((const void *)k, kThreads, lds));
    }
    p.n = (int)t->n; p.rows_x = (int)t->hx.rows; p.rows_z = (int)t->hz.rows; p.nlx = (int)t->lx.rows; p.nlz = (int)t->lz.rows;
    p.cplx = t->cplx; p.cplz = t->cplz; p.image_stride = t->image_stride; p.batch = batch;
    p.hx_ptr = t->hx.row_ptr; p.hx_col = t->hx.csr_col; p.hz_ptr = t->hz.row_ptr; p.hz_col = t->hz.csr_col;
    p.lx_ptr = t->lx.row_ptr; p.lx_col = t->lx.csr_col; p.lz_ptr = t->lz.row_ptr; p.lz_col = t->lz.csr_col;
    const int64_t ngroups = (batch + cpb - 1) / cpb;
    const int64_t grid = std::min<int64_t>(ngroups, (int64_t)t->per_cu[mode] * std::max(t->num_cus, 32));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)kThreads), lds, stream, p);
    LDPC_HIP_TRY(hipGetLastError());
    return t->calls.leave(stream);
}

// (uint64)(rate * 2^64) for a rate in [0, 1): a power-of-two scaling, truncated
static bool rate_threshold(double rate, tu64 *t)
{
    if (!(rate >= 0.0 && rate < 1.0)) return false;
    *t = (tu64)(rate * 18446744073709551616.0);
    return true;
}

static ldpc_status check_sample_args(int64_t batch, int64_t column0, double px, double py, double pz, const void *ex, const void *ez,
                                     tu64 thresholds[3])
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (column0 < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative column0");
    tu64 tx, ty, tz;
    if (!rate_threshold(px, &tx) || !rate_threshold(py, &ty) || !rate_threshold(pz, &tz))
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "px, py and pz must each lie in [0, 1) (and not be NaN)");
    thresholds[0] = tx;
    if (__builtin_add_overflow(tx, ty, &thresholds[1]) || __builtin_add_overflow(thresholds[1], tz, &thresholds[2]))
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "px + py + pz: a sum of the thresholds overflows 64 bits (the rates sum to 1 or more)");
    if (batch > 0 && !ex) return set_error(LDPC_ERR_INVALID_ARGUMENT, "ex errors pointer is NULL");
    if (batch > 0 && !ez) return set_error(LDPC_ERR_INVALID_ARGUMENT, "ez errors pointer is NULL");
    return LDPC_OK;
}

static ldpc_status check_score_args(int64_t batch, const void *gx, const void *gz, const void *ex, const void *ez, const void *counts)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch > 0 && !gx) return set_error(LDPC_ERR_INVALID_ARGUMENT, "gx guesses pointer is NULL");
    if (batch > 0 && !gz) return set_error(LDPC_ERR_INVALID_ARGUMENT, "gz guesses pointer is NULL");
    if (batch > 0 && !ex) return set_error(LDPC_ERR_INVALID_ARGUMENT, "ex errors pointer is NULL");
    if (batch > 0 && !ez) return set_error(LDPC_ERR_INVALID_ARGUMENT, "ez errors pointer is NULL");
    if (batch > 0 && !counts) return set_error(LDPC_ERR_INVALID_ARGUMENT, "counts pointer is NULL");
    return LDPC_OK;
}

// One of the four patterns of a create: the checks of ldpc_trials_create, the message names the pattern.
static ldpc_status check_pattern(const char *name, const ldpc_css_pattern *m, int64_t n, bool required)
{
    const std::string who = std::string(name) + ": ";
    if (!m) {
        if (required) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "pattern is NULL");
        return LDPC_OK;
    }
    if (!required) {   // logical rows: rows = 0 needs no arrays
        if (m->rows < 0 || m->nnz < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "negative dimension of the logical rows (rows, nnz)");
        if (m->rows == 0) {
            if (m->nnz != 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "nnz must be 0 when rows is 0");
            return LDPC_OK;
        }
    }
    ldpc_status st = ldpc_detail::check_csc_args(m->rows, n, m->nnz, m->colptr, m->rowval, 0);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(m->rows, n, m->nnz, m->colptr, m->rowval)) != LDPC_OK)
        return set_error(st, who + ldpc_detail::last_error());
    return LDPC_OK;
}

static bool upload_graph(CssGraph *g, const ldpc_css_pattern *m, int64_t n)
{
    if (!m || m->rows == 0) return true;   // (no row is ever walked)
    g->rows = m->rows;
    const ldpc_detail::TannerGraph tg = ldpc_detail::tanner_graph(m->rows, n, m->nnz, m->colptr, m->rowval);
    return ldpc_detail::upload_ints(&g->row_ptr, tg.row_ptr) && ldpc_detail::upload_ints(&g->csr_col, tg.csr_col);
}

extern "C" {

ldpc_status ldpc_css_trials_create(int64_t n, const ldpc_css_pattern *hx, const ldpc_css_pattern *hz, const ldpc_css_pattern *lx,
                                   const ldpc_css_pattern *lz, const ldpc_css_trials_options *options, ldpc_css_trials **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (n < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative dimension (n)");
    ldpc_status st;
    if ((st = check_pattern("Hx", hx, n, true)) != LDPC_OK || (st = check_pattern("Hz", hz, n, true)) != LDPC_OK ||
        (st = check_pattern("Lx", lx, n, false)) != LDPC_OK || (st = check_pattern("Lz", lz, n, false)) != LDPC_OK)
        return st;
    const int variant = options ? options->kernel_variant : 0;
    int device = options ? options->device : -1;
    if (variant < 0 || variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    const int64_t lim = (int64_t)1 << 28;
    const ldpc_css_pattern *all[] = {hx, hz, lx, lz};
    bool too_large = n >= lim;
    for (const ldpc_css_pattern *m : all) too_large |= m && (m->rows >= lim || m->nnz >= lim);
    if (too_large) return set_error(LDPC_ERR_UNSUPPORTED, "CSS trial kernels: graph too large for 32-bit edge indexing");

    ldpc_css_trials *t = new (std::nothrow) ldpc_css_trials();
    if (!t) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    t->n = n; t->device = device; t->num_cus = prop.multiProcessorCount;
    t->wpc = n <= kCssWaveColumn ? 1 : 4;
    t->image_stride = (image_words(n) + 7) & ~7;   // (16-byte granules)
    t->cplx = hx->rows >= 4 * 64 * (int64_t)t->wpc ? 4 : 1;
    t->cplz = hz->rows >= 4 * 64 * (int64_t)t->wpc ? 4 : 1;
    const bool fits = (size_t)(kThreads / (64 * t->wpc)) * 2 * t->image_stride * sizeof(unsigned short) <= kCssImageLds;
    if (variant == 1 && !fits) {
        delete t;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the two bit images of a column do not fit the LDS");
    }
    t->tier = variant ? variant : fits ? 1 : 2;
    const bool ok = upload_graph(&t->hx, hx, n) && upload_graph(&t->hz, hz, n) && upload_graph(&t->lx, lx, n) && upload_graph(&t->lz, lz, n);
    if (!ok || t->calls.create() != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graphs failed");
    }
    *out = t;
    return LDPC_OK;
}

int32_t ldpc_css_trials_kernel(const ldpc_css_trials *t) { return t ? t->tier : 0; }

ldpc_status ldpc_css_trials_destroy(ldpc_css_trials *t)
{
    if (!t) return LDPC_OK;
    (void)hipSetDevice(t->device);
    const ldpc_status st = ldpc_detail::wait_device(t->device, "ldpc_css_trials_destroy (device synchronise)");
    delete t;
    return st;
}

ldpc_status ldpc_css_trials_sample_device(ldpc_css_trials *t, int64_t batch, int64_t column0, double px, double py, double pz,
                                          uint64_t seed, uint8_t *d_ex, uint8_t *d_ez, uint8_t *d_sx, uint8_t *d_sz, void *stream)
{
    tu64 th[3];
    const ldpc_status st = check_sample_args(batch, column0, px, py, pz, d_ex, d_ez, th);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    if (t->hx.rows > 0 && t->hz.rows > 0 && !d_sx != !d_sz)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "sx and sz syndromes pointers must both be given or both be NULL");
    CssParams p{};
    p.column0 = (tu64)column0; p.seed = seed;
    p.ta = th[0]; p.tb = th[1]; p.tc = th[2];
    p.ex_out = d_ex; p.ez_out = d_ez;
    p.sx = t->hx.rows > 0 ? d_sx : nullptr;
    p.sz = t->hz.rows > 0 ? d_sz : nullptr;
    return css_launch(t, kSample, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_css_trials_syndromes_device(ldpc_css_trials *t, int64_t batch, const uint8_t *d_ex, const uint8_t *d_ez,
                                             uint8_t *d_sx, uint8_t *d_sz, void *stream)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch > 0 && !d_ex) return set_error(LDPC_ERR_INVALID_ARGUMENT, "ex errors pointer is NULL");
    if (batch > 0 && !d_ez) return set_error(LDPC_ERR_INVALID_ARGUMENT, "ez errors pointer is NULL");
    if (batch > 0 && !d_sx) return set_error(LDPC_ERR_INVALID_ARGUMENT, "sx syndromes pointer is NULL");
    if (batch > 0 && !d_sz) return set_error(LDPC_ERR_INVALID_ARGUMENT, "sz syndromes pointer is NULL");
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0 || (t->hx.rows == 0 && t->hz.rows == 0)) return LDPC_OK;
    CssParams p{};
    p.ex = d_ex; p.ez = d_ez;
    p.sx = t->hx.rows > 0 ? d_sx : nullptr;
    p.sz = t->hz.rows > 0 ? d_sz : nullptr;
    return css_launch(t, kSyndromes, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_css_trials_score_device(ldpc_css_trials *t, int64_t batch, const uint8_t *d_gx, const uint8_t *d_gz,
                                         const uint8_t *d_ex, const uint8_t *d_ez, uint8_t *d_flags, int64_t *d_counts, void *stream)
{
    const ldpc_status st = check_score_args(batch, d_gx, d_gz, d_ex, d_ez, d_counts);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    CssParams p{};
    p.gx = d_gx; p.gz = d_gz; p.ex = d_ex; p.ez = d_ez; p.flags = d_flags; p.counts = (tu64 *)d_counts;
    return css_launch(t, kScore, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_css_trials_sample(ldpc_css_trials *t, int64_t batch, int64_t column0, double px, double py, double pz, uint64_t seed,
                                   uint8_t *ex, uint8_t *ez, uint8_t *sx, uint8_t *sz)
{
    tu64 th[3];
    ldpc_status st = check_sample_args(batch, column0, px, py, pz, ex, ez, th);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(t->device));
    const size_t n = (size_t)t->n, rx = (size_t)t->hx.rows, rz = (size_t)t->hz.rows, B = (size_t)batch;
    ldpc_detail::Carve image;   // [ex][ez][sx][sz]
    image.take(B * n);
    const size_t o_ez = image.take(B * n), o_sx = image.take(B * rx), o_sz = image.take(B * rz);
    st = ldpc_detail::grow_device_buffer(&t->stage, &t->stage_cap, std::max<size_t>(image.at, 256), t->device,
                                         "CSS trials staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    uint8_t *dp = (uint8_t *)t->stage;
    if (rx > 0 && rz > 0 && !sx != !sz)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "sx and sz syndromes pointers must both be given or both be NULL");
    const bool want_sx = sx && rx > 0, want_sz = sz && rz > 0;
    st = ldpc_css_trials_sample_device(t, batch, column0, px, py, pz, seed, dp, dp + o_ez, want_sx ? dp + o_sx : nullptr,
                                       want_sz ? dp + o_sz : nullptr, nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) {
        LDPC_HIP_TRY(hipMemcpyAsync(ex, dp, B * n, hipMemcpyDeviceToHost, nullptr));
        LDPC_HIP_TRY(hipMemcpyAsync(ez, dp + o_ez, B * n, hipMemcpyDeviceToHost, nullptr));
    }
    if (want_sx) LDPC_HIP_TRY(hipMemcpyAsync(sx, dp + o_sx, B * rx, hipMemcpyDeviceToHost, nullptr));
    if (want_sz) LDPC_HIP_TRY(hipMemcpyAsync(sz, dp + o_sz, B * rz, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, t->device, "ldpc_css_trials_sample (stream synchronise)");
}

ldpc_status ldpc_css_trials_score(ldpc_css_trials *t, int64_t batch, const uint8_t *gx, const uint8_t *gz, const uint8_t *ex,
                                  const uint8_t *ez, uint8_t *flags, int64_t counts[6])
{
    ldpc_status st = check_score_args(batch, gx, gz, ex, ez, counts);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(t->device));
    const size_t n = (size_t)t->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [gx][gz][ex][ez][flags][counts]
    image.take(B * n);
    const size_t o_gz = image.take(B * n), o_ex = image.take(B * n), o_ez = image.take(B * n), o_flags = image.take(B),
                 o_counts = image.take(6 * sizeof(int64_t));
    st = ldpc_detail::grow_device_buffer(&t->stage, &t->stage_cap, image.at, t->device,
                                         "CSS trials staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    uint8_t *dp = (uint8_t *)t->stage;
    if (n > 0) {
        LDPC_HIP_TRY(hipMemcpyAsync(dp, gx, B * n, hipMemcpyHostToDevice, nullptr));
        LDPC_HIP_TRY(hipMemcpyAsync(dp + o_gz, gz, B * n, hipMemcpyHostToDevice, nullptr));
        LDPC_HIP_TRY(hipMemcpyAsync(dp + o_ex, ex, B * n, hipMemcpyHostToDevice, nullptr));
        LDPC_HIP_TRY(hipMemcpyAsync(dp + o_ez, ez, B * n, hipMemcpyHostToDevice, nullptr));
    }
    LDPC_HIP_TRY(hipMemcpyAsync(dp + o_counts, counts, 6 * sizeof(int64_t), hipMemcpyHostToDevice, nullptr));
    st = ldpc_css_trials_score_device(t, batch, dp, dp + o_gz, dp + o_ex, dp + o_ez, dp + o_flags, (int64_t *)(dp + o_counts), nullptr);
    if (st != LDPC_OK) return st;
    if (flags) LDPC_HIP_TRY(hipMemcpyAsync(flags, dp + o_flags, B, hipMemcpyDeviceToHost, nullptr));
    LDPC_HIP_TRY(hipMemcpyAsync(counts, dp + o_counts, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, t->device, "ldpc_css_trials_score (stream synchronise)");
}

}  // extern "C"
