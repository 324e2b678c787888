// ldpc_trials.hip -- host side of the Monte-Carlo trial steps: the ldpc_trials_* and ldpc_css_trials_* entry points of
// include/ldpc_mi355x.h.  What the reference does around every decode on the host (test/test_bp_decoder.jl:19-30:
// rand(n, B) .< per, H * errors .% 2, guesses[:, i] == errors[:, i]) as device-resident steps, and the same for a CSS
// pair: Pauli errors on n qubits (one draw per qubit gives its X part and its Z part), the two syndromes sz = Hz ex and
// sx = Hx ez, and the joint score with logical X and logical Z failures.  Device code: trial_kernels.hpp, whose sides
// are filled here: one matrix = one side (H, L); CSS = side 0 (ex, gx, sz; Hz, Lz) and side 1 (ez, gz, sx; Hx, Lx).
// Tiers (ldpc_trials_kernel, ldpc_css_trials_kernel): 1 = a column's bit images in LDS while its checks are walked,
// 2 = unlimited.  No CPU path.  A one-matrix handle may hold a table of per-bit thresholds (ldpc_trials_set_rates) for
// the per-bit sample, a fourth step of the same kernel template.
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

// What a handle of either kind holds.
struct TrialsCore {
    struct Side {               // the CSRs on the device (the walks go check by check) of the checks and the logical rows
        int64_t rows = 0, nl = 0;
        int cpl = 1;
        int *row_ptr = nullptr, *csr_col = nullptr, *lrow_ptr = nullptr, *lcsr_col = nullptr;
    } side[2];
    int64_t n = 0;
    int device = 0, num_cus = 0, tier = 0, wpc = 1, image_stride = 0;
    void *stage = nullptr;      // device staging for the host-pointer entries
    size_t stage_cap = 0;
    int per_cu[4] = {0, 0, 0, 0};  // workgroups a CU holds, per step (0 = not asked yet)
    tu64 *rates = nullptr;      // one matrix: the threshold of every bit (trial_kernels.hpp), while a table is set
    ldpc_detail::CallOrder calls;
    ~TrialsCore()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        for (const Side &s : side)
            for (void *q : {(void *)s.row_ptr, (void *)s.csr_col, (void *)s.lrow_ptr, (void *)s.lcsr_col})
                if (q) (void)hipFree(q);
        if (stage) (void)hipFree(stage);
        if (rates) (void)hipFree(rates);
        calls.destroy();
    }
};

struct ldpc_trials : TrialsCore {};
struct ldpc_css_trials : TrialsCore {};

template <int SIDES>
static auto trial_kernel_of(int mode, int wpc, bool image) -> void (*)(TrialParams<SIDES>)
{
#define LDPC_TRIAL_STEP(MODE) {{trial_kernel<SIDES, 1, MODE, false>, trial_kernel<SIDES, 1, MODE, true>}, \
                               {trial_kernel<SIDES, 4, MODE, false>, trial_kernel<SIDES, 4, MODE, true>}}
    static void (*const table[3][2][2])(TrialParams<SIDES>) = {LDPC_TRIAL_STEP(kSample), LDPC_TRIAL_STEP(kSyndromes), LDPC_TRIAL_STEP(kScore)};
    if constexpr (SIDES == 1) {   // the per-bit sample exists for one matrix only
        static void (*const by_rates[2][2])(TrialParams<1>) = LDPC_TRIAL_STEP(kSampleRates);
        if (mode == kSampleRates) return by_rates[wpc == 4][image];
    }
#undef LDPC_TRIAL_STEP
    return table[mode][wpc == 4][image];
}

// One step: the arguments are checked, the handle is not NULL, batch > 0; the caller has filled the arrays of every side
// and what belongs to the step, the handle's part is filled here.
template <int SIDES>
static ldpc_status trials_launch(TrialsCore *t, int mode, TrialParams<SIDES> p, int64_t batch, hipStream_t stream)
{
    // (2^36: with the grid below, no workgroup's 32-bit running counts of the score step can wrap)
    if (batch > ((int64_t)1 << 36)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call (more than 2^36 columns)");
    LDPC_HIP_TRY(hipSetDevice(t->device));
    if (ldpc_detail::device_stalled(t->device)) return ldpc_detail::stalled_error(t->device);
    ldpc_status st = t->calls.enter(stream);
    if (st != LDPC_OK) return st;
    const bool image = t->tier == 1;
    const int cpb = kThreads / (64 * t->wpc);
    const size_t lds = image ? (size_t)cpb * SIDES * t->image_stride * sizeof(unsigned short) : 0;
    const auto k = trial_kernel_of<SIDES>(mode, t->wpc, image);
    if (!t->per_cu[mode]) {
        // always the whole budget, never this handle's own size: the cap belongs to the kernel, not to the handle, and a
        // later handle of a smaller n must not lower it under an earlier, larger one
        if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrialsImageLds));
        t->per_cu[mode] = std::min(8, ldpc_detail::blocks_per_cu((const void *)k, kThreads, lds));
    }
    p.n = (int)t->n; p.image_stride = t->image_stride; p.batch = batch; p.rates = t->rates;
    for (int i = 0; i < SIDES; ++i) {
        const TrialsCore::Side &s = t->side[i];
        TrialSide &d = p.side[i];
        d.rows = (int)s.rows; d.nl = (int)s.nl; d.cpl = s.cpl;
        d.row_ptr = s.row_ptr; d.csr_col = s.csr_col; d.lrow_ptr = s.lrow_ptr; d.lcsr_col = s.lcsr_col;
    }
    const int64_t ngroups = (batch + cpb - 1) / cpb;
    const int64_t grid = std::min<int64_t>(ngroups, (int64_t)t->per_cu[mode] * std::max(t->num_cus, 32));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)kThreads), lds, stream, p);
    LDPC_HIP_TRY(hipGetLastError());
    return t->calls.leave(stream);
}

static bool upload_graph(int64_t *rows, int **row_ptr, int **csr_col, const ldpc_css_pattern *m, int64_t n)
{
    if (!m || m->rows == 0) return true;   // (no row is ever walked: the arrays stay NULL, also those of an H with no checks)
    *rows = m->rows;
    const ldpc_detail::TannerGraph tg = ldpc_detail::tanner_graph(m->rows, n, m->nnz, m->colptr, m->rowval);
    return ldpc_detail::upload(row_ptr, tg.row_ptr) && ldpc_detail::upload(csr_col, tg.csr_col);
}

// What a create of either kind does once its patterns are validated (checks[k], logicals[k]: what sees side k; a
// logicals[k] may be NULL): variant and device, the 32-bit limit, the handle, geometry and tier by n, cpl by each side's
// checks, the graphs on the device.  The three messages are the caller's.
template <class Handle>
static ldpc_status trials_create(Handle **out, int sides, int64_t n, int variant, int device, const ldpc_css_pattern *const checks[],
                                 const ldpc_css_pattern *const logicals[], const char *too_large, const char *does_not_fit,
                                 const char *allocation_failed)
{
    if (variant < 0 || variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    hipDeviceProp_t prop;
    const ldpc_status st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)");
    if (st != LDPC_OK) return st;
    const int64_t lim = (int64_t)1 << 28;
    bool large = n >= lim;
    for (int k = 0; k < sides; ++k)
        for (const ldpc_css_pattern *m : {checks[k], logicals[k]}) large |= m && (m->rows >= lim || m->nnz >= lim);
    if (large) return set_error(LDPC_ERR_UNSUPPORTED, too_large);

    Handle *t = new (std::nothrow) Handle();
    if (!t) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    t->n = n; t->device = device; t->num_cus = prop.multiProcessorCount;
    t->wpc = n <= kTrialsWaveColumn ? 1 : 4;
    t->image_stride = (image_words(n) + 7) & ~7;   // (16-byte granules)
    const bool fits = (size_t)(kThreads / (64 * t->wpc)) * sides * t->image_stride * sizeof(unsigned short) <= kTrialsImageLds;
    if (variant == 1 && !fits) {
        delete t;
        return set_error(LDPC_ERR_UNSUPPORTED, does_not_fit);
    }
    t->tier = variant ? variant : fits ? 1 : 2;
    bool ok = true;
    for (int k = 0; k < sides; ++k) {
        TrialsCore::Side &s = t->side[k];
        s.cpl = checks[k]->rows >= 4 * 64 * (int64_t)t->wpc ? 4 : 1;
        ok = ok && upload_graph(&s.rows, &s.row_ptr, &s.csr_col, checks[k], n) && upload_graph(&s.nl, &s.lrow_ptr, &s.lcsr_col, logicals[k], n);
    }
    if (!ok || t->calls.create() != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, allocation_failed);
    }
    *out = t;
    return LDPC_OK;
}

template <class Handle>
static ldpc_status trials_destroy(Handle *t, const char *what)
{
    if (!t) return LDPC_OK;
    (void)hipSetDevice(t->device);
    const ldpc_status st = ldpc_detail::wait_device(t->device, what);
    delete t;
    return st;
}

// ---- one check matrix ----------------------------------------------------------------------------------------------------

static ldpc_status check_sample_args(int64_t batch, int64_t column0, double per, const void *errors)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (column0 < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative column0");
    if (!(per >= 0.0 && per <= 1.0)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "per must lie in [0, 1] (and not be NaN)");
    if (batch > 0 && !errors) return set_error(LDPC_ERR_INVALID_ARGUMENT, "errors pointer is NULL");
    return LDPC_OK;
}

// the per-bit sample: its rates were checked by ldpc_trials_set_rates, and without a table there is nothing to draw from
static ldpc_status check_sample_rates_args(const ldpc_trials *t, int64_t batch, int64_t column0, const void *errors)
{
    const ldpc_status st = check_sample_args(batch, column0, 0.0, errors);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (!t->rates) return set_error(LDPC_ERR_INVALID_ARGUMENT, "no rates are set (ldpc_trials_set_rates)");
    return LDPC_OK;
}

// The host form of either sample: the device form `sample_device(d_errors, d_syndromes)` into the staging buffer, then
// the copies out.  The arguments are checked, the handle is not NULL, batch > 0.
template <class F>
static ldpc_status sample_to_host(ldpc_trials *t, int64_t batch, uint8_t *errors, uint8_t *syndromes, const char *what, F sample_device)
{
    LDPC_HIP_TRY(hipSetDevice(t->device));
    const size_t s = (size_t)t->side[0].rows, n = (size_t)t->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [errors][syndromes]
    image.take(B * n);
    const size_t o_syn = image.take(B * s);
    ldpc_status st = ldpc_detail::grow_device_buffer(&t->stage, &t->stage_cap, std::max<size_t>(image.at, 256), t->device,
                                                     "trials staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    uint8_t *dp = (uint8_t *)t->stage;
    const bool want_syn = syndromes && s > 0;
    st = sample_device(dp, want_syn ? dp + o_syn : nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) LDPC_HIP_TRY(hipMemcpyAsync(errors, dp, B * n, hipMemcpyDeviceToHost, nullptr));
    if (want_syn) LDPC_HIP_TRY(hipMemcpyAsync(syndromes, dp + o_syn, B * s, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, t->device, what);
}

static ldpc_status check_score_args(int64_t batch, const void *guesses, const void *errors, const void *counts)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch > 0 && !guesses) return set_error(LDPC_ERR_INVALID_ARGUMENT, "guesses pointer is NULL");
    if (batch > 0 && !errors) return set_error(LDPC_ERR_INVALID_ARGUMENT, "errors pointer is NULL");
    if (batch > 0 && !counts) return set_error(LDPC_ERR_INVALID_ARGUMENT, "counts pointer is NULL");
    return LDPC_OK;
}

// ---- a CSS pair ----------------------------------------------------------------------------------------------------------

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

// The sides of a CSS step: the X parts are seen by Hz (-> sz), the Z parts by Hx (-> sx).
static void css_sides(const ldpc_css_trials *t, TrialParams<2> *p, uint8_t *d_sx, uint8_t *d_sz)
{
    p->side[0].syn = t->side[0].rows > 0 ? d_sz : nullptr;
    p->side[1].syn = t->side[1].rows > 0 ? d_sx : nullptr;
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
    const ldpc_css_pattern h = {s, nnz, colptr, rowval}, l = {nl, lnnz, lcolptr, lrowval};
    const ldpc_css_pattern *const checks[] = {&h}, *const logicals[] = {&l};
    return trials_create(out, 1, n, options ? options->kernel_variant : 0, options ? options->device : -1, checks, logicals,
                         "trial kernels: graph too large for 32-bit edge indexing",
                         "kernel_variant 1: the bit image of a column does not fit the LDS", "device allocation of the Tanner graph failed");
}

int32_t ldpc_trials_kernel(const ldpc_trials *t) { return t ? t->tier : 0; }

ldpc_status ldpc_trials_destroy(ldpc_trials *t) { return trials_destroy(t, "ldpc_trials_destroy (device synchronise)"); }

ldpc_status ldpc_trials_sample_device(ldpc_trials *t, int64_t batch, int64_t column0, double per, uint64_t seed,
                                      uint8_t *d_errors, uint8_t *d_syndromes, void *stream)
{
    const ldpc_status st = check_sample_args(batch, column0, per, d_errors);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    TrialParams<1> p{};
    p.column0 = (tu64)column0; p.seed = seed;
    p.all_ones = per >= 1.0;
    p.side[0].hi = per >= 1.0 ? ~0ull : (tu64)(per * 18446744073709551616.0);
    p.side[0].err_out = d_errors; p.side[0].syn = t->side[0].rows > 0 ? d_syndromes : nullptr;
    return trials_launch(t, kSample, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_syndromes_device(ldpc_trials *t, int64_t batch, const uint8_t *d_errors, uint8_t *d_syndromes,
                                         void *stream)
{
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch > 0 && !d_errors) return set_error(LDPC_ERR_INVALID_ARGUMENT, "errors pointer is NULL");
    if (batch > 0 && !d_syndromes) return set_error(LDPC_ERR_INVALID_ARGUMENT, "syndromes pointer is NULL");
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0 || t->side[0].rows == 0) return LDPC_OK;
    TrialParams<1> p{};
    p.side[0].err = d_errors; p.side[0].syn = d_syndromes;
    return trials_launch(t, kSyndromes, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_score_device(ldpc_trials *t, int64_t batch, const uint8_t *d_guesses, const uint8_t *d_errors,
                                     uint8_t *d_flags, int64_t *d_counts, void *stream)
{
    const ldpc_status st = check_score_args(batch, d_guesses, d_errors, d_counts);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    TrialParams<1> p{};
    p.side[0].guess = d_guesses; p.side[0].err = d_errors; p.flags = d_flags; p.counts = (tu64 *)d_counts;
    return trials_launch(t, kScore, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_sample(ldpc_trials *t, int64_t batch, int64_t column0, double per, uint64_t seed, uint8_t *errors,
                               uint8_t *syndromes)
{
    const ldpc_status st = check_sample_args(batch, column0, per, errors);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    return sample_to_host(t, batch, errors, syndromes, "ldpc_trials_sample (stream synchronise)", [&](uint8_t *d_errors, uint8_t *d_syndromes) {
        return ldpc_trials_sample_device(t, batch, column0, per, seed, d_errors, d_syndromes, nullptr);
    });
}

ldpc_status ldpc_trials_set_rates(ldpc_trials *t, int64_t n, const double *rates)
{
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "trials handle is NULL");
    if (n != t->n) return set_error(LDPC_ERR_INVALID_ARGUMENT, "n is not the handle's n (one rate per bit)");
    std::vector<tu64> table;
    if (rates) {
        table.resize((size_t)std::max<int64_t>(n, 1), 0);
        for (int64_t j = 0; j < n; ++j) {
            if (!(rates[j] >= 0.0 && rates[j] <= 1.0))
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "rates[" + std::to_string(j) + "] must lie in [0, 1] (and not be NaN)");
            // below 1 the threshold is at most 2^64 - 2^11, so all ones is free as the mark of "always"
            table[(size_t)j] = rates[j] >= 1.0 ? ~0ull : (tu64)(rates[j] * 18446744073709551616.0);
        }
    }
    LDPC_HIP_TRY(hipSetDevice(t->device));
    if (ldpc_detail::device_stalled(t->device)) return ldpc_detail::stalled_error(t->device);
    // after every earlier call on the handle: a sample still in flight reads the table it was launched with to its end
    if (t->calls.have) {
        const ldpc_status st = ldpc_detail::wait_event(t->calls.done, t->device, "ldpc_trials_set_rates (wait for the earlier calls)");
        if (st != LDPC_OK) return st;
    }
    if (!rates) {
        if (t->rates) LDPC_HIP_TRY(hipFree(t->rates));
        t->rates = nullptr;
        return LDPC_OK;
    }
    tu64 *fresh = t->rates;
    if (!fresh) LDPC_HIP_TRY(hipMalloc((void **)&fresh, table.size() * sizeof(tu64)));
    const hipError_t e = hipMemcpy(fresh, table.data(), table.size() * sizeof(tu64), hipMemcpyHostToDevice);
    if (e != hipSuccess && !t->rates) (void)hipFree(fresh);
    LDPC_HIP_TRY(e);
    t->rates = fresh;
    return LDPC_OK;
}

ldpc_status ldpc_trials_sample_rates_device(ldpc_trials *t, int64_t batch, int64_t column0, uint64_t seed, uint8_t *d_errors,
                                            uint8_t *d_syndromes, void *stream)
{
    const ldpc_status st = check_sample_rates_args(t, batch, column0, d_errors);
    if (st != LDPC_OK) return st;
    if (batch == 0) return LDPC_OK;
    TrialParams<1> p{};
    p.column0 = (tu64)column0; p.seed = seed;
    p.side[0].err_out = d_errors; p.side[0].syn = t->side[0].rows > 0 ? d_syndromes : nullptr;
    return trials_launch(t, kSampleRates, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_trials_sample_rates(ldpc_trials *t, int64_t batch, int64_t column0, uint64_t seed, uint8_t *errors, uint8_t *syndromes)
{
    const ldpc_status st = check_sample_rates_args(t, batch, column0, errors);
    if (st != LDPC_OK) return st;
    if (batch == 0) return LDPC_OK;
    return sample_to_host(t, batch, errors, syndromes, "ldpc_trials_sample_rates (stream synchronise)", [&](uint8_t *d_errors, uint8_t *d_syndromes) {
        return ldpc_trials_sample_rates_device(t, batch, column0, seed, d_errors, d_syndromes, nullptr);
    });
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
    const ldpc_css_pattern *const checks[] = {hz, hx}, *const logicals[] = {lz, lx};   // side 0: the X parts, side 1: the Z parts
    return trials_create(out, 2, n, options ? options->kernel_variant : 0, options ? options->device : -1, checks, logicals,
                         "CSS trial kernels: graph too large for 32-bit edge indexing",
                         "kernel_variant 1: the two bit images of a column do not fit the LDS", "device allocation of the Tanner graphs failed");
}

int32_t ldpc_css_trials_kernel(const ldpc_css_trials *t) { return t ? t->tier : 0; }

ldpc_status ldpc_css_trials_destroy(ldpc_css_trials *t) { return trials_destroy(t, "ldpc_css_trials_destroy (device synchronise)"); }

ldpc_status ldpc_css_trials_sample_device(ldpc_css_trials *t, int64_t batch, int64_t column0, double px, double py, double pz,
                                          uint64_t seed, uint8_t *d_ex, uint8_t *d_ez, uint8_t *d_sx, uint8_t *d_sz, void *stream)
{
    tu64 th[3];
    const ldpc_status st = check_sample_args(batch, column0, px, py, pz, d_ex, d_ez, th);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    if (t->side[1].rows > 0 && t->side[0].rows > 0 && !d_sx != !d_sz)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "sx and sz syndromes pointers must both be given or both be NULL");
    TrialParams<2> p{};
    p.column0 = (tu64)column0; p.seed = seed;
    p.side[0].hi = th[1];                        // X or Y: r < tb
    p.side[1].lo = th[0]; p.side[1].hi = th[2];  // Y or Z: ta <= r < tc
    p.side[0].err_out = d_ex; p.side[1].err_out = d_ez;
    css_sides(t, &p, d_sx, d_sz);
    return trials_launch(t, kSample, p, batch, (hipStream_t)stream);
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
    if (batch == 0 || (t->side[1].rows == 0 && t->side[0].rows == 0)) return LDPC_OK;
    TrialParams<2> p{};
    p.side[0].err = d_ex; p.side[1].err = d_ez;
    css_sides(t, &p, d_sx, d_sz);
    return trials_launch(t, kSyndromes, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_css_trials_score_device(ldpc_css_trials *t, int64_t batch, const uint8_t *d_gx, const uint8_t *d_gz,
                                         const uint8_t *d_ex, const uint8_t *d_ez, uint8_t *d_flags, int64_t *d_counts, void *stream)
{
    const ldpc_status st = check_score_args(batch, d_gx, d_gz, d_ex, d_ez, d_counts);
    if (st != LDPC_OK) return st;
    if (!t) return set_error(LDPC_ERR_INVALID_ARGUMENT, "CSS trials handle is NULL");
    if (batch == 0) return LDPC_OK;
    TrialParams<2> p{};
    p.side[0].guess = d_gx; p.side[0].err = d_ex; p.side[1].guess = d_gz; p.side[1].err = d_ez;
    p.flags = d_flags; p.counts = (tu64 *)d_counts;
    return trials_launch(t, kScore, p, batch, (hipStream_t)stream);
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
    const size_t n = (size_t)t->n, rx = (size_t)t->side[1].rows, rz = (size_t)t->side[0].rows, B = (size_t)batch;
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
