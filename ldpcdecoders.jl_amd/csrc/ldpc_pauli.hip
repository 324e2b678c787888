// ldpc_pauli.hip -- host side of the joint X/Z (Pauli) min-sum decoder of CSS codes: the ldpc_pauli_minsum_* entry points
// of include/ldpc_mi355x.h (the rule is stated there).  Device code: pauli_kernels.hpp.  The checks of both sides are one
// Tanner graph here -- Hx rows first, then Hz rows -- so the create-time scaffolding of the binary decoders serves as it
// is.  Tiers (ldpc_pauli_minsum_kernel), chosen by pauli_tile_plan() of tile_plan.hpp:
//   1  on-chip: the state of the S syndromes a workgroup holds lives in LDS for the whole decode
//   2  unlimited: tiles of 64 syndromes, the state in a global workspace, one slot per workgroup of a persistent grid
// No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "../../include/ldpc_mi355x_debug.h"
#include "pauli_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr int kPauliLdsWaves = 8, kPauliGlobalWaves = 16;   // as the min-sum kernels
static constexpr size_t kPauliWorkspaceCap = (size_t)6 << 30;      // the unlimited tier's grid shrinks to keep its slots below this
static constexpr float kPauliAlphaDefault = 0.75f, kPauliClipDefault = 1.0e6f;

struct ldpc_pauli_minsum_decoder {
    int64_t rx = 0, rz = 0, n = 0, max_iters = 0;
    float alpha = kPauliAlphaDefault, clip = kPauliClipDefault;
    int device = 0, num_cus = 0, rec_words = 0;
    TilePlan plan;
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *col_mid = nullptr, *edge_rec = nullptr,
        *edge_pos = nullptr;
    float *priors = nullptr;       // [3][n]: prior_x, prior_y, prior_z
    void *stage = nullptr;         // device staging for the host-pointer entry
    size_t stage_cap = 0;
    unsigned char *ws = nullptr;   // tier 2: [grid][slot]
    size_t ws_cap = 0;
    bool kernel_ready = false;
    int per_cu = 1;
    int last_grid = 0;             // workgroups of the most recent launch
    ldpc_detail::CallOrder calls;  // calls on a handle run in call order whatever streams they are given (they share the workspace)
    ~ldpc_pauli_minsum_decoder()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {row_ptr, csr_col, rec_off, col_ptr, col_mid, edge_rec, edge_pos, priors, stage, ws};
        for (void *q : all)
            if (q) (void)hipFree(q);
        calls.destroy();
    }
};

typedef void (*pauli_kernel_t)(PauliParams);
static pauli_kernel_t pauli_kernel_of(int tier)
{
    return tier == 1 ? pauli_minsum_kernel<kPauliLdsWaves, false> : pauli_minsum_kernel<kPauliGlobalWaves, true>;
}

// One side of a create: the checks ldpc_bp_create makes on a pattern, and at least one row; the message names the side.
static ldpc_status pauli_check_side(const char *name, const ldpc_css_pattern *m, int64_t n)
{
    const std::string who = std::string(name) + ": ";
    if (!m) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "pattern is NULL");
    ldpc_status st = ldpc_detail::check_csc_args(m->rows, n, m->nnz, m->colptr, m->rowval, 0);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(m->rows, n, m->nnz, m->colptr, m->rowval)) != LDPC_OK)
        return set_error(st, who + ldpc_detail::last_error());
    if (m->rows < 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "a side needs at least one row");
    return LDPC_OK;
}

// what every entry checks before any device work; batch == 0 is the caller's to answer
static ldpc_status pauli_check_batch(const ldpc_pauli_minsum_decoder *d, int64_t batch, const void *sx, const void *sz, const void *gx,
                                     const void *gz, const void *conv)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if (!sx || !sz || (d->n > 0 && (!gx || !gz)) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    return LDPC_OK;
}

extern "C" {

ldpc_status ldpc_pauli_minsum_create(int64_t n, const ldpc_css_pattern *hx, const ldpc_css_pattern *hz, const float *prior_x,
                                     const float *prior_y, const float *prior_z, int64_t max_iters,
                                     const ldpc_pauli_minsum_options *options, ldpc_pauli_minsum_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (n < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative dimension (n)");
    if (max_iters < 0 || max_iters > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "max_iters must lie in 0 .. 2^31 - 1");
    ldpc_status st;
    if ((st = pauli_check_side("hx", hx, n)) != LDPC_OK || (st = pauli_check_side("hz", hz, n)) != LDPC_OK) return st;
    const float alpha = options && options->alpha != 0.0f ? options->alpha : kPauliAlphaDefault;   // a zeroed struct: defaults
    const float clip = options && options->clip != 0.0f ? options->clip : kPauliClipDefault;
    const int variant = options ? options->kernel_variant : 0;
    int device = options ? options->device : -1;
    if (!(alpha > 0.0f && alpha <= 1.0f)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "alpha must lie in (0, 1]");
    if (!(clip > 0.0f) || std::isinf(clip)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "clip must be finite and > 0");
    if (variant < 0 || variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    const float *const tables[3] = {prior_x, prior_y, prior_z};
    const char *const names[3] = {"prior_x", "prior_y", "prior_z"};
    for (int k = 0; k < 3; ++k) {
        if (n > 0 && !tables[k]) return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + " is NULL");
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(tables[k][j]))
                return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + "[" + std::to_string(j) + "] is not finite");
    }
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    const int64_t rx = hx->rows, rz = hz->rows, s = rx + rz, nnz = hx->nnz + hz->nnz;
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "Pauli min-sum kernels: graph too large for 32-bit edge indexing");

    // one graph: the Hx rows, then the Hz rows; a qubit's edges are its Hx checks, then its Hz checks, each ascending
    std::vector<int64_t> colptr((size_t)n + 1, 0), rowval((size_t)std::max<int64_t>(nnz, 1), 0);
    std::vector<int> col_mid((size_t)std::max<int64_t>(n, 1), 0);
    int64_t at = 0;
    for (int64_t j = 0; j < n; ++j) {
        colptr[(size_t)j] = at;
        for (int64_t e = hx->colptr[j]; e < hx->colptr[j + 1]; ++e) rowval[(size_t)at++] = hx->rowval[e];
        col_mid[(size_t)j] = (int)at;
        for (int64_t e = hz->colptr[j]; e < hz->colptr[j + 1]; ++e) rowval[(size_t)at++] = rx + hz->rowval[e];
    }
    colptr[(size_t)n] = at;

    ldpc_pauli_minsum_decoder *d = new (std::nothrow) ldpc_pauli_minsum_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->rx = rx; d->rz = rz; d->n = n; d->max_iters = max_iters; d->alpha = alpha; d->clip = clip;
    d->device = device; d->num_cus = prop.multiProcessorCount;
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr.data(), rowval.data());
    std::vector<int> rec_off((size_t)s, 0), edge_rec(g.csc_row.size(), 0), edge_pos(g.csc_row.size(), 0);
    int64_t words = 0;
    for (int64_t i = 0; i < s; ++i) {
        rec_off[(size_t)i] = (int)words;
        words += ms_record_words(g.row_ptr[(size_t)i + 1] - g.row_ptr[(size_t)i]);   // <= 4 nnz + ... < 2^31
    }
    for (int64_t e = 0; e < nnz; ++e) {
        const int i = g.csc_row[(size_t)e], k = g.csc2csr[(size_t)e] - g.row_ptr[(size_t)i];
        edge_rec[(size_t)e] = rec_off[(size_t)i];
        edge_pos[(size_t)e] = g.row_ptr[(size_t)i + 1] - g.row_ptr[(size_t)i] > 64 ? (k | kMsPosEdge) : k;
    }
    if (2 * n + words >= ((int64_t)1 << 31)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "Pauli min-sum kernels: the state of one syndrome is too large for 32-bit word indexing");
    }
    d->rec_words = (int)words;
    if (!pauli_tile_plan(s, n, words, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    std::vector<float> priors((size_t)std::max<int64_t>(3 * n, 1), 0.0f);
    for (int k = 0; k < 3; ++k)
        for (int64_t j = 0; j < n; ++j) priors[(size_t)(k * n + j)] = tables[k][j];
    using ldpc_detail::upload_ints;
    bool ok = upload_ints(&d->row_ptr, g.row_ptr) && upload_ints(&d->csr_col, g.csr_col) && upload_ints(&d->rec_off, rec_off) &&
              upload_ints(&d->col_ptr, g.col_ptr) && upload_ints(&d->col_mid, col_mid) && upload_ints(&d->edge_rec, edge_rec) &&
              upload_ints(&d->edge_pos, edge_pos) && hipMalloc((void **)&d->priors, priors.size() * sizeof(float)) == hipSuccess &&
              hipMemcpy(d->priors, priors.data(), priors.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
              d->calls.create() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

// (include/ldpc_mi355x_debug.h) the choice create makes, without a device
ldpc_status ldpc_debug_pauli_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t kernel_variant, int32_t *tier,
                                       int32_t *tile_syndromes, int64_t *state_bytes)
{
    if (s < 0 || n < 0 || rec_words < 0 || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28) || 2 * n + rec_words >= ((int64_t)1 << 31))
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "s, n and rec_words must be >= 0 and within what create accepts");
    if (kernel_variant < 0 || kernel_variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    TilePlan plan;
    if (!pauli_tile_plan(s, n, rec_words, kernel_variant, &plan))
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    if (tier) *tier = plan.tier;
    if (tile_syndromes) *tile_syndromes = plan.S;
    if (state_bytes) *state_bytes = (int64_t)plan.state_bytes;
    return LDPC_OK;
}

int32_t ldpc_pauli_minsum_kernel(const ldpc_pauli_minsum_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_pauli_minsum_tile_syndromes(const ldpc_pauli_minsum_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_pauli_minsum_last_grid(const ldpc_pauli_minsum_decoder *d) { return d ? d->last_grid : 0; }

ldpc_status ldpc_pauli_minsum_destroy(ldpc_pauli_minsum_decoder *d)
{
    if (!d) return LDPC_OK;
    (void)hipSetDevice(d->device);
    const ldpc_status st = ldpc_detail::wait_device(d->device, "ldpc_pauli_minsum_destroy (device synchronise)");
    delete d;
    return st;
}

ldpc_status ldpc_pauli_minsum_decode_batch_device(ldpc_pauli_minsum_decoder *d, int64_t batch, const uint8_t *d_sx, const uint8_t *d_sz,
                                                  uint8_t *d_gx, uint8_t *d_gz, uint8_t *d_conv, double *d_llr, int32_t *d_iters,
                                                  void *stream_v)
{
    ldpc_status st = pauli_check_batch(d, batch, d_sx, d_sz, d_gx, d_gz, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(d->device));
    if (ldpc_detail::device_stalled(d->device)) return ldpc_detail::stalled_error(d->device);
    if ((st = d->calls.enter(stream)) != LDPC_OK) return st;
    if (d->max_iters == 0) {   // no iteration runs: zeros, converged = 0, llr = 0
        if (d->n > 0) {
            LDPC_HIP_TRY(hipMemsetAsync(d_gx, 0, (size_t)batch * d->n, stream));
            LDPC_HIP_TRY(hipMemsetAsync(d_gz, 0, (size_t)batch * d->n, stream));
            if (d_llr) LDPC_HIP_TRY(hipMemsetAsync(d_llr, 0, (size_t)batch * 3 * d->n * sizeof(double), stream));
        }
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
    } else {
        const int tier = d->plan.tier, S = d->plan.S, shift = d->plan.shift;
        const bool global = tier == 2;
        const int threads = (global ? kPauliGlobalWaves : kPauliLdsWaves) * 64;
        const size_t state = d->plan.state_bytes, lds = global ? 0 : state;
        const pauli_kernel_t k = pauli_kernel_of(tier);
        if (!d->kernel_ready) {
            // (the limit belongs to the kernel, not to the handle: every handle asks for the tier's maximum, so none lowers another's)
            if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTileLdsOne));
            d->per_cu = ldpc_detail::blocks_per_cu((const void *)k, threads, lds);
            d->kernel_ready = true;
        }
        const int64_t tiles = (batch + S - 1) >> shift;
        int64_t grid = std::min<int64_t>(tiles, (int64_t)d->per_cu * d->num_cus);
        if (global) {
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(kPauliWorkspaceCap / state)));
            st = ldpc_detail::grow_device_buffer((void **)&d->ws, &d->ws_cap, (size_t)grid * state, d->device,
                                                 "Pauli min-sum workspace regrow (device synchronise before the free)");
            if (st != LDPC_OK) return st;
        }
        PauliParams p{};
        p.rx = (int)d->rx; p.s = (int)(d->rx + d->rz); p.n = (int)d->n; p.max_iters = (int)d->max_iters; p.S = S; p.shift = shift;
        p.batch = batch; p.alpha = d->alpha; p.clip = d->clip;
        p.sx = d_sx; p.sz = d_sz; p.gx = d_gx; p.gz = d_gz; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters;
        p.prior_x = d->priors; p.prior_y = d->priors + d->n; p.prior_z = d->priors + 2 * d->n;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.rec_off = d->rec_off; p.col_ptr = d->col_ptr; p.col_mid = d->col_mid;
        p.edge_rec = d->edge_rec; p.edge_pos = d->edge_pos; p.rec_words = d->rec_words;
        p.ws = d->ws; p.slot_bytes = (long long)state;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
        d->last_grid = (int)grid;
    }
    return d->calls.leave(stream);
}

ldpc_status ldpc_pauli_minsum_decode_batch(ldpc_pauli_minsum_decoder *d, int64_t batch, const uint8_t *sx, const uint8_t *sz, uint8_t *gx,
                                           uint8_t *gz, uint8_t *conv, double *llr, int32_t *iters)
{
    ldpc_status st = pauli_check_batch(d, batch, sx, sz, gx, gz, conv);
    if (st != LDPC_OK || batch == 0) return st;
    LDPC_HIP_TRY(hipSetDevice(d->device));
    const size_t rx = (size_t)d->rx, rz = (size_t)d->rz, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [sx][sz][gx][gz][converged][iterations][LLRs]
    image.take(B * rx);
    const size_t o_sz = image.take(B * rz), o_gx = image.take(B * n), o_gz = image.take(B * n), o_conv = image.take(B), o_it = image.take(B * 4);
    const size_t o_llr = image.take(llr ? B * 3 * n * sizeof(double) : 0), total = image.at;
    st = ldpc_detail::grow_device_buffer(&d->stage, &d->stage_cap, total, d->device, "Pauli min-sum staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    char *dp = (char *)d->stage;
    LDPC_HIP_TRY(hipMemcpyAsync(dp, sx, B * rx, hipMemcpyHostToDevice, nullptr));
    LDPC_HIP_TRY(hipMemcpyAsync(dp + o_sz, sz, B * rz, hipMemcpyHostToDevice, nullptr));
    st = ldpc_pauli_minsum_decode_batch_device(d, batch, (const uint8_t *)dp, (const uint8_t *)(dp + o_sz), (uint8_t *)(dp + o_gx),
                                               (uint8_t *)(dp + o_gz), (uint8_t *)(dp + o_conv), llr ? (double *)(dp + o_llr) : nullptr,
                                               (int32_t *)(dp + o_it), nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) {
        LDPC_HIP_TRY(hipMemcpyAsync(gx, dp + o_gx, B * n, hipMemcpyDeviceToHost, nullptr));
        LDPC_HIP_TRY(hipMemcpyAsync(gz, dp + o_gz, B * n, hipMemcpyDeviceToHost, nullptr));
        if (llr) LDPC_HIP_TRY(hipMemcpyAsync(llr, dp + o_llr, B * 3 * n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    }
    LDPC_HIP_TRY(hipMemcpyAsync(conv, dp + o_conv, B, hipMemcpyDeviceToHost, nullptr));
    if (iters) LDPC_HIP_TRY(hipMemcpyAsync(iters, dp + o_it, B * 4, hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, d->device, "ldpc_pauli_minsum_decode_batch (stream synchronise)");
}

}  // extern "C"
