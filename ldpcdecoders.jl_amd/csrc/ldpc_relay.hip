// ldpc_relay.hip -- host side of the relay min-sum decoder (min-sum with a per-bit memory, run as a chain of legs, the
// lightest of the first solutions returned): the ldpc_relay_* entry points of include/ldpc_mi355x.h (the rule is stated
// there).  Device code: relay_kernels.hpp.  Tiers (ldpc_relay_kernel), by the rule of ldpc_minsum.hip with the larger state:
//   1  on-chip: the state of the S syndromes a workgroup holds lives in LDS for the whole decode
//   2  unlimited: tiles of 64 syndromes, the state in a global workspace, one slot per workgroup of a persistent grid
// Legs of 0 iterations are dropped here, so the kernel sees only legs that run.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "relay_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_env.hpp"      // exp_env: LDPC_MS_GRID_MAX, experiments build only
#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr int kRlLdsWaves = 8, kRlGlobalWaves = 16;   // as min-sum
static constexpr size_t kRlWorkspaceCap = (size_t)6 << 30;   // the unlimited tier's grid shrinks to keep its slots below this
static constexpr float kRlAlphaDefault = 0.75f, kRlClipDefault = 1.0e6f;
static constexpr int64_t kRlMaxBits = (int64_t)1 << 22;      // a weight is a sum of at most 2^22 terms below 2^41

struct ldpc_relay_decoder {
    int64_t s = 0, n = 0, nnz = 0;
    int legs = 0, stop_after = 1;   // legs: those that run
    float alpha = kRlAlphaDefault, clip = kRlClipDefault;
    int device = 0, num_cus = 0, tier = 0, S = 64, shift = 6, rec_words = 0;
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *edge_rec = nullptr, *edge_pos = nullptr;
    int *leg_iters = nullptr;
    float *prior = nullptr, *gammas = nullptr, *g0 = nullptr;
    long long *weight = nullptr;
    void *stage = nullptr;      // device staging for the host-pointer entry
    size_t stage_cap = 0;
    unsigned char *ws = nullptr;   // tier 2: [grid][slot]
    size_t ws_cap = 0;
    bool kernel_ready = false;
    int per_cu = 1;
    int grid_max = 0;    // LDPC_MS_GRID_MAX (experiments build): workgroups a launch takes at most; 0 = no cap
    int last_grid = 0;   // workgroups of the most recent launch
    ldpc_detail::CallOrder calls;   // calls on a handle run in call order whatever streams they are given (they share the workspace)
    ~ldpc_relay_decoder()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        void *all[] = {row_ptr, csr_col, rec_off, col_ptr, edge_rec, edge_pos, leg_iters, prior, gammas, g0, weight, stage, ws};
        for (void *q : all)
            if (q) (void)hipFree(q);
        calls.destroy();
    }
};

typedef void (*relay_kernel_t)(RelayParams);
static relay_kernel_t relay_kernel_of(int tier) { return tier == 1 ? relay_kernel<kRlLdsWaves, false> : relay_kernel<kRlGlobalWaves, true>; }

template <class V>
static bool upload(V **dst, const std::vector<V> &v)   // hipMalloc (at least one element) + hipMemcpy
{
    if (hipMalloc((void **)dst, std::max<size_t>(v.size(), 1) * sizeof(V)) != hipSuccess) return false;
    return v.empty() || hipMemcpy(*dst, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice) == hipSuccess;
}

extern "C" {

ldpc_status ldpc_relay_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                              const float *channel_llr, int64_t legs, const float *gammas, const int32_t *leg_iters,
                              const ldpc_relay_options *options, ldpc_relay_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, 0);
    if (st != LDPC_OK) return st;
    if (n > 0 && !channel_llr) return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr is NULL");
    if (legs < 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, "legs must be >= 1");
    if (legs > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "legs must fit int32");
    if (n > 0 && !gammas) return set_error(LDPC_ERR_INVALID_ARGUMENT, "gammas is NULL");
    if (!leg_iters) return set_error(LDPC_ERR_INVALID_ARGUMENT, "leg_iters is NULL");
    const float alpha = options && options->alpha != 0.0f ? options->alpha : kRlAlphaDefault;   // a zeroed struct: defaults
    const float clip = options && options->clip != 0.0f ? options->clip : kRlClipDefault;
    const int variant = options ? options->kernel_variant : 0;
    const int stop_after = options && options->stop_after != 0 ? options->stop_after : 1;
    int device = options ? options->device : -1;
    if (!(alpha > 0.0f && alpha <= 1.0f)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "alpha must lie in (0, 1]");
    if (!(clip > 0.0f) || std::isinf(clip)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "clip must be finite and > 0");
    if (variant < 0 || variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    if (stop_after < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "stop_after must be >= 1 (0 = default 1)");
    int64_t total_iters = 0;
    for (int64_t r = 0; r < legs; ++r) {
        if (leg_iters[r] < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "leg_iters[" + std::to_string(r) + "] is negative");
        if ((total_iters += leg_iters[r]) > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "the sum of leg_iters exceeds INT32_MAX");
    }
    for (int64_t j = 0; j < n; ++j)
        if (!std::isfinite(channel_llr[j]))
            return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr[" + std::to_string(j) + "] is not finite");
    for (int64_t r = 0; r < legs; ++r)
        for (int64_t j = 0; j < n; ++j) {
            const float g = gammas[r * n + j];
            if (!(g > -1.0f && g < 1.0f))   // (false for NaN as well)
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "gammas[" + std::to_string(r) + "][" + std::to_string(j) + "] must be finite and lie in (-1, 1)");
        }
    if ((st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "relay kernels: graph too large for 32-bit edge indexing");
    if (n > kRlMaxBits) return set_error(LDPC_ERR_UNSUPPORTED, "relay kernels: n > 2^22 (a solution's weight must fit int64)");

    ldpc_relay_decoder *d = new (std::nothrow) ldpc_relay_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->alpha = alpha; d->clip = clip; d->stop_after = stop_after;
    d->device = device; d->num_cus = prop.multiProcessorCount;
    // what the rule derives once per handle, for the legs that run: g0 = (1 - gamma) * channel_llr; q = rint(clamp(llr) * 2^16)
    std::vector<float> h_gam, h_g0;
    std::vector<int> h_iters;
    for (int64_t r = 0; r < legs; ++r) {
        if (leg_iters[r] == 0) continue;
        h_iters.push_back(leg_iters[r]);
        for (int64_t j = 0; j < n; ++j) {
            const float g = gammas[r * n + j];
            const float one_minus = 1.0f - g;
            h_gam.push_back(g);
            h_g0.push_back(one_minus * channel_llr[j]);
        }
    }
    d->legs = (int)h_iters.size();
    std::vector<long long> h_weight((size_t)n);
    for (int64_t j = 0; j < n; ++j)
        h_weight[(size_t)j] = (long long)std::rint(std::min(std::max((double)channel_llr[j], -16777216.0), 16777216.0) * 65536.0);
    // CSR (checks -> bits, ascending) next to the caller's CSC; a record per check; per CSC edge its record and position
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    std::vector<int> rec_off((size_t)std::max<int64_t>(s, 1), 0), edge_rec(g.csc_row.size(), 0), edge_pos(g.csc_row.size(), 0);
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
    d->rec_words = (int)words;
    TilePlan plan;   // the tier and the tile width (tile_plan.hpp)
    if (!tile_plan(s, n, words, true, variant, &plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    d->tier = plan.tier; d->S = plan.S; d->shift = plan.shift;
    if (const char *e = exp_env("LDPC_MS_GRID_MAX")) d->grid_max = std::max(1, std::atoi(e));   // (experiments build: tests cap the grid)
    using ldpc_detail::upload_ints;
    const std::vector<float> h_prior(channel_llr, channel_llr + n);
    bool ok = upload_ints(&d->row_ptr, g.row_ptr) && upload_ints(&d->csr_col, g.csr_col) && upload_ints(&d->rec_off, rec_off) &&
              upload_ints(&d->col_ptr, g.col_ptr) && upload_ints(&d->edge_rec, edge_rec) && upload_ints(&d->edge_pos, edge_pos) &&
              upload_ints(&d->leg_iters, h_iters) && upload(&d->prior, h_prior) && upload(&d->gammas, h_gam) && upload(&d->g0, h_g0) &&
              upload(&d->weight, h_weight) && d->calls.create() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

int32_t ldpc_relay_kernel(const ldpc_relay_decoder *d) { return d ? d->tier : 0; }
int32_t ldpc_relay_tile_syndromes(const ldpc_relay_decoder *d) { return d ? d->S : 0; }
int32_t ldpc_relay_last_grid(const ldpc_relay_decoder *d) { return d ? d->last_grid : 0; }

ldpc_status ldpc_relay_destroy(ldpc_relay_decoder *d)
{
    if (!d) return LDPC_OK;
    (void)hipSetDevice(d->device);
    const ldpc_status st = ldpc_detail::wait_device(d->device, "ldpc_relay_destroy (device synchronise)");
    delete d;
    return st;
}

ldpc_status ldpc_relay_decode_batch_device(ldpc_relay_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                           uint8_t *d_conv, double *d_llr, int32_t *d_iters, int32_t *d_solutions, void *stream_v)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !d_syn) || (d->n > 0 && !d_err) || !d_conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(d->device));
    if (ldpc_detail::device_stalled(d->device)) return ldpc_detail::stalled_error(d->device);
    ldpc_status st = d->calls.enter(stream);
    if (st != LDPC_OK) return st;
    if (d->legs == 0) {   // no iteration runs: zeros, converged = 0, llr = 0
        if (d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_llr && d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_llr, 0, (size_t)batch * d->n * sizeof(double), stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        if (d_solutions) LDPC_HIP_TRY(hipMemsetAsync(d_solutions, 0, (size_t)batch * sizeof(int32_t), stream));
    } else {
        const bool global = d->tier == 2;
        const int threads = (global ? kRlGlobalWaves : kRlLdsWaves) * 64;
        const size_t state = relay_state_bytes(d->s, d->n, d->rec_words, d->S);
        const size_t lds = global ? 0 : state;
        relay_kernel_t k = relay_kernel_of(d->tier);
        if (!d->kernel_ready) {
            // (the limit belongs to the kernel, not to the handle: every handle asks for the tier's maximum, so none lowers another's)
            if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTileLdsOne));
            d->per_cu = ldpc_detail::blocks_per_cu((const void *)k, threads, lds);
            d->kernel_ready = true;
        }
        const int64_t tiles = (batch + d->S - 1) >> d->shift;
        int64_t grid = std::min<int64_t>(tiles, (int64_t)d->per_cu * d->num_cus);
        if (d->grid_max > 0) grid = std::min<int64_t>(grid, d->grid_max);
        if (global) {
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(kRlWorkspaceCap / state)));
            st = ldpc_detail::grow_device_buffer((void **)&d->ws, &d->ws_cap, (size_t)grid * state, d->device,
                                                 "relay workspace regrow (device synchronise before the free)");
            if (st != LDPC_OK) return st;
        }
        RelayParams p{};
        p.s = (int)d->s; p.n = (int)d->n; p.legs = d->legs; p.stop_after = d->stop_after; p.S = d->S; p.shift = d->shift;
        p.batch = batch; p.alpha = d->alpha; p.clip = d->clip;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.solutions = d_solutions;
        p.prior = d->prior; p.gammas = d->gammas; p.g0 = d->g0; p.leg_iters = d->leg_iters; p.weight = d->weight;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.rec_off = d->rec_off;
        p.col_ptr = d->col_ptr; p.edge_rec = d->edge_rec; p.edge_pos = d->edge_pos; p.rec_words = d->rec_words;
        p.ws = d->ws; p.slot_bytes = (long long)state;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
        d->last_grid = (int)grid;
    }
    return d->calls.leave(stream);
}

ldpc_status ldpc_relay_decode_batch(ldpc_relay_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err, uint8_t *conv,
                                    double *llr, int32_t *iters, int32_t *solutions)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    LDPC_HIP_TRY(hipSetDevice(d->device));
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::Carve image;   // [syndromes][errors][converged][iterations][solutions][LLRs]
    image.take(B * s);
    const size_t o_err = image.take(B * n), o_conv = image.take(B), o_it = image.take(B * 4), o_sol = image.take(B * 4);
    const size_t o_llr = image.take(llr ? B * n * sizeof(double) : 0), total = image.at;
    ldpc_status st = ldpc_detail::grow_device_buffer(&d->stage, &d->stage_cap, total, d->device, "relay staging regrow (device synchronise before the free)");
    if (st != LDPC_OK) return st;
    char *dp = (char *)d->stage;
    if (s > 0) LDPC_HIP_TRY(hipMemcpyAsync(dp, syn, B * s, hipMemcpyHostToDevice, nullptr));
    st = ldpc_relay_decode_batch_device(d, batch, (const uint8_t *)dp, (uint8_t *)(dp + o_err), (uint8_t *)(dp + o_conv),
                                        llr ? (double *)(dp + o_llr) : nullptr, (int32_t *)(dp + o_it), (int32_t *)(dp + o_sol), nullptr);
    if (st != LDPC_OK) return st;
    if (n > 0) LDPC_HIP_TRY(hipMemcpyAsync(err, dp + o_err, B * n, hipMemcpyDeviceToHost, nullptr));
    LDPC_HIP_TRY(hipMemcpyAsync(conv, dp + o_conv, B, hipMemcpyDeviceToHost, nullptr));
    if (iters) LDPC_HIP_TRY(hipMemcpyAsync(iters, dp + o_it, B * 4, hipMemcpyDeviceToHost, nullptr));
    if (solutions) LDPC_HIP_TRY(hipMemcpyAsync(solutions, dp + o_sol, B * 4, hipMemcpyDeviceToHost, nullptr));
    if (llr && n > 0) LDPC_HIP_TRY(hipMemcpyAsync(llr, dp + o_llr, B * n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    return ldpc_detail::wait_stream(nullptr, d->device, "ldpc_relay_decode_batch (stream synchronise)");
}

}  // extern "C"
