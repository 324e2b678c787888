// ldpc_relay.hip -- host side of the relay min-sum decoder (min-sum with a per-bit memory, run as a chain of legs, the
// lightest of the first solutions returned): the ldpc_relay_* entry points of include/ldpc_mi355x.h (the rule is stated
// there).  Device code: relay_kernels.hpp.  The tiers (ldpc_relay_kernel) and the tile width: tile_plan.hpp, over the relay
// state; the launch geometry and the rest of what the min-sum family shares on the host: tile_host.hpp.  Legs of 0
// iterations are dropped here, so the kernel sees only legs that run.  No CPU path.
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
#include "tile_host.hpp"
using ldpc_detail::set_error;

static constexpr int64_t kRlMaxBits = (int64_t)1 << 22;      // a weight is a sum of at most 2^22 terms below 2^41

struct ldpc_relay_decoder {
    int64_t s = 0, n = 0, nnz = 0;
    int legs = 0, stop_after = 1;   // legs: those that run
    float alpha = 0.0f, clip = 0.0f;
    int rec_words = 0;
    TilePlan plan;
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *edge_rec = nullptr, *edge_pos = nullptr;
    int *leg_iters = nullptr;
    float *prior = nullptr, *gammas = nullptr, *g0 = nullptr;
    long long *weight = nullptr;
    ldpc_detail::TileHost tile;   // (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernel;
    ~ldpc_relay_decoder() { tile.release({row_ptr, csr_col, rec_off, col_ptr, edge_rec, edge_pos, leg_iters, prior, gammas, g0, weight}); }
};

typedef void (*relay_kernel_t)(RelayParams);
static relay_kernel_t relay_kernel_of(int tier) { return tier == 1 ? relay_kernel<ldpc_detail::kTileLdsWaves, false> : relay_kernel<ldpc_detail::kTileGlobalWaves, true>; }

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
    float alpha, clip;
    int variant, device;
    if ((st = ldpc_detail::tile_options(options, &alpha, &clip, &variant, &device)) != LDPC_OK) return st;
    const int stop_after = options && options->stop_after != 0 ? options->stop_after : 1;
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
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount;
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
    const MsRecords rec = ms_records(s, nnz, g.row_ptr.data(), g.csc_row.data(), g.csc2csr.data());   // words <= 4 s + nnz < 2^31
    d->rec_words = (int)rec.words;
    if (!tile_plan(s, n, rec.words, true, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    if (const char *e = exp_env("LDPC_MS_GRID_MAX")) d->tile.grid_max = std::max(1, std::atoi(e));   // (experiments build: tests cap the grid)
    using ldpc_detail::upload;
    const std::vector<float> h_prior(channel_llr, channel_llr + n);
    bool ok = upload(&d->row_ptr, g.row_ptr) && upload(&d->csr_col, g.csr_col) && upload(&d->rec_off, rec.rec_off) &&
              upload(&d->col_ptr, g.col_ptr) && upload(&d->edge_rec, rec.edge_rec) && upload(&d->edge_pos, rec.edge_pos) &&
              upload(&d->leg_iters, h_iters) && upload(&d->prior, h_prior) && upload(&d->gammas, h_gam) && upload(&d->g0, h_g0) &&
              upload(&d->weight, h_weight) && d->tile.calls.create() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

int32_t ldpc_relay_kernel(const ldpc_relay_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_relay_tile_syndromes(const ldpc_relay_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_relay_last_grid(const ldpc_relay_decoder *d) { return d ? d->tile.last_grid : 0; }

ldpc_status ldpc_relay_destroy(ldpc_relay_decoder *d) { return ldpc_detail::tile_destroy(d, "ldpc_relay_destroy (device synchronise)"); }

ldpc_status ldpc_relay_decode_batch_device(ldpc_relay_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                           uint8_t *d_conv, double *d_llr, int32_t *d_iters, int32_t *d_solutions, void *stream_v)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !d_syn) || (d->n > 0 && !d_err) || !d_conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(d->tile.device));
    if (ldpc_detail::device_stalled(d->tile.device)) return ldpc_detail::stalled_error(d->tile.device);
    ldpc_status st = d->tile.calls.enter(stream);
    if (st != LDPC_OK) return st;
    if (d->legs == 0) {   // no iteration runs: zeros, converged = 0, llr = 0
        if (d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_llr && d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_llr, 0, (size_t)batch * d->n * sizeof(double), stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        if (d_solutions) LDPC_HIP_TRY(hipMemsetAsync(d_solutions, 0, (size_t)batch * sizeof(int32_t), stream));
    } else {
        const relay_kernel_t k = relay_kernel_of(d->plan.tier);
        const int threads = ldpc_detail::tile_threads(d->plan.tier);
        int64_t grid;
        size_t lds;
        st = ldpc_detail::tile_geometry(&d->tile, &d->kernel, (const void *)k, threads, d->plan, batch,
                                        "relay workspace regrow (device synchronise before the free)", &grid, &lds);
        if (st != LDPC_OK) return st;
        RelayParams p{};
        p.s = (int)d->s; p.n = (int)d->n; p.legs = d->legs; p.stop_after = d->stop_after; p.S = d->plan.S; p.shift = d->plan.shift;
        p.batch = batch; p.alpha = d->alpha; p.clip = d->clip;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.solutions = d_solutions;
        p.prior = d->prior; p.gammas = d->gammas; p.g0 = d->g0; p.leg_iters = d->leg_iters; p.weight = d->weight;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.rec_off = d->rec_off;
        p.col_ptr = d->col_ptr; p.edge_rec = d->edge_rec; p.edge_pos = d->edge_pos; p.rec_words = d->rec_words;
        p.ws = d->tile.ws; p.slot_bytes = (long long)d->plan.state_bytes;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
        d->tile.last_grid = (int)grid;
    }
    return d->tile.calls.leave(stream);
}

ldpc_status ldpc_relay_decode_batch(ldpc_relay_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err, uint8_t *conv,
                                    double *llr, int32_t *iters, int32_t *solutions)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::StageRegion r[] = {{syn, nullptr, B * s},   {nullptr, err, B * n},       {nullptr, conv, B},
                                    {nullptr, iters, B * 4}, {nullptr, solutions, B * 4}, {nullptr, llr, llr ? B * n * sizeof(double) : 0}};
    return ldpc_detail::staged_call(&d->tile, r, "relay staging regrow (device synchronise before the free)",
                                    "ldpc_relay_decode_batch (stream synchronise)", [&](char *dp) {
                                        return ldpc_relay_decode_batch_device(d, batch, (const uint8_t *)dp, (uint8_t *)(dp + r[1].at),
                                                                              (uint8_t *)(dp + r[2].at), llr ? (double *)(dp + r[5].at) : nullptr,
                                                                              (int32_t *)(dp + r[3].at), (int32_t *)(dp + r[4].at), nullptr);
                                    });
}

}  // extern "C"
