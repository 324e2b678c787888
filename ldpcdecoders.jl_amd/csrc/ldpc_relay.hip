// ldpc_relay.hip -- host side of the relay min-sum decoder (min-sum with a per-bit memory, run as a chain of legs, the
// lightest of the first solutions returned): the ldpc_relay_* entry points of include/ldpc_mi355x.h (the rule is stated
// there).  Device code: relay_kernels.hpp.  The tiers (ldpc_relay_kernel) and the tile width: tile_plan.hpp, over the relay
// state.  Shared with the rest of the min-sum family (tile_host.hpp): the graph of a handle, the check of an entry's
// arguments, the launch (tile_run) and its geometry, the staging of the host-pointer entry, the end of a create; with
// ldpc_pauli_relay.hip (relay_host.hpp): the checks of the legs, the legs that run -- legs of 0 iterations are dropped, so
// the kernel sees none --, the weight of a prior.  Here: the order of the create's checks, RelayParams, the tables of the
// legs.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "relay_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
#include "relay_host.hpp"
using ldpc_detail::set_error;

struct ldpc_relay_decoder {
    int64_t s = 0, n = 0, nnz = 0;
    int legs = 0, stop_after = 1;   // legs: those that run
    float alpha = 0.0f, clip = 0.0f;
    TilePlan plan;
    int *leg_iters = nullptr;
    float *prior = nullptr, *gammas = nullptr, *g0 = nullptr;
    long long *weight = nullptr;
    ldpc_detail::TileHost tile;   // the graph and what a launch needs (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernel;
    ~ldpc_relay_decoder() { tile.release({leg_iters, prior, gammas, g0, weight}); }
};

typedef void (*relay_kernel_t)(RelayParams);
static relay_kernel_t relay_kernel_of(int tier) { return tier == 1 ? relay_kernel<ldpc_detail::kTileLdsWaves, false> : relay_kernel<ldpc_detail::kTileGlobalWaves, true>; }

// what every entry checks before any device work; batch == 0 is the caller's to answer
static ldpc_status relay_check_batch(const ldpc_relay_decoder *d, int64_t batch, const void *syn, const void *err, const void *conv)
{
    return ldpc_detail::tile_check_batch(d, batch, {{syn, &ldpc_relay_decoder::s}, {err, &ldpc_relay_decoder::n}, {conv, nullptr}});
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
    float alpha, clip;
    int variant, device, stop_after;
    st = ldpc_detail::relay_check_legs(n, legs, gammas, leg_iters, options, &alpha, &clip, &variant, &device, &stop_after, [&] {
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(channel_llr[j]))
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr[" + std::to_string(j) + "] is not finite");
        return LDPC_OK;
    });
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    if ((st = ldpc_detail::relay_index_limits("relay", s, n, nnz)) != LDPC_OK) return st;

    ldpc_relay_decoder *d = new (std::nothrow) ldpc_relay_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->alpha = alpha; d->clip = clip; d->stop_after = stop_after;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount;
    // what the rule derives once per handle, for the legs that run: g0 = (1 - gamma) * channel_llr; q = relay_weight(llr)
    std::vector<float> h_gam, h_g0;
    const std::vector<int> h_iters = ldpc_detail::relay_running_legs(legs, leg_iters, [&](int64_t r) {
        for (int64_t j = 0; j < n; ++j) {
            const float g = gammas[r * n + j];
            const float one_minus = 1.0f - g;
            h_gam.push_back(g);
            h_g0.push_back(one_minus * channel_llr[j]);
        }
    });
    d->legs = (int)h_iters.size();
    std::vector<long long> h_weight((size_t)n);
    for (int64_t j = 0; j < n; ++j) h_weight[(size_t)j] = ldpc_detail::relay_weight(channel_llr[j]);
    d->tile.graph.build(s, n, nnz, colptr, rowval);
    if (!tile_plan(s, n, d->tile.graph.rec.words, true, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    ldpc_detail::tile_grid_max_env(&d->tile);
    using ldpc_detail::upload;
    return ldpc_detail::tile_create_finish(d, out, [&] {
        return upload(&d->leg_iters, h_iters) && upload(&d->prior, std::vector<float>(channel_llr, channel_llr + n)) &&
               upload(&d->gammas, h_gam) && upload(&d->g0, h_g0) && upload(&d->weight, h_weight);
    });
}

int32_t ldpc_relay_kernel(const ldpc_relay_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_relay_tile_syndromes(const ldpc_relay_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_relay_last_grid(const ldpc_relay_decoder *d) { return d ? d->tile.last_grid : 0; }

ldpc_status ldpc_relay_destroy(ldpc_relay_decoder *d) { return ldpc_detail::tile_destroy(d, "ldpc_relay_destroy (device synchronise)"); }

ldpc_status ldpc_relay_decode_batch_device(ldpc_relay_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                           uint8_t *d_conv, double *d_llr, int32_t *d_iters, int32_t *d_solutions, void *stream_v)
{
    const ldpc_status st = relay_check_batch(d, batch, d_syn, d_err, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t B = (size_t)batch, n = (size_t)d->n;
    if (d->legs == 0)   // no iteration runs
        return ldpc_detail::tile_zero(&d->tile, (hipStream_t)stream_v,
                                      {{d_err, B * n}, {d_conv, B}, {d_llr, B * n * sizeof(double)}, {d_iters, B * 4}, {d_solutions, B * 4}});
    return ldpc_detail::tile_run(&d->tile, &d->kernel, relay_kernel_of(d->plan.tier), d->plan, batch, (hipStream_t)stream_v,
                                 "relay workspace regrow (device synchronise before the free)", [&](RelayParams &p) {
                                     d->tile.fill(p, d->plan, batch);
                                     p.s = (int)d->s; p.n = (int)d->n; p.legs = d->legs; p.stop_after = d->stop_after;
                                     p.alpha = d->alpha; p.clip = d->clip;
                                     p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.solutions = d_solutions;
                                     p.prior = d->prior; p.gammas = d->gammas; p.g0 = d->g0; p.leg_iters = d->leg_iters; p.weight = d->weight;
                                 });
}

ldpc_status ldpc_relay_decode_batch(ldpc_relay_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err, uint8_t *conv,
                                    double *llr, int32_t *iters, int32_t *solutions)
{
    const ldpc_status st = relay_check_batch(d, batch, syn, err, conv);
    if (st != LDPC_OK || batch == 0) return st;
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
