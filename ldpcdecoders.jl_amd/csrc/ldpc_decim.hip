// ldpc_decim.hip -- host side of the guided-decimation min-sum decoder (min-sum in rounds; a round that does not converge
// hard-fixes the most reliable undecided bit and the next one goes on from the same messages): the ldpc_decim_* entry
// points of include/ldpc_mi355x.h (the rule is stated there).  Device code: decim_kernels.hpp.  The tiers
// (ldpc_decim_kernel) and the tile width: tile_plan.hpp, over the decimation state.  Shared with the rest of the min-sum
// family (tile_host.hpp): the graph of a handle, the check of an entry's arguments, the launch (tile_run) and its geometry,
// the staging of the host-pointer entry, the end of a create.  Here: the order of the create's checks and DecimParams.
// No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "../../include/ldpc_mi355x_debug.h"
#include "decim_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
#include "tile_host.hpp"
using ldpc_detail::set_error;

struct ldpc_decim_decoder {
    int64_t s = 0, n = 0, nnz = 0;
    int round_iters = 0, max_dec = 0;
    float alpha = 0.0f, clip = 0.0f, pin = 0.0f;
    TilePlan plan;
    float *prior = nullptr;
    ldpc_detail::TileHost tile;   // the graph and what a launch needs (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernel;
    ~ldpc_decim_decoder() { tile.release({prior}); }
};

typedef void (*decim_kernel_t)(DecimParams);
static decim_kernel_t decim_kernel_of(int tier) { return tier == 1 ? decim_kernel<ldpc_detail::kTileLdsWaves, false> : decim_kernel<ldpc_detail::kTileGlobalWaves, true>; }

// what every entry checks before any device work; batch == 0 is the caller's to answer
static ldpc_status decim_check_batch(const ldpc_decim_decoder *d, int64_t batch, const void *syn, const void *err, const void *conv)
{
    return ldpc_detail::tile_check_batch(d, batch, {{syn, &ldpc_decim_decoder::s}, {err, &ldpc_decim_decoder::n}, {conv, nullptr}});
}

extern "C" {

ldpc_status ldpc_decim_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                              const float *channel_llr, int64_t round_iters, int64_t max_decimations,
                              const ldpc_decim_options *options, ldpc_decim_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, 0);
    if (st != LDPC_OK) return st;
    if (n > 0 && !channel_llr) return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr is NULL");
    if (round_iters < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "round_iters must be >= 0");
    if (max_decimations < 0 || max_decimations > n) return set_error(LDPC_ERR_INVALID_ARGUMENT, "max_decimations must lie in 0 .. n");
    if (round_iters > 0 && max_decimations + 1 > (int64_t)INT32_MAX / round_iters)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "round_iters * (max_decimations + 1) exceeds INT32_MAX");
    float alpha, clip;
    int variant, device;
    if ((st = ldpc_detail::tile_options(options, &alpha, &clip, &variant, &device)) != LDPC_OK) return st;
    const float pin = 2.0f * clip;
    if (!std::isfinite(pin)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "2 * clip (the pin of a decimated bit) must be finite");
    for (int64_t j = 0; j < n; ++j)
        if (!std::isfinite(channel_llr[j]))
            return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr[" + std::to_string(j) + "] is not finite");
    if ((st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    if ((st = ldpc_detail::tile_index_limits("decimation", s, n, nnz, true)) != LDPC_OK) return st;

    ldpc_decim_decoder *d = new (std::nothrow) ldpc_decim_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->alpha = alpha; d->clip = clip; d->pin = pin;
    d->round_iters = (int)round_iters; d->max_dec = (int)max_decimations;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount;
    d->tile.graph.build(s, n, nnz, colptr, rowval);
    if (!decim_tile_plan(s, n, d->tile.graph.rec.words, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    ldpc_detail::tile_grid_max_env(&d->tile);
    return ldpc_detail::tile_create_finish(d, out, [&] { return ldpc_detail::upload(&d->prior, std::vector<float>(channel_llr, channel_llr + n)); });
}

// (include/ldpc_mi355x_debug.h) the choice create makes, without a device
ldpc_status ldpc_debug_decim_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t kernel_variant, int32_t *tier,
                                       int32_t *tile_syndromes, int64_t *state_bytes)
{
    const ldpc_status st = ldpc_detail::tile_debug_args(s, n, rec_words, rec_words + ((n + 31) >> 5), kernel_variant);   // (the records and D)
    if (st != LDPC_OK) return st;
    TilePlan plan;
    return ldpc_detail::tile_debug_answer(decim_tile_plan(s, n, rec_words, kernel_variant, &plan), plan,
                                          "kernel_variant 1: the state of one syndrome does not fit the on-chip tier", tier, tile_syndromes, state_bytes);
}

int32_t ldpc_decim_kernel(const ldpc_decim_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_decim_tile_syndromes(const ldpc_decim_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_decim_last_grid(const ldpc_decim_decoder *d) { return d ? d->tile.last_grid : 0; }

ldpc_status ldpc_decim_destroy(ldpc_decim_decoder *d) { return ldpc_detail::tile_destroy(d, "ldpc_decim_destroy (device synchronise)"); }

ldpc_status ldpc_decim_decode_batch_device(ldpc_decim_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                           uint8_t *d_conv, double *d_llr, int32_t *d_iters, int32_t *d_decimated, void *stream_v)
{
    const ldpc_status st = decim_check_batch(d, batch, d_syn, d_err, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t B = (size_t)batch, n = (size_t)d->n;
    if (d->round_iters == 0)   // no iteration runs
        return ldpc_detail::tile_zero(&d->tile, (hipStream_t)stream_v,
                                      {{d_err, B * n}, {d_conv, B}, {d_llr, B * n * sizeof(double)}, {d_iters, B * 4}, {d_decimated, B * 4}});
    return ldpc_detail::tile_run(&d->tile, &d->kernel, decim_kernel_of(d->plan.tier), d->plan, batch, (hipStream_t)stream_v,
                                 "decimation workspace regrow (device synchronise before the free)", [&](DecimParams &p) {
                                     d->tile.fill(p, d->plan, batch);
                                     p.s = (int)d->s; p.n = (int)d->n; p.round_iters = d->round_iters; p.max_dec = d->max_dec;
                                     p.total_iters = d->round_iters * (d->max_dec + 1);   // (create: fits int32)
                                     p.alpha = d->alpha; p.clip = d->clip; p.pin = d->pin;
                                     p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.decimated = d_decimated;
                                     p.prior = d->prior;
                                 });
}

ldpc_status ldpc_decim_decode_batch(ldpc_decim_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err, uint8_t *conv,
                                    double *llr, int32_t *iters, int32_t *decimated)
{
    const ldpc_status st = decim_check_batch(d, batch, syn, err, conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::StageRegion r[] = {{syn, nullptr, B * s},   {nullptr, err, B * n},       {nullptr, conv, B},
                                    {nullptr, iters, B * 4}, {nullptr, decimated, B * 4}, {nullptr, llr, llr ? B * n * sizeof(double) : 0}};
    return ldpc_detail::staged_call(&d->tile, r, "decimation staging regrow (device synchronise before the free)",
                                    "ldpc_decim_decode_batch (stream synchronise)", [&](char *dp) {
                                        return ldpc_decim_decode_batch_device(d, batch, (const uint8_t *)dp, (uint8_t *)(dp + r[1].at),
                                                                              (uint8_t *)(dp + r[2].at), llr ? (double *)(dp + r[5].at) : nullptr,
                                                                              (int32_t *)(dp + r[3].at), (int32_t *)(dp + r[4].at), nullptr);
                                    });
}

}  // extern "C"
