// ldpc_minsum.hip -- host side of the normalised min-sum decoder with per-bit channel LLRs: the ldpc_minsum_* entry
// points of include/ldpc_mi355x.h (the rule is stated there).  Device code: minsum_kernels.hpp (the flooding schedule) and
// layered_kernels.hpp (the layered one, over the layers of layer_plan.hpp).  The tiers (ldpc_minsum_kernel) and the tile
// width of both schedules: tile_plan.hpp.  Shared with the rest of the min-sum family (tile_host.hpp): the graph of a
// handle, the check of an entry's arguments, the launch (tile_run) and its geometry, the staging of the host-pointer
// entries, the end of a create.  Here: the order of the create's checks, the choice among the six kernels and their three
// Params structs (ms_launch), the layers.  The entries with per-syndrome priors (decode_batch_priors /
// decode_batch_given) run the same kernel templates with another prior source and, in the flooding schedule, a larger
// state (the staged priors): a handle holds a second plan for them (priors_tile_plan), computed at create.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "../../include/ldpc_mi355x_debug.h"
#include "minsum_kernels.hpp"
#include "layered_kernels.hpp"
#include "layer_plan.hpp"

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
using ldpc_detail::kTileLdsWaves;
using ldpc_detail::kTileGlobalWaves;

struct ldpc_minsum_decoder {
    int64_t s = 0, n = 0, nnz = 0, max_iters = 0;
    float alpha = 0.0f, clip = 0.0f;
    TilePlan plan;              // of the plain entries
    TilePlan pplan;             // of the priors / given entries; tier 0: kernel_variant 1 and their state does not fit
    int schedule = 0, layers = 0;   // 1 = layered: K layers, layer_ptr [K + 1] and layer_checks on the device
    int *layer_ptr = nullptr, *layer_checks = nullptr;
    float *prior = nullptr;
    float *cond = nullptr;      // [2][n]: llr_if0, llr_if1, once ldpc_minsum_set_conditional_priors has been called
    ldpc_detail::TileHost tile;            // the graph and what a launch needs (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernels[3];    // per prior source (kMsPrior*): each is a kernel function of its own
    ~ldpc_minsum_decoder() { tile.release({layer_ptr, layer_checks, prior, cond}); }
};

typedef void (*ms_kernel_t)(MsParams);
static ms_kernel_t ms_kernel_of(int tier) { return tier == 1 ? minsum_kernel<kTileLdsWaves, false> : minsum_kernel<kTileGlobalWaves, true>; }
typedef void (*layered_kernel_t)(LayeredParams);
static layered_kernel_t layered_kernel_of(int tier)
{
    return tier == 1 ? layered_minsum_kernel<kTileLdsWaves, false> : layered_minsum_kernel<kTileGlobalWaves, true>;
}
// ... and with per-syndrome priors
typedef void (*ms_priors_kernel_t)(MsPriorsParams);
template <int SRC> static ms_priors_kernel_t ms_priors_kernel_of(int tier)
{
    return tier == 1 ? minsum_kernel<kTileLdsWaves, false, SRC> : minsum_kernel<kTileGlobalWaves, true, SRC>;
}
typedef void (*layered_priors_kernel_t)(LayeredPriorsParams);
template <int SRC> static layered_priors_kernel_t layered_priors_kernel_of(int tier)
{
    return tier == 1 ? layered_minsum_kernel<kTileLdsWaves, false, SRC> : layered_minsum_kernel<kTileGlobalWaves, true, SRC>;
}

// One decode on `stream`, whatever the prior source: the plan and the state of the plain entries for the table, of the
// priors entries otherwise.  The arguments are checked, batch > 0.
static ldpc_status ms_launch(ldpc_minsum_decoder *d, int src_kind, const MsPriorSource &src, int64_t batch, const uint8_t *d_syn,
                             uint8_t *d_err, uint8_t *d_conv, double *d_llr, int32_t *d_iters, hipStream_t stream)
{
    const size_t B = (size_t)batch, n = (size_t)d->n;
    if (d->max_iters == 0)   // no iteration runs
        return ldpc_detail::tile_zero(&d->tile, stream, {{d_err, B * n}, {d_conv, B}, {d_llr, B * n * sizeof(double)}, {d_iters, B * 4}});
    const bool staged = src_kind != kMsPriorTable, layered = d->schedule == 1;
    const TilePlan &plan = staged ? d->pplan : d->plan;
    const int tier = plan.tier;
    const auto run = [&](auto kernel, auto fill) {
        return ldpc_detail::tile_run(&d->tile, &d->kernels[src_kind], kernel, plan, batch, stream,
                                     "min-sum workspace regrow (device synchronise before the free)", fill);
    };
    const auto table = [&](MsParams &p) {
        d->tile.fill(p, plan, batch);
        p.s = (int)d->s; p.n = (int)d->n; p.max_iters = (int)d->max_iters; p.alpha = d->alpha; p.clip = d->clip;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.prior = d->prior;
    };
    const auto sourced = [&](MsPriorsParams &pp) { table(pp); pp.src = src; };
    const auto layers = [&](LayeredParams &lp) { table(lp.ms); lp.K = d->layers; lp.layer_ptr = d->layer_ptr; lp.layer_checks = d->layer_checks; };
    const auto layers_sourced = [&](LayeredPriorsParams &lp) { layers(lp); lp.src = src; };
    if (src_kind == kMsPriorFloats)
        return layered ? run(layered_priors_kernel_of<kMsPriorFloats>(tier), layers_sourced) : run(ms_priors_kernel_of<kMsPriorFloats>(tier), sourced);
    if (src_kind == kMsPriorGiven)
        return layered ? run(layered_priors_kernel_of<kMsPriorGiven>(tier), layers_sourced) : run(ms_priors_kernel_of<kMsPriorGiven>(tier), sourced);
    return layered ? run(layered_kernel_of(tier), layers) : run(ms_kernel_of(tier), table);
}

// what every entry checks before any device work; batch == 0 is the caller's to answer
static ldpc_status ms_check_batch(const ldpc_minsum_decoder *d, int64_t batch, const void *syn, const void *err, const void *conv)
{
    return ldpc_detail::tile_check_batch(d, batch, {{syn, &ldpc_minsum_decoder::s}, {err, &ldpc_minsum_decoder::n}, {conv, nullptr}});
}

// ... and the priors / given entries on top: their own pointer, the tables of the given form, the second plan
static ldpc_status ms_check_priors(const ldpc_minsum_decoder *d, int64_t batch, const void *syn, const void *per_syndrome, bool given,
                                   const void *err, const void *conv)
{
    const ldpc_status st = ms_check_batch(d, batch, syn, err, conv);
    if (st != LDPC_OK) return st;
    if (given && !d->cond) return set_error(LDPC_ERR_INVALID_ARGUMENT, "no conditional priors are set (ldpc_minsum_set_conditional_priors)");
    if (batch > 0 && d->n > 0 && !per_syndrome) return set_error(LDPC_ERR_INVALID_ARGUMENT, given ? "given pointer is NULL" : "priors pointer is NULL");
    if (d->pplan.tier == 0)
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome with its priors does not fit the on-chip tier");
    return LDPC_OK;
}

// The host form of every entry: the syndromes and `extra` (extra_bytes per syndrome: the priors or the given bits, or
// nothing) into the staging buffer, `decode` on the null stream, the copies out.  The arguments are checked, batch > 0.
template <class F>
static ldpc_status ms_decode_to_host(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *syn, const void *extra, size_t extra_bytes,
                                     uint8_t *err, uint8_t *conv, double *llr, int32_t *iters, const char *what, F decode)
{
    const size_t s = (size_t)d->s, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::StageRegion r[] = {{syn, nullptr, B * s}, {nullptr, err, B * n}, {nullptr, conv, B}, {nullptr, iters, B * 4},
                                    {nullptr, llr, llr ? B * n * sizeof(double) : 0}, {extra, nullptr, B * extra_bytes}};
    return ldpc_detail::staged_call(&d->tile, r, "min-sum staging regrow (device synchronise before the free)", what, [&](char *dp) {
        return decode((const uint8_t *)dp, (const void *)(dp + r[5].at), (uint8_t *)(dp + r[1].at), (uint8_t *)(dp + r[2].at),
                      llr ? (double *)(dp + r[4].at) : nullptr, (int32_t *)(dp + r[3].at));
    });
}

extern "C" {

ldpc_status ldpc_minsum_create(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                               const float *channel_llr, int64_t max_iters, const ldpc_minsum_options *options,
                               ldpc_minsum_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, max_iters);
    if (st != LDPC_OK) return st;
    if (n > 0 && !channel_llr) return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr is NULL");
    float alpha, clip;
    int variant, device;
    if ((st = ldpc_detail::tile_options(options, &alpha, &clip, &variant, &device)) != LDPC_OK) return st;
    const int schedule = options ? options->schedule : 0;
    if (schedule < 0 || schedule > 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, "schedule must be 0 (flooding) or 1 (layered)");
    for (int64_t j = 0; j < n; ++j)
        if (!std::isfinite(channel_llr[j]))
            return set_error(LDPC_ERR_INVALID_ARGUMENT, "channel_llr[" + std::to_string(j) + "] is not finite");
    if ((st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    if ((st = ldpc_detail::tile_index_limits("min-sum", s, n, nnz, true)) != LDPC_OK) return st;

    ldpc_minsum_decoder *d = new (std::nothrow) ldpc_minsum_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->max_iters = max_iters; d->alpha = alpha; d->clip = clip;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount; d->schedule = schedule;
    d->tile.graph.build(s, n, nnz, colptr, rowval);
    const ldpc_detail::TannerGraph &g = d->tile.graph.host;
    const int64_t words = d->tile.graph.rec.words;
    if (!tile_plan(s, n, words, false, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    if (!priors_tile_plan(s, n, words, schedule == 1, variant, &d->pplan)) d->pplan = TilePlan();   // (tier 0: those entries answer UNSUPPORTED)
    LayerPlan layers;   // the layered schedule: first-fit layers (layer_plan.hpp), verified before they reach the device
    if (schedule == 1) {
        std::string why;
        const LayerPlanStatus ls = layer_plan_build(s, n, g.row_ptr.data(), g.csr_col.data(), &layers, &why);
        if (ls != kLayerPlanOk) {
            delete d;
            return set_error(ls == kLayerPlanNoMemory ? LDPC_ERR_OUT_OF_MEMORY : ls == kLayerPlanTooLarge ? LDPC_ERR_UNSUPPORTED : LDPC_ERR_INVALID_ARGUMENT, why);
        }
        if (!layer_plan_verify(s, n, g.row_ptr.data(), g.csr_col.data(), layers, &why)) {   // (a slip would be a data race in the kernel)
            delete d;
            return set_error(LDPC_ERR_HIP, "internal error: " + why);
        }
        d->layers = layers.K;
    }
    ldpc_detail::tile_grid_max_env(&d->tile);
    using ldpc_detail::upload;
    return ldpc_detail::tile_create_finish(d, out, [&] {
        return (schedule == 0 || (upload(&d->layer_ptr, layers.layer_ptr) && upload(&d->layer_checks, layers.layer_checks))) &&
               upload(&d->prior, std::vector<float>(channel_llr, channel_llr + n));
    });
}

// (include/ldpc_mi355x_debug.h) the choice both create routines make, without a device
ldpc_status ldpc_debug_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t relay, int32_t kernel_variant, int32_t *tier,
                                 int32_t *tile_syndromes, int64_t *state_bytes)
{
    const ldpc_status st = ldpc_detail::tile_debug_args(s, n, rec_words, rec_words, kernel_variant);
    if (st != LDPC_OK) return st;
    TilePlan plan;
    return ldpc_detail::tile_debug_answer(tile_plan(s, n, rec_words, relay != 0, kernel_variant, &plan), plan,
                                          "kernel_variant 1: the state of one syndrome does not fit the on-chip tier", tier, tile_syndromes, state_bytes);
}

// (include/ldpc_mi355x_debug.h) ... and the second plan, of the entries with per-syndrome priors
ldpc_status ldpc_debug_priors_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t schedule, int32_t kernel_variant, int32_t *tier,
                                        int32_t *tile_syndromes, int64_t *state_bytes)
{
    const ldpc_status st = ldpc_detail::tile_debug_args(s, n, rec_words, rec_words, kernel_variant);
    if (st != LDPC_OK) return st;
    if (schedule < 0 || schedule > 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, "schedule must be 0 (flooding) or 1 (layered)");
    TilePlan plan;
    return ldpc_detail::tile_debug_answer(priors_tile_plan(s, n, rec_words, schedule == 1, kernel_variant, &plan), plan,
                                          "kernel_variant 1: the state of one syndrome with its priors does not fit the on-chip tier", tier,
                                          tile_syndromes, state_bytes);
}

// (include/ldpc_mi355x_debug.h) the layers create uploads for a layered handle, without a device
ldpc_status ldpc_debug_layer_plan(int64_t s, int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t *layer_of, int32_t *K)
{
    if (s < 0 || n < 0 || !colptr) return set_error(LDPC_ERR_INVALID_ARGUMENT, "s and n must be >= 0 and colptr not NULL");
    const int64_t nnz = n > 0 ? colptr[n] : 0;
    ldpc_status st = ldpc_detail::check_csc_args(s, n, nnz, colptr, rowval, 0);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(s, n, nnz, colptr, rowval)) != LDPC_OK) return st;
    if ((st = ldpc_detail::tile_index_limits("min-sum", s, n, nnz, true)) != LDPC_OK) return st;
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    LayerPlan plan;
    std::string why;
    const LayerPlanStatus ls = layer_plan_build(s, n, g.row_ptr.data(), g.csr_col.data(), &plan, &why);
    if (ls != kLayerPlanOk)
        return set_error(ls == kLayerPlanNoMemory ? LDPC_ERR_OUT_OF_MEMORY : ls == kLayerPlanTooLarge ? LDPC_ERR_UNSUPPORTED : LDPC_ERR_INVALID_ARGUMENT, why);
    if (!layer_plan_verify(s, n, g.row_ptr.data(), g.csr_col.data(), plan, &why)) return set_error(LDPC_ERR_HIP, "internal error: " + why);
    if (layer_of)
        for (int64_t i = 0; i < s; ++i) layer_of[i] = plan.layer_of[(size_t)i];
    if (K) *K = plan.K;
    return LDPC_OK;
}

int32_t ldpc_minsum_kernel(const ldpc_minsum_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_minsum_tile_syndromes(const ldpc_minsum_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_minsum_priors_kernel(const ldpc_minsum_decoder *d) { return d ? d->pplan.tier : 0; }
int32_t ldpc_minsum_priors_tile_syndromes(const ldpc_minsum_decoder *d) { return d && d->pplan.tier ? d->pplan.S : 0; }
int32_t ldpc_minsum_last_grid(const ldpc_minsum_decoder *d) { return d ? d->tile.last_grid : 0; }
int32_t ldpc_minsum_layers(const ldpc_minsum_decoder *d) { return d && d->schedule == 1 ? d->layers : 0; }

ldpc_status ldpc_minsum_destroy(ldpc_minsum_decoder *d) { return ldpc_detail::tile_destroy(d, "ldpc_minsum_destroy (device synchronise)"); }

ldpc_status ldpc_minsum_decode_batch_device(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_err,
                                            uint8_t *d_conv, double *d_llr, int32_t *d_iters, void *stream_v)
{
    const ldpc_status st = ms_check_batch(d, batch, d_syn, d_err, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    return ms_launch(d, kMsPriorTable, MsPriorSource{}, batch, d_syn, d_err, d_conv, d_llr, d_iters, (hipStream_t)stream_v);
}

ldpc_status ldpc_minsum_decode_batch(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err, uint8_t *conv,
                                     double *llr, int32_t *iters)
{
    const ldpc_status st = ms_check_batch(d, batch, syn, err, conv);
    if (st != LDPC_OK || batch == 0) return st;
    return ms_decode_to_host(d, batch, syn, nullptr, 0, err, conv, llr, iters, "ldpc_minsum_decode_batch (stream synchronise)",
                             [&](const uint8_t *d_syn, const void *, uint8_t *d_err, uint8_t *d_conv, double *d_llr, int32_t *d_iters) {
                                 return ldpc_minsum_decode_batch_device(d, batch, d_syn, d_err, d_conv, d_llr, d_iters, nullptr);
                             });
}

// ---- per-syndrome priors ---------------------------------------------------------------------------------------------------

ldpc_status ldpc_minsum_decode_batch_priors_device(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *d_syn, const float *d_priors,
                                                   uint8_t *d_err, uint8_t *d_conv, double *d_llr, int32_t *d_iters, void *stream_v)
{
    const ldpc_status st = ms_check_priors(d, batch, d_syn, d_priors, false, d_err, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    MsPriorSource src{};
    src.priors = d_priors;
    return ms_launch(d, kMsPriorFloats, src, batch, d_syn, d_err, d_conv, d_llr, d_iters, (hipStream_t)stream_v);
}

ldpc_status ldpc_minsum_decode_batch_priors(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *syn, const float *priors, uint8_t *err,
                                            uint8_t *conv, double *llr, int32_t *iters)
{
    const ldpc_status st = ms_check_priors(d, batch, syn, priors, false, err, conv);
    if (st != LDPC_OK || batch == 0) return st;
    return ms_decode_to_host(d, batch, syn, priors, (size_t)d->n * sizeof(float), err, conv, llr, iters,
                             "ldpc_minsum_decode_batch_priors (stream synchronise)",
                             [&](const uint8_t *d_syn, const void *d_extra, uint8_t *d_err, uint8_t *d_conv, double *d_llr, int32_t *d_iters) {
                                 return ldpc_minsum_decode_batch_priors_device(d, batch, d_syn, (const float *)d_extra, d_err, d_conv, d_llr,
                                                                               d_iters, nullptr);
                             });
}

ldpc_status ldpc_minsum_set_conditional_priors(ldpc_minsum_decoder *d, const float *llr_if0, const float *llr_if1)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (d->n > 0 && (!llr_if0 || !llr_if1)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "llr_if0 or llr_if1 is NULL");
    const size_t n = (size_t)d->n;
    std::vector<float> both(std::max<size_t>(2 * n, 1), 0.0f);
    for (size_t j = 0; j < n; ++j) {
        if (!std::isfinite(llr_if0[j])) return set_error(LDPC_ERR_INVALID_ARGUMENT, "llr_if0[" + std::to_string(j) + "] is not finite");
        if (!std::isfinite(llr_if1[j])) return set_error(LDPC_ERR_INVALID_ARGUMENT, "llr_if1[" + std::to_string(j) + "] is not finite");
        both[j] = llr_if0[j];
        both[n + j] = llr_if1[j];
    }
    LDPC_HIP_TRY(hipSetDevice(d->tile.device));
    if (ldpc_detail::device_stalled(d->tile.device)) return ldpc_detail::stalled_error(d->tile.device);
    // after every earlier call on the handle: a decode still in flight reads the tables it was launched with to its end
    if (d->tile.calls.have) {
        const ldpc_status st = ldpc_detail::wait_event(d->tile.calls.done, d->tile.device, "ldpc_minsum_set_conditional_priors (wait for the earlier calls)");
        if (st != LDPC_OK) return st;
    }
    float *fresh = d->cond;
    if (!fresh) LDPC_HIP_TRY(hipMalloc((void **)&fresh, both.size() * sizeof(float)));
    const hipError_t e = hipMemcpy(fresh, both.data(), both.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess && !d->cond) (void)hipFree(fresh);
    LDPC_HIP_TRY(e);
    d->cond = fresh;
    return LDPC_OK;
}

ldpc_status ldpc_minsum_decode_batch_given_device(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *d_syn, const uint8_t *d_given,
                                                  uint8_t *d_err, uint8_t *d_conv, double *d_llr, int32_t *d_iters, void *stream_v)
{
    const ldpc_status st = ms_check_priors(d, batch, d_syn, d_given, true, d_err, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    MsPriorSource src{};
    src.given = d_given; src.llr_if0 = d->cond; src.llr_if1 = d->cond + d->n;
    return ms_launch(d, kMsPriorGiven, src, batch, d_syn, d_err, d_conv, d_llr, d_iters, (hipStream_t)stream_v);
}

ldpc_status ldpc_minsum_decode_batch_given(ldpc_minsum_decoder *d, int64_t batch, const uint8_t *syn, const uint8_t *given, uint8_t *err,
                                           uint8_t *conv, double *llr, int32_t *iters)
{
    const ldpc_status st = ms_check_priors(d, batch, syn, given, true, err, conv);
    if (st != LDPC_OK || batch == 0) return st;
    return ms_decode_to_host(d, batch, syn, given, (size_t)d->n, err, conv, llr, iters, "ldpc_minsum_decode_batch_given (stream synchronise)",
                             [&](const uint8_t *d_syn, const void *d_extra, uint8_t *d_err, uint8_t *d_conv, double *d_llr, int32_t *d_iters) {
                                 return ldpc_minsum_decode_batch_given_device(d, batch, d_syn, (const uint8_t *)d_extra, d_err, d_conv, d_llr,
                                                                              d_iters, nullptr);
                             });
}

}  // extern "C"
