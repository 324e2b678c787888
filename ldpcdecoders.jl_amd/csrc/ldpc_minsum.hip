// ldpc_minsum.hip -- host side of the normalised min-sum decoder with per-bit channel LLRs: the ldpc_minsum_* entry
// points of include/ldpc_mi355x.h (the rule is stated there).  Device code: minsum_kernels.hpp (the flooding schedule) and
// layered_kernels.hpp (the layered one, over the layers of layer_plan.hpp).  The tiers (ldpc_minsum_kernel) and the tile
// width of both schedules: tile_plan.hpp; the launch geometry, the staging of the host-pointer entries and the rest of
// what the min-sum family shares on the host: tile_host.hpp.  The entries with per-syndrome priors (decode_batch_priors /
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

#include "host_env.hpp"      // exp_env: LDPC_MS_GRID_MAX, experiments build only
#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
#include "tile_host.hpp"
using ldpc_detail::set_error;
using ldpc_detail::kTileLdsWaves;
using ldpc_detail::kTileGlobalWaves;

struct ldpc_minsum_decoder {
    int64_t s = 0, n = 0, nnz = 0, max_iters = 0;
    float alpha = 0.0f, clip = 0.0f;
    int rec_words = 0;
    TilePlan plan;              // of the plain entries
    TilePlan pplan;             // of the priors / given entries; tier 0: kernel_variant 1 and their state does not fit
    int schedule = 0, layers = 0;   // 1 = layered: K layers, layer_ptr [K + 1] and layer_checks on the device
    int *layer_ptr = nullptr, *layer_checks = nullptr;
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *edge_rec = nullptr, *edge_pos = nullptr;
    float *prior = nullptr;
    float *cond = nullptr;      // [2][n]: llr_if0, llr_if1, once ldpc_minsum_set_conditional_priors has been called
    ldpc_detail::TileHost tile;            // (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernels[3];    // per prior source (kMsPrior*): each is a kernel function of its own
    ~ldpc_minsum_decoder() { tile.release({row_ptr, csr_col, rec_off, col_ptr, edge_rec, edge_pos, layer_ptr, layer_checks, prior, cond}); }
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
    LDPC_HIP_TRY(hipSetDevice(d->tile.device));
    if (ldpc_detail::device_stalled(d->tile.device)) return ldpc_detail::stalled_error(d->tile.device);
    ldpc_status st = d->tile.calls.enter(stream);
    if (st != LDPC_OK) return st;
    if (d->max_iters == 0) {   // no iteration runs: zeros, converged = 0, llr = 0
        if (d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_llr && d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_llr, 0, (size_t)batch * d->n * sizeof(double), stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
    } else {
        const bool staged = src_kind != kMsPriorTable, layered = d->schedule == 1;
        const TilePlan &plan = staged ? d->pplan : d->plan;
        const int tier = plan.tier, threads = ldpc_detail::tile_threads(tier);
        const void *k;
        if (src_kind == kMsPriorFloats)
            k = layered ? (const void *)layered_priors_kernel_of<kMsPriorFloats>(tier) : (const void *)ms_priors_kernel_of<kMsPriorFloats>(tier);
        else if (src_kind == kMsPriorGiven)
            k = layered ? (const void *)layered_priors_kernel_of<kMsPriorGiven>(tier) : (const void *)ms_priors_kernel_of<kMsPriorGiven>(tier);
        else
            k = layered ? (const void *)layered_kernel_of(tier) : (const void *)ms_kernel_of(tier);
        int64_t grid;
        size_t lds;
        st = ldpc_detail::tile_geometry(&d->tile, &d->kernels[src_kind], k, threads, plan, batch,
                                        "min-sum workspace regrow (device synchronise before the free)", &grid, &lds);
        if (st != LDPC_OK) return st;
        MsParams p{};
        p.s = (int)d->s; p.n = (int)d->n; p.max_iters = (int)d->max_iters; p.S = plan.S; p.shift = plan.shift;
        p.batch = batch; p.alpha = d->alpha; p.clip = d->clip;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters;
        p.prior = d->prior; p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.rec_off = d->rec_off;
        p.col_ptr = d->col_ptr; p.edge_rec = d->edge_rec; p.edge_pos = d->edge_pos; p.rec_words = d->rec_words;
        p.ws = d->tile.ws; p.slot_bytes = (long long)plan.state_bytes;
        const dim3 g((unsigned)grid), b((unsigned)threads);
        if (layered) {
            LayeredPriorsParams lp{};
            lp.ms = p; lp.K = d->layers; lp.layer_ptr = d->layer_ptr; lp.layer_checks = d->layer_checks; lp.src = src;
            if (src_kind == kMsPriorFloats) hipLaunchKernelGGL(layered_priors_kernel_of<kMsPriorFloats>(tier), g, b, lds, stream, lp);
            else if (src_kind == kMsPriorGiven) hipLaunchKernelGGL(layered_priors_kernel_of<kMsPriorGiven>(tier), g, b, lds, stream, lp);
            else hipLaunchKernelGGL(layered_kernel_of(tier), g, b, lds, stream, (const LayeredParams &)lp);
        } else {
            MsPriorsParams pp{};
            (MsParams &)pp = p; pp.src = src;
            if (src_kind == kMsPriorFloats) hipLaunchKernelGGL(ms_priors_kernel_of<kMsPriorFloats>(tier), g, b, lds, stream, pp);
            else if (src_kind == kMsPriorGiven) hipLaunchKernelGGL(ms_priors_kernel_of<kMsPriorGiven>(tier), g, b, lds, stream, pp);
            else hipLaunchKernelGGL(ms_kernel_of(tier), g, b, lds, stream, p);
        }
        LDPC_HIP_TRY(hipGetLastError());
        d->tile.last_grid = (int)grid;
    }
    return d->tile.calls.leave(stream);
}

// what every device entry checks before any device work; batch == 0 is the caller's to answer
static ldpc_status ms_check_batch(const ldpc_minsum_decoder *d, int64_t batch, const void *syn, const void *err, const void *conv)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    return LDPC_OK;
}

// ... and the priors / given entries on top: their own pointer, the tables of the given form, the second plan
static ldpc_status ms_check_priors(const ldpc_minsum_decoder *d, int64_t batch, const void *syn, const void *per_syndrome, bool given,
                                   const void *err, const void *conv)
{
    const ldpc_status st = ms_check_batch(d, batch, syn, err, conv);
    if (st != LDPC_OK) return st;
    if (given && !d->cond) return set_error(LDPC_ERR_INVALID_ARGUMENT, "no conditional priors are set (ldpc_minsum_set_conditional_priors)");
    if (batch > 0 && d->n > 0 && !per_syndrome) return set_error(LDPC_ERR_INVALID_ARGUMENT, given ? "given pointer is NULL" : "priors pointer is NULL");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
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
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "min-sum kernels: graph too large for 32-bit edge indexing");

    ldpc_minsum_decoder *d = new (std::nothrow) ldpc_minsum_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->max_iters = max_iters; d->alpha = alpha; d->clip = clip;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount; d->schedule = schedule;
    // CSR (checks -> bits, ascending) next to the caller's CSC; a record per check; per CSC edge its record and position
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    const MsRecords rec = ms_records(s, nnz, g.row_ptr.data(), g.csc_row.data(), g.csc2csr.data());   // words <= 4 s + nnz < 2^31
    d->rec_words = (int)rec.words;
    if (!tile_plan(s, n, rec.words, false, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    if (!priors_tile_plan(s, n, rec.words, schedule == 1, variant, &d->pplan)) d->pplan = TilePlan();   // (tier 0: those entries answer UNSUPPORTED)
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
    if (const char *e = exp_env("LDPC_MS_GRID_MAX")) d->tile.grid_max = std::max(1, std::atoi(e));   // (experiments build: tests cap the grid)
    using ldpc_detail::upload;
    bool ok = upload(&d->row_ptr, g.row_ptr) && upload(&d->csr_col, g.csr_col) && upload(&d->rec_off, rec.rec_off) &&
              upload(&d->col_ptr, g.col_ptr) && upload(&d->edge_rec, rec.edge_rec) && upload(&d->edge_pos, rec.edge_pos) &&
              (schedule == 0 || (upload(&d->layer_ptr, layers.layer_ptr) && upload(&d->layer_checks, layers.layer_checks))) &&
              upload(&d->prior, std::vector<float>(channel_llr, channel_llr + n)) && d->tile.calls.create() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
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
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "min-sum kernels: graph too large for 32-bit edge indexing");
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
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
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
