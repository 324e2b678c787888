// ldpc_decim.hip -- host side of the guided-decimation min-sum decoder (min-sum in rounds; a round that does not converge
// hard-fixes the most reliable undecided bit and the next one goes on from the same messages): the ldpc_decim_* entry
// points of include/ldpc_mi355x.h (the rule is stated there).  Device code: decim_kernels.hpp.  The tiers
// (ldpc_decim_kernel) and the tile width: tile_plan.hpp, over the decimation state; the launch geometry and the rest of
// what the min-sum family shares on the host: tile_host.hpp.  No CPU path.
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

#include "host_env.hpp"      // exp_env: LDPC_MS_GRID_MAX, experiments build only
#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
#include "tile_host.hpp"
using ldpc_detail::set_error;

struct ldpc_decim_decoder {
    int64_t s = 0, n = 0, nnz = 0;
    int round_iters = 0, max_dec = 0;
    float alpha = 0.0f, clip = 0.0f, pin = 0.0f;
    int rec_words = 0;
    TilePlan plan;
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *edge_rec = nullptr, *edge_pos = nullptr;
    float *prior = nullptr;
    ldpc_detail::TileHost tile;   // (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernel;
    ~ldpc_decim_decoder() { tile.release({row_ptr, csr_col, rec_off, col_ptr, edge_rec, edge_pos, prior}); }
};

typedef void (*decim_kernel_t)(DecimParams);
static decim_kernel_t decim_kernel_of(int tier) { return tier == 1 ? decim_kernel<ldpc_detail::kTileLdsWaves, false> : decim_kernel<ldpc_detail::kTileGlobalWaves, true>; }

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
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "decimation kernels: graph too large for 32-bit edge indexing");

    ldpc_decim_decoder *d = new (std::nothrow) ldpc_decim_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->s = s; d->n = n; d->nnz = nnz; d->alpha = alpha; d->clip = clip; d->pin = pin;
    d->round_iters = (int)round_iters; d->max_dec = (int)max_decimations;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount;
    // CSR (checks -> bits, ascending) next to the caller's CSC; a record per check; per CSC edge its record and position
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr, rowval);
    const MsRecords rec = ms_records(s, nnz, g.row_ptr.data(), g.csc_row.data(), g.csc2csr.data());   // words <= 4 s + nnz < 2^31
    d->rec_words = (int)rec.words;
    if (!decim_tile_plan(s, n, rec.words, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    if (const char *e = exp_env("LDPC_MS_GRID_MAX")) d->tile.grid_max = std::max(1, std::atoi(e));   // (experiments build: tests cap the grid)
    using ldpc_detail::upload;
    bool ok = upload(&d->row_ptr, g.row_ptr) && upload(&d->csr_col, g.csr_col) && upload(&d->rec_off, rec.rec_off) &&
              upload(&d->col_ptr, g.col_ptr) && upload(&d->edge_rec, rec.edge_rec) && upload(&d->edge_pos, rec.edge_pos) &&
              upload(&d->prior, std::vector<float>(channel_llr, channel_llr + n)) && d->tile.calls.create() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
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
    if (d->round_iters == 0) {   // no iteration runs: zeros, converged = 0, llr = 0
        if (d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_err, 0, (size_t)batch * d->n, stream));
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_llr && d->n > 0) LDPC_HIP_TRY(hipMemsetAsync(d_llr, 0, (size_t)batch * d->n * sizeof(double), stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        if (d_decimated) LDPC_HIP_TRY(hipMemsetAsync(d_decimated, 0, (size_t)batch * sizeof(int32_t), stream));
    } else {
        const decim_kernel_t k = decim_kernel_of(d->plan.tier);
        const int threads = ldpc_detail::tile_threads(d->plan.tier);
        int64_t grid;
        size_t lds;
        st = ldpc_detail::tile_geometry(&d->tile, &d->kernel, (const void *)k, threads, d->plan, batch,
                                        "decimation workspace regrow (device synchronise before the free)", &grid, &lds);
        if (st != LDPC_OK) return st;
        DecimParams p{};
        p.s = (int)d->s; p.n = (int)d->n; p.round_iters = d->round_iters; p.max_dec = d->max_dec;
        p.total_iters = d->round_iters * (d->max_dec + 1);   // (create: fits int32)
        p.S = d->plan.S; p.shift = d->plan.shift;
        p.batch = batch; p.alpha = d->alpha; p.clip = d->clip; p.pin = d->pin;
        p.syn = d_syn; p.err = d_err; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.decimated = d_decimated;
        p.prior = d->prior;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.rec_off = d->rec_off;
        p.col_ptr = d->col_ptr; p.edge_rec = d->edge_rec; p.edge_pos = d->edge_pos; p.rec_words = d->rec_words;
        p.ws = d->tile.ws; p.slot_bytes = (long long)d->plan.state_bytes;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
        d->tile.last_grid = (int)grid;
    }
    return d->tile.calls.leave(stream);
}

ldpc_status ldpc_decim_decode_batch(ldpc_decim_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *err, uint8_t *conv,
                                    double *llr, int32_t *iters, int32_t *decimated)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if ((d->s > 0 && !syn) || (d->n > 0 && !err) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
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
