// ldpc_pauli_relay.hip -- host side of the Pauli relay min-sum decoder (the joint X/Z min-sum of a CSS code, run with
// per-qubit memory strengths as a chain of legs, the lightest of the first solutions returned): the ldpc_pauli_relay_* entry
// points of include/ldpc_mi355x_pauli_relay.h (the rule is stated in include/ldpc_mi355x.h).  Device code:
// pauli_relay_kernels.hpp.  The checks of both sides are one Tanner graph -- Hx rows first, then Hz rows -- as in
// ldpc_pauli.hip.  The tiers (ldpc_pauli_relay_kernel) and the tile width: pauli_relay_tile_plan() of tile_plan.hpp; the
// launch geometry and the rest of what the min-sum family shares on the host: tile_host.hpp.  Legs of 0 iterations are
// dropped here, so the kernel sees only legs that run.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "../../include/ldpc_mi355x_debug.h"
#include "pauli_relay_kernels.hpp"

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

static constexpr int64_t kPrMaxBits = (int64_t)1 << 22;      // a weight is a sum of at most 2^22 terms below 2^41

struct ldpc_pauli_relay_decoder {
    int64_t rx = 0, rz = 0, n = 0;
    int legs = 0, stop_after = 1;   // legs: those that run
    float alpha = 0.0f, clip = 0.0f;
    int rec_words = 0;
    TilePlan plan;
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *col_mid = nullptr, *edge_rec = nullptr,
        *edge_pos = nullptr;
    int *leg_iters = nullptr;
    float *priors = nullptr;       // [3][n]: prior_x, prior_y, prior_z
    float *tab = nullptr;          // [legs][4][n]: gammas, g0X, g0Y, g0Z
    long long *weight = nullptr;   // [3][n]: qX, qY, qZ
    ldpc_detail::TileHost tile;    // (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernel;
    ~ldpc_pauli_relay_decoder() { tile.release({row_ptr, csr_col, rec_off, col_ptr, col_mid, edge_rec, edge_pos, leg_iters, priors, tab, weight}); }
};

typedef void (*pauli_relay_kernel_t)(PauliRelayParams);
static pauli_relay_kernel_t pauli_relay_kernel_of(int tier)
{
    return tier == 1 ? pauli_relay_kernel<ldpc_detail::kTileLdsWaves, false> : pauli_relay_kernel<ldpc_detail::kTileGlobalWaves, true>;
}

// One side of a create: the checks ldpc_bp_create makes on a pattern, and at least one row; the message names the side.
static ldpc_status pauli_relay_check_side(const char *name, const ldpc_css_pattern *m, int64_t n)
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
static ldpc_status pauli_relay_check_batch(const ldpc_pauli_relay_decoder *d, int64_t batch, const void *sx, const void *sz,
                                           const void *gx, const void *gz, const void *conv)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    if (!sx || !sz || (d->n > 0 && (!gx || !gz)) || !conv) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    return LDPC_OK;
}

extern "C" {

ldpc_status ldpc_pauli_relay_create(int64_t n, const ldpc_css_pattern *hx, const ldpc_css_pattern *hz, const float *prior_x,
                                    const float *prior_y, const float *prior_z, int64_t legs, const float *gammas,
                                    const int32_t *leg_iters, const ldpc_pauli_relay_options *options, ldpc_pauli_relay_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (n < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative dimension (n)");
    ldpc_status st;
    if ((st = pauli_relay_check_side("hx", hx, n)) != LDPC_OK || (st = pauli_relay_check_side("hz", hz, n)) != LDPC_OK) return st;
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
    const float *const tables[3] = {prior_x, prior_y, prior_z};
    const char *const names[3] = {"prior_x", "prior_y", "prior_z"};
    for (int k = 0; k < 3; ++k) {
        if (n > 0 && !tables[k]) return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + " is NULL");
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(tables[k][j]))
                return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + "[" + std::to_string(j) + "] is not finite");
    }
    for (int64_t r = 0; r < legs; ++r)
        for (int64_t j = 0; j < n; ++j) {
            const float g = gammas[r * n + j];
            if (!(g > -1.0f && g < 1.0f))   // (false for NaN as well)
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "gammas[" + std::to_string(r) + "][" + std::to_string(j) + "] must be finite and lie in (-1, 1)");
        }
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    const int64_t rx = hx->rows, rz = hz->rows, s = rx + rz, nnz = hx->nnz + hz->nnz;
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28))
        return set_error(LDPC_ERR_UNSUPPORTED, "Pauli relay kernels: graph too large for 32-bit edge indexing");
    if (n > kPrMaxBits) return set_error(LDPC_ERR_UNSUPPORTED, "Pauli relay kernels: n > 2^22 (a solution's weight must fit int64)");

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

    ldpc_pauli_relay_decoder *d = new (std::nothrow) ldpc_pauli_relay_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->rx = rx; d->rz = rz; d->n = n; d->alpha = alpha; d->clip = clip; d->stop_after = stop_after;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount;
    // what the rule derives once per handle, for the legs that run: g0W = (1 - gamma) * prior_W; qW = rint(clamp(prior_W) * 2^16)
    std::vector<float> h_tab;
    std::vector<int> h_iters;
    for (int64_t r = 0; r < legs; ++r) {
        if (leg_iters[r] == 0) continue;
        h_iters.push_back(leg_iters[r]);
        for (int64_t j = 0; j < n; ++j) h_tab.push_back(gammas[r * n + j]);
        for (int k = 0; k < 3; ++k)
            for (int64_t j = 0; j < n; ++j) {
                const float one_minus = 1.0f - gammas[r * n + j];
                h_tab.push_back(one_minus * tables[k][j]);
            }
    }
    d->legs = (int)h_iters.size();
    std::vector<long long> h_weight((size_t)(3 * n), 0);
    std::vector<float> h_priors((size_t)(3 * n), 0.0f);
    for (int k = 0; k < 3; ++k)
        for (int64_t j = 0; j < n; ++j) {
            h_priors[(size_t)(k * n + j)] = tables[k][j];
            h_weight[(size_t)(k * n + j)] = (long long)std::rint(std::min(std::max((double)tables[k][j], -16777216.0), 16777216.0) * 65536.0);
        }
    const ldpc_detail::TannerGraph g = ldpc_detail::tanner_graph(s, n, nnz, colptr.data(), rowval.data());
    const MsRecords rec = ms_records(s, nnz, g.row_ptr.data(), g.csc_row.data(), g.csc2csr.data());   // words <= 4 s + nnz < 2^31
    if (6 * n + rec.words + 2 * ((n + 31) >> 5) >= ((int64_t)1 << 31)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "Pauli relay kernels: the state of one syndrome is too large for 32-bit word indexing");
    }
    d->rec_words = (int)rec.words;
    if (!pauli_relay_tile_plan(s, n, rec.words, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    if (const char *e = exp_env("LDPC_MS_GRID_MAX")) d->tile.grid_max = std::max(1, std::atoi(e));   // (experiments build: tests cap the grid)
    using ldpc_detail::upload;
    bool ok = upload(&d->row_ptr, g.row_ptr) && upload(&d->csr_col, g.csr_col) && upload(&d->rec_off, rec.rec_off) &&
              upload(&d->col_ptr, g.col_ptr) && upload(&d->col_mid, col_mid) && upload(&d->edge_rec, rec.edge_rec) &&
              upload(&d->edge_pos, rec.edge_pos) && upload(&d->leg_iters, h_iters) && upload(&d->priors, h_priors) &&
              upload(&d->tab, h_tab) && upload(&d->weight, h_weight) && d->tile.calls.create() == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

// (include/ldpc_mi355x_pauli_relay_debug.h) the choice create makes, without a device
ldpc_status ldpc_debug_pauli_relay_tile_plan(int64_t s, int64_t n, int64_t rec_words, int32_t kernel_variant, int32_t *tier,
                                             int32_t *tile_syndromes, int64_t *state_bytes)
{
    // (G, M, the records and best are indexed in words)
    const int64_t indexed = n >= 0 && n < ((int64_t)1 << 28) ? 6 * n + rec_words + 2 * ((n + 31) >> 5) : 0;
    const ldpc_status st = ldpc_detail::tile_debug_args(s, n, rec_words, indexed, kernel_variant);
    if (st != LDPC_OK) return st;
    TilePlan plan;
    return ldpc_detail::tile_debug_answer(pauli_relay_tile_plan(s, n, rec_words, kernel_variant, &plan), plan,
                                          "kernel_variant 1: the state of one syndrome does not fit the on-chip tier", tier, tile_syndromes, state_bytes);
}

int32_t ldpc_pauli_relay_kernel(const ldpc_pauli_relay_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_pauli_relay_tile_syndromes(const ldpc_pauli_relay_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_pauli_relay_last_grid(const ldpc_pauli_relay_decoder *d) { return d ? d->tile.last_grid : 0; }

ldpc_status ldpc_pauli_relay_destroy(ldpc_pauli_relay_decoder *d)
{
    return ldpc_detail::tile_destroy(d, "ldpc_pauli_relay_destroy (device synchronise)");
}

ldpc_status ldpc_pauli_relay_decode_batch_device(ldpc_pauli_relay_decoder *d, int64_t batch, const uint8_t *d_sx, const uint8_t *d_sz,
                                                 uint8_t *d_gx, uint8_t *d_gz, uint8_t *d_conv, double *d_llr, int32_t *d_iters,
                                                 int32_t *d_solutions, void *stream_v)
{
    ldpc_status st = pauli_relay_check_batch(d, batch, d_sx, d_sz, d_gx, d_gz, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    hipStream_t stream = (hipStream_t)stream_v;
    LDPC_HIP_TRY(hipSetDevice(d->tile.device));
    if (ldpc_detail::device_stalled(d->tile.device)) return ldpc_detail::stalled_error(d->tile.device);
    if ((st = d->tile.calls.enter(stream)) != LDPC_OK) return st;
    if (d->legs == 0) {   // no iteration runs: zeros, converged = 0, llr = 0
        if (d->n > 0) {
            LDPC_HIP_TRY(hipMemsetAsync(d_gx, 0, (size_t)batch * d->n, stream));
            LDPC_HIP_TRY(hipMemsetAsync(d_gz, 0, (size_t)batch * d->n, stream));
            if (d_llr) LDPC_HIP_TRY(hipMemsetAsync(d_llr, 0, (size_t)batch * 3 * d->n * sizeof(double), stream));
        }
        LDPC_HIP_TRY(hipMemsetAsync(d_conv, 0, (size_t)batch, stream));
        if (d_iters) LDPC_HIP_TRY(hipMemsetAsync(d_iters, 0, (size_t)batch * sizeof(int32_t), stream));
        if (d_solutions) LDPC_HIP_TRY(hipMemsetAsync(d_solutions, 0, (size_t)batch * sizeof(int32_t), stream));
    } else {
        const pauli_relay_kernel_t k = pauli_relay_kernel_of(d->plan.tier);
        const int threads = ldpc_detail::tile_threads(d->plan.tier);
        int64_t grid;
        size_t lds;
        st = ldpc_detail::tile_geometry(&d->tile, &d->kernel, (const void *)k, threads, d->plan, batch,
                                        "Pauli relay workspace regrow (device synchronise before the free)", &grid, &lds);
        if (st != LDPC_OK) return st;
        PauliRelayParams p{};
        p.rx = (int)d->rx; p.s = (int)(d->rx + d->rz); p.n = (int)d->n; p.legs = d->legs; p.stop_after = d->stop_after;
        p.S = d->plan.S; p.shift = d->plan.shift;
        p.batch = batch; p.alpha = d->alpha; p.clip = d->clip;
        p.sx = d_sx; p.sz = d_sz; p.gx = d_gx; p.gz = d_gz; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.solutions = d_solutions;
        p.prior = d->priors; p.tab = d->tab; p.leg_iters = d->leg_iters; p.weight = d->weight;
        p.row_ptr = d->row_ptr; p.csr_col = d->csr_col; p.rec_off = d->rec_off; p.col_ptr = d->col_ptr; p.col_mid = d->col_mid;
        p.edge_rec = d->edge_rec; p.edge_pos = d->edge_pos; p.rec_words = d->rec_words;
        p.ws = d->tile.ws; p.slot_bytes = (long long)d->plan.state_bytes;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
        LDPC_HIP_TRY(hipGetLastError());
        d->tile.last_grid = (int)grid;
    }
    return d->tile.calls.leave(stream);
}

ldpc_status ldpc_pauli_relay_decode_batch(ldpc_pauli_relay_decoder *d, int64_t batch, const uint8_t *sx, const uint8_t *sz, uint8_t *gx,
                                          uint8_t *gz, uint8_t *conv, double *llr, int32_t *iters, int32_t *solutions)
{
    ldpc_status st = pauli_relay_check_batch(d, batch, sx, sz, gx, gz, conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t rx = (size_t)d->rx, rz = (size_t)d->rz, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::StageRegion r[] = {{sx, nullptr, B * rx},   {sz, nullptr, B * rz},       {nullptr, gx, B * n},
                                    {nullptr, gz, B * n},    {nullptr, conv, B},          {nullptr, iters, B * 4},
                                    {nullptr, solutions, B * 4}, {nullptr, llr, llr ? B * 3 * n * sizeof(double) : 0}};
    return ldpc_detail::staged_call(&d->tile, r, "Pauli relay staging regrow (device synchronise before the free)",
                                    "ldpc_pauli_relay_decode_batch (stream synchronise)", [&](char *dp) {
                                        return ldpc_pauli_relay_decode_batch_device(
                                            d, batch, (const uint8_t *)dp, (const uint8_t *)(dp + r[1].at), (uint8_t *)(dp + r[2].at),
                                            (uint8_t *)(dp + r[3].at), (uint8_t *)(dp + r[4].at), llr ? (double *)(dp + r[7].at) : nullptr,
                                            (int32_t *)(dp + r[5].at), (int32_t *)(dp + r[6].at), nullptr);
                                    });
}

}  // extern "C"
