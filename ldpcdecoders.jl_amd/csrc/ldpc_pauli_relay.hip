// ldpc_pauli_relay.hip -- host side of the Pauli relay min-sum decoder (the joint X/Z min-sum of a CSS code, run with
// per-qubit memory strengths as a chain of legs, the lightest of the first solutions returned): the ldpc_pauli_relay_* entry
// points of include/ldpc_mi355x_pauli_relay.h (the rule is stated in include/ldpc_mi355x.h).  Device code:
// pauli_relay_kernels.hpp.  The checks of both sides are one Tanner graph -- Hx rows first, then Hz rows -- as in
// ldpc_pauli.hip.  The tiers (ldpc_pauli_relay_kernel) and the tile width: pauli_relay_tile_plan() of tile_plan.hpp.
// Shared with the rest of the min-sum family (tile_host.hpp): the graph of a handle (with col_mid), the check of an entry's
// arguments, the launch (tile_run) and its geometry, the staging of the host-pointer entry, the end of a create; with
// ldpc_relay.hip (relay_host.hpp): the checks of the legs, the legs that run -- legs of 0 iterations are dropped, so the
// kernel sees none --, the weight of a prior.  Here: the two sides made one graph, the order of the create's checks,
// PauliRelayParams and the table of the legs.  No CPU path.
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

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
#include "relay_host.hpp"
using ldpc_detail::set_error;

struct ldpc_pauli_relay_decoder {
    int64_t rx = 0, rz = 0, n = 0;
    int legs = 0, stop_after = 1;   // legs: those that run
    float alpha = 0.0f, clip = 0.0f;
    TilePlan plan;
    int *leg_iters = nullptr;
    float *priors = nullptr;       // [3][n]: prior_x, prior_y, prior_z
    float *tab = nullptr;          // [legs][4][n]: gammas, g0X, g0Y, g0Z
    long long *weight = nullptr;   // [3][n]: qX, qY, qZ
    ldpc_detail::TileHost tile;    // the graph (with col_mid) and what a launch needs (grid_max: LDPC_MS_GRID_MAX of the experiments build)
    ldpc_detail::TileKernel kernel;
    ~ldpc_pauli_relay_decoder() { tile.release({leg_iters, priors, tab, weight}); }
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
    typedef ldpc_pauli_relay_decoder D;
    return ldpc_detail::tile_check_batch(d, batch, {{sx, nullptr}, {sz, nullptr}, {gx, &D::n}, {gz, &D::n}, {conv, nullptr}});
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
    float alpha, clip;
    int variant, device, stop_after;
    const float *const tables[3] = {prior_x, prior_y, prior_z};
    const char *const names[3] = {"prior_x", "prior_y", "prior_z"};
    st = ldpc_detail::relay_check_legs(n, legs, gammas, leg_iters, options, &alpha, &clip, &variant, &device, &stop_after, [&] {
        for (int k = 0; k < 3; ++k) {
            if (n > 0 && !tables[k]) return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + " is NULL");
            for (int64_t j = 0; j < n; ++j)
                if (!std::isfinite(tables[k][j]))
                    return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + "[" + std::to_string(j) + "] is not finite");
        }
        return LDPC_OK;
    });
    if (st != LDPC_OK) return st;
    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;
    const int64_t rx = hx->rows, rz = hz->rows, s = rx + rz, nnz = hx->nnz + hz->nnz;
    if ((st = ldpc_detail::relay_index_limits("Pauli relay", s, n, nnz)) != LDPC_OK) return st;

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
    // what the rule derives once per handle, for the legs that run: g0W = (1 - gamma) * prior_W; qW = relay_weight(prior_W)
    std::vector<float> h_tab;
    const std::vector<int> h_iters = ldpc_detail::relay_running_legs(legs, leg_iters, [&](int64_t r) {
        for (int64_t j = 0; j < n; ++j) h_tab.push_back(gammas[r * n + j]);
        for (int k = 0; k < 3; ++k)
            for (int64_t j = 0; j < n; ++j) {
                const float one_minus = 1.0f - gammas[r * n + j];
                h_tab.push_back(one_minus * tables[k][j]);
            }
    });
    d->legs = (int)h_iters.size();
    std::vector<long long> h_weight((size_t)(3 * n), 0);
    std::vector<float> h_priors((size_t)(3 * n), 0.0f);
    for (int k = 0; k < 3; ++k)
        for (int64_t j = 0; j < n; ++j) {
            h_priors[(size_t)(k * n + j)] = tables[k][j];
            h_weight[(size_t)(k * n + j)] = ldpc_detail::relay_weight(tables[k][j]);
        }
    d->tile.graph.build(s, n, nnz, colptr.data(), rowval.data(), std::move(col_mid));
    const int64_t words = d->tile.graph.rec.words;
    if (6 * n + words + 2 * ((n + 31) >> 5) >= ((int64_t)1 << 31)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "Pauli relay kernels: the state of one syndrome is too large for 32-bit word indexing");
    }
    if (!pauli_relay_tile_plan(s, n, words, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    ldpc_detail::tile_grid_max_env(&d->tile);
    using ldpc_detail::upload;
    return ldpc_detail::tile_create_finish(d, out, [&] {
        return upload(&d->leg_iters, h_iters) && upload(&d->priors, h_priors) && upload(&d->tab, h_tab) && upload(&d->weight, h_weight);
    });
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
    const ldpc_status st = pauli_relay_check_batch(d, batch, d_sx, d_sz, d_gx, d_gz, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t B = (size_t)batch, n = (size_t)d->n;
    if (d->legs == 0)   // no iteration runs
        return ldpc_detail::tile_zero(&d->tile, (hipStream_t)stream_v, {{d_gx, B * n}, {d_gz, B * n}, {d_llr, B * 3 * n * sizeof(double)},
                                                                         {d_conv, B}, {d_iters, B * 4}, {d_solutions, B * 4}});
    return ldpc_detail::tile_run(&d->tile, &d->kernel, pauli_relay_kernel_of(d->plan.tier), d->plan, batch, (hipStream_t)stream_v,
                                 "Pauli relay workspace regrow (device synchronise before the free)", [&](PauliRelayParams &p) {
                                     d->tile.fill(p, d->plan, batch);
                                     p.rx = (int)d->rx; p.s = (int)(d->rx + d->rz); p.n = (int)d->n; p.legs = d->legs; p.stop_after = d->stop_after;
                                     p.alpha = d->alpha; p.clip = d->clip;
                                     p.sx = d_sx; p.sz = d_sz; p.gx = d_gx; p.gz = d_gz; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters; p.solutions = d_solutions;
                                     p.prior = d->priors; p.tab = d->tab; p.leg_iters = d->leg_iters; p.weight = d->weight;
                                 });
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
