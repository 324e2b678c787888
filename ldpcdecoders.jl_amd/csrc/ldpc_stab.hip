// ldpc_stab.hip -- host side of the joint Pauli min-sum decoder of a general (non-CSS) stabilizer code: the
// ldpc_stab_minsum_* entry points of include/ldpc_mi355x_stab.h (the rule is stated there).  Device code: stab_kernels.hpp.
// The two patterns of a create (where the stabilizers have an X part, where a Z part) are merged into ONE Tanner graph
// whose edges carry their Pauli type; the type travels in spare bits of two tables the kernel reads anyway (csr_col,
// edge_pos), so the arrays of the family's TileGraph serve as they are.  The tiers (ldpc_stab_minsum_kernel) and the tile
// width: stab_tile_plan() of tile_plan.hpp.  Shared with the rest of the min-sum family (tile_host.hpp): the graph of a
// handle, the check of an entry's arguments, the launch (tile_run) and its geometry, the staging of the host-pointer entry,
// the end of a create.  Here: the merge, the order of the create's checks and StabParams.  This unit reads no environment
// variable.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "../../include/ldpc_mi355x_debug.h"
#include "stab_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, the create-time scaffolding and (host_wait.hpp) the bounded waits
#include "tile_host.hpp"
using ldpc_detail::set_error;

struct ldpc_stab_minsum_decoder {
    int64_t r = 0, n = 0, max_iters = 0;
    float alpha = 0.0f, clip = 0.0f;
    TilePlan plan;
    float *priors = nullptr;       // [3][n]: prior_x, prior_y, prior_z
    ldpc_detail::TileHost tile;    // the graph and what a launch needs (grid_max stays 0: no cap)
    ldpc_detail::TileKernel kernel;
    ~ldpc_stab_minsum_decoder() { tile.release({priors}); }
};

typedef void (*stab_kernel_t)(StabParams);
static stab_kernel_t stab_kernel_of(int tier)
{
    return tier == 1 ? stab_minsum_kernel<ldpc_detail::kTileLdsWaves, false> : stab_minsum_kernel<ldpc_detail::kTileGlobalWaves, true>;
}

// One pattern of a create: the checks ldpc_bp_create makes on a pattern; the message names the argument.
static ldpc_status stab_check_part(const char *name, const ldpc_css_pattern *m, int64_t n)
{
    const std::string who = std::string(name) + ": ";
    if (!m) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "pattern is NULL");
    ldpc_status st = ldpc_detail::check_csc_args(m->rows, n, m->nnz, m->colptr, m->rowval, 0);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(m->rows, n, m->nnz, m->colptr, m->rowval)) != LDPC_OK)
        return set_error(st, who + ldpc_detail::last_error());
    return LDPC_OK;
}

// what every entry checks before any device work; batch == 0 is the caller's to answer
static ldpc_status stab_check_batch(const ldpc_stab_minsum_decoder *d, int64_t batch, const void *syn, const void *gx, const void *gz,
                                    const void *conv)
{
    typedef ldpc_stab_minsum_decoder D;
    return ldpc_detail::tile_check_batch(d, batch, {{syn, nullptr}, {gx, &D::n}, {gz, &D::n}, {conv, nullptr}});
}

extern "C" {

ldpc_status ldpc_stab_minsum_create(int64_t n, const ldpc_css_pattern *sx_part, const ldpc_css_pattern *sz_part, const float *prior_x,
                                    const float *prior_y, const float *prior_z, int64_t max_iters,
                                    const ldpc_stab_minsum_options *options, ldpc_stab_minsum_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (n < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative dimension (n)");
    if (max_iters < 0 || max_iters > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "max_iters must lie in 0 .. 2^31 - 1");
    ldpc_status st;
    if ((st = stab_check_part("sx_part", sx_part, n)) != LDPC_OK || (st = stab_check_part("sz_part", sz_part, n)) != LDPC_OK) return st;
    if (sx_part->rows != sz_part->rows)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "sx_part and sz_part: the two patterns must have the same number of rows (" +
                                                        std::to_string(sx_part->rows) + " and " + std::to_string(sz_part->rows) + ")");
    if (sx_part->rows < 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, "sx_part and sz_part: a code needs at least one row (r >= 1)");
    float alpha, clip;
    int variant, device;
    if ((st = ldpc_detail::tile_options(options, &alpha, &clip, &variant, &device)) != LDPC_OK) return st;
    const float *const tables[3] = {prior_x, prior_y, prior_z};
    const char *const names[3] = {"prior_x", "prior_y", "prior_z"};
    for (int k = 0; k < 3; ++k) {
        if (n > 0 && !tables[k]) return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + " is NULL");
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(tables[k][j]))
                return set_error(LDPC_ERR_INVALID_ARGUMENT, std::string(names[k]) + "[" + std::to_string(j) + "] is not finite");
    }
    const int64_t r = sx_part->rows;
    if ((st = ldpc_detail::tile_index_limits("Stabilizer min-sum", r, n, std::max(sx_part->nnz, sz_part->nnz), true)) != LDPC_OK) return st;
    // the union of the two patterns, each column a merge of two ascending lists; the type of an edge: bit 0 = sx_part stores
    // it, bit 1 = sz_part does.  (nnz <= the two counts together, each an int64 that check_csc_args has bounded by rows * n.)
    std::vector<int64_t> colptr((size_t)n + 1, 0), rowval;
    std::vector<unsigned char> type;
    rowval.reserve((size_t)std::max<int64_t>(std::max(sx_part->nnz, sz_part->nnz), 1));
    type.reserve(rowval.capacity());
    for (int64_t j = 0; j < n; ++j) {
        colptr[(size_t)j] = (int64_t)rowval.size();
        int64_t a = sx_part->colptr[j], b = sz_part->colptr[j];
        const int64_t ae = sx_part->colptr[j + 1], be = sz_part->colptr[j + 1];
        while (a < ae || b < be) {
            const int64_t ia = a < ae ? sx_part->rowval[a] : r, ib = b < be ? sz_part->rowval[b] : r, i = std::min(ia, ib);
            rowval.push_back(i);
            type.push_back((unsigned char)((ia == i ? 1 : 0) | (ib == i ? 2 : 0)));
            a += ia == i;
            b += ib == i;
        }
    }
    const int64_t nnz = (int64_t)rowval.size();
    colptr[(size_t)n] = nnz;
    if (rowval.empty()) rowval.push_back(0);
    if ((st = ldpc_detail::tile_index_limits("Stabilizer min-sum", r, n, nnz, true)) != LDPC_OK) return st;   // (the union's edges)

    hipDeviceProp_t prop;
    if ((st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)")) != LDPC_OK)
        return st;

    ldpc_stab_minsum_decoder *d = new (std::nothrow) ldpc_stab_minsum_decoder();
    if (!d) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    d->r = r; d->n = n; d->max_iters = max_iters; d->alpha = alpha; d->clip = clip;
    d->tile.device = device; d->tile.num_cus = prop.multiProcessorCount;
    d->tile.graph.build(r, n, nnz, colptr.data(), rowval.data());
    const int64_t words = d->tile.graph.rec.words;
    if (3 * n + words >= ((int64_t)1 << 31)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "Stabilizer min-sum kernels: the state of one syndrome is too large for 32-bit word indexing");
    }
    if (!stab_tile_plan(r, n, words, variant, &d->plan)) {
        delete d;
        return set_error(LDPC_ERR_UNSUPPORTED, "kernel_variant 1: the state of one syndrome does not fit the on-chip tier");
    }
    // the type of every edge into the two tables the sweeps read: per CSR edge next to the qubit, per CSC edge next to the
    // position (both below 2^28: tile_index_limits)
    ldpc_detail::TannerGraph &g = d->tile.graph.host;
    for (int64_t e = 0; e < nnz; ++e) {
        const int ty = (int)type[(size_t)e] << kStabTypeShift;
        g.csr_col[(size_t)g.csc2csr[(size_t)e]] |= ty;
        d->tile.graph.rec.edge_pos[(size_t)e] |= ty;
    }
    std::vector<float> priors((size_t)std::max<int64_t>(3 * n, 1), 0.0f);
    for (int k = 0; k < 3; ++k)
        for (int64_t j = 0; j < n; ++j) priors[(size_t)(k * n + j)] = tables[k][j];
    return ldpc_detail::tile_create_finish(d, out, [&] { return ldpc_detail::upload(&d->priors, priors); });
}

// (include/ldpc_mi355x_stab_debug.h) the choice create makes, without a device
ldpc_status ldpc_debug_stab_tile_plan(int64_t r, int64_t n, int64_t rec_words, int32_t kernel_variant, int32_t *tier,
                                      int32_t *tile_syndromes, int64_t *state_bytes)
{
    const ldpc_status st = ldpc_detail::tile_debug_args(r, n, rec_words, 3 * n + rec_words, kernel_variant);   // (MX, MY, MZ and the records)
    if (st != LDPC_OK) return st;
    TilePlan plan;
    return ldpc_detail::tile_debug_answer(stab_tile_plan(r, n, rec_words, kernel_variant, &plan), plan,
                                          "kernel_variant 1: the state of one syndrome does not fit the on-chip tier", tier, tile_syndromes, state_bytes);
}

int32_t ldpc_stab_minsum_kernel(const ldpc_stab_minsum_decoder *d) { return d ? d->plan.tier : 0; }
int32_t ldpc_stab_minsum_tile_syndromes(const ldpc_stab_minsum_decoder *d) { return d ? d->plan.S : 0; }
int32_t ldpc_stab_minsum_last_grid(const ldpc_stab_minsum_decoder *d) { return d ? d->tile.last_grid : 0; }

ldpc_status ldpc_stab_minsum_destroy(ldpc_stab_minsum_decoder *d)
{
    return ldpc_detail::tile_destroy(d, "ldpc_stab_minsum_destroy (device synchronise)");
}

ldpc_status ldpc_stab_minsum_decode_batch_device(ldpc_stab_minsum_decoder *d, int64_t batch, const uint8_t *d_syn, uint8_t *d_gx,
                                                 uint8_t *d_gz, uint8_t *d_conv, double *d_llr, int32_t *d_iters, void *stream_v)
{
    const ldpc_status st = stab_check_batch(d, batch, d_syn, d_gx, d_gz, d_conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t B = (size_t)batch, n = (size_t)d->n;
    if (d->max_iters == 0)   // no iteration runs
        return ldpc_detail::tile_zero(&d->tile, (hipStream_t)stream_v,
                                      {{d_gx, B * n}, {d_gz, B * n}, {d_llr, B * 3 * n * sizeof(double)}, {d_conv, B}, {d_iters, B * 4}});
    return ldpc_detail::tile_run(&d->tile, &d->kernel, stab_kernel_of(d->plan.tier), d->plan, batch, (hipStream_t)stream_v,
                                 "Stabilizer min-sum workspace regrow (device synchronise before the free)", [&](StabParams &p) {
                                     d->tile.fill(p, d->plan, batch);
                                     p.r = (int)d->r; p.n = (int)d->n; p.max_iters = (int)d->max_iters;
                                     p.alpha = d->alpha; p.clip = d->clip;
                                     p.syn = d_syn; p.gx = d_gx; p.gz = d_gz; p.conv = d_conv; p.llr = d_llr; p.iters = d_iters;
                                     p.prior_x = d->priors; p.prior_y = d->priors + d->n; p.prior_z = d->priors + 2 * d->n;
                                 });
}

ldpc_status ldpc_stab_minsum_decode_batch(ldpc_stab_minsum_decoder *d, int64_t batch, const uint8_t *syn, uint8_t *gx, uint8_t *gz,
                                          uint8_t *conv, double *llr, int32_t *iters)
{
    ldpc_status st = stab_check_batch(d, batch, syn, gx, gz, conv);
    if (st != LDPC_OK || batch == 0) return st;
    const size_t r = (size_t)d->r, n = (size_t)d->n, B = (size_t)batch;
    ldpc_detail::StageRegion rg[] = {{syn, nullptr, B * r},  {nullptr, gx, B * n},       {nullptr, gz, B * n},
                                     {nullptr, conv, B},     {nullptr, iters, B * 4},    {nullptr, llr, llr ? B * 3 * n * sizeof(double) : 0}};
    return ldpc_detail::staged_call(&d->tile, rg, "Stabilizer min-sum staging regrow (device synchronise before the free)",
                                    "ldpc_stab_minsum_decode_batch (stream synchronise)", [&](char *dp) {
                                        return ldpc_stab_minsum_decode_batch_device(
                                            d, batch, (const uint8_t *)dp, (uint8_t *)(dp + rg[1].at), (uint8_t *)(dp + rg[2].at),
                                            (uint8_t *)(dp + rg[3].at), llr ? (double *)(dp + rg[5].at) : nullptr,
                                            (int32_t *)(dp + rg[4].at), nullptr);
                                    });
}

}  // extern "C"
