// tile_host.hpp -- the host scaffolding that the decoders of the min-sum family share (ldpc_minsum.hip, ldpc_relay.hip,
// ldpc_decim.hip, ldpc_pauli.hip, ldpc_pauli_relay.hip) on top of host_common.hpp: a syndrome in a lane, tiles of S <= 64
// syndromes on a persistent grid, the state of a tile in LDS (tier 1) or in a workspace slot (tier 2; the plan:
// tile_plan.hpp).  Here, once each: the constants of the design, the validation of the common options, the size limits and
// the end of a create, the Tanner graph and check records of a handle (TileGraph), the rest of what every launch needs
// (TileHost), the check of an entry's arguments (tile_check_batch), the geometry of a launch (tile_geometry, the one place
// the grid rule lives), the launch itself (tile_run, the one hipLaunchKernelGGL of the family) and its twin for a handle
// on which no iteration runs (tile_zero), the host-pointer form of an entry (staged_call), destroy and the body of the
// ldpc_debug_*tile_plan entries.  A decoder keeps its own Params struct, the choice of its kernel and the fields of its
// own.  What the two relay decoders share on top: relay_host.hpp.  The one environment variable read here, in the
// experiments build only: LDPC_MS_GRID_MAX (tile_grid_max_env).
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>

#include "host_common.hpp"
#include "host_env.hpp"
#include "tile_plan.hpp"

namespace ldpc_detail {

constexpr int kTileLdsWaves = 8, kTileGlobalWaves = 16;   // (16 waves: 2.2x the speed of 4 at n = 16384, the sweeps are latency-bound)
constexpr size_t kTileWorkspaceCap = (size_t)6 << 30;     // the unlimited tier's grid shrinks to keep its slots below this
constexpr float kTileAlphaDefault = 0.75f, kTileClipDefault = 1.0e6f;

inline int tile_threads(int tier) { return (tier == 2 ? kTileGlobalWaves : kTileLdsWaves) * 64; }

// alpha, clip, kernel_variant and device of a create's options struct (NULL or zeroed fields: the defaults)
template <class Options>
inline ldpc_status tile_options(const Options *options, float *alpha, float *clip, int *variant, int *device)
{
    *alpha = options && options->alpha != 0.0f ? options->alpha : kTileAlphaDefault;
    *clip = options && options->clip != 0.0f ? options->clip : kTileClipDefault;
    *variant = options ? options->kernel_variant : 0;
    *device = options ? options->device : -1;
    if (!(*alpha > 0.0f && *alpha <= 1.0f)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "alpha must lie in (0, 1]");
    if (!(*clip > 0.0f) || std::isinf(*clip)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "clip must be finite and > 0");
    if (*variant < 0 || *variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    return LDPC_OK;
}

struct TileKernel {   // per kernel function: what its first launch asks the runtime
    bool ready = false;
    int per_cu = 1;
};

// The device arrays of a handle's Tanner graph and check records, the same in every Params struct of the family.  build()
// keeps the host vectors (the layer planner and *_tile_plan() read them) until upload() has sent them.
struct TileGraph {
    int *row_ptr = nullptr, *csr_col = nullptr, *rec_off = nullptr, *col_ptr = nullptr, *edge_rec = nullptr, *edge_pos = nullptr;
    int *col_mid = nullptr;        // the Pauli decoders: where a qubit's Hz edges begin; NULL otherwise
    int rec_words = 0;
    TannerGraph host;              // CSR (checks -> bits, ascending) next to the caller's CSC
    ldpc::MsRecords rec;           // a record per check; per CSC edge its record and position; words <= 4 s + nnz < 2^31
    std::vector<int> host_mid;
    void build(int64_t s, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval, std::vector<int> mid = {})
    {
        host = tanner_graph(s, n, nnz, colptr, rowval);
        rec = ldpc::ms_records(s, nnz, host.row_ptr.data(), host.csc_row.data(), host.csc2csr.data());
        rec_words = (int)rec.words;
        host_mid = std::move(mid);
    }
    bool upload()   // false on the first failure
    {
        const bool ok = ldpc_detail::upload(&row_ptr, host.row_ptr) && ldpc_detail::upload(&csr_col, host.csr_col) &&
                        ldpc_detail::upload(&rec_off, rec.rec_off) && ldpc_detail::upload(&col_ptr, host.col_ptr) &&
                        (host_mid.empty() || ldpc_detail::upload(&col_mid, host_mid)) && ldpc_detail::upload(&edge_rec, rec.edge_rec) &&
                        ldpc_detail::upload(&edge_pos, rec.edge_pos);
        host = TannerGraph();
        rec = ldpc::MsRecords();
        host_mid = std::vector<int>();
        return ok;
    }
};

template <class P, class = void> struct has_col_mid : std::false_type {};
template <class P> struct has_col_mid<P, std::void_t<decltype(std::declval<P &>().col_mid)>> : std::true_type {};

struct TileHost {
    int device = 0, num_cus = 0;
    TileGraph graph;
    unsigned char *ws = nullptr;   // tier 2: [grid][slot]
    size_t ws_cap = 0;
    void *stage = nullptr;         // device staging for the host-pointer entries
    size_t stage_cap = 0;
    int grid_max = 0;              // workgroups a launch takes at most; 0 = no cap (the experiments build's tests set one)
    int last_grid = 0;             // workgroups of the most recent launch
    CallOrder calls;               // calls on a handle run in call order whatever streams they are given (they share the workspace)
    // a handle's destructor: its own device arrays, then what is held here
    void release(std::initializer_list<void *> own)
    {
        if (device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        for (void *q : own)
            if (q) (void)hipFree(q);
        for (void *q : {(void *)graph.row_ptr, (void *)graph.csr_col, (void *)graph.rec_off, (void *)graph.col_ptr, (void *)graph.col_mid,
                        (void *)graph.edge_rec, (void *)graph.edge_pos, stage, (void *)ws})
            if (q) (void)hipFree(q);
        calls.destroy();
    }
    // the fields every Params struct of the family spells the same (after tile_geometry: the workspace may have been regrown)
    template <class P> void fill(P &p, const ldpc::TilePlan &plan, int64_t batch) const
    {
        p.S = plan.S; p.shift = plan.shift; p.batch = batch;
        p.row_ptr = graph.row_ptr; p.csr_col = graph.csr_col; p.rec_off = graph.rec_off;
        p.col_ptr = graph.col_ptr; p.edge_rec = graph.edge_rec; p.edge_pos = graph.edge_pos; p.rec_words = graph.rec_words;
        if constexpr (has_col_mid<P>::value) p.col_mid = graph.col_mid;
        p.ws = ws; p.slot_bytes = (long long)plan.state_bytes;
    }
};

// ---- the end of a create ----------------------------------------------------------------------------------------------------
// what the kernels of `family` index in 32 bits: edges and checks, and bits where nothing smaller bounds n
inline ldpc_status tile_index_limits(const char *family, int64_t s, int64_t n, int64_t nnz, bool bound_n)
{
    if (nnz >= ((int64_t)1 << 28) || s >= ((int64_t)1 << 28) || (bound_n && n >= ((int64_t)1 << 28)))
        return set_error(LDPC_ERR_UNSUPPORTED, std::string(family) + " kernels: graph too large for 32-bit edge indexing");
    return LDPC_OK;
}

// (experiments build: tests cap the grid.  Internal linkage: the two builds share objects that never call it)
static inline void tile_grid_max_env(TileHost *h)
{
    if (const char *e = ldpc::exp_env("LDPC_MS_GRID_MAX")) h->grid_max = std::max(1, std::atoi(e));
}

// the graph, then the handle's own arrays (upload_own), then the call order; a failure frees the handle
template <class Handle, class Own> inline ldpc_status tile_create_finish(Handle *d, Handle **out, Own upload_own)
{
    if (!(d->tile.graph.upload() && upload_own() && d->tile.calls.create() == hipSuccess)) {
        (void)hipGetLastError();
        delete d;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the Tanner graph failed");
    }
    *out = d;
    return LDPC_OK;
}

// ---- an entry ---------------------------------------------------------------------------------------------------------------
// One pointer of an entry: required where the handle's dimension `dim` is > 0, always where `dim` is null.
template <class Handle> struct BatchPointer {
    const void *p;
    int64_t Handle::*dim;
};
// What every entry, device or host form, checks before any device work; batch == 0 is the caller's to answer.
template <class Handle> inline ldpc_status tile_check_batch(const Handle *d, int64_t batch, std::initializer_list<BatchPointer<Handle>> pointers)
{
    if (!d) return set_error(LDPC_ERR_INVALID_ARGUMENT, "decoder is NULL");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    if (batch == 0) return LDPC_OK;
    for (const BatchPointer<Handle> &q : pointers)
        if (!q.p && (!q.dim || d->*q.dim > 0)) return set_error(LDPC_ERR_INVALID_ARGUMENT, "NULL batch pointer");
    if (batch > ((int64_t)1 << 40)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call");
    return LDPC_OK;
}

// The geometry of one launch of `kernel` (`threads` a workgroup) over `batch` syndromes under `plan`: the workgroups of the
// persistent grid -- a tile each, at most what the device holds at once, at most grid_max, and in tier 2 at most the slots
// that fit kTileWorkspaceCap (at least one), with the workspace grown to them -- and the dynamic LDS.
inline ldpc_status tile_geometry(TileHost *h, TileKernel *k, const void *kernel, int threads, const ldpc::TilePlan &plan, int64_t batch,
                                 const char *ws_what, int64_t *grid_out, size_t *lds_out)
{
    const bool global = plan.tier == 2;
    const size_t state = plan.state_bytes, lds = global ? 0 : state;
    if (!k->ready) {
        // (the limit belongs to the kernel, not to the handle: every handle asks for the tier's maximum, so none lowers another's)
        if (lds) LDPC_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldpc::kTileLdsOne));
        k->per_cu = blocks_per_cu(kernel, threads, lds);
        k->ready = true;
    }
    const int64_t tiles = (batch + plan.S - 1) >> plan.shift;
    int64_t grid = std::min<int64_t>(tiles, (int64_t)k->per_cu * h->num_cus);
    if (h->grid_max > 0) grid = std::min<int64_t>(grid, h->grid_max);
    if (global) {
        grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(kTileWorkspaceCap / state)));
        const ldpc_status st = grow_device_buffer((void **)&h->ws, &h->ws_cap, (size_t)grid * state, h->device, ws_what);
        if (st != LDPC_OK) return st;
    }
    *grid_out = grid;
    *lds_out = lds;
    return LDPC_OK;
}

// How every device entry begins: the handle's device, not stalled, after the handle's earlier calls.
inline ldpc_status tile_enter(TileHost *h, hipStream_t stream)
{
    LDPC_HIP_TRY(hipSetDevice(h->device));
    if (device_stalled(h->device)) return stalled_error(h->device);
    return h->calls.enter(stream);
}

// One decode of `batch` > 0 syndromes on `stream`: `kernel` under `plan`, its Params zeroed and filled by fill(p) once the
// geometry stands.  (A HIP error between enter and leave returns without the leave, as it always has.)
template <class Params, class Fill>
inline ldpc_status tile_run(TileHost *h, TileKernel *k, void (*kernel)(Params), const ldpc::TilePlan &plan, int64_t batch, hipStream_t stream,
                            const char *ws_what, Fill fill)
{
    ldpc_status st = tile_enter(h, stream);
    if (st != LDPC_OK) return st;
    const int threads = tile_threads(plan.tier);
    int64_t grid;
    size_t lds;
    if ((st = tile_geometry(h, k, (const void *)kernel, threads, plan, batch, ws_what, &grid, &lds)) != LDPC_OK) return st;
    Params p{};
    fill(p);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, p);
    LDPC_HIP_TRY(hipGetLastError());
    h->last_grid = (int)grid;
    return h->calls.leave(stream);
}

// ... and of a handle on which no iteration runs: every output zero (converged = 0, llr = 0), absent ones skipped.
struct ZeroRegion {
    void *p;
    size_t bytes;
};
inline ldpc_status tile_zero(TileHost *h, hipStream_t stream, std::initializer_list<ZeroRegion> outputs)
{
    const ldpc_status st = tile_enter(h, stream);
    if (st != LDPC_OK) return st;
    for (const ZeroRegion &r : outputs)
        if (r.p && r.bytes > 0) LDPC_HIP_TRY(hipMemsetAsync(r.p, 0, r.bytes, stream));
    return h->calls.leave(stream);
}

// One region of a host-pointer entry's staging image: `bytes` on the device, copied from `in` before the decode or to
// `out` after it.  Both NULL: the region is carved and nothing is copied.
struct StageRegion {
    const void *in;
    void *out;
    size_t bytes;
    size_t at = 0;   // its offset in the image, set by staged_call
};

// The host form of an entry: the regions carved in their order, each on a 256-byte boundary, into the handle's staging
// buffer, the copies in, decode(image) -- the device entry on the null stream -- the copies out, the bounded wait.
template <size_t N, class Decode>
inline ldpc_status staged_call(TileHost *h, StageRegion (&regions)[N], const char *regrow_what, const char *wait_what, Decode decode)
{
    LDPC_HIP_TRY(hipSetDevice(h->device));
    Carve image;
    for (StageRegion &r : regions) r.at = image.take(r.bytes);
    ldpc_status st = grow_device_buffer(&h->stage, &h->stage_cap, image.at, h->device, regrow_what);
    if (st != LDPC_OK) return st;
    char *dp = (char *)h->stage;
    for (const StageRegion &r : regions)
        if (r.in && r.bytes > 0) LDPC_HIP_TRY(hipMemcpyAsync(dp + r.at, r.in, r.bytes, hipMemcpyHostToDevice, nullptr));
    if ((st = decode(dp)) != LDPC_OK) return st;
    for (const StageRegion &r : regions)
        if (r.out && r.bytes > 0) LDPC_HIP_TRY(hipMemcpyAsync(r.out, dp + r.at, r.bytes, hipMemcpyDeviceToHost, nullptr));
    return wait_stream(nullptr, h->device, wait_what);
}

// *_destroy: everything the device still runs for the handle ends first (bounded: `what` names that wait)
template <class Handle> inline ldpc_status tile_destroy(Handle *d, const char *what)
{
    if (!d) return LDPC_OK;
    (void)hipSetDevice(d->tile.device);
    const ldpc_status st = wait_device(d->tile.device, what);
    delete d;
    return st;
}

// The ldpc_debug_*tile_plan entries: their arguments, within what the create accepts (`indexed`: the words of a syndrome's
// state that the kernels index in 32 bits) ...
inline ldpc_status tile_debug_args(int64_t s, int64_t n, int64_t rec_words, int64_t indexed, int kernel_variant)
{
    if (s < 0 || n < 0 || rec_words < 0 || s >= ((int64_t)1 << 28) || n >= ((int64_t)1 << 28) || indexed >= ((int64_t)1 << 31))
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "s, n and rec_words must be >= 0 and within what create accepts");
    if (kernel_variant < 0 || kernel_variant > 2) return set_error(LDPC_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 or 2");
    return LDPC_OK;
}
// ... and their answer: `fits` and `plan` from the planner, `no_fit` the create's text where it refuses
inline ldpc_status tile_debug_answer(bool fits, const ldpc::TilePlan &plan, const char *no_fit, int32_t *tier, int32_t *tile_syndromes,
                                     int64_t *state_bytes)
{
    if (!fits) return set_error(LDPC_ERR_UNSUPPORTED, no_fit);
    if (tier) *tier = plan.tier;
    if (tile_syndromes) *tile_syndromes = plan.S;
    if (state_bytes) *state_bytes = (int64_t)plan.state_bytes;
    return LDPC_OK;
}

}  // namespace ldpc_detail
