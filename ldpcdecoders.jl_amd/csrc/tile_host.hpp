// tile_host.hpp -- the host scaffolding that the decoders of the min-sum family share (ldpc_minsum.hip, ldpc_relay.hip,
// ldpc_pauli.hip, ldpc_decim.hip) on top of host_common.hpp: a syndrome in a lane, tiles of S <= 64 syndromes on a persistent grid, the
// state of a tile in LDS (tier 1) or in a workspace slot (tier 2; the plan: tile_plan.hpp).  Here, once each: the constants
// of the design, the validation of the common options, the part of a handle that every launch needs (TileHost), the
// geometry of a launch (tile_geometry, the one place the grid rule lives), the host-pointer form of an entry
// (staged_call), destroy and the body of the ldpc_debug_*tile_plan entries.  A decoder keeps its own Params struct and its
// own hipLaunchKernelGGL.  Nothing here reads the environment.
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "host_common.hpp"
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

struct TileHost {
    int device = 0, num_cus = 0;
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
        if (stage) (void)hipFree(stage);
        if (ws) (void)hipFree(ws);
        calls.destroy();
    }
};

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
