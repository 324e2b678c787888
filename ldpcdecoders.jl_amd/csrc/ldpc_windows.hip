// ldpc_windows.hip -- host side of the sliding-window step: the ldpc_windows_* entry points of include/ldpc_mi355x.h.
// A create validates the model and the window lists, builds the tables on the host (window_plan.cpp, HIP-free) and
// uploads them as one array of 32-bit indices; a gather or a commit is one launch of window_kernels.hpp's kernel on the
// caller's stream.  Tiers (by the longest guess column of any window): a column's bit image in LDS, or -- beyond the LDS
// budget -- the guess bytes read out of global memory.  No CPU path.
#include "../../include/ldpc_mi355x.h"
#include "window_kernels.hpp"
#include "window_plan.hpp"

#include <algorithm>
#include <new>
#include <string>

using namespace ldpc_windows_k;

#include "host_common.hpp"   // set_error, LDPC_HIP_TRY, select_device, CallOrder and (host_wait.hpp) the bounded waits
using ldpc_detail::set_error;

static constexpr size_t kWindowImageLds = (size_t)159 * 1024;
static constexpr int kWindowWaveColumn = 4096;   // columns of up to this much work take one wave each, four to a workgroup

struct ldpc_windows {
    int64_t D = 0, N = 0, K = 0;
    int device = 0, num_cus = 0, wpc = 1, image_stride = 0;
    bool image = true;
    std::vector<ldpc::WindowTable> win;
    int *ints = nullptr;        // every table, on the device
    int per_cu = 0;             // workgroups a CU holds (0 = not asked yet)
    ldpc_detail::CallOrder calls;
    ~ldpc_windows()
    {
        if (ldpc_detail::device_stalled(device)) return;   // (host_wait.hpp: nothing a stalled device may still use is freed)
        if (ints) (void)hipFree(ints);
        calls.destroy();
    }
};

static auto window_kernel_of(int wpc, bool image) -> void (*)(WindowParams)
{
    static void (*const table[2][2])(WindowParams) = {{window_kernel<1, false>, window_kernel<1, true>},
                                                      {window_kernel<4, false>, window_kernel<4, true>}};
    return table[wpc == 4][image];
}

// One step: the arguments are checked, batch > 0; the caller has filled what belongs to the step.
static ldpc_status window_launch(ldpc_windows *w, WindowParams p, int64_t batch, hipStream_t stream)
{
    if (batch > ((int64_t)1 << 36)) return set_error(LDPC_ERR_UNSUPPORTED, "batch too large for one call (more than 2^36 columns)");
    LDPC_HIP_TRY(hipSetDevice(w->device));
    if (ldpc_detail::device_stalled(w->device)) return ldpc_detail::stalled_error(w->device);
    ldpc_status st = w->calls.enter(stream);
    if (st != LDPC_OK) return st;
    const int cpb = kThreads / (64 * w->wpc);
    const size_t lds = w->image ? (size_t)cpb * w->image_stride * sizeof(unsigned short) : 0;
    const auto k = window_kernel_of(w->wpc, w->image);
    if (!w->per_cu) {
        // always the whole budget, never this handle's own size: the cap belongs to the kernel, not to the handle
        if (lds) LDPC_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWindowImageLds));
        w->per_cu = std::min(8, ldpc_detail::blocks_per_cu((const void *)k, kThreads, lds));
    }
    p.batch = batch; p.image_stride = w->image_stride; p.N = (int)w->N; p.D = (int)w->D;
    const int64_t ngroups = (batch + cpb - 1) / cpb;
    const int64_t grid = std::min<int64_t>(ngroups, (int64_t)w->per_cu * std::max(w->num_cus, 32));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((unsigned)kThreads), lds, stream, p);
    LDPC_HIP_TRY(hipGetLastError());
    return w->calls.leave(stream);
}

static ldpc_status check_window(const ldpc_windows *w, int64_t k, int64_t batch)
{
    if (!w) return set_error(LDPC_ERR_INVALID_ARGUMENT, "windows handle is NULL");
    if (k < 0 || k >= w->K)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, "window " + std::to_string(k) + " is outside [0, " + std::to_string(w->K) + ")");
    if (batch < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative batch");
    return LDPC_OK;
}

extern "C" {

ldpc_status ldpc_windows_create(int64_t D, int64_t N, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                                int64_t K, const int64_t *det_ptr, const int64_t *det_idx,
                                const int64_t *mech_ptr, const int64_t *mech_idx,
                                const int64_t *commit_ptr, const int64_t *commit_idx,
                                const ldpc_windows_options *options, ldpc_windows **out)
{
    if (!out) return set_error(LDPC_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ldpc_status st = ldpc_detail::check_csc_args(D, N, nnz, colptr, rowval, 0);
    if (st != LDPC_OK || (st = ldpc_detail::check_csc_pattern(D, N, nnz, colptr, rowval)) != LDPC_OK) return st;
    if (K < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "negative number of windows (K)");
    ldpc::WindowPlanIn in;
    in.D = D; in.N = N; in.nnz = nnz; in.colptr = colptr; in.rowval = rowval; in.K = K;
    in.det_ptr = det_ptr; in.det_idx = det_idx; in.mech_ptr = mech_ptr; in.mech_idx = mech_idx;
    in.commit_ptr = commit_ptr; in.commit_idx = commit_idx;
    ldpc::WindowTables tables;
    std::string why;
    switch (ldpc::window_tables_build(in, &tables, &why)) {
    case ldpc::kWindowPlanOk: break;
    case ldpc::kWindowPlanInvalid: return set_error(LDPC_ERR_INVALID_ARGUMENT, why);
    case ldpc::kWindowPlanTooLarge: return set_error(LDPC_ERR_UNSUPPORTED, why);
    default: return set_error(LDPC_ERR_OUT_OF_MEMORY, why);
    }
    hipDeviceProp_t prop;
    int device = options ? options->device : -1;
    st = ldpc_detail::select_device(device, &device, &prop, "no HIP device available (this library has no CPU fallback)");
    if (st != LDPC_OK) return st;

    ldpc_windows *w = new (std::nothrow) ldpc_windows();
    if (!w) return set_error(LDPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    w->D = D; w->N = N; w->K = K; w->device = device; w->num_cus = prop.multiProcessorCount;
    w->wpc = tables.longest <= kWindowWaveColumn ? 1 : 4;
    w->image_stride = (ldpc_trials_k::image_words(tables.max_mech) + 7) & ~7;   // (16-byte granules)
    w->image = (size_t)(kThreads / (64 * w->wpc)) * w->image_stride * sizeof(unsigned short) <= kWindowImageLds;
    w->win = std::move(tables.win);
    if (!ldpc_detail::upload(&w->ints, tables.ints) || w->calls.create() != hipSuccess) {
        (void)hipGetLastError();
        delete w;
        return set_error(LDPC_ERR_OUT_OF_MEMORY, "device allocation of the window tables failed");
    }
    *out = w;
    return LDPC_OK;
}

ldpc_status ldpc_windows_destroy(ldpc_windows *w)
{
    if (!w) return LDPC_OK;
    (void)hipSetDevice(w->device);
    const ldpc_status st = ldpc_detail::wait_device(w->device, "ldpc_windows_destroy (device synchronise)");
    delete w;
    return st;
}

int64_t ldpc_windows_count(const ldpc_windows *w) { return w ? w->K : 0; }

ldpc_status ldpc_windows_gather_device(ldpc_windows *w, int64_t k, int64_t batch, const uint8_t *d_residual,
                                       uint8_t *d_win_syndromes, void *stream)
{
    const ldpc_status st = check_window(w, k, batch);
    if (st != LDPC_OK) return st;
    if (batch == 0) return LDPC_OK;
    if (!d_residual) return set_error(LDPC_ERR_INVALID_ARGUMENT, "window " + std::to_string(k) + ": residual pointer is NULL");
    if (!d_win_syndromes) return set_error(LDPC_ERR_INVALID_ARGUMENT, "window " + std::to_string(k) + ": window syndromes pointer is NULL");
    const ldpc::WindowTable &t = w->win[(size_t)k];
    if (t.ndet == 0) return LDPC_OK;
    WindowParams p{};
    p.residual = const_cast<uint8_t *>(d_residual);   // (no range is given, so no residual byte is stored)
    p.nu = t.ndet; p.u_det = w->ints + t.det;
    p.next = d_win_syndromes; p.nnext = t.ndet;
    return window_launch(w, p, batch, (hipStream_t)stream);
}

ldpc_status ldpc_windows_commit_device(ldpc_windows *w, int64_t k, int64_t batch, const uint8_t *d_win_guess,
                                       const uint8_t *d_win_conv, uint8_t *d_residual, uint8_t *d_guess,
                                       uint8_t *d_conv, uint8_t *d_next_syndromes, void *stream)
{
    const ldpc_status st = check_window(w, k, batch);
    if (st != LDPC_OK) return st;
    const std::string who = "window " + std::to_string(k) + ": ";
    if (d_next_syndromes && k == w->K - 1)
        return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "the last window has no next window (next syndromes pointer must be NULL)");
    if (batch == 0) return LDPC_OK;
    if (!d_win_guess) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "window guess pointer is NULL");
    if (!d_residual) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "residual pointer is NULL");
    if (!d_guess) return set_error(LDPC_ERR_INVALID_ARGUMENT, who + "guess pointer is NULL");
    const ldpc::WindowTable &t = w->win[(size_t)k];
    WindowParams p{};
    p.win_guess = d_win_guess; p.nmech = t.nmech;
    p.nc = t.nc; p.c_pos = w->ints + t.c_pos; p.c_mech = w->ints + t.c_mech;
    p.guess = d_guess; p.residual = d_residual;
    p.nu = t.nu; p.u_det = w->ints + t.u_det; p.u_ptr = w->ints + t.u_ptr; p.u_pos = w->ints + t.u_pos; p.u_next = w->ints + t.u_next;
    p.next = d_next_syndromes; p.nnext = t.nnext;
    p.first = k == 0;
    if (d_win_conv && d_conv) { p.win_conv = d_win_conv; p.conv = d_conv; }
    return window_launch(w, p, batch, (hipStream_t)stream);
}

}  // extern "C"
