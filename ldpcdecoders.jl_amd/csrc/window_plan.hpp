// window_plan.hpp -- the index tables of the sliding-window step (ldpc_windows_* of include/ldpc_mi355x.h): the caller's
// window lists are validated and turned, once per handle, into what window_kernels.hpp reads.  Pure host code over the
// standard library -- no HIP, no handle, no environment -- so that it builds with a plain C++ compiler and runs under the
// sanitizers on the CPU (tests/native/window_plan_sanitize.cpp).  Nothing here aborts: a refusal is a status and a
// message, an allocation that fails is a status too.  ldpc_windows.hip fills the input and uploads `ints`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ldpc {

// The caller's arrays as ldpc_windows_create takes them.  H (D x N, zero-based CSC) must be a valid pattern already
// (columns in range, rows ascending and distinct: check_csc_pattern of host_common.hpp); the window lists are checked here.
struct WindowPlanIn {
    int64_t D = 0, N = 0, nnz = 0;
    const int64_t *colptr = nullptr, *rowval = nullptr;
    int64_t K = 0;
    const int64_t *det_ptr = nullptr, *det_idx = nullptr;        // det_k  = det_idx[det_ptr[k] .. det_ptr[k + 1])
    const int64_t *mech_ptr = nullptr, *mech_idx = nullptr;      // mech_k likewise
    const int64_t *commit_ptr = nullptr, *commit_idx = nullptr;  // commit_k: positions in mech_k
};

// One window's tables: counts, and where each table starts in WindowTables::ints.
//   det    [ndet]    det_k (the gather reads it as its list of owned detectors)
//   c_pos  [nc]      the committed positions in mech_k, ascending;  c_mech [nc]: their global mechanism indices
//   u_det  [nu]      U_k, ascending: the detectors that a committed column touches (its FULL column in H), united with det_{k+1}
//   u_ptr  [nu + 1]  entry u's committed positions are u_pos[u_ptr[u] .. u_ptr[u + 1]) (ascending; empty for a detector
//                    that is in U_k through det_{k+1} alone)
//   u_next [nu]      entry u's place in det_{k+1}, or -1
struct WindowTable {
    int ndet = 0, nmech = 0, nc = 0, nu = 0, nnext = 0, nupos = 0;   // nnext = |det_{k+1}| (0 for the last window)
    size_t det = 0, c_pos = 0, c_mech = 0, u_det = 0, u_ptr = 0, u_pos = 0, u_next = 0;
};

struct WindowTables {
    std::vector<WindowTable> win;
    std::vector<int32_t> ints;
    int longest = 0;      // the largest of every window's nmech, ndet and nu (what sizes a column's work)
    int max_mech = 0;     // the largest nmech (what sizes a column's bit image)
};

enum WindowPlanStatus { kWindowPlanOk = 0, kWindowPlanInvalid = 1, kWindowPlanTooLarge = 2, kWindowPlanNoMemory = 3 };

// Validates the lists (every message names the window and the index) and builds the tables.  On anything but
// kWindowPlanOk `*error` says why and `*out` is left empty.
WindowPlanStatus window_tables_build(const WindowPlanIn &in, WindowTables *out, std::string *error);

}  // namespace ldpc
