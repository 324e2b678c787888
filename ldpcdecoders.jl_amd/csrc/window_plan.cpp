// window_plan.cpp -- see window_plan.hpp.  No HIP header, no abort.
#include "window_plan.hpp"

#include <algorithm>
#include <new>
#include <utility>

namespace ldpc {

namespace {

constexpr int64_t kIndexLimit = (int64_t)1 << 28;   // every index and count is an int32 on the device

struct Refusal {
    WindowPlanStatus status;
    std::string text;
};

std::string at(const char *list, int64_t k, int64_t i) { return "window " + std::to_string(k) + ": " + list + "[" + std::to_string(i) + "]"; }

// ptr[0 .. K] starts at 0 and never falls; -> false with the message
bool check_ptr(const char *name, const int64_t *ptr, int64_t K, Refusal *r)
{
    if (ptr[0] != 0) {
        *r = {kWindowPlanInvalid, std::string("window 0: ") + name + "[0] must be 0"};
        return false;
    }
    for (int64_t k = 0; k < K; ++k)
        if (ptr[k + 1] < ptr[k]) {
            *r = {kWindowPlanInvalid, "window " + std::to_string(k) + ": " + name + "[" + std::to_string(k + 1) + "] is below " + name + "[" + std::to_string(k) + "]"};
            return false;
        }
    return true;
}

// idx[lo .. hi) lies in [0, bound) and rises strictly; `i` in a message counts from the start of the window's list
bool check_list(const char *name, const int64_t *idx, int64_t lo, int64_t hi, int64_t bound, int64_t k, Refusal *r)
{
    for (int64_t q = lo; q < hi; ++q) {
        if (idx[q] < 0 || idx[q] >= bound) {
            *r = {kWindowPlanInvalid, at(name, k, q - lo) + " = " + std::to_string(idx[q]) + " is out of range [0, " + std::to_string(bound) + ")"};
            return false;
        }
        if (q > lo && idx[q] <= idx[q - 1]) {
            *r = {kWindowPlanInvalid, at(name, k, q - lo) + " = " + std::to_string(idx[q]) + " does not rise above the entry before it (" +
                                          std::to_string(idx[q - 1]) + "): a list must be ascending and distinct"};
            return false;
        }
    }
    return true;
}

bool build(const WindowPlanIn &in, WindowTables *out, Refusal *r)
{
    const int64_t K = in.K;
    if (in.D < 0 || in.N < 0 || in.nnz < 0 || K < 0) {
        *r = {kWindowPlanInvalid, "negative dimension (D, N, nnz, K)"};
        return false;
    }
    if (!in.colptr || (in.nnz > 0 && !in.rowval)) {
        *r = {kWindowPlanInvalid, "colptr/rowval is NULL"};
        return false;
    }
    if (!in.det_ptr || !in.mech_ptr || !in.commit_ptr) {
        *r = {kWindowPlanInvalid, "det_ptr, mech_ptr or commit_ptr is NULL"};
        return false;
    }
    if (!check_ptr("det_ptr", in.det_ptr, K, r) || !check_ptr("mech_ptr", in.mech_ptr, K, r) || !check_ptr("commit_ptr", in.commit_ptr, K, r))
        return false;
    if ((in.det_ptr[K] > 0 && !in.det_idx) || (in.mech_ptr[K] > 0 && !in.mech_idx) || (in.commit_ptr[K] > 0 && !in.commit_idx)) {
        *r = {kWindowPlanInvalid, "det_idx, mech_idx or commit_idx is NULL although its list is not empty"};
        return false;
    }
    if (in.D >= kIndexLimit || in.N >= kIndexLimit || in.nnz >= kIndexLimit || K >= kIndexLimit) {
        *r = {kWindowPlanTooLarge, "window tables: model too large for 32-bit indexing"};
        return false;
    }
    std::vector<int32_t> owner((size_t)in.N, -1);   // the window that commits a mechanism
    for (int64_t k = 0; k < K; ++k) {
        const int64_t m0 = in.mech_ptr[k], nmech = in.mech_ptr[k + 1] - m0;
        if (!check_list("det_idx", in.det_idx, in.det_ptr[k], in.det_ptr[k + 1], in.D, k, r) ||
            !check_list("mech_idx", in.mech_idx, m0, in.mech_ptr[k + 1], in.N, k, r) ||
            !check_list("commit_idx", in.commit_idx, in.commit_ptr[k], in.commit_ptr[k + 1], nmech, k, r))
            return false;
        for (int64_t q = in.commit_ptr[k]; q < in.commit_ptr[k + 1]; ++q) {
            const int64_t j = in.mech_idx[m0 + in.commit_idx[q]];
            if (owner[(size_t)j] >= 0) {
                *r = {kWindowPlanInvalid, at("commit_idx", k, q - in.commit_ptr[k]) + ": mechanism " + std::to_string(j) +
                                              " is committed by window " + std::to_string(owner[(size_t)j]) + " already"};
                return false;
            }
            owner[(size_t)j] = (int32_t)k;
        }
    }

    // the tables, window by window; `ints` grows as they are laid down
    out->win.assign((size_t)K, WindowTable());
    std::vector<int32_t> &ints = out->ints;
    std::vector<std::pair<int32_t, int32_t>> touched;   // (detector, committed position)
    for (int64_t k = 0; k < K; ++k) {
        WindowTable &w = out->win[(size_t)k];
        const int64_t d0 = in.det_ptr[k], m0 = in.mech_ptr[k], c0 = in.commit_ptr[k];
        const int64_t ndet = in.det_ptr[k + 1] - d0, nc = in.commit_ptr[k + 1] - c0;
        const int64_t n0 = k + 1 < K ? in.det_ptr[k + 1] : 0, nnext = k + 1 < K ? in.det_ptr[k + 2] - n0 : 0;
        touched.clear();
        for (int64_t q = 0; q < nc; ++q) {
            const int64_t c = in.commit_idx[c0 + q], j = in.mech_idx[m0 + c];
            for (int64_t e = in.colptr[j]; e < in.colptr[j + 1]; ++e) touched.emplace_back((int32_t)in.rowval[e], (int32_t)c);
        }
        std::sort(touched.begin(), touched.end());
        if ((int64_t)ints.size() + ndet + 2 * nc + 3 * ((int64_t)touched.size() + nnext) + (int64_t)touched.size() + 1 >= (int64_t)1 << 31) {
            *r = {kWindowPlanTooLarge, "window tables: more than 2^31 table entries"};
            return false;
        }
        w.ndet = (int)ndet; w.nmech = (int)(in.mech_ptr[k + 1] - m0); w.nc = (int)nc; w.nnext = (int)nnext;
        w.det = ints.size();
        for (int64_t q = 0; q < ndet; ++q) ints.push_back((int32_t)in.det_idx[d0 + q]);
        w.c_pos = ints.size();
        for (int64_t q = 0; q < nc; ++q) ints.push_back((int32_t)in.commit_idx[c0 + q]);
        w.c_mech = ints.size();
        for (int64_t q = 0; q < nc; ++q) ints.push_back((int32_t)in.mech_idx[m0 + in.commit_idx[c0 + q]]);
        // U_k: the detectors of `touched` merged with det_{k+1}, both ascending
        std::vector<int32_t> u_det, u_ptr, u_next;
        u_ptr.push_back(0);
        size_t t = 0;
        int64_t x = 0;
        while (t < touched.size() || x < nnext) {
            const int64_t dt = t < touched.size() ? touched[t].first : INT64_MAX, dx = x < nnext ? in.det_idx[n0 + x] : INT64_MAX;
            const int64_t d = std::min(dt, dx);
            while (t < touched.size() && touched[t].first == d) ++t;
            u_det.push_back((int32_t)d);
            u_ptr.push_back((int32_t)t);
            u_next.push_back(dx == d ? (int32_t)x : -1);
            if (dx == d) ++x;
        }
        w.nu = (int)u_det.size(); w.nupos = (int)touched.size();
        w.u_det = ints.size();
        ints.insert(ints.end(), u_det.begin(), u_det.end());
        w.u_ptr = ints.size();
        ints.insert(ints.end(), u_ptr.begin(), u_ptr.end());
        w.u_pos = ints.size();
        for (const auto &pr : touched) ints.push_back(pr.second);
        w.u_next = ints.size();
        ints.insert(ints.end(), u_next.begin(), u_next.end());
        out->longest = std::max({out->longest, w.nmech, w.ndet, w.nu});
        out->max_mech = std::max(out->max_mech, w.nmech);
    }
    return true;
}

}  // namespace

WindowPlanStatus window_tables_build(const WindowPlanIn &in, WindowTables *out, std::string *error)
{
    *out = WindowTables();
    Refusal r{kWindowPlanOk, std::string()};
    try {
        if (build(in, out, &r)) return kWindowPlanOk;
    } catch (const std::bad_alloc &) {
        r = {kWindowPlanNoMemory, "window tables: host allocation failed"};
    }
    *out = WindowTables();
    if (error) *error = r.text;
    return r.status;
}

}  // namespace ldpc
