// layer_plan.cpp -- see layer_plan.hpp.  No HIP header, no abort.
#include "layer_plan.hpp"

#include <new>

namespace ldpc {

namespace {

constexpr int64_t kIndexLimit = (int64_t)1 << 28;   // every index and count is an int32 on the device

struct Refusal {
    LayerPlanStatus status;
    std::string text;
};

inline int lowest_zero(uint64_t w)   // w != all ones
{
    int b = 0;
    while ((w >> b) & 1u) ++b;
    return b;
}

bool check_pattern(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, Refusal *r)
{
    if (s < 0 || n < 0) {
        *r = {kLayerPlanInvalid, "layer plan: negative dimension (s, n)"};
        return false;
    }
    if (s >= kIndexLimit || n >= kIndexLimit) {
        *r = {kLayerPlanTooLarge, "layer plan: graph too large for 32-bit indexing"};
        return false;
    }
    if (!row_ptr) {
        *r = {kLayerPlanInvalid, "layer plan: row_ptr is NULL"};
        return false;
    }
    if (row_ptr[0] != 0) {
        *r = {kLayerPlanInvalid, "layer plan: row_ptr[0] must be 0"};
        return false;
    }
    for (int64_t i = 0; i < s; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) {
            *r = {kLayerPlanInvalid, "layer plan: row_ptr[" + std::to_string(i + 1) + "] is below row_ptr[" + std::to_string(i) + "]"};
            return false;
        }
    if (row_ptr[s] >= kIndexLimit) {
        *r = {kLayerPlanTooLarge, "layer plan: graph too large for 32-bit indexing"};
        return false;
    }
    if (row_ptr[s] > 0 && !csr_col) {
        *r = {kLayerPlanInvalid, "layer plan: csr_col is NULL although the graph has edges"};
        return false;
    }
    for (int64_t e = 0; e < row_ptr[s]; ++e)
        if (csr_col[e] < 0 || csr_col[e] >= n) {
            *r = {kLayerPlanInvalid, "layer plan: csr_col[" + std::to_string(e) + "] = " + std::to_string(csr_col[e]) + " is out of range [0, " +
                                         std::to_string(n) + ")"};
            return false;
        }
    return true;
}

bool build(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, LayerPlan *out, Refusal *r)
{
    if (!check_pattern(s, n, row_ptr, csr_col, r)) return false;
    // used[j]: bit l of the words = a check holding bit j sits in layer l; grows with the layers the bit has seen
    std::vector<std::vector<uint64_t>> used((size_t)n);
    out->layer_of.assign((size_t)s, -1);
    std::vector<int32_t> count;
    for (int64_t i = 0; i < s; ++i) {
        const int32_t ra = row_ptr[i], rb = row_ptr[i + 1];
        if (ra == rb) continue;
        int layer = -1;
        for (size_t w = 0; layer < 0; ++w) {   // ends: a word no bit of the check has reached yet is all zeros
            uint64_t taken = 0;
            for (int32_t e = ra; e < rb; ++e) {
                const std::vector<uint64_t> &u = used[(size_t)csr_col[e]];
                if (w < u.size()) taken |= u[w];
            }
            if (~taken) layer = (int)(w * 64) + lowest_zero(taken);
        }
        for (int32_t e = ra; e < rb; ++e) {
            std::vector<uint64_t> &u = used[(size_t)csr_col[e]];
            if (u.size() <= (size_t)layer / 64) u.resize((size_t)layer / 64 + 1, 0);
            u[(size_t)layer / 64] |= (uint64_t)1 << (layer % 64);
        }
        out->layer_of[(size_t)i] = layer;
        if ((size_t)layer >= count.size()) count.resize((size_t)layer + 1, 0);   // first fit: layer <= the number of layers so far
        ++count[(size_t)layer];
    }
    out->K = (int)count.size();
    out->layer_ptr.assign((size_t)out->K + 1, 0);
    for (int l = 0; l < out->K; ++l) out->layer_ptr[(size_t)l + 1] = out->layer_ptr[(size_t)l] + count[(size_t)l];
    out->layer_checks.assign((size_t)out->layer_ptr[(size_t)out->K], 0);
    std::vector<int32_t> at(out->layer_ptr.begin(), out->layer_ptr.end() - 1);
    for (int64_t i = 0; i < s; ++i)   // ascending i: ascending inside a layer
        if (out->layer_of[(size_t)i] >= 0) out->layer_checks[(size_t)at[(size_t)out->layer_of[(size_t)i]]++] = (int32_t)i;
    return true;
}

bool verify(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, const LayerPlan &p, std::string *why)
{
    if (p.K < 0 || p.layer_ptr.size() != (size_t)p.K + 1 || p.layer_of.size() != (size_t)s || p.layer_ptr[0] != 0) {
        *why = "layer plan: the arrays do not have the sizes of K layers and s checks";
        return false;
    }
    for (int l = 0; l < p.K; ++l)
        if (p.layer_ptr[(size_t)l + 1] < p.layer_ptr[(size_t)l]) {
            *why = "layer plan: layer_ptr falls at layer " + std::to_string(l);
            return false;
        }
    if ((size_t)p.layer_ptr[(size_t)p.K] != p.layer_checks.size()) {
        *why = "layer plan: layer_ptr[K] is not the number of listed checks";
        return false;
    }
    std::vector<int32_t> seen((size_t)s, 0), stamp((size_t)n, -1);   // stamp[j]: the last layer that touched bit j
    for (int l = 0; l < p.K; ++l)
        for (int32_t q = p.layer_ptr[(size_t)l]; q < p.layer_ptr[(size_t)l + 1]; ++q) {
            const int32_t i = p.layer_checks[(size_t)q];
            if (i < 0 || i >= s || row_ptr[i] == row_ptr[i + 1] || p.layer_of[(size_t)i] != l || seen[(size_t)i]++) {
                *why = "layer plan: layer " + std::to_string(l) + " lists check " + std::to_string(i) + ", which is out of range, empty, listed twice or assigned elsewhere";
                return false;
            }
            for (int32_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
                if (stamp[(size_t)csr_col[e]] == l) {
                    *why = "layer plan: two edges of layer " + std::to_string(l) + " meet in bit " + std::to_string(csr_col[e]) + " (check " + std::to_string(i) + ")";
                    return false;
                }
                stamp[(size_t)csr_col[e]] = l;
            }
        }
    for (int64_t i = 0; i < s; ++i)
        if ((row_ptr[i] < row_ptr[i + 1]) != (seen[(size_t)i] == 1) || (row_ptr[i] == row_ptr[i + 1] && p.layer_of[(size_t)i] != -1)) {
            *why = "layer plan: check " + std::to_string(i) + " is not in exactly one layer (an empty check: in none)";
            return false;
        }
    return true;
}

}  // namespace

LayerPlanStatus layer_plan_build(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, LayerPlan *out, std::string *error)
{
    *out = LayerPlan();
    Refusal r{kLayerPlanOk, std::string()};
    try {
        if (build(s, n, row_ptr, csr_col, out, &r)) return kLayerPlanOk;
    } catch (const std::bad_alloc &) {
        r = {kLayerPlanNoMemory, "layer plan: host allocation failed"};
    }
    *out = LayerPlan();
    if (error) *error = r.text;
    return r.status;
}

bool layer_plan_verify(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, const LayerPlan &plan, std::string *error)
{
    std::string why;
    bool ok = false;
    try {
        Refusal r{kLayerPlanOk, std::string()};
        ok = check_pattern(s, n, row_ptr, csr_col, &r);
        if (!ok) why = r.text;
        else ok = verify(s, n, row_ptr, csr_col, plan, &why);
    } catch (const std::bad_alloc &) {
        why = "layer plan: host allocation failed";
        ok = false;
    }
    if (!ok && error) *error = why;
    return ok;
}

}  // namespace ldpc
