// layer_plan.hpp -- the layers of the layered min-sum schedule (THE LAYERED RULE of include/ldpc_mi355x.h, the
// ldpc_minsum_* section): first fit over the checks in ascending index, so that the checks of a layer share no bit and the
// threads of a workgroup may update them side by side (layered_kernels.hpp).  Pure host code over the standard library --
// no HIP, no decoder handle, no environment -- so that it builds with a plain C++ compiler and runs under the sanitizers
// on the CPU (tests/native/layer_plan_sanitize.cpp).  Nothing here aborts: a refusal is a status and a message, an
// allocation that fails is a status too.  ldpc_minsum_create builds the plan, verifies it and uploads layer_ptr and
// layer_checks; ldpc_debug_layer_plan (include/ldpc_mi355x_debug.h) hands it to the CPU tests.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ldpc {

struct LayerPlan {
    int K = 0;                            // layers
    std::vector<int32_t> layer_ptr;       // [K + 1]: layer l holds layer_checks[layer_ptr[l] .. layer_ptr[l + 1])
    std::vector<int32_t> layer_checks;    // the non-empty checks, layer by layer, ascending inside a layer
    std::vector<int32_t> layer_of;        // [s]: the layer of a check, -1 for a check with no bits
};

enum LayerPlanStatus { kLayerPlanOk = 0, kLayerPlanInvalid = 1, kLayerPlanTooLarge = 2, kLayerPlanNoMemory = 3 };

// The CSR pattern: check i has the bits csr_col[row_ptr[i] .. row_ptr[i + 1]), each in [0, n).  row_ptr[0] = 0 and
// row_ptr never falls (both checked here, as is the range of every bit; a bit twice in a check is refused by the
// verification below, not here).  Cost: about nnz * K / 64 word operations -- one growing bitset of used layers per bit.
// On anything but kLayerPlanOk `*error` says why and `*out` is left empty.
LayerPlanStatus layer_plan_build(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, LayerPlan *out, std::string *error);

// What the kernel relies on: no two checks of a layer share a bit (no bit twice inside a check either), every non-empty
// check appears in exactly one layer, no empty check in any, the arrays have the sizes above.  A slip would be a data
// race on the device, so create runs this on every finished plan.  false: `*error` says what is wrong.
bool layer_plan_verify(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, const LayerPlan &plan, std::string *error);

}  // namespace ldpc
