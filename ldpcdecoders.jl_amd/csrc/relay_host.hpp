// relay_host.hpp -- what the two relay decoders (ldpc_relay.hip, ldpc_pauli_relay.hip) share on the host on top of
// tile_host.hpp: the create-time checks of the legs, the legs that run, the quantised weight of a prior and the size limits.
#pragma once
#include <vector>

#include "tile_host.hpp"

namespace ldpc_detail {

constexpr int64_t kRelayMaxBits = (int64_t)1 << 22;   // a weight is a sum of at most 2^22 terms below 2^41

// The checks a relay create makes on legs, gammas [legs][n], leg_iters [legs] and its options, in the order both creates
// keep: the arguments of the legs, tile_options(), stop_after and the iterations, the decoder's own check of its priors
// (priors_finite), the range of the memory strengths.
template <class Options, class PriorCheck>
inline ldpc_status relay_check_legs(int64_t n, int64_t legs, const float *gammas, const int32_t *leg_iters, const Options *options, float *alpha,
                                    float *clip, int *variant, int *device, int *stop_after, PriorCheck priors_finite)
{
    if (legs < 1) return set_error(LDPC_ERR_INVALID_ARGUMENT, "legs must be >= 1");
    if (legs > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "legs must fit int32");
    if (n > 0 && !gammas) return set_error(LDPC_ERR_INVALID_ARGUMENT, "gammas is NULL");
    if (!leg_iters) return set_error(LDPC_ERR_INVALID_ARGUMENT, "leg_iters is NULL");
    ldpc_status st = tile_options(options, alpha, clip, variant, device);
    if (st != LDPC_OK) return st;
    *stop_after = options && options->stop_after != 0 ? options->stop_after : 1;
    if (*stop_after < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "stop_after must be >= 1 (0 = default 1)");
    int64_t total_iters = 0;
    for (int64_t r = 0; r < legs; ++r) {
        if (leg_iters[r] < 0) return set_error(LDPC_ERR_INVALID_ARGUMENT, "leg_iters[" + std::to_string(r) + "] is negative");
        if ((total_iters += leg_iters[r]) > INT32_MAX) return set_error(LDPC_ERR_INVALID_ARGUMENT, "the sum of leg_iters exceeds INT32_MAX");
    }
    if ((st = priors_finite()) != LDPC_OK) return st;
    for (int64_t r = 0; r < legs; ++r)
        for (int64_t j = 0; j < n; ++j) {
            const float g = gammas[r * n + j];
            if (!(g > -1.0f && g < 1.0f))   // (false for NaN as well)
                return set_error(LDPC_ERR_INVALID_ARGUMENT, "gammas[" + std::to_string(r) + "][" + std::to_string(j) + "] must be finite and lie in (-1, 1)");
        }
    return LDPC_OK;
}

// The iterations of the legs that run (legs of 0 iterations are dropped, so the kernel sees none); per_leg(r) for each of
// them, in order: the decoder appends the leg's rows to its own table.
template <class PerLeg> inline std::vector<int> relay_running_legs(int64_t legs, const int32_t *leg_iters, PerLeg per_leg)
{
    std::vector<int> iters;
    for (int64_t r = 0; r < legs; ++r) {
        if (leg_iters[r] == 0) continue;
        iters.push_back(leg_iters[r]);
        per_leg(r);
    }
    return iters;
}

// q = rint(clamp(llr, +-2^24) * 2^16): what a set bit adds to a solution's weight
inline long long relay_weight(float llr) { return (long long)std::rint(std::min(std::max((double)llr, -16777216.0), 16777216.0) * 65536.0); }

// the limits of tile_index_limits(), and n <= 2^22 in place of its bound on n
inline ldpc_status relay_index_limits(const char *family, int64_t s, int64_t n, int64_t nnz)
{
    const ldpc_status st = tile_index_limits(family, s, n, nnz, false);
    if (st != LDPC_OK) return st;
    if (n > kRelayMaxBits) return set_error(LDPC_ERR_UNSUPPORTED, std::string(family) + " kernels: n > 2^22 (a solution's weight must fit int64)");
    return LDPC_OK;
}

}  // namespace ldpc_detail
