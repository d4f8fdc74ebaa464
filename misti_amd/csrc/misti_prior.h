// What a prior adds to misti_ens.h (misti_ensemble_sample_prior / misti_tempered_sample_prior; the rule is optimize.ensemble_prior_rule,
// operation for operation): the map from a sampling coordinate to the engine's, the log prior of a walker and the decision that carries
// it.  Host and device call the same functions: what the CPU suite checks through misti_ens_log_prior and misti_ens_accept_prior is what
// the kernels of misti_ens.hip compute.  Arithmetic as in misti_ens.h: one rounding per operation, a product through ens_rn().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/misti_hip.h"

#include "misti_ens.h"

namespace misti {

// The engine's value of sampling coordinate y: y itself (MISTI_COORD_LINEAR) or ens_exp(y) (MISTI_COORD_LOG).
__host__ __device__ __forceinline__ double ens_natural(int32_t scale, double y) { return scale == MISTI_COORD_LOG ? ens_exp(y) : y; }

// The log prior of a walker at y[N] in the box [lo, hi]: from +0.0, in increasing k, one term per coordinate that is neither fixed
// (lo == hi) nor MISTI_PRIOR_FLAT.  NORMAL(mean p0, sd p1): u = (y - p0) / p1, -0.5 (u u).  EXPONENTIAL(scale p0): -((y - lo) / p0).
// Unnormalised.  `hi` tells a fixed coordinate only.
__host__ __device__ __forceinline__ double ens_log_prior(int N, const int32_t* kind, const double* p0, const double* p1, const double* lo,
                                                         const double* hi, const double* y) {
    double lp = 0.0;
    for (int k = 0; k < N; ++k) {
        if (lo[k] == hi[k] || kind[k] == MISTI_PRIOR_FLAT) continue;
        if (kind[k] == MISTI_PRIOR_NORMAL) {
            const double u = (y[k] - p0[k]) / p1[k];
            lp = lp + ens_rn(-0.5 * ens_rn(u * u));
        } else {
            lp = lp + -((y[k] - lo[k]) / p0[k]);
        }
    }
    return lp;
}

// ens_decide with a prior: e = (llk_new - llk_old) / T + (lp_new - lp_old) - the prior is not tempered.
__host__ __device__ __forceinline__ bool ens_decide_prior(double z, int d, double llk_old, double llk_new, double T, double lp_old, double lp_new,
                                                          double u_acc) {
    if (!ens_has(llk_new)) return false;
    if (!ens_has(llk_old)) return true;
    double g = 1.0;
    for (int k = 0; k < d; ++k) g = ens_rn(g * z);
    const double e = (llk_new - llk_old) / T + (lp_new - lp_old);
    const double p = ens_rn(g * ens_exp(e));
    return u_acc < p;
}

}  // namespace misti
