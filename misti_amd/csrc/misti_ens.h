// What the ensemble sampler (misti_ensemble_sample; the rule is optimize.ensemble_rule, operation for operation) draws, its exponential
// and its decision.  Host and device call the same functions: what the CPU suite checks through misti_ens_draws, misti_ens_exp and
// misti_ens_accept is what the kernels of misti_ens.hip compute.  Arithmetic: one rounding per operation; a product that feeds a sum
// passes through ens_rn(), so no compiler contracts it into a fused multiply-add.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "misti_boot.h"

namespace misti {

// the value as rounded so far, opaque to the optimiser (misti_device.h's rn(), for both sides of the compilation)
__host__ __device__ __forceinline__ double ens_rn(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+v"(v));
    return v;
#else
    volatile double t = v;
    return t;
#endif
}

// Walker `walker` of step `step` (>= 1) of an ensemble of W walkers owns block step W + walker of Philox(key=[seed, id]):
// w[0] the partner among the W / 2 walkers of the other half, w[1] the stretch's uniform, w[2] the decision's.
struct EnsDraw {
    int partner;
    double u_z, u_acc;
};
__host__ __device__ __forceinline__ EnsDraw ens_draw(uint64_t seed, uint64_t id, int64_t step, int walker, int W) {
    uint64_t w[4];
    philox4x64_10_block(seed, id, (uint64_t)step * (uint64_t)W + (uint64_t)walker, w);
    EnsDraw d;
    d.partner = (int)boot_index(w[0], W / 2);
    d.u_z = (double)(w[1] >> 11) * 0x1p-53;          // numpy's next_double
    d.u_acc = (double)(w[2] >> 11) * 0x1p-53;
    return d;
}

// The stretch z = ((a - 1) u + 1)^2 / a; am1 = a - 1 as rounded once.
__host__ __device__ __forceinline__ double ens_stretch(double a, double am1, double u) {
    const double s = ens_rn(am1 * u) + 1.0;
    return ens_rn(s * s) / a;
}

// The project's own exponential: k = nearest integer to x / ln 2 (the 1.5 x 2^52 addition rounds it), r = x - k ln 2 with ln 2 in two
// pieces (the high one has 32 trailing zero bits: k x high is exact for |k| < 2^11), the Taylor polynomial of degree 13 in Horner form
// on |r| <= 0.35, then ldexp by k.  0 below -746, +inf above 710, a NaN comes back.  Additions, multiplications, comparisons and one
// ldexp, each rounded on its own.
__host__ __device__ __forceinline__ double ens_exp(double x) {
    if (x != x) return x;
    if (x > 710.0) return INFINITY;
    if (x < -746.0) return 0.0;
    constexpr double INV_LN2 = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42feep-1, LN2_LO = 0x1.a39ef35793c76p-33, ROUND = 0x1.8p52;
    constexpr double C[14] = {1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880, 1.0 / 3628800,
                              1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0};
    const double kd = ens_rn(ens_rn(x * INV_LN2) + ROUND) - ROUND;
    double r = x - ens_rn(kd * LN2_HI);
    r = r - ens_rn(kd * LN2_LO);
    double p = C[13];
#pragma unroll
    for (int n = 12; n >= 0; --n) p = ens_rn(p * r) + C[n];
    return ldexp(p, (int)kd);
}

// a log-likelihood the engine has a value for
__host__ __device__ __forceinline__ bool ens_has(double llk) { return llk == llk && llk > -INFINITY && llk < INFINITY; }

// The decision on a proposal that was evaluated: d = N_free - 1, T the search's temperature.
__host__ __device__ __forceinline__ bool ens_decide(double z, int d, double llk_old, double llk_new, double T, double u_acc) {
    if (!ens_has(llk_new)) return false;
    if (!ens_has(llk_old)) return true;
    double g = 1.0;
    for (int k = 0; k < d; ++k) g = ens_rn(g * z);
    const double e = (llk_new - llk_old) / T;
    const double p = ens_rn(g * ens_exp(e));
    return u_acc < p;
}

}  // namespace misti
