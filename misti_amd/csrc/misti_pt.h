// What the tempered ensemble sampler (misti_tempered_sample; the rule is optimize.tempered_rule, operation for operation) adds to
// misti_ens.h: the uniform of a swap and its decision.  Host and device call the same functions: what the CPU suite checks through
// misti_pt_swap is what the swap kernel of misti_pt.hip computes.  Arithmetic as in misti_ens.h: one rounding per operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "misti_boot.h"
#include "misti_ens.h"

namespace misti {

// Walker `walker` of rung `rung` of step `step` of a fit with L rungs owns block (step L + rung) W + walker of Philox(key=[seed, id]):
// ens_draw(seed, id, step L + rung, walker, W) reads w[0 ... 2] of it; the swap of the pair (rung, rung + 1) reads w[3].
__host__ __device__ __forceinline__ double pt_swap_uniform(uint64_t seed, uint64_t id, int64_t step, int L, int rung, int walker, int W) {
    uint64_t w[4];
    philox4x64_10_block(seed, id, ((uint64_t)step * (uint64_t)L + (uint64_t)rung) * (uint64_t)W + (uint64_t)walker, w);
    return (double)(w[3] >> 11) * 0x1p-53;
}

// The decision on walker i of the rungs at T_lo < T_hi: no swap where either has no value; db = 1 / T_lo - 1 / T_hi,
// e = db (llk_hi - llk_lo), swapped iff u < ens_exp(e).
__host__ __device__ __forceinline__ bool pt_swap_decide(double T_lo, double T_hi, double llk_lo, double llk_hi, double u) {
    if (!ens_has(llk_lo) || !ens_has(llk_hi)) return false;
    const double db = ens_rn(1.0 / T_lo) - ens_rn(1.0 / T_hi);
    const double e = ens_rn(db * (llk_hi - llk_lo));
    return u < ens_exp(e);
}

// One term of the thermodynamic integral: (0.5 (E_lo + E_hi)) (1 / T_lo - 1 / T_hi), each operation rounded on its own.
__host__ __device__ __forceinline__ double pt_trapezoid(double T_lo, double T_hi, double E_lo, double E_hi) {
    const double db = ens_rn(1.0 / T_lo) - ens_rn(1.0 / T_hi);
    return ens_rn(ens_rn(0.5 * (E_lo + E_hi)) * db);
}

}  // namespace misti
