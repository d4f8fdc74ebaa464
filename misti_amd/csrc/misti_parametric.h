// The rule of the parametric bootstrap (misti_parametric_rows_dev, misti_parametric_thresholds, misti_parametric_counts; stated in
// NumPy as optimize.parametric_thresholds / optimize.parametric_rows): a spectrum's six integer thresholds and the class of a draw.
// Host and device call the same functions: what the CPU suite checks through the two host hooks is what the kernel counts.
#pragma once
#include <cmath>

#include "misti_boot.h"

namespace misti {

// T_k = ceil(q_k 2^53), q_k = c_k / c_6, c_k the running sum ((p0 + p1) + ...) + pk: one float64 addition per class, one division per
// threshold, a scaling by a power of two (exact) and ceil (exact) - correctly rounded float64 throughout, the same on host and device
// and in NumPy.  The running sum never decreases (a rounded addition of a non-negative term is monotone), so q_k <= 1 and T_k is in
// [0, 2^53], non-decreasing in k.  Returns false - T is then all zero - for a spectrum no replicate can be drawn from: an entry
// that is negative or not finite, or a total that is not finite (the sum overflowed) or not > 0.
__host__ __device__ __forceinline__ bool param_thresholds(const double* __restrict__ p, uint64_t T[6]) {
    constexpr double DBL_LARGEST = 1.7976931348623157e308;
    double c[7], run = 0.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double v = p[k];
        ok = ok && v >= 0.0 && v <= DBL_LARGEST;          // (a NaN fails both comparisons)
        run = k == 0 ? v : run + v;
        c[k] = run;
    }
    ok = ok && c[6] > 0.0 && c[6] <= DBL_LARGEST;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double q = c[k] / c[6];
        T[k] = ok ? (uint64_t)ceil(q * 9007199254740992.0) : 0ull;
    }
    return ok;
}

// What a raw 64-bit value of the stream is compared with: its high 53 bits, the integer numpy.random.Generator.random scales by 2^-53.
__host__ __device__ __forceinline__ uint64_t param_u(uint64_t raw) { return raw >> 11; }

// The class of a draw: the number of thresholds it has reached (numpy.searchsorted(q, u 2^-53, side='right')).
__host__ __device__ __forceinline__ int param_class(uint64_t u, const uint64_t T[6]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) k += u >= T[i] ? 1 : 0;
    return k;
}

}  // namespace misti
