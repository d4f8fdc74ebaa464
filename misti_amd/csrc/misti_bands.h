// What the trajectory bands (misti_traj_bands_dev / misti_traj_bands; the rule is optimize.trajectory_bands_rule) share between the host
// layer and the kernels of misti_bands.hip: the rank of a quantile among n members (a function of n and the probability alone, but n
// varies per series, so the device computes it as the host does), the tile of the gather, and the launch record.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/misti_hip.h"
#include "misti_post.h"

namespace misti {

constexpr int BANDS_TILE = 64;                             // the gather's tile: 64 samples x 64 columns of 8 bytes, a padded 33 KiB of LDS

// h = double(n - 1) p, i = floor(h), g = h - i; g == 0 or i >= n - 1: x_(min(i, n - 1)) exactly (lo == hi), otherwise x_(lo) +
// g (x_(hi) - x_(lo)) with hi = lo + 1.  n >= 1, p in [0, 1].  misti_bands_rank is this function.
__host__ __device__ __forceinline__ void bands_rank(int64_t n, double p, int64_t* lo, int64_t* hi, double* g) {
    const double h = (double)(n - 1) * p;
    const double fl = floor(h);
    int64_t i = (int64_t)fl;
    *g = h - fl;
    if (*g == 0.0 || i >= n - 1) {
        if (i > n - 1) i = n - 1;
        *lo = *hi = i;
    } else {
        *lo = i; *hi = i + 1;
    }
}

// One pass: G groups of lc[G][m][T1][2] (T1 = numT + 1; row numT is never read), split[G][m], status[G][m] or NULL.  A series is
// (group, interval, population): C = 2 numT of them per group, series (g, c) with c = 2 j + pop; its keys lie at
// ws[side][(g C + c) m ...], side 0 or 1 (side 1 only where m exceeds the sort's tile).  Every output is [G][C] (quant: [G][C][n_prob])
// in device memory; one that is NULL is not computed.
struct BandsArgs {
    int64_t G, m;
    int32_t numT, n_prob;
    const double* lc;
    const double* split;
    const int32_t* status;
    uint64_t* ws;
    int32_t* count;
    double *mean, *quant, *lo, *hi;
    double probs[MISTI_POST_MAX_PROBS];
};
hipError_t launch_bands(const BandsArgs& a, hipStream_t stream);

}  // namespace misti
