// What the joint credible regions of coordinate pairs (misti_ens_joint_dev / misti_ensemble_sample_joint / misti_tempered_sample_joint;
// the rule is optimize.ensemble_joint_rule) share between the host layer and the kernels of misti_joint.hip: the bin of a sample, the
// samples in a region of a given mass, the slab of samples a histogram workgroup takes, and the launch record.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/misti_hip.h"

namespace misti {

#define MISTI_JOINT_SLAB 4096                              /* mirrored as _lib.JOINT_SLAB: the tests aim at its edges */
constexpr int JOINT_SLAB = MISTI_JOINT_SLAB;               // samples a histogram workgroup bins: 16 per thread
constexpr int JOINT_MAX_CELLS = MISTI_JOINT_MAX_BINS * MISTI_JOINT_MAX_BINS;

// The bin of an INSIDE sample (lo <= x && x <= hi) on an axis of B bins, scale = double(B) / (hi - lo): one subtraction and one
// product, each rounded on its own.  !(t >= 0) covers hi == lo (0 inf is NaN) and an infinite hi - lo; x == hi lands in bin B - 1.
__host__ __device__ __forceinline__ int joint_bin(double x, double lo, double scale, int B) {
    const double t = (x - lo) * scale;
    if (!(t >= 0.0)) return 0;
    if (t >= (double)B) return B - 1;
    return (int)t;
}

// The samples a region of mass p in (0, 1] must hold: the smallest integer k with double(k) >= double(inside) p (one rounded
// product), clamped to 1 ... inside - the HPD rule's window, on `inside`.  inside >= 1.
__host__ __device__ __forceinline__ int32_t joint_need(int32_t inside, double p) {
    const double k = ceil((double)inside * p);
    return k < 1.0 ? 1 : k > (double)inside ? inside : (int32_t)k;
}

// One call: S searches of chain[S][K][W][N], the kept steps burn ... K - 1 (n of them), n_pair pairs.  Every pointer is device memory.
// `window` is what the histogram reads: the caller's ranges, or where range_kernel leaves those taken from the data (range_out, or
// the call's workspace); `counts` is the caller's or the call's workspace (NULL: no histogram is built).  An output that is NULL is
// not computed.  The pairs travel in the launch record: a coordinate and a bin count fit a byte.
struct JointArgs {
    int64_t S, K, burn, n;
    int32_t W, N, n_pair, n_mass, n_coord, slabs;
    int64_t cells;                                         // sum_q Ba Bb: a search's counts
    const double* chain;
    const double* window;                                  // [S][n_pair][2][2]
    double* from_data;                                     // == window where the ranges are taken from the data, else NULL
    int32_t* counts;                                       // [S][cells]
    int32_t *inside, *mode, *level, *held;
    int32_t* n_cells;                                      // the descriptor's `cells`
    double mass[MISTI_POST_MAX_PROBS];
    int32_t off[MISTI_JOINT_MAX_PAIRS];                    // pair q's cells begin at off[q]
    uint8_t a[MISTI_JOINT_MAX_PAIRS], b[MISTI_JOINT_MAX_PAIRS], Ba[MISTI_JOINT_MAX_PAIRS], Bb[MISTI_JOINT_MAX_PAIRS];
    uint8_t coord[MISTI_MAX_PARAMS];                       // the coordinates that occur in a pair, ascending: n_coord of them
    bool levels() const { return inside || mode || level || n_cells || held; }
};
hipError_t launch_joint(const JointArgs& a, hipStream_t stream);

}  // namespace misti
