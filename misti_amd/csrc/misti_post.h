// What the posterior summaries of a chain (misti_ens_summary_dev / misti_ensemble_posterior; the rule is
// optimize.ensemble_posterior_rule, operation for operation) share between the host layer and the kernels of misti_post.hip: the
// order key, the wanted order statistics of a search (a function of m = n W and the probabilities alone, so the host computes them
// once), the window length of a shortest (HPD) interval (optimize.ensemble_hpd_rule; a function of m and the mass alone), the tile of
// the sort, and the launch record.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/misti_hip.h"

namespace misti {

constexpr int POST_MAX_RANKS = 2 * MISTI_POST_MAX_PROBS;   // a probability needs x_(i) and x_(i+1)
constexpr int POST_LANES = 64;                             // lsum's partials: one per lane of a wave
#define MISTI_POST_SORT_TILE 2048                          /* mirrored as _lib.POST_SORT_TILE: the tests aim at its edges */
constexpr int POST_SORT_TILE = MISTI_POST_SORT_TILE;       // keys a workgroup sorts in LDS (16 KiB), and the keys a merge workgroup emits

// lsum's fold (misti_post.hip's sums over steps, misti_pt.hip's reduction): a partial is a lane of a wave; every lane ends with partial[0]
__device__ __forceinline__ double post_fold(double v) {
#pragma unroll
    for (int stride = POST_LANES / 2; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride, POST_LANES);
    return __shfl(v, 0, POST_LANES);
}

// what is stored of a result: IEEE leaves the sign and the payload of a NaN to the implementation, the rule does not - the canonical quiet NaN
__device__ __forceinline__ double post_out(double v) { return v != v ? __longlong_as_double(0x7ff8000000000000ll) : v; }

// The total order of the rule: the 64-bit key of a double's bits.  A set sign bit flips all bits, a clear one only the sign bit:
// -0.0 before +0.0, NaNs of a clear sign bit last.
__host__ __device__ __forceinline__ uint64_t post_key(uint64_t bits) { return (bits >> 63) ? ~bits : bits ^ 0x8000000000000000ull; }
__host__ __device__ __forceinline__ uint64_t post_unkey(uint64_t key) { return (key >> 63) ? key ^ 0x8000000000000000ull : ~key; }

// The order statistics a search's quantiles need: rank[] ascending and distinct; probability p reads x_(rank[lo[p]]) and, where it
// interpolates (hi[p] != lo[p]), x_(rank[hi[p]]) with weight g[p].
struct PostSelect {
    int32_t n_prob, n_rank;
    int32_t rank[POST_MAX_RANKS];
    int32_t lo[MISTI_POST_MAX_PROBS], hi[MISTI_POST_MAX_PROBS];
    double g[MISTI_POST_MAX_PROBS];
};

// h = double(m - 1) p, i = floor(h), g = h - i; g == 0 or i >= m - 1: x_(min(i, m - 1)) exactly.  probs: n_prob values in [0, 1].
inline PostSelect post_select(int64_t m, int n_prob, const double* probs) {
    PostSelect s{};
    s.n_prob = n_prob;
    int32_t want[POST_MAX_RANKS];
    int n_want = 0;
    int32_t a[MISTI_POST_MAX_PROBS], b[MISTI_POST_MAX_PROBS];
    for (int p = 0; p < n_prob; ++p) {
        const double h = (double)(m - 1) * probs[p];
        const double fl = floor(h);
        int64_t i = (int64_t)fl;
        s.g[p] = h - fl;
        if (s.g[p] == 0.0 || i >= m - 1) {
            if (i > m - 1) i = m - 1;
            a[p] = b[p] = (int32_t)i;
            want[n_want++] = (int32_t)i;
        } else {
            a[p] = (int32_t)i; b[p] = (int32_t)(i + 1);
            want[n_want++] = a[p]; want[n_want++] = b[p];
        }
    }
    for (int i = 1; i < n_want; ++i)                        // insertion sort: at most 16
        for (int k = i; k > 0 && want[k] < want[k - 1]; --k) { const int32_t t = want[k]; want[k] = want[k - 1]; want[k - 1] = t; }
    for (int i = 0; i < n_want; ++i)
        if (!s.n_rank || s.rank[s.n_rank - 1] != want[i]) s.rank[s.n_rank++] = want[i];
    for (int p = 0; p < n_prob; ++p)
        for (int r = 0; r < s.n_rank; ++r) {
            if (s.rank[r] == a[p]) s.lo[p] = r;
            if (s.rank[r] == b[p]) s.hi[p] = r;
        }
    return s;
}

// The window of a shortest interval of mass p in (0, 1]: k samples, the smallest integer with double(k) >= double(m) p (one rounded
// product), clamped to 1 ... m.
inline int32_t post_hpd_window(int64_t m, double p) {
    int64_t k = (int64_t)ceil((double)m * p);
    if (k < 1) k = 1;
    if (k > m) k = m;
    return (int32_t)k;
}

// One call: S searches of chain[S][K][W][N], the kept steps burn ... K - 1 (n of them), lags 0 ... L.  Every pointer is device
// memory; an output that is NULL is not computed.  ws_mean[S][N] and ws_y[S][N][n] are the call's workspace: the mean and the
// centred ensemble-mean series (1 / W of the kept chain).  hpd / hpd_at / order need the sorted marginals: ws_sort[2][S][N][m], the
// ping-pong pair of the sort, is theirs alone (NULL where none of the three is asked for) - twice the kept chain's bytes, no more.
struct PostArgs {
    int64_t S, K, burn, n, L;
    int64_t llh_K;                   // rows of chain_llh from one search to the next: K, or (the tempered sampler keeps the values of
                                     // every rung, [S][rungs][K][W], and summarises rung 0) rungs x K
    int32_t W, N;
    double c;
    const double* chain;
    const double* chain_llh;         // or NULL: no best sample
    double *ws_mean, *ws_y;
    double *mean, *cov, *quant, *tau;
    int32_t* window;
    double *best_llh, *best_x;
    int32_t* best_at;
    PostSelect sel;
    int32_t n_mass;
    int32_t hpd_k[MISTI_POST_MAX_PROBS];                   // post_hpd_window per mass
    uint64_t* ws_sort;
    double* hpd;                     // [S][N][n_mass][2]
    int32_t* hpd_at;                 // [S][N][n_mass]
    double* order;                   // [S][N][m]
    bool sorted() const { return hpd || hpd_at || order; }
};
hipError_t launch_post(const PostArgs& a, hipStream_t stream);

}  // namespace misti
