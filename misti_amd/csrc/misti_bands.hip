// Trajectory bands (MI355X / gfx950): misti_traj_bands_dev, misti_traj_bands.  Per group, interval of the common grid and population
// the members among m samples of the corrected coalescence rates lc, their count, quantiles, mean and extremes.  The rule is THE
// PROJECT'S OWN: optimize.trajectory_bands_rule states it in NumPy and every kernel here restates it operation for operation - one
// rounding per operation, a product that feeds a sum passes through ens_rn().  A series' result is a function of its own samples alone.
//
//   bands_gather_kernel  workgroup = (group, tile of 64 samples; tile of 64 columns): a sample's lc is 2 (numT + 1) contiguous doubles,
//                        a series wants its m samples contiguous - THE transpose of the feature.  Lanes run along the columns for the
//                        loads (512 bytes of one sample per wave) and along the samples for the stores (512 bytes of one series per
//                        wave); in between the keys cross LDS in a tile padded to 65 words of 8 bytes: a half-wave's 32 lanes then
//                        touch 32 distinct bank pairs on either side.  A value becomes post_key(bits), a non-member ~0ull: behind
//                        every real key, so a sorted series is its members and then nothing
//   bands_sort_kernel    workgroup = (series, tile of POST_SORT_TILE keys): a bitonic network in 16 KiB of LDS, in place on side 0
//   bands_merge_kernel   one pass per doubling of the run length, through the ping-pong pair in HBM, merge-path cuts per output tile:
//                        misti_post.hip's merge on a series view (base, length, count of series) in place of a chain
//   bands_select_kernel  wave = series: n is the first ~0ull by binary search - no atomics, no counter buffer -, the ranks come from n
//                        in double arithmetic as the rule states them, the mean is lsum over the sorted members (a partial is a lane,
//                        the fold post_fold); plain vector stores
// Series lie on blockIdx.x, the axis without a 65 535 limit.  The only memory that scales with m is the ping-pong pair.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "misti_bands.h"
#include "misti_ens.h"
#include "misti_post.h"

namespace misti {

namespace {

constexpr int BANDS_THREADS = 256;
constexpr int BANDS_SORT_ITEMS = POST_SORT_TILE / BANDS_THREADS;

__device__ __forceinline__ uint64_t* bands_side(const BandsArgs& a, int side, int64_t series) {
    return a.ws + ((int64_t)side * a.G * 2 * a.numT + series) * a.m;
}

__device__ __forceinline__ double bands_value(uint64_t key) { return __longlong_as_double((long long)post_unkey(key)); }

// the merge path: how many of the first d keys of merge(A[0 .. la), B[0 .. lb)) come from A; a tie takes A's
template <class P>
__device__ __forceinline__ int64_t bands_cut(P A, int64_t la, P B, int64_t lb, int64_t d) {
    int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(BANDS_THREADS)
void bands_gather_kernel(BandsArgs a) {
    __shared__ uint64_t tile[BANDS_TILE][BANDS_TILE + 1];
    const int64_t m = a.m, s_tiles = (m + BANDS_TILE - 1) / BANDS_TILE;
    const int64_t g = blockIdx.x / s_tiles, s0 = (blockIdx.x % s_tiles) * BANDS_TILE;
    const int C = 2 * a.numT, row = 2 * (a.numT + 1), c0 = blockIdx.y * BANDS_TILE;
    const int lane = threadIdx.x % BANDS_TILE, first = threadIdx.x / BANDS_TILE;
    constexpr int STEP = BANDS_THREADS / BANDS_TILE;
    // loads: lane = column, so a wave reads 512 contiguous bytes of one sample
    for (int r = first; r < BANDS_TILE; r += STEP) {
        const int64_t s = s0 + r;
        const int c = c0 + lane;
        uint64_t key = ~0ull;
        if (s < m && c < C) {
            const int64_t i = g * m + s;
            const double v = a.lc[i * row + c];
            const bool ok = a.status ? a.status[i] == MISTI_OK : true;
            if (ok && (double)(c >> 1) < a.split[i] && v == v) key = post_key((uint64_t)__double_as_longlong(v));
        }
        tile[r][lane] = key;
    }
    __syncthreads();
    // stores: lane = sample, so a wave writes 512 contiguous bytes of one series
    for (int r = first; r < BANDS_TILE; r += STEP) {
        const int c = c0 + r;
        const int64_t s = s0 + lane;
        if (s < m && c < C) bands_side(a, 0, g * C + c)[s] = tile[lane][r];
    }
}

__global__ __launch_bounds__(BANDS_THREADS)
void bands_sort_kernel(BandsArgs a) {
    __shared__ uint64_t key[POST_SORT_TILE];
    const int64_t m = a.m, tiles = (m + POST_SORT_TILE - 1) / POST_SORT_TILE;
    const int64_t series = blockIdx.x / tiles, first = (blockIdx.x % tiles) * POST_SORT_TILE;
    const int tid = threadIdx.x;
    const int cnt = (int)(m - first < POST_SORT_TILE ? m - first : POST_SORT_TILE);
    int Tp = 2;
    while (Tp < cnt) Tp <<= 1;
    uint64_t* x = bands_side(a, 0, series) + first;
    for (int e = tid; e < Tp; e += BANDS_THREADS) key[e] = e < cnt ? x[e] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= Tp; k <<= 1)
        for (int h = k >> 1; h > 0; h >>= 1) {
            for (int p = tid; p < Tp / 2; p += BANDS_THREADS) {
                const int i = ((p & ~(h - 1)) << 1) | (p & (h - 1)), l = i | h;
                const uint64_t u = key[i], v = key[l];
                if ((u > v) == ((i & k) == 0)) { key[i] = v; key[l] = u; }
            }
            __syncthreads();
        }
    for (int e = tid; e < cnt; e += BANDS_THREADS) x[e] = key[e];
}

// One merge pass, runs of `width` keys (a multiple of the tile; the last run of a series may be short or absent) to runs of twice that,
// from side `src` to the other.  workgroup = (series, a tile of the OUTPUT).
__global__ __launch_bounds__(BANDS_THREADS)
void bands_merge_kernel(BandsArgs a, int64_t width, int src) {
    __shared__ uint64_t key[POST_SORT_TILE];
    __shared__ int64_t cut[2];
    const int64_t m = a.m, tiles = (m + POST_SORT_TILE - 1) / POST_SORT_TILE;
    const int64_t series = blockIdx.x / tiles, first = (blockIdx.x % tiles) * POST_SORT_TILE;
    const int tid = threadIdx.x;
    const uint64_t* in = bands_side(a, src, series);
    uint64_t* out = bands_side(a, src ^ 1, series);
    const int64_t start = first / (2 * width) * (2 * width);            // the pair of runs this tile lies in
    const int64_t la = m - start < width ? m - start : width, lb = m - start - la < width ? m - start - la : width;
    const uint64_t *A = in + start, *B = A + la;
    const int64_t d0 = first - start, d1 = d0 + POST_SORT_TILE < la + lb ? d0 + POST_SORT_TILE : la + lb;
    if (tid < 2) cut[tid] = bands_cut(A, la, B, lb, tid ? d1 : d0);
    __syncthreads();
    const int64_t a0 = cut[0], b0 = d0 - a0;
    const int na = (int)(cut[1] - a0), total = (int)(d1 - d0), nb = total - na;
    for (int e = tid; e < total; e += BANDS_THREADS) key[e] = e < na ? A[a0 + e] : B[b0 + (e - na)];
    __syncthreads();
    const uint64_t *sa = key, *sb = key + na;
    const int o = tid * BANDS_SORT_ITEMS;
    uint64_t r[BANDS_SORT_ITEMS];
    if (o < total) {
        int ai = (int)bands_cut(sa, (int64_t)na, sb, (int64_t)nb, (int64_t)o), bi = o - ai;
#pragma unroll
        for (int q = 0; q < BANDS_SORT_ITEMS; ++q)
            if (o + q < total) {
                const bool from_a = bi >= nb || (ai < na && sa[ai] <= sb[bi]);
                r[q] = from_a ? sa[ai] : sb[bi];
                ai += from_a ? 1 : 0; bi += from_a ? 0 : 1;
            }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BANDS_SORT_ITEMS; ++q)
        if (o + q < total) key[o + q] = r[q];
    __syncthreads();
    for (int e = tid; e < total; e += BANDS_THREADS) out[first + e] = key[e];
}

// wave = series, on the sorted keys
__global__ __launch_bounds__(POST_LANES)
void bands_select_kernel(BandsArgs a, int side) {
    const int64_t series = blockIdx.x, m = a.m;
    const int l = threadIdx.x;
    const uint64_t* key = bands_side(a, side, series);
    int64_t n = 0, end = m;                                   // the first ~0ull: every lane runs the same search
    while (n < end) {
        const int64_t mid = (n + end) >> 1;
        if (key[mid] != ~0ull) n = mid + 1; else end = mid;
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (a.count && l == 0) a.count[series] = (int32_t)n;
    if (a.lo && l == 0) a.lo[series] = n ? bands_value(key[0]) : qnan;
    if (a.hi && l == 0) a.hi[series] = n ? bands_value(key[n - 1]) : qnan;
    if (a.quant && l < a.n_prob) {
        double q = qnan;
        if (n) {
            int64_t lo, hi;
            double g;
            bands_rank(n, a.probs[l], &lo, &hi, &g);
            const double x0 = bands_value(key[lo]);
            q = x0;
            if (hi != lo) q = x0 + ens_rn(g * (bands_value(key[hi]) - x0));
        }
        a.quant[series * a.n_prob + l] = post_out(q);
    }
    if (a.mean) {
        const int64_t rows = (n + POST_LANES - 1) / POST_LANES;
        double acc = 0.0;
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t t = r * POST_LANES + l;
            const double v = t < n ? bands_value(key[t]) : 0.0;
            acc = r == 0 ? v : acc + v;
        }
        const double sum = post_fold(acc);
        const double mean = n ? sum / (double)n : qnan;
        if (l == 0) a.mean[series] = post_out(mean);
    }
}

hipError_t launch_bands(const BandsArgs& a, hipStream_t stream) {
    const int64_t C = 2 * (int64_t)a.numT, series = a.G * C;
    const int64_t s_tiles = (a.m + BANDS_TILE - 1) / BANDS_TILE, tiles = (a.m + POST_SORT_TILE - 1) / POST_SORT_TILE;
    if (a.G * s_tiles > INT32_MAX || series * tiles > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bands_gather_kernel, dim3((unsigned)(a.G * s_tiles), (unsigned)((C + BANDS_TILE - 1) / BANDS_TILE)), dim3(BANDS_THREADS), 0, stream, a);
    hipLaunchKernelGGL(bands_sort_kernel, dim3((unsigned)(series * tiles)), dim3(BANDS_THREADS), 0, stream, a);
    int side = 0;
    for (int64_t width = POST_SORT_TILE; width < a.m; width *= 2, side ^= 1)
        hipLaunchKernelGGL(bands_merge_kernel, dim3((unsigned)(series * tiles)), dim3(BANDS_THREADS), 0, stream, a, width, side);
    hipLaunchKernelGGL(bands_select_kernel, dim3((unsigned)series), dim3(POST_LANES), 0, stream, a, side);
    return hipGetLastError();
}

}  // namespace misti
