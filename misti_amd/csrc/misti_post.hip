// Posterior summaries of a chain that is already in HBM (MI355X / gfx950): misti_ens_summary_dev, misti_ensemble_posterior.
//
// Per search: exact order statistics and the quantiles interpolated between them, the mean and the covariance, the integrated
// autocorrelation time of the ensemble-mean series with Sokal's window, and the best sample.  The rule is THE PROJECT'S OWN:
// optimize.ensemble_posterior_rule states it in NumPy and every kernel here restates it operation for operation - one rounding per
// operation, a product that feeds a sum passes through ens_rn().  A search's result is a function of its own chain alone.
//
// Every sum over steps is lsum: 64 partials, partial l = v[l] + v[l + 64] + ... over ceil(count / 64) terms with +0.0 for an absent
// one, then partial[l] += partial[l + stride] for stride 32 ... 1.  Here a partial is a lane of a wave and the fold six shuffles.
//
//   post_mean_kernel    wave = (search, coordinate): the ensemble-mean series e_t, its lsum, and y_t = e_t - mean into the workspace
//   post_cov_kernel     wave = (search, j <= k)
//   post_acf_kernel     workgroup = (search, coordinate), a wave per lag, four lags at a time; a thread walks the window over each
//                       four and the workgroup stops at the first lag that closes it: lags behind the window are never computed
//   post_select_kernel  workgroup = (search, coordinate): most-significant-digit radix select on the order key, 8 passes of 8 bits,
//                       LDS histograms; ranks that still share a prefix share a histogram.  No second buffer, no sort
//   post_best_kernel    workgroup = search
// The only memory beyond the chain is the series y[S][N][n]: 1 / W of the kept chain.
//
// Shortest (HPD) intervals and the sorted marginal itself (optimize.ensemble_hpd_rule) need every order statistic - a full sort per
// (search, coordinate), launched only where hpd, hpd_at or order is asked for:
//   post_sort_tile_kernel  workgroup = (search, tile of POST_SORT_TILE samples; coordinate): the strided chain gathered into keys, once,
//                          and a bitonic network in 16 KiB of LDS - eight workgroups a CU, the wave limit, not LDS, caps residency
//   post_merge_kernel      one pass per doubling of the run length, through the ping-pong pair ws_sort[2][S][N][m] in HBM: a marginal
//                          (32 000 keys = 250 KiB at W = 16, 2 000 steps) does not fit one workgroup's LDS; merge-path cuts per tile
//   post_hpd_kernel        workgroup = (search, coordinate): the window scan per mass with the rule's pair reduction; plain stores
// Consecutive lanes touch consecutive 8-byte keys in the gather's stores, the merge's loads and stores and the scan (a 32-lane half
// covers one 256-byte bank row: no conflict); the network's strides below 32 and the serial merge's data-dependent reads do conflict.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "misti_ens.h"
#include "misti_post.h"

namespace misti {

namespace {

constexpr int POST_THREADS = 256;
constexpr int POST_WAVES = POST_THREADS / POST_LANES;

__device__ __forceinline__ const double* kept(const PostArgs& a, int64_t s) { return a.chain + (s * a.K + a.burn) * a.W * (int64_t)a.N; }

}  // namespace

__global__ __launch_bounds__(POST_LANES)
void post_mean_kernel(PostArgs a) {
    const int64_t s = blockIdx.x;
    const int j = blockIdx.y, l = threadIdx.x, W = a.W, N = a.N;
    const int64_t n = a.n, rows = (n + POST_LANES - 1) / POST_LANES;
    const double* x = kept(a, s) + j;
    double* y = a.ws_y + (s * N + j) * n;
    double acc = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t t = r * POST_LANES + l;
        double v = 0.0;
        if (t < n) {
            const double* p = x + t * W * (int64_t)N;
            double e = p[0];
            for (int w = 1; w < W; ++w) e = e + p[(int64_t)w * N];
            v = e / (double)W;
            y[t] = v;
        }
        acc = r == 0 ? v : acc + v;
    }
    const double mean = post_fold(acc) / (double)n;
    if (l == 0) {
        a.ws_mean[s * N + j] = mean;
        if (a.mean) a.mean[s * N + j] = post_out(mean);
    }
    for (int64_t t = l; t < n; t += POST_LANES) y[t] = y[t] - mean;      // each lane rereads what it wrote
}

__global__ __launch_bounds__(POST_LANES)
void post_cov_kernel(PostArgs a) {
    const int64_t s = blockIdx.x;
    const int l = threadIdx.x, W = a.W, N = a.N;
    int j = 0, k = (int)blockIdx.y;                           // pair index -> j <= k, rows of the upper triangle
    while (k >= N - j) { k -= N - j; ++j; }
    k += j;
    const int64_t n = a.n, rows = (n + POST_LANES - 1) / POST_LANES;
    const double mj = a.ws_mean[s * N + j], mk = a.ws_mean[s * N + k];
    const double* x = kept(a, s);
    double acc = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t t = r * POST_LANES + l;
        double v = 0.0;
        if (t < n) {
            const double* p = x + t * W * (int64_t)N;
            v = ens_rn((p[j] - mj) * (p[k] - mk));
            for (int w = 1; w < W; ++w) v = v + ens_rn((p[(int64_t)w * N + j] - mj) * (p[(int64_t)w * N + k] - mk));
        }
        acc = r == 0 ? v : acc + v;
    }
    const double cv = post_out(post_fold(acc) / (double)(n * W - 1));
    if (l == 0) {
        a.cov[(s * N + j) * N + k] = cv;
        a.cov[(s * N + k) * N + j] = cv;
    }
}

__global__ __launch_bounds__(POST_THREADS)
void post_acf_kernel(PostArgs a) {
    __shared__ double c_blk[POST_WAVES];
    __shared__ int stop;
    const int64_t s = blockIdx.x;
    const int j = blockIdx.y, N = a.N, wave = threadIdx.x / POST_LANES, l = threadIdx.x % POST_LANES;
    const int64_t n = a.n, L = a.L;
    const double* y = a.ws_y + (s * N + j) * n;
    double c0 = 0.0, tau = 1.0;                               // thread 0's: the window scan
    int64_t window = -1;
    for (int64_t k0 = 0; k0 <= L; k0 += POST_WAVES) {
        const int64_t k = k0 + wave;
        if (k <= L) {
            const int64_t cnt = n - k, rows = (cnt + POST_LANES - 1) / POST_LANES;
            double acc = 0.0;
            for (int64_t r = 0; r < rows; ++r) {
                const int64_t t = r * POST_LANES + l;
                const double v = t < cnt ? ens_rn(y[t] * y[t + k]) : 0.0;
                acc = r == 0 ? v : acc + v;
            }
            acc = post_fold(acc);
            if (l == 0) c_blk[wave] = acc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            bool found = false;
            for (int i = 0; i < POST_WAVES && k0 + i <= L && !found; ++i) {
                const int64_t M = k0 + i;
                if (M == 0) {
                    c0 = c_blk[0];
                    if (c0 == 0.0 && L >= 1) { window = 0; found = true; continue; }
                } else {
                    const double rho = c_blk[i] / c0;
                    tau = tau + ens_rn(2.0 * rho);
                }
                if ((double)M >= ens_rn(a.c * tau)) { window = M; found = true; }
            }
            stop = found ? 1 : 0;
        }
        __syncthreads();
        if (stop) break;
    }
    if (threadIdx.x == 0) {
        if (a.tau) a.tau[s * N + j] = post_out(tau < 1.0 ? 1.0 : tau);
        if (a.window) a.window[s * N + j] = (int32_t)window;
    }
}

__global__ __launch_bounds__(POST_THREADS)
void post_select_kernel(PostArgs a) {
    __shared__ uint32_t hist[POST_MAX_RANKS][256];
    __shared__ uint64_t prefix[POST_MAX_RANKS];
    __shared__ uint32_t rem[POST_MAX_RANKS];
    __shared__ int32_t leader[POST_MAX_RANKS];                // the lowest rank with this rank's prefix: its histogram serves both
    const int64_t s = blockIdx.x;
    const int j = blockIdx.y, N = a.N, tid = threadIdx.x, R = a.sel.n_rank;
    const int64_t m = a.n * a.W;
    const double* x = kept(a, s) + j;
    if (tid < R) { prefix[tid] = 0; rem[tid] = (uint32_t)a.sel.rank[tid]; leader[tid] = 0; }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < POST_MAX_RANKS * 256; i += POST_THREADS) (&hist[0][0])[i] = 0;
        __syncthreads();
        for (int64_t idx = tid; idx < m; idx += POST_THREADS) {
            const uint64_t key = post_key((uint64_t)__double_as_longlong(x[idx * N]));
            const uint64_t head = pass ? key >> (shift + 8) : 0;
            for (int r = 0; r < R; ++r)
                if (leader[r] == r && prefix[r] == head) { atomicAdd(&hist[r][(key >> shift) & 255], 1u); break; }
        }
        __syncthreads();
        uint64_t np_ = 0;
        uint32_t nr = 0;
        if (tid < R) {
            const uint32_t* h = hist[leader[tid]];
            const uint32_t want = rem[tid];
            uint32_t below = 0;
            int b = 0;
            for (; b < 255; ++b) {                            // the bucket that holds the wanted rank
                const uint32_t cnt = h[b];
                if (want - below < cnt) break;
                below += cnt;
            }
            np_ = (prefix[tid] << 8) | (uint64_t)b;
            nr = want - below;
        }
        __syncthreads();
        if (tid < R) { prefix[tid] = np_; rem[tid] = nr; }
        __syncthreads();
        if (tid == 0)
            for (int r = 1; r < R; ++r) leader[r] = prefix[r] == prefix[r - 1] ? leader[r - 1] : r;
        __syncthreads();
    }
    if (tid < a.sel.n_prob) {
        const double lo = __longlong_as_double((long long)post_unkey(prefix[a.sel.lo[tid]]));
        double q = lo;
        if (a.sel.hi[tid] != a.sel.lo[tid]) {
            const double hi = __longlong_as_double((long long)post_unkey(prefix[a.sel.hi[tid]]));
            q = lo + ens_rn(a.sel.g[tid] * (hi - lo));
        }
        a.quant[(s * N + j) * a.sel.n_prob + tid] = post_out(q);
    }
}

__global__ __launch_bounds__(POST_THREADS)
void post_best_kernel(PostArgs a) {
    __shared__ double sv[POST_THREADS];
    __shared__ int64_t si[POST_THREADS];
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, N = a.N;
    const int64_t m = a.n * a.W;
    double bv = -INFINITY;
    int64_t bi = -1;
    if (a.chain_llh) {
        const double* v = a.chain_llh + (s * a.llh_K + a.burn) * a.W;
        for (int64_t idx = tid; idx < m; idx += POST_THREADS) {
            const double f = v[idx];
            if (f == f && f != -INFINITY && (bi < 0 || f > bv)) { bv = f; bi = idx; }
        }
    }
    sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int stride = POST_THREADS / 2; stride >= 1; stride >>= 1) {
        if (tid < stride) {
            const double ov = sv[tid + stride];
            const int64_t oi = si[tid + stride];
            if (oi >= 0 && (si[tid] < 0 || ov > sv[tid] || (ov == sv[tid] && oi < si[tid]))) { sv[tid] = ov; si[tid] = oi; }
        }
        __syncthreads();
    }
    bv = sv[0]; bi = si[0];
    if (tid == 0) {
        if (a.best_llh) a.best_llh[s] = bi >= 0 ? bv : -INFINITY;
        if (a.best_at) {
            a.best_at[2 * s] = bi >= 0 ? (int32_t)(bi / a.W) : -1;
            a.best_at[2 * s + 1] = bi >= 0 ? (int32_t)(bi % a.W) : -1;
        }
    }
    if (a.best_x && tid < N)
        a.best_x[s * N + tid] = bi >= 0 ? kept(a, s)[bi * N + tid] : __longlong_as_double(0x7ff8000000000000ll);
}

// ---- the sorted marginals and the shortest intervals (optimize.ensemble_hpd_rule) -----------------------------------------------------
// Keys only: equal keys are equal bits, so no payload travels and stability does not matter.  A marginal lies at
// ws_sort[side][(s N + j) m ...], side 0 or 1.
__device__ __forceinline__ uint64_t* sort_side(const PostArgs& a, int side, int64_t s, int j) {
    const int64_t m = a.n * a.W;
    return a.ws_sort + ((int64_t)side * a.S * a.N + s * a.N + j) * m;
}

// workgroup = (search, tile; coordinate): gathers the tile's keys from the strided chain - the only strided read of the sort - and
// sorts them in LDS by a bitonic network over the next power of two, the absent keys being the largest key.
__global__ __launch_bounds__(POST_THREADS)
void post_sort_tile_kernel(PostArgs a) {
    __shared__ uint64_t key[POST_SORT_TILE];
    const int64_t m = a.n * a.W, tiles = (m + POST_SORT_TILE - 1) / POST_SORT_TILE;
    const int64_t s = blockIdx.x / tiles, first = (blockIdx.x % tiles) * POST_SORT_TILE;
    const int j = blockIdx.y, N = a.N, tid = threadIdx.x;
    const int cnt = (int)(m - first < POST_SORT_TILE ? m - first : POST_SORT_TILE);
    int Tp = 2;
    while (Tp < cnt) Tp <<= 1;
    const double* x = kept(a, s) + j;
    for (int e = tid; e < Tp; e += POST_THREADS)
        key[e] = e < cnt ? post_key((uint64_t)__double_as_longlong(x[(first + e) * N])) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= Tp; k <<= 1)
        for (int h = k >> 1; h > 0; h >>= 1) {
            for (int p = tid; p < Tp / 2; p += POST_THREADS) {
                const int i = ((p & ~(h - 1)) << 1) | (p & (h - 1)), l = i | h;
                const uint64_t u = key[i], v = key[l];
                if ((u > v) == ((i & k) == 0)) { key[i] = v; key[l] = u; }
            }
            __syncthreads();
        }
    uint64_t* out = sort_side(a, 0, s, j) + first;
    for (int e = tid; e < cnt; e += POST_THREADS) out[e] = key[e];
}

// the merge path: how many of the first d keys of merge(A[0 .. la), B[0 .. lb)) come from A; a tie takes A's
template <class P>
__device__ __forceinline__ int64_t merge_split(P A, int64_t la, P B, int64_t lb, int64_t d) {
    int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One merge pass, runs of `width` keys (a multiple of the tile; the last run of a marginal may be short or absent) to runs of twice
// that, from side `src` to the other.  workgroup = (search, a tile of the OUTPUT; coordinate): two searches in HBM cut the piece of
// each run that the tile comes from (together at most a tile), LDS takes them, a thread cuts its POST_SORT_ITEMS outputs out of LDS
// and merges them serially, and the tile leaves through LDS in whole lines.
constexpr int POST_SORT_ITEMS = POST_SORT_TILE / POST_THREADS;

__global__ __launch_bounds__(POST_THREADS)
void post_merge_kernel(PostArgs a, int64_t width, int src) {
    __shared__ uint64_t key[POST_SORT_TILE];
    __shared__ int64_t cut[2];
    const int64_t m = a.n * a.W, tiles = (m + POST_SORT_TILE - 1) / POST_SORT_TILE;
    const int64_t s = blockIdx.x / tiles, first = (blockIdx.x % tiles) * POST_SORT_TILE;
    const int j = blockIdx.y, tid = threadIdx.x;
    const uint64_t* in = sort_side(a, src, s, j);
    uint64_t* out = sort_side(a, src ^ 1, s, j);
    const int64_t start = first / (2 * width) * (2 * width);            // the pair of runs this tile lies in
    const int64_t la = m - start < width ? m - start : width, lb = m - start - la < width ? m - start - la : width;
    const uint64_t *A = in + start, *B = A + la;
    const int64_t d0 = first - start, d1 = d0 + POST_SORT_TILE < la + lb ? d0 + POST_SORT_TILE : la + lb;
    if (tid < 2) cut[tid] = merge_split(A, la, B, lb, tid ? d1 : d0);
    __syncthreads();
    const int64_t a0 = cut[0], b0 = d0 - a0;
    const int na = (int)(cut[1] - a0), total = (int)(d1 - d0), nb = total - na;
    for (int e = tid; e < total; e += POST_THREADS) key[e] = e < na ? A[a0 + e] : B[b0 + (e - na)];
    __syncthreads();
    const uint64_t *sa = key, *sb = key + na;
    const int o = tid * POST_SORT_ITEMS;
    uint64_t r[POST_SORT_ITEMS];
    if (o < total) {
        int ai = (int)merge_split(sa, (int64_t)na, sb, (int64_t)nb, (int64_t)o), bi = o - ai;
#pragma unroll
        for (int q = 0; q < POST_SORT_ITEMS; ++q)
            if (o + q < total) {
                const bool from_a = bi >= nb || (ai < na && sa[ai] <= sb[bi]);
                r[q] = from_a ? sa[ai] : sb[bi];
                ai += from_a ? 1 : 0; bi += from_a ? 0 : 1;
            }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < POST_SORT_ITEMS; ++q)
        if (o + q < total) key[o + q] = r[q];
    __syncthreads();
    for (int e = tid; e < total; e += POST_THREADS) out[first + e] = key[e];
}

// the rule's order on (isnan(w), w, i): does window (wa, ia) come before window (wb, ib)?  A total order, so the reduction below and
// the rule's walk over i agree: any number before a NaN, the narrower before the wider, the lower i before the higher.
__device__ __forceinline__ bool hpd_before(double wa, int64_t ia, double wb, int64_t ib) {
    const bool na = wa != wa, nb = wb != wb;
    if (na != nb) return nb;
    if (!na && wa != wb) return wa < wb;
    return ia < ib;
}

// workgroup = (search, coordinate), on the sorted marginal: `order`, and per mass the window scan - w_i = x_(i+k-1) - x_(i), one
// rounded subtraction - with the pair reduction; hpd copies the two samples' bits.
__global__ __launch_bounds__(POST_THREADS)
void post_hpd_kernel(PostArgs a, int side) {
    __shared__ double sw[POST_THREADS];
    __shared__ int64_t si[POST_THREADS];
    const int64_t s = blockIdx.x, m = a.n * a.W;
    const int j = blockIdx.y, N = a.N, tid = threadIdx.x;
    const uint64_t* key = sort_side(a, side, s, j);
    if (a.order) {
        long long* o = reinterpret_cast<long long*>(a.order) + (s * N + j) * m;
        for (int64_t i = tid; i < m; i += POST_THREADS) o[i] = (long long)post_unkey(key[i]);
    }
    if (!a.hpd && !a.hpd_at) return;
    for (int q = 0; q < a.n_mass; ++q) {
        const int64_t k = a.hpd_k[q], count = m - k + 1;
        double bw = 0.0;
        int64_t bi = -1;                                      // none yet
        for (int64_t i = tid; i < count; i += POST_THREADS) {
            const double lo = __longlong_as_double((long long)post_unkey(key[i])), hi = __longlong_as_double((long long)post_unkey(key[i + k - 1]));
            const double w = hi - lo;
            if (bi < 0 || hpd_before(w, i, bw, bi)) { bw = w; bi = i; }
        }
        sw[tid] = bw; si[tid] = bi;
        __syncthreads();
        for (int stride = POST_THREADS / 2; stride >= 1; stride >>= 1) {
            if (tid < stride) {
                const double ow = sw[tid + stride];
                const int64_t oi = si[tid + stride];
                if (oi >= 0 && (si[tid] < 0 || hpd_before(ow, oi, sw[tid], si[tid]))) { sw[tid] = ow; si[tid] = oi; }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int64_t at = si[0], slot = (s * N + j) * a.n_mass + q;
            if (a.hpd) {
                long long* h = reinterpret_cast<long long*>(a.hpd) + 2 * slot;
                h[0] = (long long)post_unkey(key[at]);
                h[1] = (long long)post_unkey(key[at + k - 1]);
            }
            if (a.hpd_at) a.hpd_at[slot] = (int32_t)at;
        }
        __syncthreads();
    }
}

hipError_t launch_post(const PostArgs& a, hipStream_t stream) {
    const dim3 per_coord((unsigned)a.S, (unsigned)a.N);             // searches along x: the axis without a 65535 limit
    const bool series = a.mean || a.cov || a.tau || a.window;
    if (series) hipLaunchKernelGGL(post_mean_kernel, per_coord, dim3(POST_LANES), 0, stream, a);
    if (a.cov) hipLaunchKernelGGL(post_cov_kernel, dim3((unsigned)a.S, (unsigned)(a.N * (a.N + 1) / 2)), dim3(POST_LANES), 0, stream, a);
    if (a.tau || a.window) hipLaunchKernelGGL(post_acf_kernel, per_coord, dim3(POST_THREADS), 0, stream, a);
    if (a.quant) hipLaunchKernelGGL(post_select_kernel, per_coord, dim3(POST_THREADS), 0, stream, a);
    if (a.best_llh || a.best_x || a.best_at) hipLaunchKernelGGL(post_best_kernel, dim3((unsigned)a.S), dim3(POST_THREADS), 0, stream, a);
    if (a.sorted()) {
        const int64_t m = a.n * a.W, tiles = (m + POST_SORT_TILE - 1) / POST_SORT_TILE;
        if (a.S * tiles > INT32_MAX) return hipErrorInvalidValue;
        const dim3 per_tile((unsigned)(a.S * tiles), (unsigned)a.N);
        hipLaunchKernelGGL(post_sort_tile_kernel, per_tile, dim3(POST_THREADS), 0, stream, a);
        int side = 0;
        for (int64_t width = POST_SORT_TILE; width < m; width *= 2, side ^= 1)
            hipLaunchKernelGGL(post_merge_kernel, per_tile, dim3(POST_THREADS), 0, stream, a, width, side);
        hipLaunchKernelGGL(post_hpd_kernel, per_coord, dim3(POST_THREADS), 0, stream, a, side);
    }
    return hipGetLastError();
}

}  // namespace misti
