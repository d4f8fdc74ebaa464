// Parametric bootstrap on the device (include/misti_hip.h, "parametric bootstrap"): replicate rows drawn from a spectrum, the sites of
// one replicate spread over lanes and workgroups.  The rule is optimize.parametric_rows, restated here in integers (misti_parametric.h):
// the same thresholds, the same stream, counts that are integer sums - the same bits whatever the launch geometry.
//
// Geometry (param_blocks_per_rep, what misti_parametric_geometry returns): a replicate of n_sites sites is ceil(n_sites / 4) Philox
// blocks.  blocks_per_rep = min(ceil(PARAM_TARGET_WORKGROUPS / n_rep), ceil(Philox blocks / (256 PARAM_MIN_BLOCKS_PER_LANE))), at least
// 1: one workgroup per replicate once the replicates alone fill the device (n_rep >= PARAM_TARGET_WORKGROUPS = 8 192: four rounds of
// 8 workgroups on each of 256 compute units), more for few replicates of many sites, and never so many that a lane is left with fewer
// than PARAM_MIN_BLOCKS_PER_LANE = 16 Philox blocks (below that a workgroup's thresholds and reduction are no longer small beside
// its draws).  A function of (n_sites, n_rep) alone - not of the device.
#include <hip/hip_runtime.h>

#include <cmath>

#include "misti_ctx.h"
#include "misti_parametric.h"
#include "misti_score.h"

namespace misti {

constexpr int PARAM_THREADS = 256;                    // lanes of a workgroup of the count kernel
constexpr int PARAM_UNROLL = 4;                       // independent Philox blocks per iteration of a lane
constexpr int PARAM_MIN_BLOCKS_PER_LANE = 16;
constexpr int64_t PARAM_TARGET_WORKGROUPS = 8192;
constexpr int64_t PARAM_SLICE = 65535;                // replicates per launch: the grid's second dimension

static inline int64_t param_blocks_per_rep(int64_t n_sites, int64_t n_rep) {
    const int64_t philox = (n_sites + 3) / 4, per_wg = (int64_t)PARAM_THREADS * PARAM_MIN_BLOCKS_PER_LANE;
    const int64_t useful = (philox + per_wg - 1) / per_wg;
    const int64_t wanted = n_rep > 0 ? (PARAM_TARGET_WORKGROUPS + n_rep - 1) / n_rep : PARAM_TARGET_WORKGROUPS;
    const int64_t b = wanted < useful ? wanted : useful;
    return b < 1 ? 1 : b;
}

// The spectrum replicate r draws from, as thresholds: false (T all zero) where its index is outside 0 ... n_spec - 1, where its
// status says it has no value (status_has_value, the scorer's predicate), or where param_thresholds refuses it.
__device__ __forceinline__ bool param_spectrum(int64_t n_spec, const double* __restrict__ spectra, const int32_t* __restrict__ status,
                                               const int32_t* __restrict__ spec_of, int64_t r, uint64_t T[6]) {
    const int64_t s = spec_of ? (int64_t)spec_of[r] : 0;
    const bool known = s >= 0 && s < n_spec && !(status && !status_has_value(status[s]));
    if (!known) {
#pragma unroll
        for (int k = 0; k < 6; ++k) T[k] = 0;
        return false;
    }
    return param_thresholds(spectra + s * 7, T);
}

__device__ __forceinline__ uint64_t param_uniform(uint64_t v) {      // a value every lane holds, moved to scalar registers
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// g[k] += [u >= T[k]] for the first `valid` values of one Philox block: six compare-and-adds a draw, no indexed registers.
template <int VALID> __device__ __forceinline__ void param_count(const uint64_t raw[4], const uint64_t T[6], uint32_t g[6]) {
#pragma unroll
    for (int j = 0; j < VALID; ++j) {
        const uint64_t u = param_u(raw[j]);
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] += u >= T[k] ? 1u : 0u;
    }
}

// Grid (blocks_per_rep, replicates of this slice), 256 lanes.  Lane t of workgroup b takes the Philox blocks b 256 + t + i (256
// blocks_per_rep), i = 0, 1, ...: PARAM_UNROLL of them per iteration while that many whole blocks are left (ten rounds of 64-bit mulhi
// are one long dependent chain and nothing here waits for memory - independent chains and occupancy are what hides it), then one at a
// time, the last block of the replicate counting only the draws below n_sites.  A lane makes at most 2^36 / 256 draws: its six 32-bit
// counters cannot overflow; from the wave's sum on everything is 64-bit.  The workgroup's six totals are added to totals[r][0..6)
// (zeroed by the host) with 64-bit atomics: integer sums, independent of order and geometry.  A replicate without a usable spectrum
// adds nothing.  The launch bound asks for 8 waves a SIMD (at most 64 VGPRs): occupancy is half of what hides the multiply chain.
__global__ __launch_bounds__(PARAM_THREADS, 8)
void parametric_count_kernel(int64_t n_spec, const double* __restrict__ spectra, const int32_t* __restrict__ status,
                             const int32_t* __restrict__ spec_of, int64_t n_sites, uint64_t seed, int64_t first_rep,
                             unsigned long long* __restrict__ totals) {
    __shared__ uint64_t s_T[6];
    __shared__ int s_ok;
    __shared__ unsigned long long s_part[PARAM_THREADS / 64][6];
    const int64_t r = blockIdx.y;
    if (threadIdx.x == 0) {
        uint64_t T[6];
        s_ok = param_spectrum(n_spec, spectra, status, spec_of, r, T) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s_T[k] = T[k];
    }
    __syncthreads();
    if (!s_ok) return;                                // (the whole workgroup)
    uint64_t T[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) T[k] = param_uniform(s_T[k]);
    const uint64_t rep = (uint64_t)(first_rep + r);
    const uint64_t whole = (uint64_t)n_sites >> 2;                    // Philox blocks of which every draw counts
    const int rest = (int)(n_sites & 3);                               // draws of the block behind them
    const uint64_t stride = (uint64_t)PARAM_THREADS * gridDim.x;
    uint64_t block = (uint64_t)blockIdx.x * PARAM_THREADS + threadIdx.x;
    uint32_t g[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (; block + (PARAM_UNROLL - 1) * stride < whole; block += PARAM_UNROLL * stride) {
        uint64_t raw[PARAM_UNROLL][4];
#pragma unroll
        for (int i = 0; i < PARAM_UNROLL; ++i) philox4x64_10_block(seed, rep, block + i * stride, raw[i]);
#pragma unroll
        for (int i = 0; i < PARAM_UNROLL; ++i) param_count<4>(raw[i], T, g);
    }
    for (; block < whole; block += stride) {
        uint64_t raw[4];
        philox4x64_10_block(seed, rep, block, raw);
        param_count<4>(raw, T, g);
    }
    if (block == whole && rest) {                     // the lane the partial block falls to
        uint64_t raw[4];
        philox4x64_10_block(seed, rep, block, raw);
        if (rest == 1) param_count<1>(raw, T, g);
        else if (rest == 2) param_count<2>(raw, T, g);
        else param_count<3>(raw, T, g);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        unsigned long long v = g[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < PARAM_THREADS / 64; ++w) v += s_part[w][threadIdx.x];
        if (v) atomicAdd(&totals[r * 6 + threadIdx.x], v);
    }
}

// One lane per replicate: the six totals g_k = #{j : u_j >= T_k} become the row [genome, n_sites - g0, g0 - g1, ..., g4 - g5, g5] and
// the status.  A replicate without a usable spectrum gets [genome, 0 x 7] and status 1.
__global__ __launch_bounds__(256)
void parametric_finish_kernel(int64_t n_spec, const double* __restrict__ spectra, const int32_t* __restrict__ status,
                              const int32_t* __restrict__ spec_of, double genome, int64_t n_sites, int64_t n_rep,
                              const unsigned long long* __restrict__ totals, double* __restrict__ rows, int32_t* __restrict__ row_status) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rep) return;
    uint64_t T[6];
    const bool ok = param_spectrum(n_spec, spectra, status, spec_of, r, T);
    unsigned long long g[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = totals[r * 6 + k];
    double* row = rows + r * 8;
    row[0] = genome;
    row[1] = ok ? (double)((unsigned long long)n_sites - g[0]) : 0.0;
#pragma unroll
    for (int k = 1; k < 6; ++k) row[1 + k] = ok ? (double)(g[k - 1] - g[k]) : 0.0;
    row[7] = ok ? (double)g[5] : 0.0;
    if (row_status) row_status[r] = ok ? 0 : 1;
}

}  // namespace misti

using namespace misti_host;

extern "C" {

int misti_parametric_rows_dev(misti_ctx* c, int64_t n_spec, const double* d_spectra, const int32_t* d_status, const int32_t* d_spec_of,
                              double genome, int64_t n_sites, uint64_t seed, int64_t first_rep, int64_t n_rep, double* d_rows,
                              int32_t* d_row_status) {
    // everything that can be said about the arguments is said before the context is looked at
    if (n_spec < 1) return fail(MISTI_E_ARG, "n_spec must be at least 1 (got %lld)", (long long)n_spec);
    if (n_sites < 0 || n_rep < 0 || first_rep < 0) return fail(MISTI_E_ARG, "negative n_sites, n_rep or first_rep");
    if (!std::isfinite(genome)) return fail(MISTI_E_ARG, "genome is not finite");
    if (n_sites > MISTI_PARAM_MAX_SITES) return fail(MISTI_E_LIMIT, "n_sites beyond MISTI_PARAM_MAX_SITES = 2^36 (got %lld)", (long long)n_sites);
    if (n_rep > INT32_MAX || first_rep > INT64_MAX - n_rep) return fail(MISTI_E_LIMIT, "too many replicates for one call");
    if (n_rep > 0 && (!d_spectra || !d_rows)) return fail(MISTI_E_ARG, "spectra / rows is NULL");
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_rep == 0) return 0;
    const int64_t slice = n_rep < misti::PARAM_SLICE ? n_rep : misti::PARAM_SLICE;
    const size_t bytes = (size_t)slice * 6 * sizeof(unsigned long long);
    // (a buffer that grows frees the old one, which waits for the device: no kernel of an earlier call still adds to it)
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->param_totals.reserve(bytes));
    hipStream_t s = c->stream;
    unsigned long long* totals = c->param_totals.as<unsigned long long>();
    const unsigned bpr = (unsigned)misti::param_blocks_per_rep(n_sites, n_rep);
    // slices of at most 65 535 replicates, one behind the other on the stream: each zeroes the counts, counts, and writes its rows
    for (int64_t r0 = 0; r0 < n_rep; r0 += misti::PARAM_SLICE) {
        const int64_t n = n_rep - r0 < misti::PARAM_SLICE ? n_rep - r0 : misti::PARAM_SLICE;
        const int32_t* spec_of = d_spec_of ? d_spec_of + r0 : nullptr;
        hipError_t e = hipMemsetAsync(totals, 0, (size_t)n * 6 * sizeof(unsigned long long), s);
        if (e != hipSuccess) return fail(MISTI_E_HIP, "hipMemsetAsync of the draw counts: %s", hipGetErrorString(e));
        if (n_sites > 0)
            hipLaunchKernelGGL(misti::parametric_count_kernel, dim3(bpr, (unsigned)n), dim3(misti::PARAM_THREADS), 0, s, n_spec, d_spectra, d_status,
                               spec_of, n_sites, seed, first_rep + r0, totals);
        hipLaunchKernelGGL(misti::parametric_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_spec, d_spectra, d_status, spec_of,
                           genome, n_sites, n, totals, d_rows + r0 * 8, d_row_status ? d_row_status + r0 : nullptr);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(MISTI_E_HIP, "parametric_count_kernel / parametric_finish_kernel: %s", hipGetErrorString(e));
    }
    return 0;
}

int misti_parametric_thresholds(const double p[7], uint64_t T[6]) {
    if (!p || !T) return fail(MISTI_E_ARG, "p / T is NULL");
    return misti::param_thresholds(p, T) ? 0 : 1;
}

int misti_parametric_counts(const double p[7], int64_t n_sites, uint64_t seed, int64_t rep, int64_t counts[7]) {
    if (n_sites < 0 || rep < 0) return fail(MISTI_E_ARG, "negative n_sites or rep");
    if (n_sites > MISTI_PARAM_MAX_SITES) return fail(MISTI_E_LIMIT, "n_sites beyond MISTI_PARAM_MAX_SITES = 2^36 (got %lld)", (long long)n_sites);
    if (!p || !counts) return fail(MISTI_E_ARG, "p / counts is NULL");
    for (int k = 0; k < 7; ++k) counts[k] = 0;
    uint64_t T[6];
    if (!misti::param_thresholds(p, T)) return 1;
    for (int64_t j = 0; j < n_sites; j += 4) {
        uint64_t raw[4];
        misti::philox4x64_10_block(seed, (uint64_t)rep, (uint64_t)(j >> 2), raw);
        for (int i = 0; i < 4 && j + i < n_sites; ++i) ++counts[misti::param_class(misti::param_u(raw[i]), T)];
    }
    return 0;
}

int misti_parametric_geometry(int64_t n_sites, int64_t n_rep, int32_t* blocks_per_rep) {
    if (n_sites < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative n_sites or n_rep");
    if (n_sites > MISTI_PARAM_MAX_SITES || n_rep > INT32_MAX) return fail(MISTI_E_LIMIT, "n_sites beyond MISTI_PARAM_MAX_SITES = 2^36 or n_rep beyond INT32_MAX");
    if (!blocks_per_rep) return fail(MISTI_E_ARG, "blocks_per_rep is NULL");
    *blocks_per_rep = (int32_t)misti::param_blocks_per_rep(n_sites, n_rep);
    return 0;
}

}  // extern "C"
