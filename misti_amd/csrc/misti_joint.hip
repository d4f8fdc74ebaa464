// Joint credible regions of coordinate pairs of a chain that is already in HBM (MI355X / gfx950): misti_ens_joint_dev and the two
// sampling doors that end in it.
//
// Per search and pair of coordinates: a two-dimensional histogram of the kept samples, its mode, and per mass the count level whose
// cells enclose that mass.  The rule is THE PROJECT'S OWN: optimize.ensemble_joint_rule states it in NumPy.  Everything behind the
// bin of a sample is integer arithmetic, so neither the order of the atomics nor the launch geometry can show in a result.
//
//   joint_range_kernel  workgroup = (search, a coordinate that occurs in a pair), only where the ranges are taken from the data: the
//                       smallest and largest order key over the finite kept samples, reduced through LDS; plain stores to every
//                       pair axis that reads the coordinate
//   joint_hist_kernel   workgroup = (search, slab of JOINT_SLAB samples; pair): the Ba x Bb cells in dynamic LDS - the call's largest
//                       pair sets the size, 4 KiB at 32 x 32, the 64 KiB a workgroup may have at 128 x 128 -, integer LDS atomics;
//                       one slab: the cells leave by plain stores; more: counts is zeroed in front of the launch and the non-empty
//                       cells are added with integer global atomics.  The two coordinates are read with stride N; the pairs of a
//                       search read the same lines at the same time (post_select_kernel's argument)
//   joint_level_kernel  workgroup = (search, pair): the cells in registers (64 a thread at full size - no LDS beyond the reductions'),
//                       inside, the mode as a maximum of (count, -cell), and per mass a bisection on the count, at most 31 steps of
//                       one block sum each; plain stores
// LDS atomics of a wave on one cell serialise (a chain that sits in five cells): exact, and no slower than the loads they follow at
// W N doubles a step.  Consecutive lanes zero and store consecutive 4-byte cells: no bank conflict outside the atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "misti_joint.h"
#include "misti_post.h"

namespace misti {

namespace {

constexpr int JOINT_THREADS = 256;
constexpr int JOINT_WAVES = JOINT_THREADS / POST_LANES;
constexpr int JOINT_PER_THREAD = JOINT_MAX_CELLS / JOINT_THREADS;      // 64 cells of a full pair in a thread's registers

__device__ __forceinline__ const double* kept(const JointArgs& a, int64_t s) { return a.chain + (s * a.K + a.burn) * a.W * (int64_t)a.N; }

// the sum of v over the workgroup, in every thread; part: JOINT_WAVES words of LDS
__device__ __forceinline__ int32_t block_sum(int32_t v, int32_t* part) {
#pragma unroll
    for (int stride = POST_LANES / 2; stride >= 1; stride >>= 1) v += __shfl_down(v, stride, POST_LANES);
    if (threadIdx.x % POST_LANES == 0) part[threadIdx.x / POST_LANES] = v;
    __syncthreads();
    int32_t total = 0;
#pragma unroll
    for (int w = 0; w < JOINT_WAVES; ++w) total += part[w];
    __syncthreads();                                          // part is free again
    return total;
}

}  // namespace

__global__ __launch_bounds__(JOINT_THREADS)
void joint_range_kernel(JointArgs a) {
    __shared__ uint64_t smin[JOINT_THREADS], smax[JOINT_THREADS];
    const int64_t s = blockIdx.x, m = a.n * a.W;
    const int c = a.coord[blockIdx.y], N = a.N, tid = threadIdx.x;
    const double* x = kept(a, s) + c;
    uint64_t kmin = ~0ull, kmax = 0;                          // min above max: no finite sample yet
    for (int64_t idx = tid; idx < m; idx += JOINT_THREADS) {
        const uint64_t bits = (uint64_t)__double_as_longlong(x[idx * N]);
        if ((bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) continue;      // an infinity or a NaN
        const uint64_t key = post_key(bits);
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
    }
    smin[tid] = kmin; smax[tid] = kmax;
    __syncthreads();
    for (int stride = JOINT_THREADS / 2; stride >= 1; stride >>= 1) {
        if (tid < stride) {
            if (smin[tid + stride] < smin[tid]) smin[tid] = smin[tid + stride];
            if (smax[tid + stride] > smax[tid]) smax[tid] = smax[tid + stride];
        }
        __syncthreads();
    }
    kmin = smin[0]; kmax = smax[0];
    const bool any = kmin <= kmax;
    const long long lo = any ? (long long)post_unkey(kmin) : 0x7ff8000000000000ll, hi = any ? (long long)post_unkey(kmax) : 0x7ff8000000000000ll;
    long long* out = reinterpret_cast<long long*>(a.from_data) + s * a.n_pair * 4;
    for (int e = tid; e < 2 * a.n_pair; e += JOINT_THREADS)  // every pair axis that reads this coordinate
        if (((e & 1) ? a.b[e >> 1] : a.a[e >> 1]) == c) { out[2 * e] = lo; out[2 * e + 1] = hi; }
}

extern __shared__ int32_t joint_cells[];

__global__ __launch_bounds__(JOINT_THREADS)
void joint_hist_kernel(JointArgs a) {
    const int64_t s = blockIdx.x / a.slabs, m = a.n * a.W, first = (int64_t)(blockIdx.x % a.slabs) * JOINT_SLAB;
    const int64_t last = first + JOINT_SLAB < m ? first + JOINT_SLAB : m;
    const int q = blockIdx.y, N = a.N, tid = threadIdx.x, ca = a.a[q], cb = a.b[q], Ba = a.Ba[q], Bb = a.Bb[q], cells = Ba * Bb;
    for (int i = tid; i < cells; i += JOINT_THREADS) joint_cells[i] = 0;
    __syncthreads();
    const double* w = a.window + (s * a.n_pair + q) * 4;
    const double lo_a = w[0], hi_a = w[1], lo_b = w[2], hi_b = w[3];
    const double scale_a = (double)Ba / (hi_a - lo_a), scale_b = (double)Bb / (hi_b - lo_b);
    const double* x = kept(a, s);
    for (int64_t idx = first + tid; idx < last; idx += JOINT_THREADS) {
        const double xa = x[idx * N + ca], xb = x[idx * N + cb];
        if (lo_a <= xa && xa <= hi_a && lo_b <= xb && xb <= hi_b)
            atomicAdd(&joint_cells[joint_bin(xa, lo_a, scale_a, Ba) * Bb + joint_bin(xb, lo_b, scale_b, Bb)], 1);
    }
    __syncthreads();
    int32_t* out = a.counts + s * a.cells + a.off[q];
    if (a.slabs == 1) {
        for (int i = tid; i < cells; i += JOINT_THREADS) out[i] = joint_cells[i];
    } else {
        for (int i = tid; i < cells; i += JOINT_THREADS)
            if (joint_cells[i]) atomicAdd(&out[i], joint_cells[i]);
    }
}

__global__ __launch_bounds__(JOINT_THREADS)
void joint_level_kernel(JointArgs a) {
    __shared__ int32_t part[JOINT_WAVES];
    __shared__ uint64_t best[JOINT_THREADS];
    const int64_t s = blockIdx.x;
    const int q = blockIdx.y, tid = threadIdx.x, Bb = a.Bb[q], cells = a.Ba[q] * Bb;
    const int32_t* cnt = a.counts + s * a.cells + a.off[q];
    int32_t c[JOINT_PER_THREAD];                              // cell i JOINT_THREADS + tid; an absent cell counts nothing
    int32_t mine = 0;
    uint64_t top = 0;                                         // (count, ~cell): the largest count, then the lowest cell - (ia, ib) row-major
#pragma unroll
    for (int i = 0; i < JOINT_PER_THREAD; ++i) {
        const int cell = i * JOINT_THREADS + tid;
        c[i] = cell < cells ? cnt[cell] : 0;
        mine += c[i];
        const uint64_t key = ((uint64_t)(uint32_t)c[i] << 32) | (uint64_t)(0xffffffffu - (uint32_t)cell);
        if (c[i] > 0 && key > top) top = key;
    }
    const int32_t inside = block_sum(mine, part);
    best[tid] = top;
    __syncthreads();
    for (int stride = JOINT_THREADS / 2; stride >= 1; stride >>= 1) {
        if (tid < stride && best[tid + stride] > best[tid]) best[tid] = best[tid + stride];
        __syncthreads();
    }
    top = best[0];
    const int32_t most = (int32_t)(top >> 32);                // 0: no sample inside
    const int64_t slot = s * a.n_pair + q;
    if (tid == 0) {
        if (a.inside) a.inside[slot] = inside;
        if (a.mode) {
            const int cell = (int)(0xffffffffu - (uint32_t)top);
            a.mode[2 * slot] = inside ? cell / Bb : -1;
            a.mode[2 * slot + 1] = inside ? cell % Bb : -1;
        }
    }
    if (!a.level && !a.n_cells && !a.held) return;
    for (int p = 0; p < a.n_mass; ++p) {
        int32_t level = 0, n_cells = 0, held = 0;
        if (inside) {
            const int32_t k = joint_need(inside, a.mass[p]);
            int32_t lo = 1, hi = most;                        // the cells with count >= 1 hold `inside` >= k samples
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo + 1) / 2;
                int32_t h = 0;
#pragma unroll
                for (int i = 0; i < JOINT_PER_THREAD; ++i) h += c[i] >= mid ? c[i] : 0;
                if (block_sum(h, part) >= k) lo = mid; else hi = mid - 1;
            }
            level = lo;
            int32_t h = 0, n = 0;
#pragma unroll
            for (int i = 0; i < JOINT_PER_THREAD; ++i) { h += c[i] >= level ? c[i] : 0; n += c[i] >= level ? 1 : 0; }
            held = block_sum(h, part);
            n_cells = block_sum(n, part);
        }
        if (tid == 0) {
            if (a.level) a.level[slot * a.n_mass + p] = level;
            if (a.n_cells) a.n_cells[slot * a.n_mass + p] = n_cells;
            if (a.held) a.held[slot * a.n_mass + p] = held;
        }
    }
}

hipError_t launch_joint(const JointArgs& a, hipStream_t stream) {
    if (a.from_data) hipLaunchKernelGGL(joint_range_kernel, dim3((unsigned)a.S, (unsigned)a.n_coord), dim3(JOINT_THREADS), 0, stream, a);
    if (a.counts) {
        if (a.S * a.slabs > INT32_MAX) return hipErrorInvalidValue;
        if (a.slabs > 1) {
            hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)a.S * (size_t)a.cells * sizeof(int32_t), stream);
            if (e != hipSuccess) return e;
        }
        int most = 0;
        for (int q = 0; q < a.n_pair; ++q) most = (int)a.Ba[q] * a.Bb[q] > most ? (int)a.Ba[q] * a.Bb[q] : most;
        hipLaunchKernelGGL(joint_hist_kernel, dim3((unsigned)(a.S * a.slabs), (unsigned)a.n_pair), dim3(JOINT_THREADS), (size_t)most * sizeof(int32_t), stream, a);
    }
    if (a.levels()) hipLaunchKernelGGL(joint_level_kernel, dim3((unsigned)a.S, (unsigned)a.n_pair), dim3(JOINT_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace misti
