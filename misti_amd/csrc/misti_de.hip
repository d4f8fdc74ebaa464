// Differential evolution per search with device-resident populations (MI355X / gfx950): misti_de_search.
//
// The library's other global search, basin hopping (misti_nm.hip), follows SciPy step for step: hop k + 1 of every start waits for the
// slowest minimisation of hop k, and the tail of every minimisation runs a handful of live starts.  A population search has neither:
// a generation of every live search is ONE engine batch of searches x members points, there are no inner minimisations.
//
// The rule is THE PROJECT'S OWN, not SciPy's (scipy.optimize.differential_evolution redraws a coordinate that leaves the bounds, so the
// number of its draws depends on the data): optimize.differential_evolution_rule states it in NumPy and every kernel here restates it
// operation for operation - best1bin with dither and deferred updating, every random number from the counter-based stream of
// misti_boot.h (Philox4x64-10 as numpy.random.Philox(key=[seed, ids[s]])), member i of generation g owning the DE_BLOCKS blocks from
// (g P + i) DE_BLOCKS on.  A search's result is a function of its own arguments alone: not of the other searches in the call, their
// number, the device or the launch geometry (the one atomic, the compaction of the live searches, only decides which batch slot a
// search gets, and a point's value does not depend on its slot).
//
// Populations, values, decisions and counters live in HBM; per generation one kernel lays out the trial points (thread = live slot x
// member), the engine evaluates them as an ordinary rows-path batch (run_dev, launch_llk_rows), and one kernel takes the decisions
// (thread = live slot x member, the members of a search in one workgroup: selection per member, then member 0 finds the best member,
// applies the stop test in member order and gives a search that goes on the next free slot).  Arithmetic: one rounding per operation,
// products that feed a sum pass through rn() (misti_device.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "misti_boot.h"
#include "misti_device.h"

namespace misti {

namespace {

// Words a member owns per generation: r1, r2, jrand, F's uniform, then one uniform per coordinate - 4 + MISTI_MAX_PARAMS fit.
constexpr int DE_BLOCKS = MISTI_DE_BLOCKS;
static_assert(4 * DE_BLOCKS >= 4 + MISTI_MAX_PARAMS, "a member's words must hold four draws and a uniform per coordinate");
constexpr int DE_THREADS = 256;
static_assert(MISTI_DE_MAX_POP <= DE_THREADS, "the members of a search share one workgroup of the selection kernel");

// The words of member i of generation g of the stream Philox(key=[seed, id]), word j = 0 ... 4 DE_BLOCKS - 1; read in rising order a
// member costs DE_BLOCKS blocks at the most.
struct DeWords {
    uint64_t seed, id, first;
    int have;
    uint64_t w[4];
    __host__ __device__ DeWords(uint64_t seed_, uint64_t id_, int64_t gen, int i, int P)
        : seed(seed_), id(id_), first(((uint64_t)gen * (uint64_t)P + (uint64_t)i) * DE_BLOCKS), have(-1) {}
    __host__ __device__ uint64_t word(int j) {
        if ((j >> 2) != have) { have = j >> 2; philox4x64_10_block(seed, id, first + (uint64_t)have, w); }
        return w[j & 3];
    }
    __host__ __device__ double uniform(int j) { return (double)(word(j) >> 11) * 0x1p-53; }    // numpy's next_double
};

// r1 from the P - 1 members other than i, r2 from the P - 2 other than i and r1, jrand from the N coordinates: one word each, no rejection
__host__ __device__ __forceinline__ void de_indices(DeWords& g, int i, int P, int N, int& r1, int& r2, int& jrand) {
    r1 = (int)boot_index(g.word(0), P - 1);
    if (r1 >= i) ++r1;
    const int a = i < r1 ? i : r1, b = i < r1 ? r1 : i;
    r2 = (int)boot_index(g.word(1), P - 2);
    if (r2 >= a) ++r2;
    if (r2 >= b) ++r2;
    jrand = (int)boot_index(g.word(2), N);
}

// What a slot of the batch hands the engine beside its point, a search's box and the id of its stream: misti_device.h's put_point /
// put_none / box_of / id_of on the search's PointSource.

}  // namespace

// Generation 0: member 0 is the caller's start clipped to the box, member i > 0 is lo + u (hi - lo) per coordinate from its own words.
// Thread = (search, member); search s sits in slot s.
__global__ __launch_bounds__(DE_THREADS)
void de_init_kernel(DeState st, const double* __restrict__ starts) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int P = st.P, N = st.N;
    if (t >= st.S * P) return;
    const int64_t s = t / P;
    const int i = (int)(t - s * P);
    double* pt = st.b.pts + t * N;
    const int64_t o = box_of(st.src, s);
    DeWords g(st.seed, id_of(st.src, s), 0, i, P);
    for (int k = 0; k < N; ++k) {
        const double lo = st.src.box_lo[o + k], hi = st.src.box_hi[o + k];
        const double y = i == 0 ? starts[s * N + k] : lo + rn(g.uniform(4 + k) * rn(hi - lo));
        pt[k] = box_clip(y, lo, hi);
    }
    put_point(st.src, st.b, t, s, pt);
    if (i == 0) { st.nit[s] = 0; st.done[s] = -1; atomicAdd(st.points, (unsigned long long)P); }
}

// Generation gen >= 1: the trial point of every member of every live search.  Thread = (live slot, member).
__global__ __launch_bounds__(DE_THREADS)
void de_trial_kernel(DeState st, int64_t bound, int gen) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int P = st.P, N = st.N;
    if (t >= bound * P) return;
    const int64_t j = t / P;
    const int i = (int)(t - j * P);
    double* pt = st.b.pts + t * N;
    if (j >= st.count_cur[0]) { put_none(st.src, st.b, t, pt); return; }           // the host's count of live searches is an upper bound
    const int64_t s = st.idx_cur[j];
    const double* x = st.pop + s * (int64_t)P * N;
    const double* xb = x + (int64_t)st.best[s] * N;
    const double* xi = x + (int64_t)i * N;
    DeWords g(st.seed, id_of(st.src, s), gen, i, P);
    int r1, r2, jrand;
    de_indices(g, i, P, N, r1, r2, jrand);
    const double F = st.F_lo + rn(g.uniform(3) * rn(st.F_hi - st.F_lo));                  // dither
    const int64_t o = box_of(st.src, s);
    for (int k = 0; k < N; ++k) {
        const double lo = st.src.box_lo[o + k], hi = st.src.box_hi[o + k];
        const double u = g.uniform(4 + k);
        double y = xi[k];
        if (lo == hi) y = lo;                                                            // a fixed coordinate
        else if (k == jrand || u < st.CR) {
            const double v = xb[k] + rn(F * rn(x[r1 * N + k] - x[r2 * N + k]));          // the mutant: best1
            // outside the box: halfway between the member and the bound the mutant crossed - no extra draw
            y = v > hi ? xi[k] + rn(0.5 * rn(hi - xi[k])) : (v < lo ? xi[k] + rn(0.5 * rn(lo - xi[k])) : v);
            y = box_clip(y, lo, hi);
        }
        pt[k] = y;
    }
    put_point(st.src, st.b, t, s, pt);
    if (i == 0) atomicAdd(st.points, (unsigned long long)P);
}

// The values of generation gen are in.  Thread = (live slot, member), the 256 / P searches of a workgroup whole: member i is replaced
// iff f(trial) <= f(member) (generation 0: taken as it is), then member 0 of every search walks the P values in member order.
__global__ __launch_bounds__(DE_THREADS)
void de_select_kernel(DeState st, int64_t bound, int gen, const double* __restrict__ llk) {
    const int P = st.P, N = st.N;
    const int per = DE_THREADS / P;                      // searches of a workgroup
    const int jl = (int)threadIdx.x / P, i = (int)threadIdx.x - jl * P;
    const int64_t j = (int64_t)blockIdx.x * per + jl;
    const bool active = jl < per && j < bound && (gen == 0 || j < st.count_cur[0]);
    int64_t s = 0;
    if (active) {
        s = gen == 0 ? j : st.idx_cur[j];
        const int64_t t = j * P + i;
        const double ft = objective(llk[t]);
        double* fx = st.f + s * P + i;
        if (gen == 0 || ft <= *fx) {                     // inf <= inf replaces; neither side is ever NaN
            double* x = st.pop + (s * P + i) * (int64_t)N;
            const double* pt = st.b.pts + t * N;
            for (int k = 0; k < N; ++k) x[k] = pt[k];
            *fx = ft;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (!active || i != 0) return;
    const double* f = st.f + s * P;
    int best = 0;
    bool all = f[0] < INFINITY;
    double sum = f[0];
    for (int m = 1; m < P; ++m) {
        if (f[m] < f[best]) best = m;                    // ties: the lowest index
        all = all && f[m] < INFINITY;
        sum = sum + f[m];
    }
    st.best[s] = best;
    st.nit[s] = gen;
    bool stop = false;
    if (all) {                                           // var(f) <= (atol + tol |mean(f)|)^2, sums in member order
        const double mean = sum / (double)P;
        double q = 0.0;
        for (int m = 0; m < P; ++m) { const double d = f[m] - mean; q = q + rn(d * d); }
        const double var = q / (double)P, thr = st.atol + rn(st.tol * fabs(mean));
        stop = var <= rn(thr * thr);
    }
    if (stop) st.done[s] = 0;
    else if (gen >= st.maxiter) st.done[s] = 2;
    else st.idx_next[atomicAdd(st.count_next, 1)] = (int32_t)s;     // which slot a search gets never matters
}

__global__ __launch_bounds__(DE_THREADS)
void de_result_kernel(DeState st, double* __restrict__ x, double* __restrict__ llh, int32_t* __restrict__ nfev, int32_t* __restrict__ status,
                      double* __restrict__ pop_llh) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= st.S) return;
    const int P = st.P, N = st.N;
    const int best = st.best[s];
    for (int k = 0; k < N; ++k) x[s * N + k] = st.pop[(s * P + best) * (int64_t)N + k];
    llh[s] = -st.f[s * P + best];
    nfev[s] = P * (st.nit[s] + 1);
    status[s] = st.done[s] < 0 ? 2 : st.done[s];
    if (pop_llh) for (int m = 0; m < P; ++m) pop_llh[s * P + m] = -st.f[s * P + m];
}

static dim3 de_grid(int64_t n) { return dim3((unsigned)((n + DE_THREADS - 1) / DE_THREADS)); }

hipError_t launch_de_init(const DeState& st, const double* starts, hipStream_t stream) {
    hipLaunchKernelGGL(de_init_kernel, de_grid(st.S * st.P), dim3(DE_THREADS), 0, stream, st, starts);
    return hipGetLastError();
}
hipError_t launch_de_trial(const DeState& st, int64_t bound, int gen, hipStream_t stream) {
    hipLaunchKernelGGL(de_trial_kernel, de_grid(bound * st.P), dim3(DE_THREADS), 0, stream, st, bound, gen);
    return hipGetLastError();
}
hipError_t launch_de_select(const DeState& st, int64_t bound, int gen, const double* llk, hipStream_t stream) {
    if (st.P < 1 || st.P > DE_THREADS) return hipErrorInvalidValue;
    const int64_t per = DE_THREADS / st.P;
    hipLaunchKernelGGL(de_select_kernel, dim3((unsigned)((bound + per - 1) / per)), dim3(DE_THREADS), 0, stream, st, bound, gen, llk);
    return hipGetLastError();
}
hipError_t launch_de_result(const DeState& st, double* x, double* llh, int32_t* nfev, int32_t* status, double* pop_llh, hipStream_t stream) {
    hipLaunchKernelGGL(de_result_kernel, de_grid(st.S), dim3(DE_THREADS), 0, stream, st, x, llh, nfev, status, pop_llh);
    return hipGetLastError();
}

}  // namespace misti

// internal (misti_api.cpp): make `msg` the calling thread's last error; returns `code`
extern "C" int misti_set_error_(int code, const char* msg);

extern "C" {

int misti_de_draws(uint64_t seed, uint64_t id, int64_t generation, int32_t member, int32_t pop, int32_t n,
                   int32_t* r1, int32_t* r2, int32_t* jrand, double* u_F, double* u) {
    if (generation < 0) return misti_set_error_(MISTI_E_ARG, "negative generation");
    if (pop < 4) return misti_set_error_(MISTI_E_ARG, "pop must be >= 4");
    if (pop > MISTI_DE_MAX_POP) return misti_set_error_(MISTI_E_LIMIT, "pop exceeds MISTI_DE_MAX_POP");
    if (member < 0 || member >= pop) return misti_set_error_(MISTI_E_ARG, "member must be 0 ... pop - 1");
    if (n < 1) return misti_set_error_(MISTI_E_ARG, "n must be >= 1");
    if (n > MISTI_MAX_PARAMS) return misti_set_error_(MISTI_E_LIMIT, "n exceeds MISTI_MAX_PARAMS");
    if (!r1 || !r2 || !jrand || !u_F || !u) return misti_set_error_(MISTI_E_ARG, "r1 / r2 / jrand / u_F / u is NULL");
    misti::DeWords g(seed, id, generation, member, pop);
    int a, b, c;
    misti::de_indices(g, member, pop, n, a, b, c);
    *r1 = a; *r2 = b; *jrand = c;
    *u_F = g.uniform(3);
    for (int k = 0; k < n; ++k) u[k] = g.uniform(4 + k);
    return 0;
}

}  // extern "C"
