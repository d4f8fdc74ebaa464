// Tempered ensemble MCMC per fit with device-resident rungs (MI355X / gfx950): misti_tempered_sample.
//
// Parallel tempering (replica exchange) over the ensemble sampler of misti_ens.hip: a fit is a ladder of L ensembles at the
// temperatures T_0 < T_1 < ...; every rung moves by the stretch move against llk / T_l, neighbouring rungs trade walkers, and the cold
// rung carries the posterior.  The rungs of all fits ride through the propose / accept kernels of misti_ens.hip as fits x L searches
// (EnsState::L), so a half-step of all rungs of all fits is ONE engine batch; what is new here is what happens between steps:
//
//   pt_swap_kernel    thread = (fit, pair, walker): a swap needs no evaluation - both log-likelihoods are already in HBM.  The thread
//                     draws its uniform from the lower rung's own block, decides (misti_pt.h), exchanges N coordinates and one value,
//                     counts, and on a kept step rewrites the chain entries of the two walkers: the chain row is the state AFTER the
//                     swap round.  The pairs of a round are disjoint, so no two threads touch the same walker
//   pt_reduce_kernel  wave = fit: the per-rung mean log-likelihood over the kept steps (lsum's exact tree, misti_post.h) and their
//                     thermodynamic integral over 1 / T
//
// The rule is THE PROJECT'S OWN: optimize.tempered_rule states it in NumPy and the kernels restate it operation for operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "misti_boot.h"
#include "misti_device.h"
#include "misti_ens.h"
#include "misti_post.h"
#include "misti_pt.h"

namespace misti {

namespace {
constexpr int PT_THREADS = 256;
}

__global__ __launch_bounds__(PT_THREADS)
void pt_swap_kernel(EnsState st, PtState pt, int64_t step, int first, int n_pair) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = st.W, N = st.N, L = st.L;
    const int64_t fits = st.S / L;
    if (t >= fits * n_pair * W) return;
    const int64_t fit = t / ((int64_t)n_pair * W);
    const int rem = (int)(t - fit * n_pair * W);
    const int l = first + 2 * (rem / W), i = rem % W;      // l + 1 <= L - 1: n_pair = (L - first) / 2
    const int64_t a = (fit * L + l) * W + i, b = a + W;    // walker i of rung l, of rung l + 1
    const double fa = st.llh[a], fb = st.llh[b];
    if (!ens_has(fa) || !ens_has(fb)) return;               // nothing happens and nothing is counted
    const double* T = st.temp + (st.temp_per_start ? fit : 0) * L;
    const double u = pt_swap_uniform(st.seed, id_of(st.src, fit), step, L, l, i, W);
    atomicAdd(pt.swap_proposed + fit * (L - 1) + l, 1);
    if (!pt_swap_decide(T[l], T[l + 1], fa, fb, u)) return;
    atomicAdd(pt.swap_accepted + fit * (L - 1) + l, 1);
    double* xa = st.x + a * N;
    double* xb = st.x + b * N;
    for (int k = 0; k < N; ++k) { const double v = xa[k]; xa[k] = xb[k]; xb[k] = v; }
    st.llh[a] = fb;
    st.llh[b] = fa;
    if (st.chain_llh && step % st.thin == 0) {              // the accept kernel of half 1 wrote the row as it stood before the round
        const int64_t at = step / st.thin - 1;
        st.chain_llh[((fit * L + l) * st.n_keep + at) * W + i] = fb;
        st.chain_llh[((fit * L + l + 1) * st.n_keep + at) * W + i] = fa;
        if (st.chain && l == 0) {
            double* c = st.chain + ((fit * st.n_keep + at) * W + i) * N;
            for (int k = 0; k < N; ++k) c[k] = xa[k];
        }
    }
}

__global__ __launch_bounds__(POST_LANES)
void pt_reduce_kernel(EnsState st, int64_t burn, double* __restrict__ rung_llh, double* __restrict__ logz) {
    __shared__ double E[MISTI_PT_MAX_RUNGS];
    const int64_t fit = blockIdx.x;
    const int lane = threadIdx.x, W = st.W, L = st.L;
    const int64_t n = st.n_keep - burn, rows = (n + POST_LANES - 1) / POST_LANES;
    for (int l = 0; l < L; ++l) {
        const double* v = st.chain_llh + ((fit * L + l) * st.n_keep + burn) * W;
        double acc = 0.0;
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t t = r * POST_LANES + lane;
            double e = 0.0;
            if (t < n) {
                const double* p = v + t * W;
                e = p[0];
                for (int w = 1; w < W; ++w) e = e + p[w];
                e = e / (double)W;
            }
            acc = r == 0 ? e : acc + e;
        }
        const double mean = post_fold(acc) / (double)n;   // no kept step: 0 / 0
        if (lane == 0) { E[l] = mean; rung_llh[fit * L + l] = post_out(mean); }
    }
    if (lane == 0) {                                       // its own stores: no barrier
        const double* T = st.temp + (st.temp_per_start ? fit : 0) * L;
        double z = 0.0;
        for (int l = 0; l + 1 < L; ++l) z = z + pt_trapezoid(T[l], T[l + 1], E[l], E[l + 1]);
        logz[fit] = post_out(z);
    }
}

hipError_t launch_pt_swap(const EnsState& st, const PtState& pt, int64_t step, int first, hipStream_t stream) {
    const int n_pair = (st.L - first) / 2;
    const int64_t n = st.S / st.L * n_pair * st.W;
    hipLaunchKernelGGL(pt_swap_kernel, dim3((unsigned)((n + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, stream, st, pt, step, first, n_pair);
    return hipGetLastError();
}
hipError_t launch_pt_reduce(const EnsState& st, int64_t burn, double* rung_llh, double* logz, hipStream_t stream) {
    hipLaunchKernelGGL(pt_reduce_kernel, dim3((unsigned)(st.S / st.L)), dim3(POST_LANES), 0, stream, st, burn, rung_llh, logz);
    return hipGetLastError();
}

}  // namespace misti

// internal (misti_api.cpp): make `msg` the calling thread's last error; returns `code`
extern "C" int misti_set_error_(int code, const char* msg);

extern "C" {

int misti_pt_swap(double T_lo, double T_hi, double llk_lo, double llk_hi, double u, int32_t* swap) {
    if (!swap) return misti_set_error_(MISTI_E_ARG, "swap is NULL");
    if (!(T_lo > 0.0) || !std::isfinite(T_lo) || !(T_hi > 0.0) || !std::isfinite(T_hi))
        return misti_set_error_(MISTI_E_ARG, "the temperatures must be finite and positive");
    if (!(T_lo < T_hi)) return misti_set_error_(MISTI_E_ARG, "T_lo must be below T_hi");
    if (!(u >= 0.0 && u < 1.0)) return misti_set_error_(MISTI_E_ARG, "u must be in [0, 1)");
    *swap = misti::pt_swap_decide(T_lo, T_hi, llk_lo, llk_hi, u) ? 1 : 0;
    return 0;
}

}  // extern "C"
