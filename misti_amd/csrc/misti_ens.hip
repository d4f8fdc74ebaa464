// Ensemble MCMC per search with device-resident ensembles (MI355X / gfx950): misti_ensemble_sample.
//
// The affine-invariant ensemble sampler (Goodman & Weare's stretch move): a search is W walkers in a finite box, the target is
// llk / T inside the box where the engine has a value and zero elsewhere.  Like differential evolution (misti_de.hip) it has no inner
// minimisation and no tail: a half-step of every search is ONE engine batch of searches x W / 2 points, and since there is no stopping
// rule the host never reads anything back between steps.
//
// The rule is THE PROJECT'S OWN (emcee draws from a Mersenne Twister in an order that depends on the ensemble):
// optimize.ensemble_rule states it in NumPy and every kernel here restates it operation for operation - every random number from the
// counter-based stream of misti_boot.h (Philox4x64-10 as numpy.random.Philox(key=[seed, ids[s]])), walker i of step t owning block
// t W + i; the exponential of the decision is the project's own too (misti_ens.h).  A search's result is a function of its own arguments
// alone.
//
// Ensembles, values, counters and the chain live in HBM; per half-step one kernel lays out the proposals (thread = search x moving
// walker), the engine evaluates them as an ordinary rows-path batch (run_dev, launch_llk_rows), and one kernel takes the decisions.
// A proposal that leaves the box is rejected without an evaluation: its slot carries a negative split, which the engine refuses
// before it reads anything else of the slot.
//
// With a prior (EnsState::prior, misti_prior.h; the rule is optimize.ensemble_prior_rule) the ensemble, the stretch and the box are in
// sampling coordinates; the slot's point is their natural image (ens_natural), the proposal itself waits in prior.y, and the decision
// carries the log prior of the old walker and of the proposal (ens_decide_prior).  Without one nothing of this is read or written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "misti_boot.h"
#include "misti_device.h"
#include "misti_ens.h"
#include "misti_prior.h"

namespace misti {

namespace {

constexpr int ENS_THREADS = 256;

// What a slot of the batch hands the engine beside its point, a search's box and the id of its stream: misti_device.h's put_point /
// put_none / box_of / id_of on the search's PointSource.

// the engine's value as the sampler keeps it: -inf where there is none
__device__ __forceinline__ double ens_value(double llk) { return ens_has(llk) ? llk : -INFINITY; }

}  // namespace

// The initial ensemble as one batch.  Thread = (search, walker); walker i of search s sits in slot s W + i.
__global__ __launch_bounds__(ENS_THREADS)
void ens_init_kernel(EnsState st, const double* __restrict__ init) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = st.W, N = st.N;
    if (t >= st.S * W) return;
    const int64_t fit = t / W / st.L;
    double* pt = st.b.pts + t * N;
    double* x = st.x + t * N;
    if (st.prior.kind) {
        const int32_t* scale = st.prior.scale + prior_of(st.prior, fit, N);
        for (int k = 0; k < N; ++k) { const double v = init[t * N + k]; pt[k] = ens_natural(scale[k], v); x[k] = v; }
    } else {
        for (int k = 0; k < N; ++k) { const double v = init[t * N + k]; pt[k] = v; x[k] = v; }
    }
    put_point(st.src, st.b, t, fit, pt);
}

// Half `half` of step `step`: walker i = half H + m moves against walker j of the other half.  Thread = (search, m).
__global__ __launch_bounds__(ENS_THREADS)
void ens_propose_kernel(EnsState st, int64_t step, int half) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = st.W, N = st.N, H = W / 2;
    if (t >= st.S * H) return;
    const int64_t s = t / H, fit = s / st.L;               // search s is rung s % L of fit s / L (misti_device.h)
    const int i = half * H + (int)(t - s * H);
    const EnsDraw dr = ens_draw(st.seed, id_of(st.src, fit), step * st.L + (s - fit * st.L), i, W);
    const int j = (1 - half) * H + dr.partner;
    const double* xi = st.x + (s * W + i) * (int64_t)N;
    const double* xj = st.x + (s * W + j) * (int64_t)N;
    const double z = ens_stretch(st.a, st.am1, dr.u_z);
    const int64_t o = box_of(st.src, fit);
    double* pt = st.b.pts + t * N;
    bool inside = true;
    if (st.prior.kind) {
        const int32_t* scale = st.prior.scale + prior_of(st.prior, fit, N);
        double* yt = st.prior.y + t * N;
        for (int k = 0; k < N; ++k) {
            const double lo = st.src.box_lo[o + k], hi = st.src.box_hi[o + k];
            const double y = lo == hi ? lo : xj[k] + ens_rn(z * (xi[k] - xj[k]));
            inside = inside && y >= lo && y <= hi;
            yt[k] = y;
            pt[k] = ens_natural(scale[k], y);
        }
    } else {
        for (int k = 0; k < N; ++k) {
            const double lo = st.src.box_lo[o + k], hi = st.src.box_hi[o + k];
            const double y = lo == hi ? lo : xj[k] + ens_rn(z * (xi[k] - xj[k]));
            inside = inside && y >= lo && y <= hi;                                 // a NaN is outside
            pt[k] = y;
        }
    }
    st.u_acc[t] = dr.u_acc;
    if (inside) { st.z[t] = z; put_point(st.src, st.b, t, fit, pt); }
    else { st.z[t] = -1.0; put_none(st.src, st.b, t, pt); }
}

// The values of the batch are in.  half < 0: the initial ensemble's, thread = (search, walker).  Otherwise thread = (search, m): the
// decision on walker i = half H + m; behind half 1 of a kept step the thread writes walkers m and H + m of the ensemble's chain row
// (walker m was settled by the launch of half 0): the values of every search, the coordinates of rung 0 of a fit.
__global__ __launch_bounds__(ENS_THREADS)
void ens_accept_kernel(EnsState st, int64_t step, int half, const double* __restrict__ llk) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = st.W, N = st.N, H = W / 2;
    if (half < 0) {
        if (t >= st.S * W) return;
        st.llh[t] = ens_value(llk[t]);
        st.accepted[t] = 0;
        st.submitted[t] = 0;
        return;
    }
    if (t >= st.S * H) return;
    const int64_t s = t / H, fit = s / st.L;
    const int m = (int)(t - s * H), i = half * H + m, l = (int)(s - fit * st.L);
    const int64_t wi = s * W + i;
    const double z = st.z[t];
    if (z > 0.0) {                                          // the proposal was evaluated
        const int64_t o = box_of(st.src, fit);
        int d = -1;
        for (int k = 0; k < N; ++k) d += st.src.box_lo[o + k] != st.src.box_hi[o + k] ? 1 : 0;
        const double T = st.temp[(st.temp_per_start ? fit : 0) * st.L + l];
        const double v = ens_value(llk[t]);
        st.submitted[wi] = st.submitted[wi] + 1;
        bool take;
        const double* pt;
        if (st.prior.kind) {                                // the proposal is in prior.y: the slot's point is its natural image
            const int64_t q = prior_of(st.prior, fit, N);
            const int32_t* kind = st.prior.kind + q;
            const double *p0 = st.prior.p0 + q, *p1 = st.prior.p1 + q, *lo = st.src.box_lo + o, *hi = st.src.box_hi + o;
            pt = st.prior.y + t * N;
            const double lp_old = ens_log_prior(N, kind, p0, p1, lo, hi, st.x + wi * N);
            const double lp_new = ens_log_prior(N, kind, p0, p1, lo, hi, pt);
            take = ens_decide_prior(z, d, st.llh[wi], v, T, lp_old, lp_new, st.u_acc[t]);
        } else {
            pt = st.b.pts + t * N;
            take = ens_decide(z, d, st.llh[wi], v, T, st.u_acc[t]);
        }
        if (take) {
            double* x = st.x + wi * N;
            for (int k = 0; k < N; ++k) x[k] = pt[k];
            st.llh[wi] = v;
            st.accepted[wi] = st.accepted[wi] + 1;
        }
    }
    if (half == 1 && st.chain_llh && step % st.thin == 0) {
        const int64_t at = step / st.thin - 1, row = s * st.n_keep + at, xrow = fit * st.n_keep + at;
        for (int h = 0; h < 2; ++h) {
            const int w = h * H + m;
            const int64_t src = s * W + w;
            st.chain_llh[row * W + w] = st.llh[src];
            if (st.chain && l == 0) for (int k = 0; k < N; ++k) st.chain[(xrow * W + w) * N + k] = st.x[src * N + k];
        }
    }
}

// the proposals a search handed the engine: thread = search, a plain store
__global__ __launch_bounds__(ENS_THREADS)
void ens_result_kernel(EnsState st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= st.S) return;
    long long n = 0;
    for (int i = 0; i < st.W; ++i) n += st.submitted[s * st.W + i];
    st.points[s] = n;
}

static dim3 ens_grid(int64_t n) { return dim3((unsigned)((n + ENS_THREADS - 1) / ENS_THREADS)); }

hipError_t launch_ens_init(const EnsState& st, const double* init, hipStream_t stream) {
    hipLaunchKernelGGL(ens_init_kernel, ens_grid(st.S * st.W), dim3(ENS_THREADS), 0, stream, st, init);
    return hipGetLastError();
}
hipError_t launch_ens_propose(const EnsState& st, int64_t step, int half, hipStream_t stream) {
    hipLaunchKernelGGL(ens_propose_kernel, ens_grid(st.S * (st.W / 2)), dim3(ENS_THREADS), 0, stream, st, step, half);
    return hipGetLastError();
}
hipError_t launch_ens_accept(const EnsState& st, int64_t step, int half, const double* llk, hipStream_t stream) {
    hipLaunchKernelGGL(ens_accept_kernel, ens_grid(half < 0 ? st.S * st.W : st.S * (st.W / 2)), dim3(ENS_THREADS), 0, stream, st, step, half, llk);
    return hipGetLastError();
}
hipError_t launch_ens_result(const EnsState& st, hipStream_t stream) {
    hipLaunchKernelGGL(ens_result_kernel, ens_grid(st.S), dim3(ENS_THREADS), 0, stream, st);
    return hipGetLastError();
}

}  // namespace misti

// internal (misti_api.cpp): make `msg` the calling thread's last error; returns `code`
extern "C" int misti_set_error_(int code, const char* msg);

extern "C" {

int misti_ens_draws(uint64_t seed, uint64_t id, int64_t step, int32_t walker, int32_t walkers, int32_t* partner, double* u_z, double* u_acc) {
    if (step < 0) return misti_set_error_(MISTI_E_ARG, "negative step");
    if (walkers < 4 || (walkers & 1)) return misti_set_error_(MISTI_E_ARG, "walkers must be even and >= 4");
    if (walkers > MISTI_ENS_MAX_WALKERS) return misti_set_error_(MISTI_E_LIMIT, "walkers exceeds MISTI_ENS_MAX_WALKERS");
    if (walker < 0 || walker >= walkers) return misti_set_error_(MISTI_E_ARG, "walker must be 0 ... walkers - 1");
    if (!partner || !u_z || !u_acc) return misti_set_error_(MISTI_E_ARG, "partner / u_z / u_acc is NULL");
    const misti::EnsDraw d = misti::ens_draw(seed, id, step, walker, walkers);
    *partner = d.partner; *u_z = d.u_z; *u_acc = d.u_acc;
    return 0;
}

int misti_ens_exp(double x, double* y) {
    if (!y) return misti_set_error_(MISTI_E_ARG, "y is NULL");
    *y = misti::ens_exp(x);
    return 0;
}

int misti_ens_accept(double z, int32_t d, double llk_old, double llk_new, double T, double u_acc, int32_t* accept) {
    if (!accept) return misti_set_error_(MISTI_E_ARG, "accept is NULL");
    if (d < 0 || d >= MISTI_MAX_PARAMS) return misti_set_error_(MISTI_E_ARG, "d must be 0 ... MISTI_MAX_PARAMS - 1");
    if (!(T > 0.0) || !std::isfinite(T)) return misti_set_error_(MISTI_E_ARG, "the temperature must be finite and positive");
    *accept = misti::ens_decide(z, d, llk_old, llk_new, T, u_acc) ? 1 : 0;
    return 0;
}

}  // extern "C"
