// MI355X (gfx950) kernels of the MiSTI composite-likelihood engine.
//
// A batch of candidates (split time, band rates, pulse rates) x bootstrap JSFS replicates is four
// launches:
//   setup_kernel            candidates with identical parameters share a CHAIN (hash table); dispatch order; llh_const of the
//                           replicates; the other (double-buffered) chain table cleared for the next batch
//   correct_[follow_]kernel lambda-correction of the chains, a resumable state machine per chain;
//                           with one chain per wave a second wave of the workgroup builds the
//                           chain's TRUNK (44-state propagation shared by its candidates) behind it
//   post_kernel             trunks that did not follow + tails (fractional splits)
//   spectrum_kernel         one wavefront per candidate, the 44-state vector one state per lane:
//                           own intervals after the trunk, collapse, one-population closed form,
//                           normalisation, llk of up to 8 replicates  (llk_kernel beyond that)
// fp64 throughout, no MFMA (the per-interval matrices are 3x3 / 44x44 with ~200 non-zeros).
// Behind the batch, on its spectra: misti_score.hip; the expressions this file shares with it (llh_const_of, llk_of): misti_score.h.
//
// This file holds the kernels, chain discovery, the table upload and the launchers - one translation unit.  The device functions
// the kernels are made of stand in internal headers, one per unit the suite tests (each names its entry and its tests):
//   misti_kernel_tables.h   c_tab, c_inv, c_qmax and the method constants (Q_SWITCH, ...): defined there, for this file alone
//   misti_wave.h            lane broadcasts, LDS hand-over words, scalar branch conditions
//   misti_model.h           Grid, Model, Diag, setup_candidate() and its checks, trunk_leave(), PairState, pulse_pairs()
//   misti_lsq.h             rcp64 / sqrt64, 3 x 3 solves, svd_mx2 / svd_aug, solve_tr[_n], select_step, trf_bounded, tr_update, next_step
//   misti_pair.h            taylor3, pair_reduced / pair_cascade / pair_eigen, pair_expv, ect_*, PairProblem, pair_eval
//   misti_chain.h           correct_body, wrong_phase
//   misti_twopop.h          twopop_interval, series_step, smooth_rates, trunk_body, trunk_follow
//
// Reference path restated here (cites: /root/reference):
//   JAFSLikelihood  MigrationInference.py:566-614     driver, status codes
//   CorrectLambdas  MigrationInference.py:305-378     -> correct_body(), post-split rates in spectrum_kernel
//   CorrectLambda   CorrectLambda.py:29-317           -> pair chain: pair_expv(), pair_batch(), next_step(), trf_bounded()
//   Smooth          MigrationInference.py:380-405     -> smooth_rates(), run_mean()
//   JAFSpectrum     MigrationInference.py:467-540     -> twopop_interval(), trunk_body()/trunk_follow(), spectrum_kernel
//   TwoPopulations / OnePopulation                     -> tables (misti_tables.hpp) + closed form
//   CoalescentRates MigrationInference.py:542-564     -> forward_kernel
//
// Numerical method (differs from the reference's dense Pade expm + inverse, same
// mathematics): exp(M T) P0 and the occupation integral  int_0^T exp(M t) P0 dt
// (= M^-1 (P1 - P0), MigrationInference.py:538-540) are evaluated together as an
// action on the vector by uniformisation: M T = N - q I with N >= 0, and the
// augmented series  p_{k+1} = N p_k/(k+1),  i_{k+1} = (T p_k + q i_k)/(k+1)  whose
// sums are P1 and the integral.  All terms are non-negative, so there is no
// cancellation, no inverse, and the mu = 0 generator (singular: the reference
// deletes 7 stationary states and restores their mass, TwoPopulations.py:231-309)
// needs no special case.  After the split the chain is the Kingman coalescent in
// rescaled time, whose 8x8 generator has eigenvalues -6,-3,-1: closed form.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "misti_chain.h"
#include "misti_device.h"
#include "misti_kernel_tables.h"
#include "misti_lsq.h"
#include "misti_model.h"
#include "misti_pair.h"
#include "misti_score.h"
#include "misti_twopop.h"
#include "misti_wave.h"

namespace misti {

// ------------------------------------------------------------ forward map ----
// MigrationInference.CoalescentRates (MigrationInference.py:542-564) with CorrectLambda.CoalRates
// (CorrectLambda.py:112-122): the model's own rates lh are taken as the TRUE per-population rates;
// for every two-population interval the rate a single-genome (PSMC) analysis would see is
// -log(P[no coalescence in the interval]) / T under the pair chain started from that genome's
// pair-state distribution.  No solver: one 3-state exponential action per genome and interval, so
// one thread per candidate.  Rates after the split are returned unchanged (the loop at :563 is empty).
// hold_mu: the reference's CoalescentRates never sets the migration rates of its CorrectLambda
// object, so every interval is evaluated with what the preceding CorrectLambdas loop left there
// (:324) - the rates of the LAST two-population interval.  hold_mu = 1 reproduces that; 0 applies
// each interval's own rates (the model as specified; what data generation wants).
__global__ __launch_bounds__(64)
void forward_kernel(DevModel m, int64_t n_cand, const double* __restrict__ split_time, const double* __restrict__ params, int hold_mu,
                    double* __restrict__ lh_out, double* __restrict__ pr_out, int32_t* __restrict__ status_out) {
    const int64_t cand = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (cand >= n_cand) return;
    Grid G;
    const double* par = params ? params + cand * m.n_param : nullptr;
    const int status = setup_candidate(m, split_time[cand], par, G);
    const int rows = m.numT + 1;
    double* lh_o = lh_out + cand * (int64_t)rows * 2;
    double* pr_o = pr_out ? pr_out + cand * (int64_t)(m.numT + 2) * 6 : nullptr;
    if (status_out) status_out[cand] = status;
    if (pr_o) for (int i = 0; i < (m.numT + 2) * 6; ++i) pr_o[i] = 0.0;
    if (status != MISTI_OK && status != MISTI_INF_COAL) {
        for (int i = 0; i < 2 * rows; ++i) lh_o[i] = NAN;
        return;
    }
    Model M; M.m = &m; M.par = par; M.split = G.split; M.cache();
    PairState ps = {{{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}}};
    Diag dg;
    double held0 = 0.0, held1 = 0.0;
    if (hold_mu && G.split >= 1) M.mig((G.split < G.numT ? G.split : G.numT - 1) - 1, held0, held1);
    for (int t = 0; t < rows; ++t) {
        double l0 = 0.0, l1 = 0.0;
        if (t < G.numT) { l0 = G.lhk(t, 0); l1 = G.lhk(t, 1); }
        if (t < G.split && t < G.numT - 1) {
            double pu0, pu1, mu0, mu1;
            M.pulse(t, pu0, pu1);
            pulse_pairs(ps, pu0, pu1);
            if (t == 0 && pr_o)
                for (int j = 0; j < 6; ++j) pr_o[j] = ps.p[j & 1][j >> 1];
            M.mig(t, mu0, mu1);
            if (hold_mu) { mu0 = held0; mu1 = held1; }
            const double T = G.T(t);
            const double a0 = l0 * T, a1 = l1 * T, b0 = mu0 * T, b1 = mu1 * T;
            const double q = fmax(fmax(2.0 * b0 + a0, 2.0 * b1 + a1), b0 + b1);
            for (int k = 0; k < 2; ++k) {
                double v[3] = {ps.p[k][0], ps.p[k][1], ps.p[k][2]};
                const double before = (v[0] + v[1]) + v[2];
                bool guard_unused = false;
                pair_expv(a0, a1, b0, b1, v, q, 0.0, true, dg, guard_unused);
                const double nc = (v[0] + v[1]) + v[2];
                // The state is chained without renormalisation, so past a cumulated rate x length of ~708 the mass is a subnormal
                // double with a few digits left (finite rates wrong in the 11th digit were measured at e^-720) and past ~745 it is zero:
                // such a rate is reported as NaN, never as a finite number.
                const double seen = (nc >= 0x1p-1022 && before >= 0x1p-1022) ? -log(nc / before) / T : NAN;
                if (k == 0) l0 = seen; else l1 = seen;
                ps.p[k][0] = v[0]; ps.p[k][1] = v[1]; ps.p[k][2] = v[2];
            }
            if (pr_o)
                for (int j = 0; j < 6; ++j) pr_o[6 * (t + 1) + j] = ps.p[j & 1][j >> 1];
        }
        lh_o[2 * t] = l0; lh_o[2 * t + 1] = l1;
    }
}

// ------------------------------------------------------------ residual probe ----
// misti_pair_residuals (include/misti_hip.h, "introspection (tests)"): pair_eval as the chain kernels call it, one problem per lane, so
// that the suite reaches every branch of the residual directly - pair_reduced and the default fit's two forms of the expected
// coalescence time are otherwise met only inside the solver.  A problem is [mu0, mu1, P[3], tgt, x0, x1, role, red], everything already
// stretched to the unit interval; sk is the sum of P in the order the chain kernel adds it (correct_body).  No solver, no model.
template <bool CPFIT>
__global__ __launch_bounds__(64)
void pair_residuals_kernel(int64_t n, const double* __restrict__ problems, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* p = problems + i * 10;
    PairProblem pb;
    pb.mu0 = p[0]; pb.mu1 = p[1];
    pb.Pk[0] = p[2]; pb.Pk[1] = p[3]; pb.Pk[2] = p[4];
    pb.sk = (pb.Pk[0] + pb.Pk[1]) + pb.Pk[2];
    pb.tgtk = p[5];
    pb.red = (int)p[9];
    Diag dg;
    double res, w[3];
    bool guard = false;
    pair_eval<CPFIT>(pb, p[6], p[7], (int)p[8], dg, res, w, guard);
    double* o = out + i * 4;
    o[0] = res; o[1] = w[0]; o[2] = w[1]; o[3] = w[2];
}

// ------------------------------------------------------------ least-squares probe ----
// misti_lsq_probe (include/misti_hip.h, "introspection (tests)"): the solver's linear algebra - rcp64 / sqrt64, the Jacobi SVD, the
// trust-region steps, select_step, tr_update and the 3 x 3 solves - one problem per lane through the device functions the chain
// kernels call (no copies: the chain kernels' own next_step, svd_aug, ... are instantiated here), so that the suite reaches each of
// them directly and not only through whole solves.  A problem is MISTI_LSQ_IN doubles, a result MISTI_LSQ_OUT, unused entries 0; the
// layouts of the kinds are in the header.  Integers travel as doubles.
// next_step is instantiated with GROUP = 8: with GROUP == 64 uni<> takes the first lane's branch for the whole wave (a chain owns
// its wave there) and the probe would test one problem per wave; for every other GROUP uni<> is the identity and each lane takes
// its own branch.  kind is the same in every lane of a launch.
__global__ __launch_bounds__(64)
void lsq_probe_kernel(int kind, int64_t n, const double* __restrict__ problems, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* q = problems + i * MISTI_LSQ_IN;
    double* o = out + i * MISTI_LSQ_OUT;
    double r[MISTI_LSQ_OUT];
    for (int k = 0; k < MISTI_LSQ_OUT; ++k) r[k] = 0.0;
    if (kind == MISTI_LSQ_SCALAR) {
        r[0] = rcp64(q[0]); r[1] = sqrt64(q[0]);
    } else if (kind == MISTI_LSQ_SVD2) {
        const double J[2][2] = {{q[0], q[1]}, {q[2], q[3]}}, f[2] = {q[4], q[5]};
        const Svd2 d = svd_mx2<2>(J, f);
        r[0] = d.s[0]; r[1] = d.s[1]; r[2] = d.V[0][0]; r[3] = d.V[0][1]; r[4] = d.V[1][0]; r[5] = d.V[1][1]; r[6] = d.uf[0]; r[7] = d.uf[1];
    } else if (kind == MISTI_LSQ_SVD4) {
        if ((int)q[12] == 1) {
            const double A[2][1] = {{q[0]}, {q[2]}}, f[2] = {q[8], q[9]};
            const SvdN<1> d = svd_aug(A, f);
            r[0] = d.s[0]; r[2] = d.V[0][0]; r[6] = d.uf[0];
        } else {
            const double A[4][2] = {{q[0], q[1]}, {q[2], q[3]}, {q[4], q[5]}, {q[6], q[7]}}, f[4] = {q[8], q[9], q[10], q[11]};
            const SvdN<2> d = svd_aug(A, f);
            r[0] = d.s[0]; r[1] = d.s[1]; r[2] = d.V[0][0]; r[3] = d.V[0][1]; r[4] = d.V[1][0]; r[5] = d.V[1][1]; r[6] = d.uf[0]; r[7] = d.uf[1];
        }
    } else if (kind == MISTI_LSQ_STEP) {
        const double J[2][2] = {{q[0], q[1]}, {q[2], q[3]}}, f[2] = {q[4], q[5]};
        double g[2];
        g[0] = J[0][0] * f[0] + J[1][0] * f[1];                     // as correct_body forms the gradient
        g[1] = J[0][1] * f[0] + J[1][1] * f[1];
        double alpha = q[7], p[2];
        int lm = 0, axis = -1;
        const double predicted = next_step<8>(J, f, g, q[6], alpha, p, lm, axis);
        r[0] = p[0]; r[1] = p[1]; r[2] = alpha; r[3] = predicted; r[4] = (double)lm; r[5] = (double)axis;
    } else if (kind == MISTI_LSQ_STEPN) {
        double alpha = q[14];
        if ((int)q[12] == 1) {
            const double A[2][1] = {{q[0]}, {q[2]}}, f[2] = {q[8], q[9]};
            const SvdN<1> d = svd_aug(A, f);
            double ph[1];
            solve_tr_n<1>(d, 1, q[13], alpha, ph);
            r[0] = ph[0];
        } else {
            const double A[4][2] = {{q[0], q[1]}, {q[2], q[3]}, {q[4], q[5]}, {q[6], q[7]}}, f[4] = {q[8], q[9], q[10], q[11]};
            const SvdN<2> d = svd_aug(A, f);
            double ph[2];
            solve_tr_n<2>(d, 2, q[13], alpha, ph);
            r[0] = ph[0]; r[1] = ph[1];
        }
        r[2] = alpha;
    } else if (kind == MISTI_LSQ_SELECT) {
        if ((int)q[19] == 1) {
            const double x[1] = {q[0]}, Jh[1][1] = {{q[2]}}, diag[1] = {q[6]}, gh[1] = {q[8]}, d[1] = {q[14]};
            double p[1] = {q[10]}, ph[1] = {q[12]}, step[1], steph[1];
            r[4] = select_step<1>(x, Jh, diag, gh, p, ph, d, q[16], q[17], q[18], step, steph);
            r[0] = step[0]; r[2] = steph[0];
        } else {
            const double x[2] = {q[0], q[1]}, Jh[2][2] = {{q[2], q[3]}, {q[4], q[5]}}, diag[2] = {q[6], q[7]}, gh[2] = {q[8], q[9]}, d[2] = {q[14], q[15]};
            double p[2] = {q[10], q[11]}, ph[2] = {q[12], q[13]}, step[2], steph[2];
            r[4] = select_step<2>(x, Jh, diag, gh, p, ph, d, q[16], q[17], q[18], step, steph);
            r[0] = step[0]; r[1] = step[1]; r[2] = steph[0]; r[3] = steph[1];
        }
    } else if (kind == MISTI_LSQ_UPDATE) {
        const double p[2] = {q[1], q[2]}, x[2] = {q[3], q[4]};
        double Delta = q[8], dq;
        int term;
        bool accept;
        tr_update(q[0] != 0.0, p, x, q[5], q[6], q[7], Delta, dq, term, accept);
        r[0] = Delta; r[1] = dq; r[2] = (double)term; r[3] = accept ? 1.0 : 0.0;
    } else if (kind == MISTI_LSQ_SOLVE3) {
        const double M[3][3] = {{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}}, b[3] = {q[9], q[10], q[11]};
        const double I3[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        double x[3], y[3], X[3][3];
        solve3(M, b, x);
        solve3_ge(M, b, y);
        mat3_solve(M, I3, X);
        for (int k = 0; k < 3; ++k) { r[k] = x[k]; r[3 + k] = y[k]; for (int j = 0; j < 3; ++j) r[6 + 3 * k + j] = X[k][j]; }
    }
    for (int k = 0; k < MISTI_LSQ_OUT; ++k) o[k] = r[k];
}

template <bool CPFIT, int GROUP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CPFIT ? 2 : MISTI_DEFAULT_FIT_WAVES, CPFIT ? 2 : MISTI_DEFAULT_FIT_WAVES)))
void correct_kernel(DevModel m, int64_t n_items, ChainBufs cb, const double* __restrict__ split_time, const double* __restrict__ params, int yield_nfev) {
    extern __shared__ double lds[];
    {   // candidate -> chain, once, by blocks that mostly have nothing else to do (the launch has one block per
        // 64/GROUP candidates, the chains occupy the first few): later kernels read it without the slot indirection
        const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
        if (i < n_items) cb.of[i] = cb.slot_chain[cb.slot_of[i]];
    }
    correct_body<CPFIT, GROUP, false>(m, n_items, cb, split_time, params, (int64_t)blockIdx.x, lds, nullptr, nullptr, nullptr, cb.chain_order,
                                      GROUP == 64 ? 0 : yield_nfev);
}

// The chains that yielded in a packed launch, one per wave (speculation tree, per-interval constants in LDS), pulled from the
// list the packed launch left; workgroups beyond its length leave at once.  LDS: grid staging [3 numT] | constants [6 numT].
template <bool CPFIT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CPFIT ? MISTI_FOLLOW_WAVES : 1, CPFIT ? MISTI_FOLLOW_WAVES : 1)))
void correct_resume_kernel(DevModel m, int64_t n_items, ChainBufs cb, const double* __restrict__ split_time, const double* __restrict__ params) {
    extern __shared__ double lds[];
    __shared__ int next;
    const int n_res = cb.n_chains[3];
    if ((int)blockIdx.x >= n_res) return;
    // the launch waits for its longest chain, and the phase-1 candidate waves of the same batch run beside it (launch_spectrum): the
    // chains get the issue priority on the SIMDs they share
    __builtin_amdgcn_s_setprio(3);
    double* pre = lds + 3 * (size_t)m.numT;
    for (;;) {
        if (threadIdx.x == 0) next = atomicAdd(&cb.n_chains[2], 1);
        __syncthreads();
        const int pos = next;
        __syncthreads();
        if (pos >= n_res) break;
        const int64_t ch = cb.resume_list[pos];
        correct_body<CPFIT, 64, false, true>(m, n_items, cb, split_time, params, ch, lds, nullptr, nullptr, pre, nullptr, 0, cb.resume_t[ch]);
        __syncthreads();
    }
}

// Kernel 1 with the trunk following: 128-thread workgroups, wave 0 = the chain (one chain per wave),
// wave 1 = its trunk.  LDS (doubles): kernel-1 staging [3 numT] | trunk xbuf [128] + rates [2 (numT+1)] |
// hand-over rates [2 numT] | count, done flag [2] | per-interval constants of the chain (mu, pulse, exp(-lh T)) [6 numT].
// Two waves per SIMD for the --cpfit instantiation: the chain wave is bound by the latency of its own dependent
// instruction stream (one instruction per ~4.7 cycles), so a second wave on the SIMD costs it nothing (single batch
// 1.884 -> 1.888 ms) and with 20 batches in flight the chip holds twice as many chains (2.38e7 -> 2.62e7 evals/s).
// The register allocator gives up the 12 AGPRs for 28 bytes of scratch.  The default fit (256 VGPRs + 108 AGPRs) stays
// at one wave.
template <bool CPFIT>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(CPFIT ? MISTI_FOLLOW_WAVES : 1, CPFIT ? MISTI_FOLLOW_WAVES : 1)))
void correct_follow_kernel(DevModel m, int64_t n_items, ChainBufs cb, const double* __restrict__ split_time, const double* __restrict__ params) {
    extern __shared__ double lds[];
    double* tk = lds + 3 * (size_t)m.numT;
    double* lc_sh = tk + 128 + 2 * (size_t)(m.numT + 1);
    volatile int* flags = (volatile int*)(lc_sh + 2 * (size_t)m.numT);          // count, done | queue position of the chain in progress
    double* pre = lc_sh + 2 * (size_t)m.numT + 4;                              // per-interval constants of the chain in progress (after 8 ints: flags, queue position, role exchange)
    // candidate -> chain (see correct_kernel)
    for (int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * 128) cb.of[i] = cb.slot_chain[cb.slot_of[i]];
    // Workgroups PULL chains from a queue, the longest first (cb.chain_order, sorted by setup_kernel; head = n_chains[2]): any
    // grid is correct, and with more chains than resident workgroups (1 024 two-wave workgroups at two waves per SIMD) a
    // workgroup that finishes a short chain takes the next one instead of waiting for a fixed stride partner.
    const int64_t n_live = cb.n_chains[0];
    if ((int64_t)blockIdx.x >= n_live) return;                                // more workgroups than chains (a generous grid): leave at once
    int* next = (int*)(flags + 2);
    // Which of the two waves runs the chain: the one on the SIMD that hosts fewer chain waves right now (of any context: a device-wide
    // table of counters per compute unit and SIMD).  A chain wave beside a trunk wave runs at full speed, beside another chain
    // wave it does not (1.66 against 1.96 ms on 1 024 chains), and which SIMDs a workgroup's waves land on is the dispatcher's choice.
    // Measured with 20 batches in flight on the headline grid: 3.60 -> 3.76e7 evals/s; alone nothing changes (the dispatcher's own
    // placement on an idle chip is already the good one).  The counters only steer - a stale or shared one costs speed, never a result.
    bool chain_role = threadIdx.x < 64;
    int32_t* my_load = nullptr;
    if (cb.simd_load) {
        int* ex = next + 1;                              // [4]: SIMD of wave 0, of wave 1, table index of the compute unit, role swap
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);          // HW_REG_HW_ID: wave [3:0] simd [5:4] cu [11:8] sh [12] se [15:13]
        const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);         // HW_REG_XCC_ID [3:0]
        const int simd = (hw >> 4) & 3;
        if ((threadIdx.x & 63) == 0) ex[threadIdx.x >> 6] = simd;
        if (threadIdx.x == 0) ex[2] = (int)((((xcc & 7) * 8 + ((hw >> 13) & 7)) * 2 + ((hw >> 12) & 1)) * 16 + ((hw >> 8) & 15)) * 4;
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t* t = cb.simd_load + ex[2];
            const int c0 = __hip_atomic_load(&t[ex[0]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int c1 = __hip_atomic_load(&t[ex[1]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int sw = c1 < c0 ? 1 : 0;              // wave 1 takes the chain
            ex[3] = sw;
            atomicAdd(&t[ex[sw]], 1);
        }
        __syncthreads();
        chain_role = ((int)(threadIdx.x >> 6) ^ ex[3]) == 0;
        my_load = cb.simd_load + ex[2] + ex[ex[3]];
        __syncthreads();
    }
    for (;;) {
        if (threadIdx.x == 0) { lds_put(flags, 0); lds_put(flags + 1, 0); *next = atomicAdd(&cb.n_chains[2], 1); }
        __syncthreads();
        const int64_t pos = *next;
        if (pos >= n_live) break;
        const int64_t ch = cb.chain_order[pos];
        if (chain_role) {
            // a launch that fills the chip: the longest chains - the ones the launch waits for - get the issue priority on the SIMD
            // they share with another wave (s_setprio; measured on 1 024 chains: 2.04 -> 1.92 ms per call).
            // A launch of at most 256 chains (the headline grid's 64): MISTI_SMALL_LAUNCH_PRIO (misti_consts.h), priority 3 for the chain wave.
            // Measured 2026-10-20 with the 4 queues a process inherits (11 batches in flight): +2 % at 512 steps, +5 % at 20; at
            // GPU_MAX_HW_QUEUES=22, where it once cost 1 %, now inside the run-to-run range.
            if (n_live > 256) {
                if (4 * pos < n_live) __builtin_amdgcn_s_setprio(3);
                else if (2 * pos < n_live) __builtin_amdgcn_s_setprio(2);
                else __builtin_amdgcn_s_setprio(1);
            }
#if MISTI_SMALL_LAUNCH_PRIO >= 1
            else __builtin_amdgcn_s_setprio(3);
#endif
            correct_body<CPFIT, 64, false, true>(m, n_items, cb, split_time, params, ch, lds, lc_sh, flags, pre);
            lds_order();
            if (lane_id() == 0) lds_put(flags + 1, 1);                       // whatever way the chain ended
#if MISTI_SMALL_LAUNCH_PRIO >= 1
            if (n_live <= 256) __builtin_amdgcn_s_setprio(0);                // back in the pull loop the wave is nobody's critical path
#endif
        } else {
#if MISTI_SMALL_LAUNCH_PRIO >= 2
            if (n_live <= 256) __builtin_amdgcn_s_setprio(0);
#endif
            trunk_follow(m, n_items, params, cb, ch, tk, lc_sh, flags);
        }
        __syncthreads();                                                     // both waves are done with the hand-over area
    }
    if (my_load && threadIdx.x == 0) atomicSub(my_load, 1);
}

// Everything that waits for the chains and that the candidate kernel waits for, in ONE launch: the
// trunks (blocks below trunk_cap, dispatched first: they are the long ones) and the tails of the
// lambda-correction (the shortened last interval of candidates with a fractional split).  A launch
// costs a queue round trip, which is what limits the rate when many batches are in flight.
template <bool CPFIT, int GROUP>
__global__ __launch_bounds__(64)
void post_kernel(DevModel m, int64_t n_cand, ChainBufs cb, int64_t trunk_blocks, const double* __restrict__ split_time, const double* __restrict__ params, int phase) {
    extern __shared__ double lds[];
    if ((int64_t)blockIdx.x < trunk_blocks) trunk_body(m, n_cand, params, cb, (int64_t)blockIdx.x, lds, phase);
    else correct_body<CPFIT, GROUP, true>(m, n_cand, cb, split_time, params, (int64_t)blockIdx.x - trunk_blocks, lds, nullptr, nullptr, nullptr, nullptr, 0, 0, phase);
}

// Default fit only: the rates after the split (FitSinglePop, CorrectLambda.py:82-92, called at MigrationInference.py:361-364).
// The weights of the two genomes depend only on the difference of their log-survival at the split (both decay by the
// same rate afterwards), so every interval is an independent bounded 1-D solve: one THREAD per (candidate, interval).
// Kept out of the spectrum kernel: the bounded trust-region code needs ~100 registers of its own, which pushed that
// kernel (128 VGPRs for four waves per SIMD) into scratch.
__global__ __launch_bounds__(256)
void postsplit_kernel(DevModel m, int64_t n_cand, const double* __restrict__ split_time, const double* __restrict__ params, ChainBufs cb) {
    const int rows = m.numT + 1;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_cand * rows) return;
    const int64_t cand = gid / rows;
    const int t = (int)(gid - cand * rows);
    cb.post_lam[gid] = 1.0;
    if (cb.post_word) cb.post_word[gid] = 0;
    Grid G;
    const double* par = params ? params + cand * m.n_param : nullptr;
    const int32_t* bb = cb.bounds ? cb.bounds + cand * 2 * m.n_band : nullptr;
    const int32_t* pt = cb.pulse_times ? cb.pulse_times + cand * m.n_pulse : nullptr;
    if (setup_candidate(m, split_time[cand], par, G, bb, pt) != MISTI_OK) return;
    if (t < G.split || t >= G.numT - 1) return;
    const int64_t ch = chain_of(cb, cand);
    const int nfull = (G.ins >= 0) ? G.ins : G.split;
    if (cb.fail_t[ch] < nfull || (G.ins >= 0 && cb.tail_status[cand] != MISTI_OK)) return;     // no value for this candidate
    const double T = G.T(t);
    if (T == 0) return;
    const double* stt = (G.ins >= 0) ? cb.tail_state + 6 * cand : cb.trace + (ch * (int64_t)(m.numT + 1) + nfull) * 6;   // pair state at the split
    const double nc0 = (stt[0] + stt[2]) + stt[4], nc1 = (stt[1] + stt[3]) + stt[5];     // :353-354 (a probability used as a log)
    const double lh0 = G.lhk(t, 0), lh1 = G.lhk(t, 1);
    // FitSinglePop :88-92 with P0 = [[exp(nc0),0,0],[exp(nc1),0,0]] (:361)
    const double pa = exp(nc0), pb = exp(nc1);
    const double w0 = pa / (pa + pb), w1 = pb / (pa + pb);
    const double Te = w0 * ect_one_pop(lh0, T) + w1 * ect_one_pop(lh1, T);
    double x[1] = {w0 * lh0 + w1 * lh1};
    auto resid = [&](const double l[1], double f[1]) { f[0] = ect_one_pop(l[0], T) - Te; };
    const int32_t word = trf_bounded<1>(resid, x, 0.01 * fmin(lh0, lh1));
    cb.post_lam[gid] = x[0];
    if (cb.post_word) cb.post_word[gid] = word;
}

// Kernel 2: post-split rates (:355-376), Smooth (:380-405) and the expected joint spectrum
// (JAFSpectrum, :467-540).  One wavefront per candidate; lane = interval in the prologue,
// lane = state of the 44-state chain afterwards.
// LDS per wave (doubles): xbuf[128] (re | im) | lc[2*(numT0+1)]
// WPB: candidates (waves) per workgroup - 4, or 1 (launch_spectrum: `single_waves`).  A four-wave workgroup needs four free wave slots
// on one compute unit at the same moment; with other contexts' chain kernels resident everywhere those seldom come free together, and
// single-wave workgroups slip into every slot as it opens: measured with 20 batches in flight, the headline grid 2.96 -> 3.59e7 evals/s,
// config2x16 8.2 -> 9.1e7.  Alone on the device the kernel itself runs the same either way.
template <bool CPFIT, int WPB = WAVES_PER_BLOCK>
__global__ __launch_bounds__(WPB * 64, 4)      // 4 waves per SIMD: a 4 096-candidate batch is resident in one round
void spectrum_kernel(DevModel m, int64_t n_cand, const int32_t* __restrict__ order, const double* __restrict__ split_time, const double* __restrict__ params,
                     ChainBufs cb, double* __restrict__ lc_out, double* __restrict__ pr_out,
                     double* __restrict__ jafs_out, int32_t* __restrict__ status_out, double* __restrict__ diag_out,
                     int n_inline, const double* __restrict__ jsfs, const double* __restrict__ consts, double* __restrict__ llk_out, int phase) {
    extern __shared__ double lds[];
    const int lane = lane_id();
    // everything per candidate is wave-uniform: keep it in scalar registers
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = (int64_t)blockIdx.x * WPB + wave;
    if (slot >= n_cand) return;
    if (phase != 0) {                              // two-phase launch (wrong_phase): a candidate of the other phase's chains leaves at once
        const int64_t cd = (int64_t)__builtin_amdgcn_readfirstlane(order[slot]);
        if (wrong_phase(cb, (int64_t)__builtin_amdgcn_readfirstlane((int)chain_of(cb, cd)), phase)) return;
    }
#ifdef MISTI_STAMP2
    long long s_[8];
#define KSTAMP(i) s_[i] = clock64();
#else
#define KSTAMP(i)
#endif
    KSTAMP(0)
    const int64_t cand = (int64_t)__builtin_amdgcn_readfirstlane(order[slot]);
    const int lc_rows = m.numT + 1;
    double* xbuf = lds + (size_t)wave * (128 + 2 * lc_rows);
    double* lcb = xbuf + 128;
    const double* par = params ? params + cand * m.n_param : nullptr;
    Grid G;
    const int32_t* bb = cb.bounds ? cb.bounds + cand * 2 * m.n_band : nullptr;
    const int32_t* pt = cb.pulse_times ? cb.pulse_times + cand * m.n_pulse : nullptr;
    int status = setup_candidate(m, split_time[cand], par, G, bb, pt);
    // a batch issued under "no fractional split times" (misti_set_hints; no tail launch was made) that has one after all: refused, never wrong
    if (status == MISTI_OK && cb.integer_splits && G.ins >= 0) status = MISTI_BAD_STRUCTURE;
    Model mod{&m, par, G.split, {0, 0, 0, 0}};
    mod.bb = bb;
    mod.pt = pt;
    mod.cache();
    // ---- this candidate's share of its chain (+ its own tail interval after a fractional split)
    const int64_t ch = (int64_t)__builtin_amdgcn_readfirstlane((int)chain_of(cb, cand));
    const int nfull = (G.ins >= 0) ? G.ins : G.split;          // intervals taken from the chain
    const double* lc_ch = cb.lc + ch * (int64_t)m.numT * 2;
    const double* tr_ch = cb.trace + ch * (int64_t)(m.numT + 1) * 6;
    int have = 0;                                               // intervals with a corrected rate (for diagnostics)
    if (status == MISTI_OK) {
        const int ft = cb.fail_t[ch];
        if (ft < nfull) { status = cb.fail_status[ch]; have = ft + 1; }
        else {
            have = nfull;
            if (G.ins >= 0) { const int ts = cb.tail_status[cand]; have = nfull + 1; if (ts != MISTI_OK) status = ts; }
        }
    }
    double* lc_o = lc_out ? lc_out + cand * (int64_t)lc_rows * 2 : nullptr;
    double* pr_o = pr_out ? pr_out + cand * (int64_t)(m.numT + 2) * 6 : nullptr;
    int32_t* sv_o = cb.cand_solver ? cb.cand_solver + cand * (int64_t)lc_rows : nullptr;
    if (sv_o) {
        // solver trace of this candidate: its share of the chain (+ the shortened interval of a fractional split);
        // the post-split intervals are added below
        for (int i = lane; i < lc_rows; i += 64) {
            int32_t wd = 0;
            if (i < nfull && i < have) wd = cb.solver[ch * (int64_t)m.numT + i];
            else if (i == nfull && G.ins >= 0 && have > nfull) wd = cb.tail_solver[cand];
            sv_o[i] = wd;
        }
    }
    if (pr_o) {
        // .Pr trace (MigrationInference.py:309,350): rows 0..split from the chain (+ tail); last row = work counters
        const int rows = (status == MISTI_OK) ? G.split + 1 : (have > nfull ? nfull + 1 : (have > 0 ? have : (status == MISTI_OK ? 1 : 0)));
        for (int i = lane; i < (m.numT + 2) * 6; i += 64) {
            const int r = i / 6, j = i - 6 * r;
            double v = 0.0;
            if (r == m.numT + 1) v = cb.work[ch * 6 + j];
            else if (r < rows) v = (G.ins >= 0 && r == nfull + 1) ? cb.tail_state[cand * 6 + j] : tr_ch[6 * r + j];
            pr_o[i] = v;
        }
    }
    if (status != MISTI_OK) {
        if (lane == 0) { status_out[cand] = status; if (diag_out) diag_out[cand] = NAN; }
        if (lane < 7) jafs_out[cand * 7 + lane] = NAN;
        if (lane < n_inline) llk_out[cand * n_inline + lane] = -INFINITY;
        if (lc_o)                            // partial rates (up to the failing interval) for diagnostics
            for (int i = lane; i < 2 * lc_rows; i += 64) {
                const int t = i >> 1;
                lc_o[i] = (t < have && t < nfull) ? lc_ch[i] : (t < have && t == nfull && G.ins >= 0) ? cb.tail_lc[2 * cand + (i & 1)] : 0.0;
            }
        return;
    }
    KSTAMP(1)
    for (int i = lane; i < 2 * lc_rows; i += 64) {
        const int t = i >> 1;
        lcb[i] = (t < nfull) ? lc_ch[i] : (t == nfull && G.ins >= 0) ? cb.tail_lc[2 * cand + (i & 1)] : 0.0;
    }
    lds_fence();
    {
        // diagnostic: largest corrected rate x interval length before smoothing.  From ~5 upwards the
        // correction's residual is nearly flat in that rate and the reference's own value is not
        // determined to 1e-9; callers can tell such candidates apart.
        double mx = 0.0;
        for (int t = lane; t < G.split; t += 64) { double T = G.T(t); mx = fmax(mx, fmax(lcb[2 * t], lcb[2 * t + 1]) * T); }
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        if (diag_out && lane == 0) diag_out[cand] = (m.flags & MISTI_TRUE_EPS) ? 0.0 : mx;
    }
    // ---- where this candidate leaves the trunk of its chain --------------------------------
    int t0 = 0;
    const bool use_trunk = trunk_active(cb, n_cand);
    int smooth_from = 0;
    if (use_trunk) {
        // first interval whose rates depend on this candidate's split (trunk_leave); the trunk stores records from the
        // smallest such interval of the chain's members on, and its last one where it ended early
        const int t_own = trunk_leave(m, G);
        t0 = min(t_own, cb.trunk_ok[ch]);
        // smoothed rates below t0 are only needed for the optional lc output: skip them otherwise (a run that
        // reaches back below t_own still reads the unsmoothed values there: smoothing writes after all reads)
        if (t0 == t_own && !lc_o) smooth_from = t_own;
    }
    KSTAMP(2)
    {
        // ---- post-split rates (:355-376); nc is a probability used as a log ----
        const double* stt = (G.ins >= 0) ? cb.tail_state + 6 * cand : tr_ch + 6 * nfull;    // pair state at the split
        const double nc0 = (stt[0] + stt[2]) + stt[4], nc1 = (stt[1] + stt[3]) + stt[5];     // :353-354
        const double delta = nc1 - nc0;
        const double ed = exp(delta);
        const int last = G.numT - 1;
        for (int base = G.split; base < G.numT; base += 64) {
            int t = base + lane;
            if (t < last) {
                double T = G.T(t);
                double lam = 1.0;
                int32_t word = 0;
                if (T != 0) {
                    double lh0 = G.lhk(t, 0), lh1 = G.lhk(t, 1);
                    if (CPFIT) {
                        double pnc = (exp(-T * lh0) + exp(delta - T * lh1)) / (1.0 + ed);   // :366
                        lam = -log(pnc) / T;
                        word = solver_word(0, 0, 1);
                    } else {
                        // FitSinglePop (default fit): solved by postsplit_kernel, one thread per interval
                        lam = cb.post_lam[cand * lc_rows + t];
                        word = cb.post_word ? cb.post_word[cand * lc_rows + t] : 0;
                    }
                }
                lcb[2 * t] = lam; lcb[2 * t + 1] = lam;
                if (sv_o) sv_o[t] = word;
            } else if (t == last) {
                double lh0 = G.lhk(t, 0), lh1 = G.lhk(t, 1);
                double lam = (1.0 + ed) / (1.0 / lh0 + ed / lh1);                            // :372-376
                lcb[2 * t] = lam; lcb[2 * t + 1] = lam;
                if (sv_o) sv_o[t] = solver_word(0, 0, 1);
            }
        }
        lds_fence();
        KSTAMP(3)
        // ---- Smooth (:380-405): time-weighted mean of lc over runs of constant lh, t < split
        if (m.flags & MISTI_SMOOTH) smooth_rates(m, G, lcb, lane, smooth_from, G.split);
        for (int i = lane; i < 2 * G.numT; i += 64) { double v = lcb[i]; if (!(v == v)) status = MISTI_NUMERIC; }
        status = __any(status != MISTI_OK) ? MISTI_NUMERIC : MISTI_OK;
        if (lc_o) for (int i = lane; i < 2 * lc_rows; i += 64) lc_o[i] = (i < 2 * G.numT) ? lcb[i] : 0.0;
    }
    double jn = NAN;                      // lane c < 7: normalised expected spectrum, class c
    KSTAMP(4)
    KSTAMP(5) KSTAMP(6) KSTAMP(7)

    if (status == MISTI_OK) {
        // ---- expected spectrum, two-population part (:467-506) ----------------
        TwoPopRow R;
        R.load(lane);
        const bool live = R.live;
        double x = (lane == 2) ? 1.0 : 0.0;
        double w_pre = 0.0, w_post = 0.0;          // occupation integrals before / from the sample date
        if (use_trunk) {
            const double* r = cb.trunk + (ch * (int64_t)m.numT + t0) * TRUNK_REC;
            if (live) { x = r[lane]; w_pre = r[NS2 + lane]; w_post = r[2 * NS2 + lane]; }
        }
        for (int t = t0; t <= G.split && t < G.numT; ++t) {
            if (t == m.sample_date) ancient_project(xbuf, lane, x);
            if (t == G.split) break;
            const int st = twopop_interval(R, m, mod, G, lcb, xbuf, lane, t, x, w_pre, w_post);
            if (st != MISTI_OK) { status = st; break; }
        }
        KSTAMP(5)
        if (status == MISTI_OK) {
            // two-population share of the spectrum: class c = sum over the states of weight_c(state) x occupation integral (w_post for
            // every class, w_pre for the two classes only the ancient sample's pre-date part feeds).  Every state lane forms its
            // seven products; the seven sums over the wave are taken together - halves of the wave swap half of the classes at
            // each of the first three butterfly steps (8 -> 4 -> 2 -> 1 classes per lane), three plain steps finish: 7 shuffles for
            // all classes instead of a 44-step loop on seven lanes (a sixth of this kernel's instructions on a shared grid), and a
            // pairwise sum instead of a running one.  Lanes 8c .. 8c + 7 end up with class c.
            double jp;
            {
                double a4[4], a2[2], z;
                {
                    double a[8];
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        const double wg = (double)c_tab.jaf[c][lane];
                        a[c] = live ? (c < 2 ? wg * w_post + wg * w_pre : wg * w_post) : 0.0;
                    }
                    a[7] = 0.0;
                    const bool hi = lane & 32;
#pragma unroll
                    for (int c = 0; c < 4; ++c) { const double keep = hi ? a[c + 4] : a[c], give = hi ? a[c] : a[c + 4]; a4[c] = keep + __shfl_xor(give, 32, 64); }
                }
                {
                    const bool hi = lane & 16;
#pragma unroll
                    for (int c = 0; c < 2; ++c) { const double keep = hi ? a4[c + 2] : a4[c], give = hi ? a4[c] : a4[c + 2]; a2[c] = keep + __shfl_xor(give, 16, 64); }
                }
                {
                    const bool hi = lane & 8;
                    const double keep = hi ? a2[1] : a2[0], give = hi ? a2[0] : a2[1];
                    z = keep + __shfl_xor(give, 8, 64);
                }
                z += __shfl_xor(z, 4, 64); z += __shfl_xor(z, 2, 64); z += __shfl_xor(z, 1, 64);
                jp = __shfl(z, 8 * (lane & 7), 64);                                   // lane c < 7: class c
            }
            // CollapsePops (:518-528)
            xbuf[lane] = live ? x : 0.0; lds_fence();
            double c8 = 0.0;
            if (lane < NS1) for (int i = c_tab.grp_lo[lane]; i < c_tab.grp_hi[lane]; ++i) c8 += xbuf[i];
            lds_fence();
            double P8[NS1];
            for (int i = 0; i < NS1; ++i) P8[i] = bcast(c8, i);
            KSTAMP(6)
            // ---- one-population part: Kingman coalescent in rescaled time --------
            // P(s) = V1 e^-s + V3 e^-3s + V6 e^-6s, s = int lc dt; occupation integral of
            // interval t is (1/lc_t) * int_{S_t}^{S_t+tau_t} P(s) ds (OnePopulation.py:153-178,
            // SolveDifEq :530-540 incl. the last, infinite interval).
            double G1 = 0, G3 = 0, G6 = 0;           // sum_t e^{-a S_t} (1 - e^{-a tau_t}) / (a lc_t)
            double carry = 0.0;
            const int last = G.numT - 1;
            for (int base = G.split; base < G.numT; base += 64) {
                int t = base + lane;
                double lam = 1.0, tau = 0.0;
                if (t < last) { lam = lcb[2 * t]; tau = lam * G.T(t); }
                else if (t == last) { lam = lcb[2 * t]; }
                double inc = tau;                      // inclusive prefix sum over the wave
                for (int o = 1; o < 64; o <<= 1) { double u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
                double S = carry + (inc - tau);
                // e^-3S and e^-6S as powers of e^-S, expm1(-3 tau) and expm1(-6 tau) from a = expm1(-tau) by (1 + a)^3 - 1 = a (3 + a (3 + a))
                // and (1 + b)^2 - 1 = b (2 + b): two transcendentals per interval instead of six, a few ulps each way
                // (one division per interval: 1 / lam, shared by the three sums)
                const double e1 = exp(-S), e3 = e1 * e1 * e1, e6 = e3 * e3;
                const double rl = 1.0 / lam, rl3 = rl * (1.0 / 3.0), rl6 = rl * (1.0 / 6.0);
                if (t < last) {
                    const double a1 = expm1(-tau), a3 = a1 * (3.0 + a1 * (3.0 + a1)), a6 = a3 * (2.0 + a3);
                    G1 += e1 * (-a1) * rl;
                    G3 += e3 * (-a3) * rl3;
                    G6 += e6 * (-a6) * rl6;
                } else if (t == last) {
                    G1 += e1 * rl; G3 += e3 * rl3; G6 += e6 * rl6;
                }
                carry += bcast(inc, 63);
            }
            {
                // the three sums over the wave together (see the class sums above): 7 shuffles instead of 18; lanes 0-15 end up
                // with G1, 16-31 with G3, 32-47 with G6
                const bool h5 = lane & 32, h4 = lane & 16;
                const double k0 = (h5 ? G6 : G1) + __shfl_xor(h5 ? G1 : G6, 32, 64);     // G1 | G6
                const double k1 = (h5 ? 0.0 : G3) + __shfl_xor(h5 ? G3 : 0.0, 32, 64);    // G3 | 0
                double z = (h4 ? k1 : k0) + __shfl_xor(h4 ? k0 : k1, 16, 64);             // lanes 0-15: G1, 16-31: G3, 32-47: G6, 48-63: 0
                z += __shfl_xor(z, 8, 64); z += __shfl_xor(z, 4, 64); z += __shfl_xor(z, 2, 64); z += __shfl_xor(z, 1, 64);
                G1 = bcast(z, 0); G3 = bcast(z, 16); G6 = bcast(z, 32);
            }
            // coefficient vectors of the three exponentials (after the sums: they are not live across the loop)
            double x0 = P8[0];
            const double a3[3] = {1.0, 4.0, 1.0};
            double X[3], V1[NS1], V3[NS1], V6[NS1];
            for (int i = 0; i < 3; ++i) X[i] = P8[1 + i] + a3[i] * x0 / 3.0;
            // b[j][i]: 3-lineage state i -> 2-lineage state 4+j (one-population generator / la)
            const double bm[4][3] = {{2, 1, 0}, {0, 1, 2}, {1, 0, 1}, {0, 1, 0}};
            V6[0] = x0; V3[0] = 0; V1[0] = 0;
            for (int i = 0; i < 3; ++i) { V6[1 + i] = -a3[i] * x0 / 3.0; V3[1 + i] = X[i]; V1[1 + i] = 0; }
            for (int j = 0; j < 4; ++j) {
                double sx = 0, sa = 0;
                for (int i = 0; i < 3; ++i) { sx += bm[j][i] * X[i]; sa += bm[j][i] * a3[i]; }
                V6[4 + j] = sa * x0 / 15.0;
                V3[4 + j] = -sx / 2.0;
                V1[4 + j] = P8[4 + j] + sx / 2.0 - sa * x0 / 15.0;
            }
            // assemble: lane c < 7 holds class c
            double j1 = 0.0;
            const unsigned w1 = lane < 7 ? c_tab.jaf1_bits[lane] : 0u;
            if (lane < 7) for (int i = 0; i < NS1; ++i) j1 += (double)(int)((w1 >> (3 * i)) & 7u) * (V1[i] * G1 + V3[i] * G3 + V6[i] * G6);
            double jc = jp + j1;
            double tot = 0.0;
            for (int c = 0; c < 7; ++c) tot += bcast(jc, c);                         // :583-584
            jn = jc / tot;                                                           // lane c < 7: class c, normalised
            if (__any(lane < 7 && !(jn == jn))) status = MISTI_NUMERIC;
        }
    }
    KSTAMP(7)
    // ---- outputs ------------------------------------------------------------
    if (lane == 0) status_out[cand] = status;
    if (lane < 7) {
        jafs_out[cand * 7 + lane] = (status == MISTI_OK) ? jn : NAN;
#ifdef MISTI_STAMP2
        jafs_out[cand * 7 + lane] = (double)(s_[lane + 1] - s_[lane]);
#endif
    }
    // ---- replicate epilogue for small replicate counts (:600-609): lane r = replicate r ----
    if (n_inline > 0) {
        const int unfolded = (m.flags & MISTI_UNFOLDED) ? 1 : 0;
        // log of class `lane` (folded: classes 0+6, 1+5, 2+4, 3), the same expression as log_class()
        const double mirror = __shfl(jn, lane < 7 ? 6 - lane : lane, 64);
        double lcl = 0.0;
        if (lane < 7 && status == MISTI_OK) lcl = unfolded ? log(jn) : (lane < 3 ? log(jn + mirror) : (lane == 3 ? log(jn) : 0.0));
        double lj[7];
        for (int i = 0; i < 7; ++i) lj[i] = bcast(lcl, i);
        if (lane < n_inline)
            llk_out[cand * n_inline + lane] = (status == MISTI_OK) ? llk_of(jsfs + (int64_t)lane * 8, consts[lane], lj, unfolded) : -INFINITY;
    }
}

// ---- chain discovery: candidates with bitwise identical parameter vectors share a chain ----
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// Every candidate is inserted into an open-addressing table keyed by the bits of its parameter
// vector (linear probing; the table was cleared during the previous batch, see setup_kernel).  The first candidate in a slot
// owns the chain and draws the chain id; equal hashes are verified against the owner's parameters
// (read-only input), so a collision costs a probe, never correctness.  Chain ids depend on the
// order of arrival - they only name buffers; no result depends on them.
// First launch of a batch, everything that depends on the inputs alone, in ONE kernel (a launch behind a long kernel
// costs its queue a scheduler round trip, which is what limits the rate with many batches in flight):
//   blocks [0, cand_blocks)   chain discovery, one thread per candidate; on the way every thread clears a slice of the
//                             OTHER chain table - the tables are double-buffered, the next batch of this context finds
//                             its table clean without a launch of its own (nothing of the previous batch is running:
//                             same stream);
//   block cand_blocks         dispatch order: candidates sorted by descending split index (counting sort).  Work per
//                             candidate grows with the number of two-population intervals and the dispatcher hands
//                             blocks out in index order, so the longest start first.  The order never affects a result;
//   the blocks after it       llh_const of every replicate.
__global__ __launch_bounds__(256)
void setup_kernel(DevModel m, int64_t n, const double* __restrict__ params, const double* __restrict__ split_time, ChainBufs cb,
                  int cand_blocks, int32_t* __restrict__ order, int64_t n_rep, const double* __restrict__ jsfs, double* __restrict__ consts, int unfolded) {
    const int numT = m.numT, P = m.n_param, NB2 = cb.bounds ? 2 * m.n_band : 0, NPU = cb.pulse_times ? m.n_pulse : 0;
    if ((int)blockIdx.x > cand_blocks) {
        const int64_t r = (int64_t)((int)blockIdx.x - cand_blocks - 1) * blockDim.x + threadIdx.x;
        if (r < n_rep) consts[r] = llh_const_of(jsfs + r * 8, unfolded);
        return;
    }
    constexpr int SORT_SUB = 32;       // copies of every bin of the candidate sort (lane mod 32 picks one: fewer conflicts, and - measured - a dispatch order within a split that kernel 2 likes better: 0.39 -> 0.36 ms on config2x16)
    __shared__ int hist[(MISTI_MAX_NUMT + 4) * SORT_SUB];
    if ((int)blockIdx.x == cand_blocks) {
        if (cb.unsorted & 1) return;          // one split for all (the caller says): candidates are dispatched in their own order (below)
        const int nb = numT + 3;
        for (int i = threadIdx.x; i < nb * SORT_SUB; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        const int sub = threadIdx.x & (SORT_SUB - 1);
        auto key = [&](double st) { int k = (st >= 0 && st < (double)(numT + 1)) ? (int)st : 0; return (numT + 1 - k) * SORT_SUB + sub; };
        // One block for the whole batch (a counting sort by descending split index).  Two things bound it, both measured on 65 536
        // candidates (0.095 ms of this kernel's 0.12): the latency of the global load of a trip - hence SORT_ILP loads in flight per
        // thread - and the shared-memory atomics: a sweep is ordered split-major, so the 64 lanes of a wave hit ONE bin, a 64-way
        // conflict per instruction - hence SORT_SUB copies of every bin (a 2-way conflict), summed in the prefix step.
        constexpr int SORT_ILP = 8;
        const int64_t step = SORT_ILP * (int64_t)blockDim.x;
        for (int64_t i0 = threadIdx.x; i0 < n; i0 += step) {
            double st[SORT_ILP];
#pragma unroll
            for (int u = 0; u < SORT_ILP; ++u) { const int64_t i = i0 + u * (int64_t)blockDim.x; st[u] = i < n ? split_time[i] : 0.0; }
#pragma unroll
            for (int u = 0; u < SORT_ILP; ++u) if (i0 + u * (int64_t)blockDim.x < n) atomicAdd(&hist[key(st[u])], 1);
        }
        __syncthreads();
        // exclusive prefix over (bin, copy): within a bin by its thread, over the bins by thread 0
        __shared__ int bin_base[MISTI_MAX_NUMT + 4];
        for (int b = threadIdx.x; b < nb; b += blockDim.x) {
            int acc = 0;
            for (int c = 0; c < SORT_SUB; ++c) { const int v = hist[b * SORT_SUB + c]; hist[b * SORT_SUB + c] = acc; acc += v; }
            bin_base[b] = acc;
        }
        __syncthreads();
        if (threadIdx.x == 0) { int acc = 0; for (int b = 0; b < nb; ++b) { const int c = bin_base[b]; bin_base[b] = acc; acc += c; } }
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += blockDim.x) for (int c = 0; c < SORT_SUB; ++c) hist[b * SORT_SUB + c] += bin_base[b];
        __syncthreads();
        for (int64_t i0 = threadIdx.x; i0 < n; i0 += step) {
            double st[SORT_ILP];
            int pos[SORT_ILP];
#pragma unroll
            for (int u = 0; u < SORT_ILP; ++u) { const int64_t i = i0 + u * (int64_t)blockDim.x; st[u] = i < n ? split_time[i] : 0.0; }
#pragma unroll
            for (int u = 0; u < SORT_ILP; ++u) pos[u] = i0 + u * (int64_t)blockDim.x < n ? atomicAdd(&hist[key(st[u])], 1) : 0;
#pragma unroll
            for (int u = 0; u < SORT_ILP; ++u) { const int64_t i = i0 + u * (int64_t)blockDim.x; if (i < n) order[pos[u]] = (int32_t)i; }
        }
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    {   // clear the other table for the next batch
        const int64_t tsize = (int64_t)cb.tmask + 1, nthr = (int64_t)cand_blocks * blockDim.x;
        for (int64_t k = i; k < tsize; k += nthr) { cb.z_table[k] = 0; cb.z_slot_len[k] = 0; cb.z_slot_keep[k] = 0; }
        if (i == 0) { cb.z_n_chains[0] = 0; cb.z_n_chains[1] = 0; cb.z_n_chains[2] = 0; cb.z_n_chains[3] = 0; }
    }
    if (i < n) {
        if (cb.unsorted & 1) order[i] = (int32_t)i;
        // the key: the parameter bits and, with per-candidate band bounds, the (start, end) pairs as given (end == -1
        // stays symbolic: members of a chain may differ in their split, never in where a band starts or ends) and, with
        // per-candidate pulse times, the times as given (the pulse acts on the pair state, CorrectLambdas :315-323)
        uint64_t h = 0x243f6a8885a308d3ull;
        const double* a = params + i * P;
        const int32_t* ab = cb.bounds ? cb.bounds + i * NB2 : nullptr;
        for (int k = 0; k < P; ++k) h = mix64(h ^ (uint64_t)__double_as_longlong(a[k]));
        if (ab) for (int k = 0; k < NB2; ++k) h = mix64(h ^ (uint64_t)(uint32_t)ab[k]);
        const int32_t* ap = cb.pulse_times ? cb.pulse_times + i * NPU : nullptr;
        if (ap) for (int k = 0; k < NPU; ++k) h = mix64(h ^ (uint64_t)(uint32_t)ap[k]);
        const double st = split_time[i];
        // a candidate without a valid split time (an EMPTY SLOT of a batched search: negative) starts probing at a slot of its own:
        // thousands of them carry one and the same parameter vector, and their inserts would queue on one table entry (measured:
        // the 32 768 empty slots of a Nelder-Mead shrink batch made this kernel 0.72 ms).  Where they end up sharing a chain it is
        // a chain of no intervals.
        if (!(st >= 0)) h = mix64(h ^ (uint64_t)i);
        uint32_t sl = (uint32_t)(h >> 20) & cb.tmask;
        for (;;) {
            const int prev = atomicCAS(&cb.table[sl], 0, (int)i + 1);
            if (prev == 0) {
                const int ch = atomicAdd(cb.n_chains, 1);
                cb.chain_slot[ch] = (int32_t)sl;
                cb.rep[ch] = (int32_t)i;
                cb.slot_chain[sl] = ch;
                if (cb.unsorted & 2) cb.chain_order[ch] = ch;
                break;
            }
            const double* b = params + (int64_t)(prev - 1) * P;
            bool same = true;
            for (int k = 0; k < P; ++k) if (__double_as_longlong(a[k]) != __double_as_longlong(b[k])) same = false;
            if (ab) { const int32_t* bbp = cb.bounds + (int64_t)(prev - 1) * NB2; for (int k = 0; k < NB2; ++k) if (ab[k] != bbp[k]) same = false; }
            if (ap) { const int32_t* pp = cb.pulse_times + (int64_t)(prev - 1) * NPU; for (int k = 0; k < NPU; ++k) if (ap[k] != pp[k]) same = false; }
            if (same) break;
            sl = (sl + 1) & cb.tmask;
        }
        cb.slot_of[i] = (int32_t)sl;
        int need = 0;
        if (st >= 0 && st <= (double)numT) { need = (int)st; if (need > numT - 1) need = numT - 1; }   // full intervals before the (fractional) split
        atomicMax(&cb.slot_len[sl], need);
        // from which interval on this candidate reads its chain's trunk (candidates without a value read nothing)
        Grid G;
        if (setup_candidate(m, st, P ? a : nullptr, G, ab, ap) == MISTI_OK) {
            int t_own = trunk_leave(m, G);
            t_own = t_own < 0 ? 0 : (t_own > numT - 1 ? numT - 1 : t_own);
            atomicMax(&cb.slot_keep[sl], numT - t_own);
        }
    }
    // The last candidate block to finish (a) sorts the chains by descending length - the dispatch order of the chain launch:
    // workgroups pull chains from a queue, the longest first - and (b) tells the host how many chains there are: pinned memory,
    // {chains, candidates, batch tag}; the host uses it for the launch shape of kernel 1 (this batch if it cares to wait a few
    // microseconds, else the next).  Lengths and owners were written by other blocks: read at device scope.
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        is_last = atomicAdd(&cb.n_chains[1], 1) == cand_blocks - 1;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    const int nch = __hip_atomic_load(cb.n_chains, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cb.unsorted & 2) {                                   // one length for all chains (the caller says): the order of arrival will do
        if (cb.hint && threadIdx.x == 0) { cb.hint[0] = nch; cb.hint[1] = (int32_t)n; __threadfence_system(); cb.hint[2] = cb.seq; }
        return;
    }
    auto len_of = [&](int ch) {
        const int sl = __hip_atomic_load(&cb.chain_slot[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int L = __hip_atomic_load(&cb.slot_len[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return numT - (L < 0 ? 0 : (L > numT ? numT : L));                                   // key 0 = the longest
    };
    for (int k = threadIdx.x; k < numT + 2; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    for (int ch = threadIdx.x; ch < nch; ch += blockDim.x) atomicAdd(&hist[len_of(ch)], 1);
    __syncthreads();
    if (threadIdx.x == 0) { int acc = 0; for (int b = 0; b < numT + 2; ++b) { int c = hist[b]; hist[b] = acc; acc += c; } }
    __syncthreads();
    for (int ch = threadIdx.x; ch < nch; ch += blockDim.x) { const int pos = atomicAdd(&hist[len_of(ch)], 1); cb.chain_order[pos] = ch; }
    if (cb.hint && threadIdx.x == 0) {
        cb.hint[0] = nch;
        cb.hint[1] = (int32_t)n;
        __threadfence_system();
        cb.hint[2] = cb.seq;
    }
}

uint32_t chain_table_size(int64_t n_cand) {
    uint32_t t = 64;
    while ((int64_t)t < 2 * n_cand) t <<= 1;
    return t;
}

hipError_t launch_setup(const DevModel& m, int64_t n, const double* params, const double* split, const ChainBufs& cb, int32_t* order,
                        int64_t n_rep, const double* jsfs, double* consts, int unfolded, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int cand_blocks = (int)((n + 255) / 256);
    const int rep_blocks = (int)((n_rep + 255) / 256);
    hipLaunchKernelGGL(setup_kernel, dim3((unsigned)(cand_blocks + 1 + rep_blocks)), dim3(256), 0, stream, m, n, params, split, cb,
                       cand_blocks, order, n_rep, jsfs, consts, unfolded);
    return hipGetLastError();
}

// ----------------------------------------------------------- launchers -------
hipError_t upload_tables(const DevTables& t) {
    static double inv[INV_TABLE];
    inv[0] = 0.0;
    for (int k = 1; k < INV_TABLE; ++k) inv[k] = 1.0 / (double)k;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_inv), inv, sizeof inv);
    if (e != hipSuccess) return e;
    {
        // c_qmax[K]: the root in (0, K - 1) of e^-q q^(K-1) / (K-1)! = 1e-19 (the Poisson weight grows with q below its mode), by bisection
        static double qmax[QMAX_TABLE];
        qmax[0] = -1.0; qmax[1] = -1.0;
        const long double tol = logl(1e-19L);
        for (int K = 2; K < QMAX_TABLE; ++K) {
            long double lo = 0.0L, hi = (long double)(K - 1);
            for (int it = 0; it < 200; ++it) {
                const long double mid = 0.5L * (lo + hi);
                const long double lw = -mid + (long double)(K - 1) * logl(mid) - lgammal((long double)K);
                if (lw < tol) lo = mid; else hi = mid;
            }
            qmax[K] = (double)lo;
        }
        qmax[QMAX_TABLE - 1] = 1e300;           // never reached: Q_SWITCH bounds q
        e = hipMemcpyToSymbol(HIP_SYMBOL(c_qmax), qmax, sizeof qmax);
        if (e != hipSuccess) return e;
    }
    return hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &t, sizeof(DevTables));
}

size_t spectrum_lds_bytes(int numT, int wpb) { return (size_t)wpb * (128 + 2 * (numT + 1)) * sizeof(double); }

// Work items per wavefront.  Kernel 1 holds two wavefronts per SIMD (208 VGPRs), 2 048 on the chip: as few
// items per wave as keep the launch within one resident round - 1, 2, 4 - and beyond that ten (six lanes per
// item, none spare).  (Measured, 16 384 chains: 10 per wave 4.5 ms, 8 per wave 4.5 ms, 4 per wave 4.9 ms,
// 2 per wave 5.4 ms; packing also executes fewer instructions in total, which is what counts when batches
// overlap: 6.8 against 6.2 and 4.8 million evaluations/s for 10, 8 and 4 per wave.)  A chain's bits do not
// depend on the packing (tests/test_gpu_trunk.py).
int correct_cands_per_wave(int64_t n_items, const Tuning& tn) {
    const int forced = tn.cands_per_wave;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 10) return forced;
    int cpw = 1;
    while (cpw < 8 && n_items / cpw > 2048) cpw *= 2;
    return cpw == 8 ? 10 : cpw;
}

Tuning read_tuning() {
    Tuning t;
    auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; };
    auto flag = [](const char* name) { const char* e = getenv(name); return e && e[0] && e[0] != '0'; };
    t.chains_per_wave = num("MISTI_CHAINS_PER_WAVE");
    t.cands_per_wave = num("MISTI_CANDS_PER_WAVE");
    t.no_follow = flag("MISTI_NO_FOLLOW");
    t.no_trunk = flag("MISTI_NO_TRUNK");
    t.follow_max = num("MISTI_FOLLOW_MAX_CHAINS");
    t.min_blocks = num("MISTI_FOLLOW_MIN_BLOCKS");
    t.busy_contexts = getenv("MISTI_FOLLOW_BUSY_CONTEXTS") ? num("MISTI_FOLLOW_BUSY_CONTEXTS") : -1;
    t.yield_nfev = getenv("MISTI_YIELD_NFEV") ? num("MISTI_YIELD_NFEV") : -1;
    t.k2_single_waves = getenv("MISTI_K2_SINGLE_WAVES") ? num("MISTI_K2_SINGLE_WAVES") : -1;
    t.pairing = !(getenv("MISTI_FOLLOW_PAIRING") && getenv("MISTI_FOLLOW_PAIRING")[0] == '0');
    t.two_phase = !(getenv("MISTI_TWO_PHASE") && getenv("MISTI_TWO_PHASE")[0] == '0');
    t.scan_slices = num("MISTI_SCAN_SLICES");
    return t;
}

static size_t correct_lds_bytes(int numT) { return (size_t)(3 * numT - 1) * sizeof(double); }
static size_t trunk_lds_bytes(int numT) { return (128 + 2 * (size_t)(numT + 1)) * sizeof(double); }

template <bool CPFIT, int GROUP>
static void launch_chains_t(const DevModel& m, int64_t n_items, const ChainBufs& cb, const double* split, const double* params, int yield_nfev,
                            hipStream_t stream, hipEvent_t after_packed, hipError_t& event_error) {
    const int per_wave = 64 / GROUP;
    dim3 grid((unsigned)((n_items + per_wave - 1) / per_wave));
    hipLaunchKernelGGL((correct_kernel<CPFIT, GROUP>), grid, dim3(64), correct_lds_bytes(m.numT), stream, m, n_items, cb, split, params, yield_nfev);
    // phase 1 of what follows the chains starts here, beside the resume launch.  A record that fails must fail the batch: the side
    // stream's wait on a never-recorded (or stale) event is a no-op, and phase 1 would race this launch.
    if (after_packed) event_error = hipEventRecord(after_packed, stream);
    if (yield_nfev > 0 && GROUP != 64) {
        // the chains that yielded, one per wave: as many workgroups as are resident (two waves per SIMD for --cpfit, one for the
        // default fit); those beyond the list's length leave at once
        const int64_t resident = CPFIT ? 2048 : 1024;
        const int64_t blocks = n_items < resident ? n_items : resident;
        const size_t lds = (9 * (size_t)m.numT) * sizeof(double);
        hipLaunchKernelGGL((correct_resume_kernel<CPFIT>), dim3((unsigned)blocks), dim3(64), lds, stream, m, n_items, cb, split, params);
    }
}

// One chain per wavefront and a trunk to build: the trunk follows its chain inside the chain launch
// (correct_follow_kernel) instead of running after it.  MISTI_NO_FOLLOW=1 keeps it in the post launch.
bool trunk_follows(int cpw_chains, int64_t trunk_cap, const Tuning& tn) {
    return !tn.no_follow && trunk_cap > 0 && cpw_chains == 1;
}

template <bool CPFIT, int GROUP>
static void launch_post_t(const DevModel& m, int64_t n_cand, const ChainBufs& cb, const double* split, const double* params, bool follow, hipStream_t stream, int phase) {
    const int per_wave = 64 / GROUP;
    const int64_t trunk_blocks = follow ? 0 : cb.trunk_cap;
    dim3 grid((unsigned)(trunk_blocks + (n_cand + per_wave - 1) / per_wave));
    size_t lds = correct_lds_bytes(m.numT);
    if (trunk_lds_bytes(m.numT) > lds) lds = trunk_lds_bytes(m.numT);
    hipLaunchKernelGGL((post_kernel<CPFIT, GROUP>), grid, dim3(64), lds, stream, m, n_cand, cb, trunk_blocks, split, params, phase);
}

#define MISTI_DISPATCH_GROUP(FN, ...)                                                                   \
    switch (cpw) {                                                                                       \
        case 10: cp ? FN<true, 6>(__VA_ARGS__) : FN<false, 6>(__VA_ARGS__); break;                       \
        case 8: cp ? FN<true, 8>(__VA_ARGS__) : FN<false, 8>(__VA_ARGS__); break;                        \
        case 4: cp ? FN<true, 16>(__VA_ARGS__) : FN<false, 16>(__VA_ARGS__); break;                      \
        case 2: cp ? FN<true, 32>(__VA_ARGS__) : FN<false, 32>(__VA_ARGS__); break;                      \
        default: cp ? FN<true, 64>(__VA_ARGS__) : FN<false, 64>(__VA_ARGS__); break;                     \
    }

// the chains (the number of live chains is read on the device: slots beyond it exit at once)
// cpw: chains per wavefront, chosen by the caller from the expected number of chains
// est_chains: chains of the previous batch of this size on the context, or < 0 when unknown
hipError_t launch_correct(const DevModel& m, int64_t n_cand, const ChainBufs& cb, const double* split, const double* params,
                          int cpw, bool follow, int64_t est_chains, const Tuning& tn, int yield_nfev, hipStream_t stream, hipEvent_t after_packed) {
    if (n_cand <= 0) return hipSuccess;
    const bool cp = m.flags & MISTI_CPFIT;
    if (follow) {
        const size_t lds = (3 * (size_t)m.numT + 128 + 2 * (size_t)(m.numT + 1) + 2 * (size_t)m.numT + 4 + 6 * (size_t)m.numT) * sizeof(double);
        // one workgroup per chain expected, at most the resident 1 024 (two waves per SIMD; 512 for the default fit at one): the
        // workgroups pull chains from a queue, so any grid is correct and a stale hint costs at most idle or missing workgroups
        int64_t blocks = (est_chains > 0 && est_chains < n_cand) ? est_chains : n_cand;
        const int64_t resident = cp ? 1024 : 512;
        if (blocks > resident) blocks = resident;
        // the hint may be stale (same batch size, other parameters): never fewer than that many workgroups for a larger batch
        // (idle workgroups find the queue empty and leave at once)
        const int64_t min_blocks = tn.min_blocks > 0 ? tn.min_blocks : FOLLOW_MIN_BLOCKS;
        const int64_t floor_blocks = n_cand < min_blocks ? n_cand : min_blocks;
        if (blocks < floor_blocks) blocks = floor_blocks;
        if (cp) hipLaunchKernelGGL(correct_follow_kernel<true>, dim3((unsigned)blocks), dim3(128), lds, stream, m, n_cand, cb, split, params);
        else hipLaunchKernelGGL(correct_follow_kernel<false>, dim3((unsigned)blocks), dim3(128), lds, stream, m, n_cand, cb, split, params);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && after_packed) e = hipEventRecord(after_packed, stream);      // never left unrecorded for a caller that waits on it
        return e;
    }
    hipError_t event_error = hipSuccess;
    MISTI_DISPATCH_GROUP(launch_chains_t, m, n_cand, cb, split, params, yield_nfev, stream, after_packed, event_error)
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : event_error;
}

// chains the trunk buffer must hold for a batch of n_cand (the trunk runs only when
// n_chains * TRUNK_MIN_SHARE <= n_cand); MISTI_NO_TRUNK=1 in the environment disables it
int64_t trunk_capacity(int64_t n_cand, const Tuning& tn) {
    if (tn.no_trunk) return 0;
    const int64_t cap = n_cand / TRUNK_MIN_SHARE;
    return cap < TRUNK_MAX_CHAINS ? cap : TRUNK_MAX_CHAINS;   // beyond that many chains candidates walk their own intervals
}

// trunks + tails in one launch, then the candidates (with the replicate epilogue when n_rep is small)
hipError_t launch_spectrum(const DevModel& m, int64_t n_cand, const int32_t* order, const double* split, const double* params,
                           const ChainBufs& cb, double* lc_out, double* pr_out, double* jafs, int32_t* status, double* diag,
                           int64_t n_rep, const double* jsfs, const double* consts, double* llk, bool follow, bool skip_post, bool single_waves,
                           const Tuning& tn, hipStream_t stream, int phase) {
    if (n_cand <= 0) return hipSuccess;
    const bool cp = m.flags & MISTI_CPFIT;
    const int cpw = correct_cands_per_wave(n_cand, tn);          // tails: one item per candidate
    // skip_post: the caller knows there is nothing for the post launch to do (no trunk left for it and no fractional split: run_dev)
    if (!skip_post) { MISTI_DISPATCH_GROUP(launch_post_t, m, n_cand, cb, split, params, follow, stream, phase) }
    if (!cp) {
        const int64_t threads = n_cand * (int64_t)(m.numT + 1);
        hipLaunchKernelGGL(postsplit_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, m, n_cand, split, params, cb);
    }
    const int n_inline = (n_rep > 0 && n_rep <= LLK_INLINE_MAX) ? (int)n_rep : 0;
    const int wpb = single_waves ? 1 : WAVES_PER_BLOCK;
    dim3 grid((unsigned)((n_cand + wpb - 1) / wpb));
#define MISTI_SPECTRUM_LAUNCH(CP, W)                                                                                                   \
    hipLaunchKernelGGL((spectrum_kernel<CP, W>), grid, dim3(W * 64), spectrum_lds_bytes(m.numT, W), stream,                            \
                       m, n_cand, order, split, params, cb, lc_out, pr_out, jafs, status, diag, n_inline, jsfs, consts, llk, phase)
    if (cp) { if (single_waves) MISTI_SPECTRUM_LAUNCH(true, 1); else MISTI_SPECTRUM_LAUNCH(true, WAVES_PER_BLOCK); }
    else { if (single_waves) MISTI_SPECTRUM_LAUNCH(false, 1); else MISTI_SPECTRUM_LAUNCH(false, WAVES_PER_BLOCK); }
#undef MISTI_SPECTRUM_LAUNCH
    return hipGetLastError();
}

hipError_t launch_forward(const DevModel& m, int64_t n_cand, const double* split, const double* params, int hold_mu, double* lh_out, double* pr_out,
                          int32_t* status, hipStream_t stream) {
    if (n_cand <= 0) return hipSuccess;
    hipLaunchKernelGGL(forward_kernel, dim3((unsigned)((n_cand + 63) / 64)), dim3(64), 0, stream, m, n_cand, split, params, hold_mu, lh_out, pr_out, status);
    return hipGetLastError();
}

hipError_t launch_pair_residuals(bool cpfit, int64_t n, const double* problems, double* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (cpfit) hipLaunchKernelGGL(pair_residuals_kernel<true>, grid, block, 0, stream, n, problems, out);
    else hipLaunchKernelGGL(pair_residuals_kernel<false>, grid, block, 0, stream, n, problems, out);
    return hipGetLastError();
}

hipError_t launch_lsq_probe(int kind, int64_t n, const double* problems, double* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lsq_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, kind, n, problems, out);
    return hipGetLastError();
}

}  // namespace misti
