// The 44-state two-population propagation: one interval by the uniformisation series or the contour quadrature (twopop_interval),
// the smoothing of the corrected rates, and the trunk a chain's candidates share (trunk_body in post_kernel, trunk_follow in
// correct_follow_kernel).  Also instantiated by spectrum_kernel for a candidate's own intervals.  Held by
// tests/test_gpu_exact_spectrum.py, test_gpu_trunk.py and test_gpu_golden.py.
#pragma once
#include <stdint.h>

#include "misti_chain.h"
#include "misti_device.h"
#include "misti_kernel_tables.h"
#include "misti_model.h"
#include "misti_wave.h"

namespace misti {

// ---- two-population propagation shared by the trunk and the candidate kernel ----
// Row view of the 44-state generator for state `lane`, kept in registers.
struct TwoPopRow {
    int srcl[MAXNZ], knd[MAXNZ];
    double mlt[MAXNZ];
    double dc0, dc1, dc2, dc3;
    bool live;
    __device__ __forceinline__ void load(int lane) {
        for (int n = 0; n < MAXNZ; ++n) { srcl[n] = c_tab.src[n][lane]; knd[n] = c_tab.kind[n][lane]; mlt[n] = (double)c_tab.mult[n][lane]; }
        dc0 = c_tab.dcnt[0][lane]; dc1 = c_tab.dcnt[1][lane]; dc2 = c_tab.dcnt[2][lane]; dc3 = c_tab.dcnt[3][lane];
        live = lane < NS2;
    }
};

// AncientSampleP0 (TwoPopulations.py:246-262)
__device__ __forceinline__ void ancient_project(double* xbuf, int lane, double& x) {
    xbuf[lane] = x; lds_fence();
    double nx = 0.0;
    for (int a = 0; a < 2; ++a) if (lane == c_tab.anc_dst[a]) for (int j = 0; j < c_tab.anc_n[a]; ++j) nx += xbuf[c_tab.anc_src[a][j]];
    lds_fence();
    x = nx;
}

// Uniformisation series of one (sub-)interval of length T with q = (largest exit rate) x T <= Q_SWITCH (up to rounding):
// M T = N - q I, p_{k+1} = N p_k/(k+1), i_{k+1} = (T p_k + q i_k)/(k+1); x <- e^{M T} x, wint <- int_0^T e^{M s} x ds
// (this lane's state).  dT: this state's exit rate x T; cf: the generator's off-diagonal entries of this row x T.
__device__ __forceinline__ void series_step(const TwoPopRow& R, double* xbuf, int lane, double q, double T, double dT, const double* cf,
                                            double& x, double& wint) {
    const double dg = q - dT;
    const double eq = exp(-q);
    double p = eq * x, ii = 0.0;
    double accp = p, acci = 0.0;
    // the number of terms from q alone (q is the same in every lane): see c_qmax
    int K = 1;
    for (int c = 0; c < QMAX_TABLE / 64; ++c) {
        const unsigned long long below = __ballot(c_qmax[1 + 64 * c + lane] < q);
        K += __popcll(below);
        if (below != ~0ull) break;
    }
    double inv_next = c_inv[1];
    for (int k = 1; k <= K; ++k) {
        const double inv = inv_next;
        inv_next = c_inv[k + 1];
        // (the four source states: an LDS write and four reads; the same gather through ds_bpermute was measured slower - config 3's
        // kernel 2 1.27 -> 1.62 ms)
        xbuf[lane] = p;
        lds_fence();
        double r0 = xbuf[R.srcl[0]], r1 = xbuf[R.srcl[1]], r2 = xbuf[R.srcl[2]], r3 = xbuf[R.srcl[3]];
        lds_fence();
        double pn = (dg * p + ((cf[0] * r0 + cf[1] * r1) + (cf[2] * r2 + cf[3] * r3))) * inv;
        ii = (T * p + q * ii) * inv;
        p = pn;
        accp += p; acci += ii;
    }
    x = accp; wint = acci;
}

// The series over n_sub equal sub-steps of an interval (q / n_sub <= Q_SWITCH each): end state and occupation integral
// accumulate.  Out of line: only intervals whose contour solve failed come here, and inlined it would cost the spectrum
// kernel registers on its hot path.  Returns (e^{M T} x, int_0^T e^{M s} x ds) of this lane's state.
__device__ __noinline__ double2 series_substeps(int s0, int s1, int s2, int s3, double c0, double c1, double c2, double c3, double* xbuf,
                                                int lane, int n_sub, double q, double T, double dT, double x) {
    TwoPopRow R;
    R.srcl[0] = s0; R.srcl[1] = s1; R.srcl[2] = s2; R.srcl[3] = s3;
    const double f = 1.0 / n_sub;
    const double cf[MAXNZ] = {c0 * f, c1 * f, c2 * f, c3 * f};
    double wint = 0.0;
    for (int j = 0; j < n_sub; ++j) {
        double wj;
        series_step(R, xbuf, lane, q * f, T * f, dT * f, cf, x, wj);
        wint += wj;
    }
    return make_double2(x, wint);
}

// One interval of the two-population loop (JAFSpectrum :483-502): pulse at the start of the
// interval, then x <- exp(M T) x and the occupation integral added to w_pre / w_post.
// lcb: this wave's (smoothed) rates in LDS.  Returns MISTI_OK / MISTI_NUMERIC / MISTI_STIFF.
__device__ __forceinline__ int twopop_interval(const TwoPopRow& R, const DevModel& m, const Model& mod, const Grid& G, const double* lcb,
                                               double* xbuf, int lane, int t, double& x, double& w_pre, double& w_post) {
    double pu0, pu1, mu0, mu1;
    mod.pulse(t, pu0, pu1);
    mod.mig(t, mu0, mu1);
    double pr = pu0 + pu1;
    if (pr > 0) {
        // PulseMigration (TwoPopulations.py:361-377)
        int from = pu0 > 0 ? 0 : 1;
        xbuf[lane] = x; lds_fence();
        double pw_s[5], pw_m[5];
        pw_s[0] = pw_m[0] = 1.0;
        for (int i = 1; i < 5; ++i) { pw_s[i] = pw_s[i - 1] * (1.0 - pr); pw_m[i] = pw_m[i - 1] * pr; }
        double nx = 0.0;
        int n = R.live ? c_tab.pulse_n[from][lane] : 0;
        for (int j = 0; j < n; ++j) {
            int ab = c_tab.pulse_ab[from][lane][j];
            int mul = ab >> 8, a = (ab >> 4) & 15, b = ab & 15;
            nx += xbuf[c_tab.pulse_src[from][lane][j]] * ((double)mul * pw_s[a] * pw_m[b]);
        }
        lds_fence();
        x = nx;
    }
    double la0 = lcb[2 * t], la1 = lcb[2 * t + 1];
    const double T = G.T(t);
    // largest total exit rate over the 44 states (4 lineages dominate)
    double r40 = 6 * la0 + 4 * mu0, r04 = 6 * la1 + 4 * mu1;
    double r31 = 3 * la0 + 3 * mu0 + mu1, r13 = 3 * la1 + 3 * mu1 + mu0;
    double r22 = la0 + la1 + 2 * mu0 + 2 * mu1;
    const double q = T * fmax(fmax(r40, r04), fmax(fmax(r31, r13), r22));
    if (!(q < 1e300)) return MISTI_NUMERIC;
    double rate[4] = {la0, la1, mu0, mu1};
    double cf[MAXNZ];
    for (int n = 0; n < MAXNZ; ++n) cf[n] = R.mlt[n] * rate[R.knd[n]] * T;
    const double dT = (R.dc0 * la0 + R.dc1 * la1 + R.dc2 * mu0 + R.dc3 * mu1) * T;   // exit rate x T of this state
    double wint = 0.0;
    if (q <= Q_SWITCH) {
        series_step(R, xbuf, lane, q, T, dT, cf, x, wint);
    } else {
        // Talbot contour, conjugate pairs folded: f = 2 Re sum_{k upper} (-c_k) (z_k - M T)^-1 x
        double accp = 0.0, acci = 0.0;
        bool solved = true;
        for (int nd = 0; nd < TALBOT_HALF && solved; ++nd) {
            const double zr = c_tab.tal_zr[nd], zi = c_tab.tal_zi[nd], cr = c_tab.tal_cr[nd], ci = c_tab.tal_ci[nd];
            const double ar = zr + dT, ai = zi;
            const double den = 1.0 / (ar * ar + ai * ai);
            const double ir = ar * den, im = -ai * den;              // 1 / (z + D_i)
            double xr = x * ir, xi = x * im;
            // Stop test: every lane's change below 4e-16 of its own value.  Past JACOBI_WATCH sweeps (the coalescence part is
            // nilpotent: a solve that is not done by then has two-way migration), every 8th sweep, against the wave's largest component
            // instead - a lane-relative test never fires where a small component alternates between two roundings - and from
            // JACOBI_FLOOR sweeps on 1e-14 of it is accepted (the rounding floor of such a limit cycle).  An iterate above
            // JACOBI_BLOWUP diverges (spectral radius > 1 at nodes left of the origin; the right-hand side is a probability
            // vector, and the contour sum of iterates that large would have lost every digit anyway); that, or no end in
            // JACOBI_MAX sweeps: the interval is taken by the series in sub-steps instead.
            // one sweep; d: this lane's change, sz: its new magnitude
            auto sweep = [&](double& d, double& sz) {
                xbuf[lane] = xr; xbuf[64 + lane] = xi;
                lds_fence();
                double sr = x + ((cf[0] * xbuf[R.srcl[0]] + cf[1] * xbuf[R.srcl[1]]) + (cf[2] * xbuf[R.srcl[2]] + cf[3] * xbuf[R.srcl[3]]));
                double si = (cf[0] * xbuf[64 + R.srcl[0]] + cf[1] * xbuf[64 + R.srcl[1]]) + (cf[2] * xbuf[64 + R.srcl[2]] + cf[3] * xbuf[64 + R.srcl[3]]);
                lds_fence();
                double nr = sr * ir - si * im, ni = sr * im + si * ir;
                d = fabs(nr - xr) + fabs(ni - xi);
                sz = fabs(nr) + fabs(ni);
                xr = nr; xi = ni;
            };
            int it = 0;
            for (; it < JACOBI_WATCH; ++it) {               // the common case, kept tight
                double d, sz;
                sweep(d, sz);
                if (!__any(d > 4e-16 * sz + 1e-300)) break;
            }
            if (it == JACOBI_WATCH) {
                for (; it < JACOBI_MAX; ++it) {
                    double d, sz;
                    sweep(d, sz);
                    if (!__any(d > 4e-16 * sz + 1e-300)) break;
                    if (it & 7) continue;                       // (every 8th sweep: the wave reduction costs)
                    for (int o = 32; o > 0; o >>= 1) sz = fmax(sz, __shfl_xor(sz, o, 64));
                    if (!(sz <= JACOBI_BLOWUP)) { it = JACOBI_MAX; break; }
                    if (!__any(d > (it < JACOBI_FLOOR ? 4e-16 : 1e-14) * sz + 1e-300)) break;
                }
            }
            if (it >= JACOBI_MAX) { solved = false; break; }
            const double wr = -(cr * xr - ci * xi), wi = -(cr * xi + ci * xr);
            const double zz = 1.0 / (zr * zr + zi * zi);
            const double gr = T * zr * zz, gi = -T * zi * zz;        // T / z
            accp += 2.0 * wr;
            acci += 2.0 * (wr * gr - wi * gi);
        }
        if (solved) {
            x = accp; wint = acci;
        } else {
            // the series over n sub-steps of q / n <= Q_SWITCH each: end state and occupation integral accumulate, every
            // term stays non-negative
            const int n_sub = (int)ceil(q / Q_SWITCH);
            if (n_sub > SUBSTEP_MAX) return MISTI_STIFF;
            const double2 r = series_substeps(R.srcl[0], R.srcl[1], R.srcl[2], R.srcl[3], cf[0], cf[1], cf[2], cf[3], xbuf, lane, n_sub, q, T, dT, x);
            x = r.x; wint = r.y;
        }
    }
    if (t < m.sample_date) w_pre += wint; else w_post += wint;
    return MISTI_OK;
}

// time-weighted mean of genome k's rates over intervals [a, b) (one smoothing run, :392-403)
__device__ __forceinline__ double run_mean(const double* lc, int k, int a, int b, const Grid& G) {
    double acc = 0.0, tt = 0.0;
    for (int j = a; j < b; ++j) { double Tj = G.T(j); acc += lc[2 * j + k] * Tj; tt += Tj; }
    return acc / tt;
}

// Smooth (:380-405) on a wave's rates in LDS: time-weighted mean of lc over runs of constant lh,
// t < bound; a run is cut at `bound` (the candidate's split index).
__device__ __forceinline__ void smooth_rates(const DevModel& m, const Grid& G, double* lcb, int lane, int lo, int bound) {
    // intervals lo <= t < bound are smoothed (lo > 0: the caller does not need the others); wave-uniform skip of
    // the 64-interval slices outside that range
    double sm[SMOOTH_REPS][2];   // intervals rep*64+lane, both genomes
#pragma unroll
    for (int rep = 0; rep < SMOOTH_REPS; ++rep) {
        sm[rep][0] = sm[rep][1] = 0.0;
        if (rep * 64 >= bound || rep * 64 + 63 < lo) continue;
        int t = rep * 64 + lane;
        for (int k = 0; k < 2; ++k) {
            double v = 0.0;
            if (t >= lo && t < bound) {
                int a = m.run_start[k * m.numT + t];
                int b = m.run_end[k * m.numT + t];
                if (b > bound) b = bound;
                v = run_mean(lcb, k, a, b, G);
            }
            sm[rep][k] = v;
        }
    }
    lds_fence();
#pragma unroll
    for (int rep = 0; rep < SMOOTH_REPS; ++rep) {
        int t = rep * 64 + lane;
        if (t >= lo && t < bound) { lcb[2 * t] = sm[rep][0]; lcb[2 * t + 1] = sm[rep][1]; }
    }
    lds_fence();
}

// Trunk kernel.  Candidates of one chain (same parameters, different split) propagate the 44-state
// chain through the SAME intervals with the SAME rates up to the smoothing run their split cuts:
// the rates of interval t, the migration rates and the pulses do not depend on the split as long
// as every smoothing run touching [0, t] ends at or before it.  One wavefront per chain walks the
// chain's intervals once and stores, before each interval t, the state vector and both occupation
// integrals (3 x 44 doubles); a candidate then starts from the record of the first interval whose
// run its split cuts (t_own in spectrum_kernel) and adds only its own 0-5 intervals - on a
// split x rate grid ~14x less propagation work.  The arithmetic per interval is the same code
// (twopop_interval) on the same inputs, so a candidate's result is bit-identical with or without
// the trunk (tests/test_gpu_trunk.py).
// Active only when sharing pays: n_chains * TRUNK_MIN_SHARE <= n_cand (decided on the device, the
// chain count never visits the host).
__device__ __forceinline__ bool trunk_active(const ChainBufs& cb, int64_t n_cand) {
    const int64_t nch = cb.n_chains[0];
    return cb.trunk_cap > 0 && nch <= cb.trunk_cap && nch * TRUNK_MIN_SHARE <= n_cand;
}

__device__ __forceinline__
void trunk_body(const DevModel& m, int64_t n_cand, const double* __restrict__ params, const ChainBufs& cb, int64_t ch, double* lds, int phase = 0) {
    const int lane = lane_id();
    if (!trunk_active(cb, n_cand) || ch >= cb.n_chains[0]) return;
    if (wrong_phase(cb, ch, phase)) return;
    double* xbuf = lds;
    double* lcb = lds + 128;
    const int ft = cb.fail_t[ch];
    int Lt = chain_len(cb, ch);
    if (ft < Lt) Lt = ft;                                   // members beyond the failing interval have no value anyway
    const double* par = params ? params + (int64_t)cb.rep[ch] * m.n_param : nullptr;
    Grid G;
    G.times = m.times; G.lh = m.lh; G.numT0 = m.numT; G.numT = m.numT; G.split = Lt; G.ins = -1; G.frac = 0.0;
    Model mod{&m, par, Lt, {0, 0, 0, 0}};
    mod.bb = cb.bounds ? cb.bounds + (int64_t)cb.rep[ch] * 2 * m.n_band : nullptr;
    mod.pt = cb.pulse_times ? cb.pulse_times + (int64_t)cb.rep[ch] * m.n_pulse : nullptr;
    mod.cache();
    const double* lc_ch = cb.lc + ch * (int64_t)m.numT * 2;
    for (int i = lane; i < 2 * (m.numT + 1); i += 64) lcb[i] = ((i >> 1) < Lt) ? lc_ch[i] : 0.0;
    lds_fence();
    if (m.flags & MISTI_SMOOTH) smooth_rates(m, G, lcb, lane, 0, Lt);
    TwoPopRow R;
    R.load(lane);
    double x = (lane == 2) ? 1.0 : 0.0;
    double w_pre = 0.0, w_post = 0.0;
    double* rec = cb.trunk + ch * (int64_t)m.numT * TRUNK_REC;
    // Records are read from the first interval at which a member leaves the trunk (setup_kernel: slot_keep), only at intervals
    // where SOME split can leave it (m.leave_ok: with smoothing, starts of the runs a split can cut - a function of the model,
    // computed in misti_create) - and at the interval the trunk ends on, wherever that is.  On the headline grid a third of the
    // records lies before the first split and three quarters of the rest inside runs: never read, no longer written.
    const int t_first = m.numT - cb.slot_keep[cb.chain_slot[ch]];
    auto store = [&](int t, double xs, double ws0, double ws1) {
        if (R.live) { double* r = rec + (int64_t)t * TRUNK_REC; r[lane] = xs; r[NS2 + lane] = ws0; r[2 * NS2 + lane] = ws1; }
    };
    int ok = 0;
    bool stored = false;
    double xs = x, ws0 = w_pre, ws1 = w_post;
    for (int t = 0; t < m.numT; ++t) {
        xs = x; ws0 = w_pre; ws1 = w_post;
        stored = t >= t_first && m.leave_ok[t] != 0;
        if (stored) store(t, xs, ws0, ws1);
        ok = t;
        if (t >= Lt) break;
        if (t == m.sample_date) ancient_project(xbuf, lane, x);
        if (twopop_interval(R, m, mod, G, lcb, xbuf, lane, t, x, w_pre, w_post) != MISTI_OK) break;
    }
    if (!stored) store(ok, xs, ws0, ws1);
    if (lane == 0) cb.trunk_ok[ch] = ok;
}

// The trunk as a FOLLOWER of its chain: second wavefront of the chain's workgroup
// (correct_follow_kernel).  The chain wave hands over each corrected interval through LDS (rates,
// then a count); this wave propagates interval t as soon as the smoothing runs containing t are
// complete, so the trunk is finished almost when the chain is - its ~0.3 ms leave the critical
// path of a batch.  Same records, same arithmetic as trunk_body (run_mean + twopop_interval).  Both
// waves are resident by construction (one workgroup), and the wait is bounded: a follower that gives up
// publishes the prefix it has, which is all the candidate kernel relies on (trunk_ok).
__device__ __forceinline__
void trunk_follow(const DevModel& m, int64_t n_cand, const double* __restrict__ params, const ChainBufs& cb, int64_t ch, double* lds,
                  const double* lc_sh, volatile int* flags) {
    const int lane = lane_id();
    if (!trunk_active(cb, n_cand) || ch >= cb.n_chains[0]) return;
    double* xbuf = lds;
    double* lcb = lds + 128;
    const int len = chain_len(cb, ch);
    const double* par = params ? params + (int64_t)cb.rep[ch] * m.n_param : nullptr;
    Grid G;
    G.times = m.times; G.lh = m.lh; G.numT0 = m.numT; G.numT = m.numT; G.split = len; G.ins = -1; G.frac = 0.0;
    Model mod{&m, par, len, {0, 0, 0, 0}};
    mod.bb = cb.bounds ? cb.bounds + (int64_t)cb.rep[ch] * 2 * m.n_band : nullptr;
    mod.pt = cb.pulse_times ? cb.pulse_times + (int64_t)cb.rep[ch] * m.n_pulse : nullptr;
    mod.cache();
    for (int i = lane; i < 2 * (m.numT + 1); i += 64) lcb[i] = 0.0;
    lds_fence();
    TwoPopRow R;
    R.load(lane);
    double x = (lane == 2) ? 1.0 : 0.0;
    double w_pre = 0.0, w_post = 0.0;
    double* rec = cb.trunk + ch * (int64_t)m.numT * TRUNK_REC;
    const bool smooth = m.flags & MISTI_SMOOTH;
    const int t_first = m.numT - cb.slot_keep[cb.chain_slot[ch]];         // see trunk_body
    auto store = [&](int t, double xs, double ws0, double ws1) {
        if (R.live) { double* r = rec + (int64_t)t * TRUNK_REC; r[lane] = xs; r[NS2 + lane] = ws0; r[2 * NS2 + lane] = ws1; }
    };
    int ok = 0, have = 0, done = 0;
    bool stored = false;
    double xs = x, ws0 = w_pre, ws1 = w_post;
    long long spins = 0;
    for (int t = 0; t < m.numT; ++t) {
        xs = x; ws0 = w_pre; ws1 = w_post;
        stored = t >= t_first && m.leave_ok[t] != 0;
        if (stored) store(t, xs, ws0, ws1);
        ok = t;
        if (t >= len) break;
        int a0 = t, b0 = t + 1, a1 = t, b1 = t + 1;
        if (smooth) { a0 = m.run_start[t]; b0 = m.run_end[t]; a1 = m.run_start[m.numT + t]; b1 = m.run_end[m.numT + t]; }
        int need = b0 > b1 ? b0 : b1;
        if (need > len) need = len;
        while (have < need && !done) {
            done = lds_get(flags + 1);             // read `done` first: the count read after it is then final
            have = lds_get(flags);
            if (have >= need || done) break;
            __builtin_amdgcn_s_sleep(16);
            if (++spins > FOLLOW_SPIN_LIMIT) break;
        }
        lds_order();                               // the rates read below were written before the count read above
        if (have < need && !done) break;           // gave up waiting: keep the prefix
        const int cut = have >= need ? len : have; // the chain ended early (failure): runs are cut where it ended
        if (t >= cut) break;
        if (b0 > cut) b0 = cut;
        if (b1 > cut) b1 = cut;
        const double l0 = smooth ? run_mean(lc_sh, 0, a0, b0, G) : lc_sh[2 * t];
        const double l1 = smooth ? run_mean(lc_sh, 1, a1, b1, G) : lc_sh[2 * t + 1];
        if (lane == 0) { lcb[2 * t] = l0; lcb[2 * t + 1] = l1; }
        lds_fence();
        if (t == m.sample_date) ancient_project(xbuf, lane, x);
        if (twopop_interval(R, m, mod, G, lcb, xbuf, lane, t, x, w_pre, w_post) != MISTI_OK) break;
    }
    if (!stored) store(ok, xs, ws0, ws1);
    if (lane == 0) cb.trunk_ok[ch] = ok;
}

}  // namespace misti
