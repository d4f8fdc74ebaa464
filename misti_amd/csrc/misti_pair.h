// The pair chain: exp(M) v of the three-state generator of one genome's two lineages by its branches (taylor3, pair_reduced,
// pair_cascade, pair_eigen, the shifted series), the expected coalescence times, and the residual of one interval (PairProblem,
// pair_eval) with the default fit's noise rule, which evaluates it (ect_reference_form, ect_noise_continues).
// Reached one problem per lane by misti_pair_residuals (pair_residuals_kernel), by forward_kernel and by every chain kernel; restated
// by tests/pair_branches.py and held against 50 digits by tests/test_gpu_pair_branches.py, test_gpu_pair_exp.py and
// test_gpu_pair_residuals.py.
#pragma once
#include <math.h>

#include "misti_kernel_tables.h"
#include "misti_lsq.h"
#include "misti_model.h"
#include "misti_wave.h"

namespace misti {

// ------------------------------------------------------------ pair chain ----
// Three states of one genome's two lineages: both in pop 0, both in pop 1, one
// in each (CorrectLambda.SetMatrix, CorrectLambda.py:55-56):
//     [ -2mu0-l0     0       mu1     ]
//     [    0      -2mu1-l1   mu0     ]
//     [  2mu0      2mu1    -mu0-mu1  ]
// v <- exp(M) v by uniformisation.  Every lane carries its own (l, v); the trip
// count is wave-uniform (bound from the largest q in the wave).
// K terms of the Taylor series of exp(M) v for the pair generator, fully unrolled.
// INT: also  vint = sum_k (M^k v / k!) / (k + 2)  =  int_0^1 u exp(u M) v du  - the default fit's expected coalescence
// time needs  M^-1 exp(M) v - M^-2 (exp(M) - I) v  (CorrectLambda.py:99-107), which is exactly that integral: the series
// has no inverse and no cancellation, where the reference's formula loses ~1/|M|^2 digits, and like the exponential it
// acts on the vector only, so a decoupled component still sees identical arithmetic in every forward-difference lane
// (the reference's finite-difference Jacobian has an exactly zero entry there; a 3x3 solve by cofactors does not keep it).
template <int K, bool INT>
__device__ __forceinline__ void taylor3(double d0, double d1, double d2, double mu0, double mu1, double v[3], Diag& dg, double vint[3]) {
    double p0 = v[0], p1 = v[1], p2 = v[2];
    double a0 = p0, a1 = p1, a2 = p2;
    double b0 = 0.5 * p0, b1 = 0.5 * p1, b2 = 0.5 * p2;
    const double twomu0 = 2.0 * mu0, twomu1 = 2.0 * mu1;
#pragma unroll
    for (int k = 1; k <= K; ++k) {
        const double inv = 1.0 / (double)k;          // a literal after unrolling
        const double t0 = (mu1 * p2 - d0 * p0) * inv;
        const double t1 = (mu0 * p2 - d1 * p1) * inv;
        const double t2 = ((twomu0 * p0 + twomu1 * p1) - d2 * p2) * inv;
        p0 = t0; p1 = t1; p2 = t2;
        a0 += p0; a1 += p1; a2 += p2;
        if (INT) { const double w2 = 1.0 / (double)(k + 2); b0 = fma(p0, w2, b0); b1 = fma(p1, w2, b1); b2 = fma(p2, w2, b2); }
    }
#if MISTI_WORK_COUNTERS
    dg.terms += K;
#endif
    v[0] = a0; v[1] = a1; v[2] = a2;
    if (INT) { vint[0] = b0; vint[1] = b1; vint[2] = b2; }
}

// Structural reduction of the pair chain.  With migration in one direction only (mu1 == 0: nothing enters "both in
// population 0") and that state empty in both genomes - it is, exactly, from the first interval in which its rate ran
// away: exp(-rate x length) underflows or falls below PAIR_EMPTY of the total - the three-state chain is the two-state one on (both in population 1, one in each), whose
// generator [[-d1, mu0], [0, -d2]] is triangular:
//     w1 = e^{-d1} v1 + mu0 phi v2,   w2 = e^{-d2} v2,   phi = (e^{-d1} - e^{-d2}) / (d2 - d1),   w0 = 0,
// three exponentials instead of a 30-45 term series or a dense scaling-and-squaring on a matrix made stiff by a rate
// (l0) that no longer enters the result.  This is exactly the solver's rank-one regime (correct_body): the Jacobian
// column of l0 is zero because l0 is not read.  Mirror case (which = 2): mu0 == 0 and "both in population 1" empty.
constexpr double PAIR_EMPTY = 1e-30;
__device__ __forceinline__ void pair_reduced(int which, double l0, double l1, double mu0, double mu1, double v[3], bool ok) {
    if (!ok) { l0 = 0.0; l1 = 0.0; }
    const double dk = which == 1 ? 2.0 * mu1 + l1 : 2.0 * mu0 + l0;      // exit rate of the state that is left
    const double d2 = mu0 + mu1;
    const double mu = which == 1 ? mu0 : mu1;                             // "one in each" -> that state
    const double vk = which == 1 ? v[1] : v[0];
    const double a = -dk, c = -d2;
    const double ax = fabs(a - c);
    const double phi = exp(fmax(a, c)) * (ax == 0.0 ? 1.0 : -expm1(-ax) / ax);
    const double wk = exp(a) * vk + mu * phi * v[2];
    const double w2 = exp(c) * v[2];
    v[0] = which == 1 ? 0.0 : wk;
    v[1] = which == 1 ? wk : 0.0;
    v[2] = w2;
    if (!ok) { v[0] = v[1] = v[2] = NAN; }
}

// exp(M) v for migration in one direction only, in closed form.  which = 1: mu1 == 0 - nothing enters "both in population 0"
// (state 0); it empties at a = 2 mu0 + l0 into "one in each" (state 2, at 2 mu0), which empties at b = mu0 into "both in
// population 1" (state 1, at mu0), which coalesces at c = l1:
//     w0 = e^-a v0,    w2 = e^-b v2 + 2 mu0 D(a, b) v0,    w1 = e^-c v1 + mu0 D(b, c) v2 + 2 mu0^2 D(a, b, c) v0
// with D the divided differences of e^{-x}:  D(x, y) = (e^-x - e^-y) / (y - x),  D(x, y, z) = (D(x, y) - D(y, z)) / (z - x).
// which = 2 is the mirror image (mu0 == 0).  Used where the generator is stiff (a rate has run away), so the largest gap
// among the three rates is large and the second difference is taken across it; D(x, y) itself goes through expm1.
__device__ __forceinline__ double dd_exp(double x, double y) {
    const double g = fabs(x - y);
    return exp(-fmin(x, y)) * (g == 0.0 ? 1.0 : -expm1(-g) / g);
}
__device__ __forceinline__ void pair_cascade(int which, double l0, double l1, double mu0, double mu1, double v[3]) {
    const double mu = which == 1 ? mu0 : mu1;
    const double a = which == 1 ? 2.0 * mu0 + l0 : 2.0 * mu1 + l1;      // exit rate of the state that is left (S)
    const double c = which == 1 ? 2.0 * mu1 + l1 : 2.0 * mu0 + l0;      // ... of the state that is entered (K)
    const double b = mu0 + mu1;                                          // ... of "one in each"
    const double vS = which == 1 ? v[0] : v[1], vK = which == 1 ? v[1] : v[0], v2 = v[2];
    // second divided difference across the largest gap: sort the three rates
    double s0 = a, s1 = b, s2 = c;
    if (s0 > s1) { const double t = s0; s0 = s1; s1 = t; }
    if (s1 > s2) { const double t = s1; s1 = s2; s2 = t; }
    if (s0 > s1) { const double t = s0; s0 = s1; s1 = t; }
    const double gap = s2 - s0;
    const double D3 = gap > 0.0 ? (dd_exp(s0, s1) - dd_exp(s1, s2)) / gap : 0.5 * exp(-s0);
    const double wS = exp(-a) * vS;
    const double w2 = exp(-b) * v2 + (2.0 * mu) * dd_exp(a, b) * vS;
    const double wK = exp(-c) * vK + mu * dd_exp(b, c) * v2 + (2.0 * mu * mu) * D3 * vS;
    v[0] = which == 1 ? wS : wK;
    v[1] = which == 1 ? wK : wS;
    v[2] = w2;
}

// exp(M) v for migration in BOTH directions, in closed form (round 5; until then the stiff two-way generator went through a dense
// degree-12 Taylor kernel and up to 17 squarings: ~2 000 instructions per evaluation, a systematic relative error of ~1e-11 at
// |M| = 1e5, and the floor of every packed launch - the resumed chains of BASELINE configs 3 and 5 spend their time there).
// In the order (both in 0, one in each, both in 1) the generator is tridiagonal with positive off-diagonal products, hence similar to
// the symmetric  [[-d0, s, 0], [s, -d2, s], [0, s, -d1]],  s^2 = 2 mu0 mu1:  three real eigenvalues -x_i, the roots of the secular
// equation   (d2 - x) = s^2 / (d0 - x) + s^2 / (d1 - x),   one below both poles d0, d1, one between them, one above, and
//     exp(M) v = sum_i e^{-x_i} r_i (l_i . v) / (l_i . r_i),     r_i = (mu1 / g0, mu0 / g1, 1),  l_i = (2 mu0 / g0, 2 mu1 / g1, 1),
//     g0 = d0 - x_i,  g1 = d1 - x_i,   l_i . r_i = 1 + s^2 / g0^2 + s^2 / g1^2
// (rows / columns 0 and 1 of (M + x) r = 0; no square root, no matrix product).  What decides the accuracy is the GAPS g0, g1, so
// every root is found in the variable "distance to the nearest pole" (as LAPACK's dlaed4 does for its secular equation): for the
// outer roots  F(t) = c + t - s^2/t - s^2/(G + t),  for the middle one  F(t) = c + t - s^2/t + s^2/(G - t)  on (0, G/2]
// (G = |d0 - d1|; c = the distance of d2 from that pole, signed) - increasing and concave, so Newton's iteration from a point left of the
// root converges monotonically, without safeguards, and two such points come from quadratics (a function above F with a computable
// root: the far pole dropped, or the near pole moved to the far one).  The smallest root when d2 lies below both poles is found as
// d2 - e instead (K(e) = e - s^2/(A0 + e) - s^2/(A1 + e), A = d - d2 > 0): the runaway rates make the poles huge and the root stays at
// d2, where a distance to a pole of 1e5 would lose eleven digits of e^{-x}.  Newton's iteration reaches rounding from the better of the two
// starts in 1 - 3 steps per root over 6 000 random generators spanning rates 1e-2 ... 3e5 and migration 1e-6 ... 3 (scratch prototype against 60-digit
// arithmetic: 7e-16 of the norm of the result in the stiff regime; the eigenvector scaling costs a factor sqrt(mu1 / mu0) where the two
// migration rates differ by orders of magnitude).  Smooth in the varied rate to a few ulps, like pair_cascade.
__device__ __forceinline__ double pe_qroot(double a, double c, double s2) {          // positive root of a t^2 + c t - s2 = 0
    const double r = sqrt64(c * c + 4.0 * a * s2);
    return c >= 0.0 ? 2.0 * s2 * rcp64(c + r) : (r - c) * rcp64(2.0 * a);
}
// Newton's steps stop for the whole wave once every lane's last correction is below PE_TOL of its root: the iteration converges
// quadratically from the left, so the correction after that one is below rounding (prototype: 1e-14 of the result's norm at worst,
// 4.4 Newton steps per evaluation for all three roots together where a fixed count needs 18).
constexpr int PE_NEWTON_MAX = 12;
constexpr double PE_TOL = 1e-9;
__device__ __forceinline__ double pe_outer(double c, double G, double s2) {
    // left starts: the far pole dropped (c + t - s2/t), or the near pole moved onto the far one (c + t - 2 s2/(G + t): t^2 + (c + G) t = 2 s2 - c G)
    const double cg = c + G, r = sqrt64((c - G) * (c - G) + 8.0 * s2);
    const double t2 = cg >= 0.0 ? 2.0 * (2.0 * s2 - c * G) * rcp64(cg + r) : 0.5 * (r - cg);
    double t = fmax(pe_qroot(1.0, c, s2), t2);
    bool done = false;                    // a lane's root is frozen by ITS OWN test: what else sits in the wave changes no bit of it
    for (int it = 0; it < PE_NEWTON_MAX; ++it) {
        const double a = rcp64(t), b = rcp64(G + t);
        const double F = ((c + t) - s2 * a) - s2 * b, dF = 1.0 + s2 * (a * a + b * b);
        const double d = F * rcp64(dF);
        t = done ? t : t - d;
        done = done || !(fabs(d) > PE_TOL * t);
        if (!__any(!done)) break;
    }
    return t;
}
__device__ __forceinline__ double pe_middle(double c, double G, double s2) {
    const double iG = rcp64(G);
    double t = fmax(pe_qroot(1.0, c + 2.0 * s2 * iG, s2), pe_qroot(1.0 + 2.0 * s2 * iG * iG, c + s2 * iG, s2));
    bool done = false;
    for (int it = 0; it < PE_NEWTON_MAX; ++it) {
        const double a = rcp64(t), b = rcp64(G - t);
        const double F = ((c + t) - s2 * a) + s2 * b, dF = 1.0 + s2 * (a * a + b * b);
        const double d = F * rcp64(dF);
        t = done ? t : t - d;
        done = done || !(fabs(d) > PE_TOL * t);
        if (!__any(!done)) break;
    }
    return t;
}
__device__ __forceinline__ double pe_below(double A0, double A1, double s2) {
    double e = fmax(pe_qroot(1.0, fmin(A0, A1), s2), pe_qroot(1.0, fmax(A0, A1), 2.0 * s2));
    bool done = false;
    for (int it = 0; it < PE_NEWTON_MAX; ++it) {
        const double a = rcp64(A0 + e), b = rcp64(A1 + e);
        const double K = (e - s2 * a) - s2 * b, dK = 1.0 + s2 * (a * a + b * b);
        const double d = K * rcp64(dK);
        e = done ? e : e - d;
        done = done || !(fabs(d) > PE_TOL * e);
        if (!__any(!done)) break;
    }
    return e;
}
__device__ __forceinline__ void pair_eigen(double l0, double l1, double mu0, double mu1, double v[3]) {
    const double d0 = 2.0 * mu0 + l0, d1 = 2.0 * mu1 + l1, d2 = mu0 + mu1, s2 = 2.0 * mu0 * mu1;
    const bool low0 = d0 <= d1;                          // which pole is the lower one
    const double p = low0 ? d0 : d1, P = low0 ? d1 : d0, G = P - p;
    // per root: x and the gaps (p - x, P - x)
    double x[3], gp[3], gP[3];
    if (d2 < p) { const double e = pe_below(p - d2, P - d2, s2); x[0] = d2 - e; gp[0] = (p - d2) + e; gP[0] = (P - d2) + e; }
    else { const double t = pe_outer(d2 - p, G, s2); x[0] = p - t; gp[0] = t; gP[0] = G + t; }
    const bool hi = d2 > p + 0.5 * G;                    // the middle root lies in the half of (p, P) on d2's side of the midpoint
    {
        const double t = G > 0.0 ? pe_middle(hi ? d2 - P : p - d2, G, s2) : 0.0;
        x[1] = hi ? P - t : p + t; gp[1] = hi ? -(G - t) : -t; gP[1] = hi ? t : G - t;
    }
    // the largest root lies above the upper pole: with a runaway rate its e^{-x} is zero beside the smallest root's - not computed then
    // (a per-lane decision: lanes that need it compute it, and a lane's result never depends on its company in the wave)
    const bool third = P - x[0] <= 745.0;
    x[2] = 0.0; gp[2] = -1.0; gP[2] = -1.0;        // placeholders of a lane without a third term (its weight below is an exact zero)
    if (third) { const double t = pe_outer(P - d2, G, s2); x[2] = P + t; gp[2] = -(G + t); gP[2] = -t; }
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i == 2 && !__any(third)) break;
        const double ex = (i == 2 && !third) ? 0.0 : exp(-x[i]);
        const double i0 = rcp64(low0 ? gp[i] : gP[i]), i1 = rcp64(low0 ? gP[i] : gp[i]);        // 1 / (d0 - x), 1 / (d1 - x)
        double cf = (((2.0 * mu0) * v[0]) * i0 + ((2.0 * mu1) * v[1]) * i1 + v[2]) * rcp64(1.0 + s2 * (i0 * i0 + i1 * i1));
        double r0 = mu1 * i0, r1 = mu0 * i1, r2 = 1.0;
        if (i == 1 && !(G > 0.0)) {
            // coinciding poles: the middle eigenvalue IS the pole, right vector (mu1, -mu0, 0), left (mu0, -mu1, 0), l . r = s^2
            cf = (mu0 * v[0] - mu1 * v[1]) * rcp64(s2); r0 = mu1; r1 = -mu0; r2 = 0.0;
        }
        const double z = ex * cf;
        w0 = fma(z, r0, w0); w1 = fma(z, r1, w1); w2 = fma(z, r2, w2);
    }
    v[0] = w0; v[1] = w1; v[2] = w2;
}

// q, neg: the SAME for every lane of the candidate's group (computed by the caller from the
// base point and both forward-difference points).  M = N - q I with N >= 0.  When a state is
// numerically decoupled (e.g. no mass and no inflow in "both in pop 0" after a runaway rate
// with one-directional migration) the forward-difference lanes then perform bit-identical
// arithmetic on the remaining components, so the Jacobian column is exactly zero - as it is in
// the reference, whose solver leaves that rate untouched.
// INT: with the series path taken, vint receives int_0^1 u exp(u M) v du and have_int is set (see taylor3); the stiff paths
// leave it unset (there |M| > 1 and the reference's inverse-based formula is well conditioned: the caller uses that).
template <bool INT = false>
__device__ __forceinline__ void pair_expv(double l0, double l1, double mu0, double mu1, double v[3], double q, double neg, bool ok, Diag& dg, bool& guard,
                                          double* vint = nullptr, bool* have_int = nullptr) {
    if (!ok) { l0 = 0.0; l1 = 0.0; }
    double d0 = 2.0 * mu0 + l0, d1 = 2.0 * mu1 + l1, d2 = mu0 + mu1;
    double nbmax = q + neg;                                  // >= ||N||_1 (column sums q - l0, q - l1, q)
    if (!(nbmax < 1e300)) {                                  // overflowing iterate: report non-finite (TRF shrinks the step)
        guard = true;
        v[0] = v[1] = v[2] = NAN;
        return;
    }
    if (nbmax > 6.0) {
        // stiff iterate (the unbounded solver can run l up to ~1e5 when the gradient
        // vanishes): closed forms.  (Until round 5: dense scaling and squaring of the 3x3 matrix, degree-12 Taylor kernel - the
        // squarings it would have taken are still what the diagnostic build counts.)
        [[maybe_unused]] int sq = 0;
        { double nrm = 2.0 * nbmax; while (nrm > 0.25) { nrm *= 0.5; ++sq; } }
#if MISTI_WORK_COUNTERS
        dg.dense += 1; dg.squarings += sq;
#endif
        if (mu1 == 0.0 || mu0 == 0.0) {
            // Migration in one direction only: the pair chain is a cascade S -> "one in each" -> K (S = both in the population that
            // is left, K = both in the other) and exp(M) is its closed form in divided differences of e^{-x} over the three exit
            // rates (pair_cascade).  A runaway rate makes M stiff but not this form: a few ulps at any norm, and smooth in the rate
            // that is varied, so the forward-difference Jacobian of a saturated residual keeps its digits - the trust region's gain
            // ratio there sits within 5e-4 of SciPy's 0.75 threshold step after step (x / (x + p) for a residual ~ 1/x), and the
            // scaled-and-squared Taylor kernel used here before (13 squarings at rate x length 700) put it on the wrong side on the
            // headline grid: one chain of 64, 2e-6 ... 4e-6 in the likelihood where the reference holds 1e-10.
            pair_cascade(mu1 == 0.0 ? 1 : 2, l0, l1, mu0, mu1, v);
#if MISTI_WORK_COUNTERS
            dg.dense += 1;
#endif
            if (!ok) { v[0] = v[1] = v[2] = NAN; }
            return;
        }
        // migration in both directions: the closed form over the three eigenvalues of the (symmetrisable) generator (pair_eigen)
        pair_eigen(l0, l1, mu0, mu1, v);
        if (!ok) { v[0] = v[1] = v[2] = NAN; }
        return;
    }
    if (2.0 * nbmax <= 2.0) {
        // small norm (the usual case: rate x interval length << 1): plain Taylor series of exp(M) v,
        // straight-line code with a degree fixed by the norm class ((2 nb)^K / K! < 1e-19) and literal
        // reciprocals.  No shift, no exp(); cancellation is bounded by e^2 ulp, and a decoupled
        // component again sees identical arithmetic in every forward-difference lane.
        const double nn = 2.0 * nbmax;                // >= ||M||_1
        if (nn <= 0.01) taylor3<8, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        else if (nn <= 0.04) taylor3<10, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        else if (nn <= 0.12) taylor3<12, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        else if (nn <= 0.25) taylor3<14, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        else if (nn <= 0.5) taylor3<17, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        else if (nn <= 1.0) taylor3<21, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        else taylor3<27, INT>(d0, d1, d2, mu0, mu1, v, dg, vint);
        if (INT) *have_int = true;
        if (!ok) { v[0] = v[1] = v[2] = NAN; }
        return;
    }
    const double qs = q, nbs = nbmax;
    double n00 = qs - d0, n11 = qs - d1, n22 = qs - d2;
    double n02 = mu1, n12 = mu0, n20 = 2.0 * mu0, n21 = 2.0 * mu1;
    double eq = exp(-qs);
    {
        double p0 = eq * v[0], p1 = eq * v[1], p2 = eq * v[2];
        double a0 = p0, a1 = p1, a2 = p2;
        double b = 1.0;                    // nbs^k / k! bounds the k-th term for every lane
        double inv_next = c_inv[1];
        for (int k = 1; k < 200; ++k) {
            const double inv = inv_next;
            inv_next = c_inv[k + 1];
            double t0 = (n00 * p0 + n02 * p2) * inv;
            double t1 = (n11 * p1 + n12 * p2) * inv;
            double t2 = (n20 * p0 + n21 * p1 + n22 * p2) * inv;
            p0 = t0; p1 = t1; p2 = t2;
            a0 += p0; a1 += p1; a2 += p2;
            b *= nbs * inv;
#if MISTI_WORK_COUNTERS
            dg.terms += 1;
#endif
            if (b < 1e-19 && (double)k > nbs) break;
        }
        v[0] = a0; v[1] = a1; v[2] = a2;
    }
    if (!ok) { v[0] = v[1] = v[2] = NAN; }
}

// ---- the REFERENCE's form of the default fit's expected coalescence time, imitated operation by operation ----
// ExpectedCoalTimeTwoPop (CorrectLambda.py:94-110, T = 1 after the stretch):
//     MET = expm(M);  Minv = inv(M);  vec1 = Minv (Minv ((MET - I) pn));  vec2 = Minv (MET pn);  ect = l . (vec2 - vec1) / (1 - sum(MET pn))
// with expm as scipy computes it for small matrices - the Pade approximant of Al-Mohy & Higham (2009), order 3 / 5 / 7 / 9 by
// the 1-norm, (V - U) X = (V + U) solved by LU - and the inverse as an explicit matrix by LU with partial pivoting (LAPACK's
// getrf order).  NOT used for any value or step: its difference to the integral series is a draw of the rounding noise the
// reference's residual carries (ect_noise_continues).  What matters is the STRUCTURE - matrix functions first, vectors last: an
// entry of exp(M) that does not depend on the rates being varied keeps its rounding error from one forward-difference point to
// the next, as in the reference, so only the error's random part reaches the Jacobian; solving with the vector as right-hand
// side instead re-draws all of it (measured on 481 solves of the random campaign against the reference's own formula: noise
// width 2.2 x the reference's at the median, 1.0 ... 5 x between the deciles; vector solves 3 x, 1.2 ... 20 x).
__constant__ double c_pade[4][10] = {{120., 60., 12., 1., 0., 0., 0., 0., 0., 0.},
                                     {30240., 15120., 3360., 420., 30., 1., 0., 0., 0., 0.},
                                     {17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1., 0., 0.},
                                     {17643225600., 8821612800., 2075673600., 302702400., 30270240., 2162160., 110880., 3960., 90., 1.}};
__device__ __forceinline__ double ect_reference_form(double mu0, double mu1, double l0, double l1, const double pn[3]) {
    const double M[3][3] = {{-2 * mu0 - l0, 0.0, mu1}, {0.0, -2 * mu1 - l1, mu0}, {2 * mu0, 2 * mu1, -mu0 - mu1}};
    // Pade coefficients b_0 .. b_m of orders 3, 5, 7, 9 and the 1-norm up to which each order is used (Al-Mohy & Higham 2009, table 2.3)
    double n1 = 0.0;
    for (int c = 0; c < 3; ++c) n1 = fmax(n1, (fabs(M[0][c]) + fabs(M[1][c])) + fabs(M[2][c]));
    const int m = n1 <= 1.495585217958292e-002 ? 3 : n1 <= 2.539398330063230e-001 ? 5 : n1 <= 9.504178996162932e-001 ? 7 : 9;
    const double* bm = c_pade[(m - 3) >> 1];
    auto coef = [&](int i) { return bm[i]; };
    double A2[3][3], P[3][3], Wm[3][3], V[3][3], T3[3][3];
    mat3_mul(M, M, A2);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { const double id = r == c ? 1.0 : 0.0; P[r][c] = id; Wm[r][c] = coef(1) * id; V[r][c] = coef(0) * id; }
#pragma unroll 1
    for (int j = 1; j <= m / 2; ++j) {
        mat3_mul(P, A2, T3);
        const double bo = coef(2 * j + 1), be = coef(2 * j);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { P[r][c] = T3[r][c]; Wm[r][c] = Wm[r][c] + bo * P[r][c]; V[r][c] = V[r][c] + be * P[r][c]; }
    }
    double U[3][3], Q[3][3], N[3][3], E[3][3], Minv[3][3];
    mat3_mul(M, Wm, U);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { Q[r][c] = V[r][c] - U[r][c]; N[r][c] = V[r][c] + U[r][c]; }
    mat3_solve(Q, N, E);
    const double I3[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    mat3_solve(M, I3, Minv);
    double EmI[3][3], t1[3], t2[3], vec1[3], w[3], vec2[3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) EmI[r][c] = E[r][c] - (r == c ? 1.0 : 0.0);
    mat3_vec(EmI, pn, t1);
    mat3_vec(Minv, t1, t2);
    mat3_vec(Minv, t2, vec1);
    mat3_vec(E, pn, w);
    const double pnc = (w[0] + w[1]) + w[2];
    mat3_vec(Minv, w, vec2);
    return (l0 * (vec2[0] - vec1[0]) + l1 * (vec2[1] - vec1[1])) / (1.0 - pnc);
}

// ExpectedCoalTimeOnePop, CorrectLambda.py:67-72 (note the lam > 100 clamp)
__device__ __forceinline__ double ect_one_pop(double lam, double T) {
    double r = lam > 100.0 ? 0.0 : T / (exp(lam * T) - 1.0);
    return 1.0 / lam - r;
}
// ExpectedCoalTimeOnePopNonConditional, CorrectLambda.py:79-80
__device__ __forceinline__ double ect_noncond(double lam, double T) { return (1.0 - exp(-lam * T) * (1.0 + lam * T)) / lam; }

// Residuals of the migrating two-population interval, evaluated for the base
// point and both forward-difference points in one pass of the candidate's lane group.
// lane (within the group) = 2*e + k: e = 0 base, 1 = x + h0 e0, 2 = x + h1 e1; k = genome.
struct PairProblem {
    double mu0, mu1;       // stretched to unit interval (CorrectLambda.py:293-298)
    // of THIS lane's genome k = role & 1 (a lane evaluates one genome for as long as it lives: keeping only its own row
    // halves what the solver loop carries)
    double Pk[3];          // pair-state vector at the start of the interval
    double sk;             // its sum
    double tgtk;           // cpfit: exp(-lh_k) * s_k (:141); default fit: one-population expected coalescence time (:74-77)
    int red;               // structural reduction of the pair generator for this interval (pair_reduced): 0 none, 1 / 2 state 0 / 1 empty and unfed
};

// One residual evaluation per lane: this lane's role r (= 2 e + k, see PairProblem) at ITS point (x0, x1).  The six
// lanes of a slot share the point; different slots of a wave may hold different points (the needed one and guesses of
// its successors, see correct_body).  A pure function of (pb, point, role): what else sits in the wave changes no bit.
// PROBE (default fit only): *probe receives, for this lane's evaluation, the difference between the REFERENCE's form of the
// expected coalescence time (ect_reference_form) and the integral series used for the value: one draw of the rounding noise the
// reference's residual carries at this point (the series' integral is accurate to a few ulps, and the quotient by 1 - pnc carries the
// rounding of pnc beside one: 16 eps (1 + 1 / (1 - pnc)) of ect bounds it - measured 1e-15 ... 8e-15 relative at |M| 0.12 ... 2, 5e-14 at 0.01 and 4e-11 at
// |M| = 1e-5, tests/test_gpu_pair_residuals.py; the formula loses ~1/|M|^2 digits).  See ect_noise_continues.
template <bool CPFIT, bool PROBE = false>
__device__ __forceinline__ void pair_eval(const PairProblem& pb, double x0, double x1, int role, Diag& dg, double& res, double w[3], bool& guard,
                                          double* probe = nullptr) {
    const double h0 = fd_step(x0), h1 = fd_step(x1);
    const double xa = x0 + h0, xb = x1 + h1;
    const int e = role >> 1;
    const double l0 = (e == 1) ? xa : x0;
    const double l1 = (e == 2) ? xb : x1;
    const bool ok = isfinite(x0) && isfinite(x1);
    // slot-uniform uniformisation rate: the largest over the three evaluation points
    const double m0 = fmax(x0, xa), m1 = fmax(x1, xb);
    const double q = fmax(fmax(2.0 * pb.mu0 + m0, 2.0 * pb.mu1 + m1), fmax(pb.mu0 + pb.mu1, 0.0));
    const double neg = fmax(0.0, fmax(-fmin(x0, xa), -fmin(x1, xb)));
    const double sk = pb.sk;
    if (CPFIT) {
        // LambdaSystem1 / LambdaEquation, CorrectLambda.py:135-144,169-173
        for (int i = 0; i < 3; ++i) w[i] = pb.Pk[i];
        if (pb.red != 0 && q + neg < 1e300) pair_reduced(pb.red, l0, l1, pb.mu0, pb.mu1, w, ok);
        else pair_expv(l0, l1, pb.mu0, pb.mu1, w, q, neg, ok, dg, guard);
        // summed in the reference's order (:141-144).  (Tried: the pieces that do not depend on a runaway rate first, so that its
        // forward difference keeps more digits than the reference's own - campaign seeds 1 and 2 then lose 2 statuses and 10
        // candidates, config 5 sixteen: the reference's decisions carry the rounding of ITS sum.)
        res = ((w[0] + w[1]) + w[2]) - pb.tgtk;
    } else {
        // LambdaSystem / ExpectedCoalTimeTwoPop, CorrectLambda.py:94-110,151-157
        double pn[3], vint[3] = {0.0, 0.0, 0.0};
        bool have_int = false;
        for (int i = 0; i < 3; ++i) { pn[i] = pb.Pk[i] / sk; w[i] = pn[i]; }
        pair_expv<true>(l0, l1, pb.mu0, pb.mu1, w, q, neg, ok, dg, guard, vint, &have_int);
        double pnc = (w[0] + w[1]) + w[2];
        double v0 = vint[0], v1 = vint[1];          // (vec2 - vec1) of the reference, T = 1 after the stretch
        if (!have_int) {
            // stiff iterate (|M| > 1): the reference's own formula, M^-1 exp(M) pn - M^-2 (exp(M) - I) pn
            double M[3][3] = {{-2 * pb.mu0 - l0, 0.0, pb.mu1}, {0.0, -2 * pb.mu1 - l1, pb.mu0}, {2 * pb.mu0, 2 * pb.mu1, -pb.mu0 - pb.mu1}};
            double dd[3] = {w[0] - pn[0], w[1] - pn[1], w[2] - pn[2]};
            double y[3], vec1[3], vec2[3];
            solve3(M, dd, y);
            solve3(M, y, vec1);
            solve3(M, w, vec2);
            v0 = vec2[0] - vec1[0]; v1 = vec2[1] - vec1[1];
        }
        double ect = (l0 * v0 + l1 * v1) / (1.0 - pnc);
        res = ect - pb.tgtk;
        if (PROBE) {
            double d = 0.0;
            if (have_int) d = ect_reference_form(pb.mu0, pb.mu1, l0, l1, pn) - ect;
            *probe = (d == d && fabs(d) < 1e300) ? d : 0.0;
        }
        // the state vector handed on is exp(M) applied to the unnormalised vector
        w[0] *= sk; w[1] *= sk; w[2] *= sk;
    }
}

// ---- default fit: would the REFERENCE stop here? ----------------------------------------------------------------------------
// SciPy stops a solve when |J^T f|_inf < gtol = 1e-10 (trf.py:452).  The reference's residual of the default fit is
// M^-1 e^M p - M^-2 (e^M - I) p (CorrectLambda.py:94-110), which carries ~eps/|M|^2 = 1e-14 ... 1e-9 of rounding noise; its
// forward-difference Jacobian (h = 1.5e-8) therefore ~1e-6 ... 1e-1, so its Gauss-Newton step from x to x + p lands
// -J^-1 dJ p off the step an exact Jacobian gives, where the residual is still f - dJ p: the reference's gradient test sees
// J^T (f - dJ p) and, wherever |J^T dJ p| >~ gtol, goes on for one more evaluation - which converges to the root - where the
// noise-free integral series used here already satisfies gtol and would stop 1e-8 ... 1e-7 short in the rate (round 2's open
// parity defect: campaign seed 2 model 35, 1.2e-8 ... 1.7e-8 in the likelihood where the reference's own spread is 6e-12).
// The reference's noise cannot be reproduced bit for bit (its expm is scipy's Pade approximant through BLAS, its inverse
// LAPACK's getri), but its SIZE can be measured: six draws per genome of (reference formula - series) at points within 3 h of
// the step's base point give the width W of the error distribution; the median |dJ p| of a forward difference of two such
// errors is 0.29 W |p| / h.  The solve goes on iff  sqrt(g_i^2 + sum_k (J_ki 0.29 W_k max_j |p_j / h_j|)^2) >= gtol  for some i
// (W: the measured width scaled by the calibrated ratio between the imitation's noise and the reference's own).
// Where that flips within the noise the reference itself flips under perturbation (its measured spread covers either
// decision: e.g. model 35's other chain, 1.9e-8); where the noise term dominates (model 35) or vanishes (a converged step:
// |p| ~ 1e-8) the decision is the reference's.  Steps and values always come from the series: a wrong guess moves the rate by
// at most what gtol leaves open anyway.
template <int GROUP>
__device__ __forceinline__ bool ect_noise_continues(const PairProblem& pb, double xo0, double xo1, const double p[2], const double J[2][2],
                                                    const double g[2], int role) {
    const double h0 = fd_step(xo0), h1 = fd_step(xo1);
    double lo0 = INFINITY, hi0 = -INFINITY, lo1 = INFINITY, hi1 = -INFINITY;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const double bx0 = xo0 + (2.0 * s) * h0, bx1 = xo1 + (2.0 * s) * h1;
        Diag dgp;
        double resp, wp[3], d = 0.0;
        bool guardp = false;
        pair_eval<false, true>(pb, bx0, bx1, role, dgp, resp, wp, guardp, &d);
        for (int e = 0; e < 3; ++e) {
            const double d0 = gbcast<GROUP>(d, 2 * e), d1 = gbcast<GROUP>(d, 2 * e + 1);
            lo0 = fmin(lo0, d0); hi0 = fmax(hi0, d0); lo1 = fmin(lo1, d1); hi1 = fmax(hi1, d1);
        }
    }
    // range of N = 6 draws -> width of the distribution: x (N + 1) / (N - 1); the imitation's width -> the reference's: / 2.2 (median
    // ratio over 481 sampled solves, see ect_reference_form)
    const double W0 = (hi0 - lo0) * (1.4 / 2.2), W1 = (hi1 - lo1) * (1.4 / 2.2);
    const double ph = fmax(fabs(p[0] / h0), fabs(p[1] / h1));
    const double A0 = 0.29 * W0 * ph, A1 = 0.29 * W1 * ph;
    const double n0 = (J[0][0] * A0) * (J[0][0] * A0) + (J[1][0] * A1) * (J[1][0] * A1);
    const double n1 = (J[0][1] * A0) * (J[0][1] * A0) + (J[1][1] * A1) * (J[1][1] * A1);
    const double e0 = g[0] * g[0] + n0, e1 = g[1] * g[1] + n1;
    return fmax(e0, e1) >= LSQ_GTOL * LSQ_GTOL;
}

}  // namespace misti
